"""CPU: the conditions tests/test_gpu_spread_ladder.py leans on -- no kernel is under test here.  On every shape, family
and rung of tests/spread_ladder.py the oracle (the reference's LogMath order) succeeds with finite results; the oracle's
own transition scores differ from the X = 0 scores by exactly the designed pattern, for every model type; the lone_max
gradient does not depend on X from 600 nats on and is rich; and the rungs visit all three regimes of exp(-X)."""
import numpy as np
import pytest

import orc
import spread_ladder as sl

GRAD_RUNGS = tuple(x for x in sl.FULL if x >= 600)


@pytest.mark.parametrize("family", sl.FAMILIES)
@pytest.mark.parametrize("shape", sl.SHAPE_NAMES)
def test_the_oracle_succeeds_with_finite_results_on_every_rung(shape, family):
    for X in sl.rungs(family, True):
        g, numer, zx = sl.reference(shape, family, X)      # (Case.oracle_gradient asserts the oracle's return code)
        assert np.isfinite(g).all() and np.isfinite(numer).all() and np.isfinite(zx).all(), X


def window_rows(c, T):
    """(end frame, duration) of every window row of an utterance of length T"""
    out = [None] * orc.num_segs(T, c.D)
    for t in range(T):
        for d in range(1, min(t + 1, c.D) + 1):
            out[orc.seg_base(t, c.D) + d - 1] = (t, d)
    return out


def in_the_pattern(c, T, d, valid):
    """d = M(X) - M(0) of one utterance brought to [matrix, previous label, current label], and which of its entries the
    model scores at all: the window models leave the utterance-initial windows (no predecessor) at 0, STDSEG also the
    previous full labels whose duration the predecessor node cannot carry, and its columns are the phones at the
    window's own duration"""
    NL = c.ocfg.num_labs
    mt = c.ocfg.model_type
    seen = np.broadcast_to(valid[None], (d.shape[0], NL, NL)).copy()
    if mt == orc.STDSEG_NO_DUR:
        for r, (t, dur) in enumerate(window_rows(c, T)):
            seen[r] &= dur <= min(t, c.D)
    elif mt == orc.STDSEG:
        full = np.zeros((d.shape[0], NL, NL))
        for r, (t, dur) in enumerate(window_rows(c, T)):
            cols = (dur - 1) * c.L + np.arange(c.L)
            full[r][:, cols] = d[r]
            ok = np.zeros((NL, NL), dtype=bool)
            if dur <= min(t, c.D):
                ok[:c.L * min(t - dur + 1, c.D), cols[0]:cols[-1] + 1] = True
            seen[r] &= ok
        d = full
    return d, seen


@pytest.mark.parametrize("family", sl.FAMILIES)
@pytest.mark.parametrize("shape", sl.SHAPE_NAMES)
def test_the_transition_scores_move_by_the_designed_pattern(shape, family):
    """M(X) - M(0) from the model's own score function: -X on the lowered entries and on the entries set to -X (which are 0 at
    X = 0), nothing (to the bit) anywhere else -- so no family is a no-op on any model type, and none moves an entry it should
    not.  Entries the n-state topology lacks are skipped."""
    X = 735
    c0, cx = sl.case(shape, family, 0), sl.case(shape, family, X)
    base = sl.case(shape, "lone_max", 0)          # lone_max at 0 leaves every transition bias as drawn
    NL = c0.ocfg.num_labs
    lowered, put, state = sl.designed_shift(c0, family, X)
    want = np.zeros((NL, NL)); valid = np.zeros((NL, NL), dtype=bool)
    for p in range(NL):
        for n in range(NL):
            i = sl.trans_bias_index(c0, p, n)
            if i is None:
                continue
            valid[p, n] = True
            if lowered[p, n] or put[p, n]:      # (a bias set to -X: against the family's own X = 0 matrix, where it is 0)
                want[p, n] = -X
    assert (lowered | put)[valid].any()
    changed = 0
    for u, (M0, MX) in enumerate(zip(sl.oracle_matrices(c0), sl.oracle_matrices(cx))):
        d, seen = in_the_pattern(c0, c0.Ts[u], MX - M0, valid)
        w = np.broadcast_to(want[None], d.shape)
        moved = seen & (w != 0)
        assert not moved.any() or np.abs(d[moved] - w[moved]).max() <= 1e-9, (shape, family, u)     # (T = 1 has no transition)
        assert not d[seen & (w == 0)].any(), (shape, family, u)
        changed += int(moved.sum())
    assert changed > 0
    # heavy families set the bias: at X = 0 the designed entries are 0 where lone_max at 0 has the drawn bias
    if family != "lone_max":
        i = sl.trans_bias_index(c0, *np.argwhere(put & valid)[0])
        assert c0.lam[i] == 0.0 and base.lam[i] != 0.0
    for l, v in state.items():
        assert cx.lam[cx.olay.state_idx[l] + cx.olay.num_state_funcs - 1] == v


@pytest.mark.parametrize("shape", sl.SHAPE_NAMES)
def test_lone_max_gradient_is_rich_and_does_not_depend_on_the_spread(shape):
    """q carries no mass, so X only prices the number of segments: from 600 nats on the posteriors are those of the
    paths with the fewest segments, whatever X is.  Rich: more than half of the gradient's entries exceed 1e-3.  Under
    STDSEG that is asked of the state weights: its transition block runs over pairs of FULL labels (previous duration,
    own duration), most of which no path through utterances this short can take (the two durations must fit into T
    frames; stdseg480 has 230400 pairs and 21 frames), so a fraction of the whole gradient says nothing there; some
    transition weights must still move."""
    g600 = sl.reference(shape, "lone_max", 600)[0]
    dev = max(np.abs(sl.reference(shape, "lone_max", X)[0] - g600).max() for X in GRAD_RUNGS)
    c = sl.case(shape, "lone_max", 600)
    state = np.zeros(g600.shape[0], dtype=bool)
    for l in range(c.ocfg.num_labs):
        state[c.olay.state_idx[l]:c.olay.state_idx[l] + c.olay.num_state_funcs] = True
    big = np.abs(g600) > 1e-3
    print("%s: lone_max gradient drifts by %.2e over the rungs from 600 on; %.0f %% of its entries exceed 1e-3 (state weights %.0f %%, "
          "transition weights %.0f %%)" % (shape, dev, 100 * big.mean(), 100 * big[state].mean(), 100 * big[~state].mean()))
    assert dev <= 1e-11
    if c.ocfg.model_type == orc.STDSEG:
        assert big[state].mean() > 0.5 and big[~state].any()
    else:
        assert big.mean() > 0.5


def test_the_rungs_visit_every_regime_of_exp():
    tiny = np.finfo(np.float64).tiny
    e = np.exp(-np.asarray(sl.FULL, dtype=np.float64))
    assert (e >= tiny).sum() >= 2 and ((e > 0) & (e < tiny)).sum() >= 2 and (e == 0).sum() >= 2
    e = np.exp(-np.asarray(sl.REDUCED, dtype=np.float64))     # the reduced ladder: one zero rung, 900 (heavy_out adds 1500)
    assert (e >= tiny).sum() >= 2 and ((e > 0) & (e < tiny)).sum() >= 2 and (e == 0).sum() >= 1
    assert (np.exp(-np.asarray(sl.rungs("heavy_out", False), dtype=np.float64)) == 0).sum() >= 2
    assert set(sl.REDUCED) <= set(sl.FULL) and set(sl.WINDOW) <= set(sl.FULL)


def test_the_existing_wide_spread_point_is_heavy_out_at_1500():
    c = sl.wide_spread_case(1)
    lay = c.olay
    assert (c.L, c.D, c.Ts) == (4, 3, [6, 9, 5]) and c.gcfg.train_precision == 1
    assert c.lam[lay.state_idx[0] + lay.num_state_funcs - 1] == 1000.0
    assert all(c.lam[lay.trans_idx[0 * c.L + n]] == -1500.0 for n in range(c.L))
    other = [c.lam[lay.trans_idx[p * c.L + n]] for p in range(1, c.L) for n in range(c.L)]
    assert max(abs(v) for v in other) < 1.0
