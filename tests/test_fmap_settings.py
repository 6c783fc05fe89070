"""The rows of tests/fmap_settings.py (the feature map's settings off their defaults) on the CPU oracle alone: the conditions
tests/test_gpu_fmap_settings.py leans on.  The oracle succeeds on every row with a finite, nonzero gradient that agrees with
finite differences of its own objective; the scores stay a few nats apart (the GPU's linear-domain recursion never has to
give up); FASTLIN's gradient bound has room; the layouts are the ones written out in the table; and a kernel that ignored a
bias value would be caught: with both values forced to 1.0 the oracle gradient moves by more than 1e-3."""
import numpy as np
import pytest

import family_shapes as fs
import fmap_settings as fm
import orc
from test_input_families import SPREAD_CAP

ROW_IDS = [fm.row_id(r) for r in fm.ROWS]
FD_H = 1e-5
FD_TOL = 1e-8       # relative to max(1, max|g|); measured on these rows: at most a few 1e-9


def objective(c, X, lam):
    """sum over utterances of numer - zx under weights lam (windows X computed once)"""
    mt = c.ocfg.model_type
    fn = {orc.STDFRAME: orc.frame_build_gradient, orc.STDSEG: orc.stdseg_build_gradient,
          orc.STDSEG_NO_DUR: orc.segtrans_build_gradient}.get(mt, orc.seg_build_gradient)
    tot = 0.0
    for u, T in enumerate(c.Ts):
        rc, _, n, z = fn(c.ocfg, c.olay, lam, X[u], c.labels[u], T)
        assert rc == 0, rc
        tot += n - z
    return tot


def fd_coordinates(c, row):
    """6 seeded coordinates; the first is a state-bias weight and the second a transition-bias weight where the row has them"""
    rng = np.random.RandomState(fm.SEEDS[(row[0], row[1])] + 7)
    sb, tb = fm.bias_masks(c)
    idx = [int(rng.choice(np.flatnonzero(m))) for m in (sb, tb) if m.any()]
    while len(idx) < 6:
        i = int(rng.randint(0, c.olay.lambda_len))
        if i not in idx:
            idx.append(i)
    return idx, bool(sb.any() or tb.any())


@pytest.mark.parametrize("row", fm.ROWS, ids=ROW_IDS)
def test_the_oracle_is_sound_on_every_row(row):
    """status 0 (oracle_gradient asserts it per utterance), gradient finite and nonzero, scores under SPREAD_CAP apart, and
    the gradient equal to central finite differences of numer - zx on 6 coordinates, a bias weight among them"""
    c, utts, (g, numer, zx) = fm.reference(*row)
    assert np.isfinite(g).all() and np.isfinite(numer).all() and np.isfinite(zx).all() and np.abs(g).max() > 0
    spread = max(float(S.max() - S.min()) for (_, S, *_rest) in utts)
    X = [u[0] for u in utts]
    idx, with_bias = fd_coordinates(c, row)
    sb, tb = fm.bias_masks(c)
    assert with_bias == bool(c.ocfg.use_state_bias or c.ocfg.use_trans_bias)
    assert not with_bias or sb[idx[0]] or tb[idx[0]]
    dev = 0.0
    for i in idx:
        lp = c.lam.copy(); lp[i] += FD_H
        lm = c.lam.copy(); lm[i] -= FD_H
        fd = (objective(c, X, lp) - objective(c, X, lm)) / (lp[i] - lm[i])
        dev = max(dev, abs(fd - g[i]))
    dev /= max(1.0, np.abs(g).max())
    print("%s: score spread %.2f nats, finite differences within %.2e (bound %.0e), max|g| %.3g" % (fm.row_id(row), spread, dev, FD_TOL, np.abs(g).max()))
    assert spread < SPREAD_CAP
    assert dev <= FD_TOL


@pytest.mark.parametrize("row", [r for r in fm.ROWS if r[1] in fs.FUSED3 and fm.fast_mode(r[0], r[1]) == 1], ids=fm.row_id)
def test_the_fastlin_bound_has_room(row):
    """the one-stream segmental rows that stay on FASTLIN's own kernels: float32(exact mean) in the average block moves the
    oracle gradient by at most 1e-7 of its largest component (tests/test_input_families.py's bound), a tenth of the tier's"""
    c, _, (g0, _, _) = fm.reference(*row)
    g1 = fs.gradient_with_exact_mean(c)
    dev = np.abs(g1 - g0).max() / np.abs(g0).max()
    print("exact mean against float average, %s: %.2e" % (fm.row_id(row), dev))
    assert dev <= 1e-7


@pytest.mark.parametrize("row", [r for r in fm.ROWS if fm.has_bias_value(r[0], r[1])], ids=fm.row_id)
def test_a_kernel_that_ignored_a_bias_value_would_be_caught(row):
    """the oracle gradient with both bias values forced to 1.0 (everything else the row's) differs from the row's by more than
    1e-3 of its largest component: far above every tier's bound"""
    c, _, (g, _, _) = fm.reference(*row)
    o = fm.overrides(row[0], row[1])
    o.update(state_bias_val=1.0, trans_bias_val=1.0)
    c1 = fm.case(row[0], row[1], row[2], fmap=o)
    assert np.array_equal(c1.lam, c.lam) and all(np.array_equal(a, b) for a, b in zip(c1.frames, c.frames))
    g1, _, _ = c1.oracle_gradient()
    dev = np.abs(g1 - g).max() / np.abs(g).max()
    print("%s: bias values at 1.0 move the gradient by %.2e of its largest component" % (fm.row_id(row), dev))
    assert dev > 1e-3


@pytest.mark.parametrize("setting", ("big+", "big-"))
@pytest.mark.parametrize("shape", fs.FUSED3)
def test_the_decode_screen_count_depends_on_the_bias_value(shape, setting):
    """what test_fast_decode_under_large_bias_values leans on: under SCRF_DECODE_BOUND_SCALE=30 the bracket predicted with
    xm = max(1, |bias value|, max|x|) is well formed, and on the two larger shapes a screen that left the bias value out of xm
    (xm = 1 on this data) would list fewer weights than the bracket's lower end.  (The smallest shape has too few scores for
    either screen to list any.)"""
    c = fm.reference(setting, shape)[0]
    lo, hi = fs.predicted_screen_count(c, 28.9), fs.predicted_screen_count(c, 31.1)
    without = fs.predicted_screen_count(c, 31.1, with_bias_value=False)
    print("%s %s: screen count %d .. %d; with the bias value left out of xm at most %d" % (setting, shape, lo, hi, without))
    assert 0 <= lo <= hi
    if shape != "fused":
        assert without < lo


@pytest.mark.parametrize("key", sorted(fm.EXPECT), ids=lambda k: "%s-%s" % k)
def test_layouts_are_the_ones_written_out(key):
    c = fm.case(*key)
    assert (c.olay.lambda_len, c.olay.num_state_funcs, c.olay.num_trans_funcs) == fm.EXPECT[key]
    assert c.lam.shape == (c.olay.lambda_len,)


def test_the_table_is_complete():
    """every row has its written-out layout; rows are unique; the refused rows are not among them; fmap=None is the old case"""
    assert set(fm.EXPECT) == {(st, sh) for st, sh, _ in fm.ROWS}
    assert len(set(fm.ROWS)) == len(fm.ROWS)
    assert not any((st, sh) in fm.REFUSED for st, sh, _ in fm.ROWS)
    assert len(set(fm.SEEDS.values())) == len(fm.SEEDS) and not set(fm.SEEDS.values()) & set(fs.SEEDS.values())
    kw = fs.SHAPES["mixed"][0]
    a, b = fs.Case(seed=5, **kw), fs.Case(seed=5, fmap={}, **kw)
    assert a.lam.tobytes() == b.lam.tobytes() and bytes(a.gcfg) == bytes(b.gcfg) and bytes(a.ocfg) == bytes(b.ocfg)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a.frames + a.labels, b.frames + b.labels))
    with pytest.raises(AssertionError):
        fs.Case(seed=5, fmap={"L": 3}, **kw)


def test_overrides_reach_both_configurations():
    c = fm.case("sub", "frame")
    for cfg in (c.ocfg, c.gcfg):
        assert (cfg.state_fidx_start, cfg.state_fidx_end, cfg.trans_fidx_start, cfg.trans_fidx_end) == (1, 1, 0, 1)
        assert (cfg.state_bias_val, cfg.trans_bias_val) == (0.25, 4.0)
    c = fm.case("nosf", "fused")
    assert c.ocfg.use_state_ftrs == 0 and c.gcfg.use_state_ftrs == 0 and c.ocfg.use_state_bias == 1
    c = fm.case("nobias", "mixed")
    assert (c.ocfg.use_state_bias, c.ocfg.use_trans_bias, c.gcfg.use_state_bias, c.gcfg.use_trans_bias) == (0, 0, 0, 0)
