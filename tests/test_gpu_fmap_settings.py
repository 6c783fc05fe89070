"""-m gpu: every kernel path under the feature map's settings off their defaults (tests/fmap_settings.py): bias values other
than 1.0 (a dropped or doubled factor), a bias switched off (an off-by-one in a column count), state columns that do not
start at column 0 or stop short of the window, transition columns that overlap the state columns or leave a gap, and a map
without state features.  The older tests run every path with both biases on at 1.0 and the full column ranges.

Decode surfaces and layouts are compared bit for bit with the oracle, the training side at the per-tier bounds of
tests/gpu_checks.py; tests/test_fmap_settings.py establishes on the CPU what these tests lean on.  Two tests need no oracle: a
power-of-two bias value with the bias weights scaled the other way changes no bit of the scores, and a bias switched off
is a bias weight of zero.  Every test prints the largest deviation it saw before it asserts."""
import numpy as np
import pytest

import align_ref as ar
import family_shapes as fs
import fmap_settings as fm
import latprune_ref as lr
import orc
import post_ref
import scrf_amd
from family_shapes import FUSED3, POST_SHAPES
from gpu_checks import (EXACT, FAST, FAST32, FASTLIN, NAME, POST_TOL, TOL, bits, check_decode_surfaces, check_posteriors,
                        check_training, same_paths)

pytestmark = pytest.mark.gpu

TIERS = (EXACT, FAST, FASTLIN, FAST32)


def check_layout(c, eng):
    """the layout hooks against the oracle's layout: lengths, function counts and the first index of every block"""
    lay, L = c.olay, c.ocfg.num_labs
    assert eng.lambda_len == lay.lambda_len
    assert eng.num_state_funcs() == lay.num_state_funcs and eng.num_trans_funcs() == lay.num_trans_funcs
    assert [eng.state_idx(l) for l in range(L)] == [int(v) for v in lay.state_idx]
    step = max(1, (L * L) // 400)     # every pair up to 20 labels, a stride over the larger tables (first and last included)
    pairs = sorted(set(range(0, L * L, step)) | {L * L - 1})
    assert [eng.trans_idx(i // L, i % L) for i in pairs] == [int(lay.trans_idx[i]) for i in pairs]


@pytest.mark.parametrize("row", fm.ROWS, ids=fm.row_id)
def test_setting_on_every_path(row, monkeypatch):
    """One row of the table: decode surfaces and layout hooks bit for bit, then gradient, Zx and numerator under every tier,
    no log-domain redo, and the batch on the path the table names under FAST (so that no row ends up silently on the general
    path, or off it).  The mixed shape runs with SCRF_FUSE_MIXED=1 and 0."""
    setting, shape, family = row
    c0, utts, ref = fm.reference(*row)
    want_fast = fm.fast_mode(setting, shape)
    for mixed in (("1", "0") if shape == "mixed" else (None,)):
        if mixed is not None:
            monkeypatch.setenv("SCRF_FUSE_MIXED", mixed)
        what = fm.row_id(row) + ("" if mixed is None else " SCRF_FUSE_MIXED=" + mixed)
        c = fm.case(setting, shape, family)
        eng = c.engine(); b = c.batch(eng, with_labels=False)
        check_layout(c, eng)
        check_decode_surfaces(c, utts, eng, b)
        b.close(); eng.close()
        for prec in TIERS:
            mode = check_training(fm.case(setting, shape, family, precision=prec), ref, prec, what)
            if mixed == "0":
                assert mode == 0
            elif prec == FAST and want_fast is not None:
                assert mode == want_fast, (what, mode, want_fast)


@pytest.mark.parametrize("row", [r for r in fm.ROWS if fm.fast_mode(r[0], r[1]) == 1], ids=fm.row_id)
def test_fused_rows_with_the_duration_table_built_per_tile(row, monkeypatch):
    """SCRF_DTAB=0: the fused score kernel folds lambda[bias] * value into its duration weights itself (dur_w) instead of
    copying k_dur_table's output -- the form every D > 40 takes.  The rows that stay on the fused kernels: best paths (the
    fast decode runs the same kernel) bit for bit, and the three tiers that train through it."""
    setting, shape, family = row
    c0, utts, ref = fm.reference(*row)
    monkeypatch.setenv("SCRF_DTAB", "0")
    c = fm.case(setting, shape, family)
    eng = c.engine(); b = c.batch(eng, with_labels=False)
    check_decode_surfaces(c, utts, eng, b)
    b.close(); eng.close()
    for prec in (FAST, FASTLIN, FAST32):
        mode = check_training(fm.case(setting, shape, family, precision=prec), ref, prec, fm.row_id(row) + " SCRF_DTAB=0")
        assert mode == (2 if prec == FASTLIN and shape in fs.FASTLIN_FORM2 else 1)


@pytest.mark.parametrize("setting,shape", fm.REFUSED)
def test_the_nstate_topology_without_a_transition_bias_is_refused(setting, shape):
    o = dict(use_trans_bias=False) if setting == "notb" else dict(use_state_bias=False, use_trans_bias=False)
    c = fs.Case(seed=1, fmap=o, **fs.SHAPES[shape][0])
    with pytest.raises(scrf_amd.ScrfError) as e:
        scrf_amd.Engine(c.gcfg)
    assert fm.REFUSAL in str(e.value)


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("setting", ("big+", "big-"))
@pytest.mark.parametrize("shape", FUSED3)
def test_fast_decode_under_large_bias_values(shape, setting, monkeypatch):
    """|state bias value| = 40 enters the fast-decode screen's bound through xm = max(1, |value|, max|x|): labels and float costs
    equal the EXACT decode's and the oracle's shortest path bit for bit, no chunk falls back, and under the widened screen
    (SCRF_DECODE_BOUND_SCALE=30) the number of recomputed weights lies in the bracket predicted from the oracle's scores with
    that xm (tests/test_fmap_settings.py: on the two larger shapes a screen that left the bias value out falls below the bracket)."""
    c0, utts, _ = fm.reference(setting, shape)
    res = {}
    for tag, env in [("exact", {"SCRF_FAST_DECODE": "0"}), ("fast", {}), ("fix", {"SCRF_DECODE_BOUND_SCALE": "30"})]:
        for k in ("SCRF_FAST_DECODE", "SCRF_DECODE_BOUND_SCALE"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        c = fm.case(setting, shape)
        eng = c.engine(); b = c.batch(eng, with_labels=False)
        assert eng.batch_is_fused(b)
        labs, cost = eng.viterbi_batch(b)
        res[tag] = (labs, cost, eng.decode_stats())
        b.close(); eng.close()
    lo, hi = fs.predicted_screen_count(c0, 28.9), fs.predicted_screen_count(c0, 31.1)
    print("%s %s: recomputed plain %d, widened %d (predicted %d .. %d)" % (setting, shape, res["fast"][2][0], res["fix"][2][0], lo, hi))
    el, ec, est = res["exact"]
    assert est == (0, 0)
    assert same_paths(el, ec, [u[6] for u in utts], [u[7] for u in utts])
    for tag in ("fast", "fix"):
        gl, gc, st = res[tag]
        assert same_paths(gl, gc, el, ec), tag
        assert st[1] == 0, tag
    assert res["fast"][2][0] <= res["fix"][2][0]
    assert lo <= res["fix"][2][0] <= hi


# ---------------------------------------------------------------------------------------------------------------------
def surfaces(c):
    """EXACT scores, lattice arcs and Zx of a case, as raw arrays"""
    eng = c.engine(); b = c.batch(eng)
    out = []
    for u, T in enumerate(c.Ts):
        S, M = eng.scores(b, u, T)
        if c.ocfg.model_type not in (orc.STDSEG, orc.STDSEG_NO_DUR):
            M = M[1:]      # the transition into frame t; the first frame has none
        arcs, ns, fin = eng.lattice_arcs(b, u)
        out.append((S.copy(), M.copy(), arcs.copy(), ns, fin))
    numer, zx = eng.fb_batch(b)
    b.close(); eng.close()
    return out, zx.copy()


def train(c, prec):
    c = fs.case_like(c, precision=prec)
    eng = c.engine(); b = c.batch(eng)
    numer, zx = eng.fb_batch(b)
    g = eng.get_grad()
    assert eng.train_stats() == 0
    b.close(); eng.close()
    return numer, zx, g


@pytest.mark.parametrize("shape", ("fused", "mixed", "stdseg_lin", "frame"))
def test_power_of_two_bias_value_changes_nothing(shape):
    """state bias value 4 with the state-bias weights over 4, transition bias value 0.5 with the transition-bias weights times
    2: every product keeps its bits, so no oracle is needed.  EXACT scores, lattice arcs and Zx are bit-identical to the
    default engine's; under every tier the gradient agrees within the tier's bound of its largest component once the bias
    components are scaled back (they are 4 times and 0.5 times the default's: d/dw of value * w)."""
    c = fm.case("vals", shape, fmap={})
    r = fm.case("vals", shape, fmap=dict(state_bias_val=4.0, trans_bias_val=0.5))
    sb, tb = fm.bias_masks(c)
    assert sb.any() and tb.any() and np.array_equal(r.lam, c.lam)
    r.lam = np.where(sb, c.lam / 4.0, np.where(tb, c.lam * 2.0, c.lam))
    (s0, z0), (s1, z1) = surfaces(c), surfaces(r)
    for (S0, M0, a0, ns0, fin0), (S1, M1, a1, ns1, fin1) in zip(s0, s1):
        assert np.array_equal(bits(S0), bits(S1)) and np.array_equal(bits(M0), bits(M1))
        assert (ns0, fin0) == (ns1, fin1) and a0.tobytes() == a1.tobytes()
    assert np.array_equal(bits(z0), bits(z1))
    for prec in TIERS:
        n0, z0, g0 = train(c, prec)
        n1, z1, g1 = train(r, prec)
        g1 = np.where(sb, g1 / 4.0, np.where(tb, g1 * 2.0, g1))     # exact
        tg, tz, tn = TOL[prec]
        e_g = np.abs(g1 - g0).max() / np.abs(g0).max()
        e_b = np.abs(g1 - g0)[sb | tb].max() / np.abs(g0).max()
        e_z = np.abs(z1 - z0).max() / np.abs(z0).max()
        e_n = np.abs(n1 - n0).max() / max(1.0, np.abs(n0).max())
        print("%s %s: gradient %.3e (bias components %.3e; bound %.0e)  Zx %.3e  numerator %.3e" % (shape, NAME[prec], e_g, e_b, tg, e_z, e_n))
        assert np.abs(g0[sb]).max() > 0 and np.abs(g0[tb]).max() > 0
        assert e_g <= tg and e_z <= tz and e_n <= tn, NAME[prec]


# ---------------------------------------------------------------------------------------------------------------------
def shared_weights(a, b):
    """index arrays (into a's lambda, into b's) of the feature weights two layouts of one shape share -- every state and
    transition column, no bias -- through the oracle layouts"""
    assert (a.ocfg.num_labs, a.ocfg.state_fidx_start, a.ocfg.state_fidx_end) == (b.ocfg.num_labs, b.ocfg.state_fidx_start, b.ocfg.state_fidx_end)
    L = a.ocfg.num_labs
    nsfe = a.olay.num_state_funcs - int(a.ocfg.use_state_bias)
    ntfe = a.olay.num_trans_funcs - int(a.ocfg.use_trans_bias)
    assert nsfe == b.olay.num_state_funcs - int(b.ocfg.use_state_bias) and ntfe == b.olay.num_trans_funcs - int(b.ocfg.use_trans_bias)
    ia, ib = [], []
    for l in range(L):
        ia.append(int(a.olay.state_idx[l]) + np.arange(nsfe)); ib.append(int(b.olay.state_idx[l]) + np.arange(nsfe))
    if ntfe:
        for i in range(L * L):
            ia.append(int(a.olay.trans_idx[i]) + np.arange(ntfe)); ib.append(int(b.olay.trans_idx[i]) + np.arange(ntfe))
    return np.concatenate(ia), np.concatenate(ib)


@pytest.mark.parametrize("setting", ("nosb", "notb", "nobias"))
@pytest.mark.parametrize("shape", ("fused", "hybrid", "mixed", "no_dur"))
def test_a_switched_off_bias_equals_a_zero_bias_weight(shape, setting):
    """the row's engine against the default layout whose bias weights in question are 0 (the other weights the row's): Zx and
    numerator within the tier's bounds, the gradient on the weights both layouts share.  A shifted column shows here without
    trusting the oracle's layout twice."""
    a = fm.case(setting, shape)
    keep = {"nosb": dict(use_trans_bias=True), "notb": dict(use_state_bias=True), "nobias": {}}[setting]
    b = fm.case(setting, shape, fmap={})
    ia, ib = shared_weights(a, b)
    sb, tb = fm.bias_masks(b)
    lam = np.zeros(b.olay.lambda_len)
    lam[ib] = a.lam[ia]
    sba, tba = fm.bias_masks(a)
    if "use_trans_bias" in keep:      # the bias the row keeps, carried over
        lam[tb] = a.lam[tba]
    if "use_state_bias" in keep:
        lam[sb] = a.lam[sba]
    assert np.count_nonzero(lam) == a.olay.lambda_len
    b.lam = lam
    for prec in TIERS:
        na, za, ga = train(a, prec)
        nb, zb, gb = train(b, prec)
        tg, tz, tn = TOL[prec]
        e_g = np.abs(ga[ia] - gb[ib]).max() / np.abs(gb).max()
        e_z = np.abs(za - zb).max() / np.abs(zb).max()
        e_n = np.abs(na - nb).max() / max(1.0, np.abs(nb).max())
        print("%s %s %s: gradient on the shared weights %.3e (%.0e)  Zx %.3e (%.0e)  numerator %.3e (%.0e)" % (setting, shape, NAME[prec], e_g, tg, e_z, tz, e_n, tn))
        assert e_g <= tg and e_z <= tz and e_n <= tn, NAME[prec]


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("setting", ("vals", "nosb"))
@pytest.mark.parametrize("shape", POST_SHAPES)
def test_posteriors_pruned_lattices_and_alignment(shape, setting):
    """posteriors_batch against tests/post_ref.py at the tier bounds, lattice_prune_batch against tests/latprune_ref.py byte for
    byte over its beams, and align_batch in both modes against tests/align_ref.py bit for bit (a seeded transcript and the best
    path's own phones)"""
    c0, utts, _ = fm.reference(setting, shape)
    pref = [post_ref.utterance(c0, u) for u in range(len(c0.Ts))]
    for prec in TIERS:
        c = fm.case(setting, shape, precision=prec)
        eng = c.engine(); b = c.batch(eng, with_labels=False)
        check_posteriors(c, pref, eng, b, POST_TOL[prec], "%s %s %s form %d" % (setting, shape, NAME[prec], eng.batch_fused_mode(b)))
        assert eng.train_stats() == 0
        b.close(); eng.close()
    c = fm.case(setting, shape)
    eng = c.engine(); b = c.batch(eng, with_labels=False)
    dist = [lr.distances(u[3], u[4], u[5]) for u in utts]
    for beam in lr.BEAMS:
        off, best = eng.lattice_prune_batch(b, beam)
        arcs = eng.pruned_arcs(b)
        assert off[0] == 0 and arcs.shape[0] == off[-1]
        for u, (X, S, M, full, ns, fin, ol, oc) in enumerate(utts):
            fwd, bwd = dist[u]
            want = full[lr.keep_mask(full, fwd, bwd, fin, beam)]
            assert off[u + 1] - off[u] == want.shape[0], (u, beam)
            assert arcs[int(off[u]):int(off[u + 1])].tobytes() == want.tobytes(), (u, beam)
            assert np.float64(best[u]).tobytes() == np.float64(fwd[fin]).tobytes(), (u, beam)
    weights = [ar.case_weights(c0, u) for u in range(len(c0.Ts))]
    rng = np.random.RandomState(fm.SEEDS[(setting, shape)] + 3)
    labs, _ = eng.viterbi_batch(b)
    seeded = [ar.random_transcript(rng, T, c.L, c.D) for T in c.Ts]
    own = [(np.asarray(l, dtype=np.int64) % c.L).astype(np.uint32) for l in labs]
    for tr in (seeded, own):
        for mode in (scrf_amd.ALIGN_ONE, scrf_amd.ALIGN_RUNS):
            al, cost = eng.align_batch(b, tr, mode)
            for u, w in enumerate(weights):
                want_l, want_c = ar.dp(w, tr[u], mode)
                assert np.float32(cost[u]).tobytes() == np.float32(want_c).tobytes(), (u, mode, cost[u], want_c)
                assert [int(x) for x in al[u]] == want_l, (u, mode)
    b.close(); eng.close()
