"""-m gpu: every recursion across a ladder of transition spreads (tests/spread_ladder.py; tests/test_spread_ladder.py pins
on the CPU what is leaned on here).  The wavefront, linear-domain and STDSEG-linear kernels take the transition step on
exp(M - max M); a batch whose scores are too spread out for that is redone in the log domain, and the caller sees what the
reference's LogMath gives.  The rule under test: whatever route the engine takes, the caller gets the oracle's answer
within the path's existing bound -- on every rung from 0 to 1500 nats, through the range 708 .. 745 nats where
exp(M - max M) is subnormal, for three ways of placing the spread, on every kernel path and tier.

Bounds are those of tests/test_gpu_input_ranges.py (per tier) and tests/test_gpu_stdseg.py (the 480-label STDSEG shape),
tests/test_gpu_posteriors.py, tests/test_gpu_sparse.py and tests/test_gpu_errors.py (node values), copied because test
modules are not imported.  Every test prints one line per rung -- the route taken (linear, or redone) and the largest
deviations -- before it asserts; DESIGN.md 4.1 / 4.6 / 4.13 tabulate them."""
import functools

import numpy as np
import pytest

import family_shapes as fs
import orc
import post_ref
import scrf_amd
import sparse_ref as sr
import spread_ladder as sl

pytestmark = pytest.mark.gpu

EXACT, FAST, FAST32, FASTLIN = scrf_amd.PREC_EXACT, scrf_amd.PREC_FAST, scrf_amd.PREC_FAST32, scrf_amd.PREC_FASTLIN
NAME = {EXACT: "EXACT", FAST: "FAST", FAST32: "FAST32", FASTLIN: "FASTLIN"}
# tests/test_gpu_input_ranges.py: gradient (relative to its largest component), Zx (relative), numerator (relative to
# max(1, |numerator|))
TOL = {EXACT: (1e-9, 1e-11, 1e-11), FAST: (1e-9, 1e-11, 1e-11), FASTLIN: (1e-6, 1e-8, 1e-6), FAST32: (1e-5, 1e-6, 1e-5)}
# tests/test_gpu_stdseg.py, test_bias_only_transitions_linear_domain_path under FAST: gradient 10 * 1e-9 of max(1, largest
# component), Zx 1e-9 relative, numerator 1e-9 of max(1, |numerator|)
STDSEG480_TOL = (1e-8, 1e-9, 1e-9)
POST_TOL = {EXACT: 1e-9, FAST: 1e-9}          # tests/test_gpu_posteriors.py
TIER_SHAPES = fs.FASTLIN_FORM2 + ("hybrid", "stdseg_lin")      # the shapes whose tier selects other kernels
TRAIN = [(s, FAST) for s in sl.SHAPE_NAMES] + [(s, p) for p in (EXACT, FASTLIN, FAST32) for s in TIER_SHAPES]
GROUP = fs.POST_SHAPES + ("frame",)                            # the smaller groups
GROUP_SEG = ("mixed", "fused", "frame")                        # of those, L <= 64: the wavefront kernel k_dp_wave


def deviations(shape, got, ref):
    """(gradient, Zx, numerator) deviations of (g, numer, zx) from the oracle's, each in the measure of its bound"""
    g, numer, zx = got
    og, on, oz = ref
    gden = max(1.0, np.abs(og).max()) if shape == "stdseg480" else np.abs(og).max()
    return (np.abs(g - og).max() / gden, np.abs(zx - oz).max() / np.abs(oz).max(), np.abs(numer - on).max() / max(1.0, np.abs(on).max()))


def bounds(shape, prec):
    return STDSEG480_TOL if shape == "stdseg480" else TOL[prec]


def redo_expected_at_1500(shape, prec):
    """heavy_out at 1500 nats empties the transition step of every kernel that works on exp(M - max M): the batch is redone
    once wherever the first pass ran one of them -- the wavefront kernels (every tier: up to 64 labels k_dp_wave or
    k_dp_lin, up to 256 k_dp_lin_mw) and STDSEG's linear path (bias-only transitions, FAST tiers).  STDSEG_NO_DUR and
    STDSEG with transition features or under EXACT run a log-domain workgroup kernel from the start."""
    kw = sl.SHAPES[shape]
    mt = kw.get("model_type")
    if mt == orc.STDSEG:
        return int(prec != EXACT and "trans_share" not in kw)
    return int(mt != orc.STDSEG_NO_DUR)


def run_rung(c, what, ref, shape, prec):
    """one fresh engine on one rung: fb_batch twice.  Returns (gradient, redone) after the checks that hold on every rung:
    no error, the oracle's results within the bound, 0 or 1 redo per call, and a second call that adds exactly the same
    gradient (nothing of a dropped first pass was committed)."""
    eng = c.engine(); b = c.batch(eng)
    assert eng.train_stats() == 0
    numer, zx = eng.fb_batch(b)               # never raises: the oracle succeeds (tests/test_spread_ladder.py)
    g = eng.get_grad()
    redone = eng.train_stats()
    e = deviations(shape, (g, numer, zx), ref)
    t = bounds(shape, prec)
    print("LADDER %s %s: gradient %.2e (%.0e)  Zx %.2e (%.0e)  numerator %.2e (%.0e)" % (what, "redone" if redone else "linear", e[0], t[0], e[1], t[1], e[2], t[2]))
    assert redone in (0, 1), redone
    assert e[0] <= t[0] and e[1] <= t[1] and e[2] <= t[2], (what, e)
    eng.fb_batch(b, want_scalars=False)
    assert eng.train_stats() == 2 * redone
    np.testing.assert_allclose(eng.get_grad(), 2 * g, rtol=1e-12, atol=1e-12 * np.abs(g).max())
    b.close(); eng.close()
    return g, redone


@pytest.mark.parametrize("family", sl.FAMILIES)
@pytest.mark.parametrize("shape,prec", TRAIN, ids=["%s-%s" % (s, NAME[p]) for s, p in TRAIN])
def test_training_across_the_ladder(shape, prec, family):
    """fb_batch on every rung (the full ladder on the FULL_SHAPES under FAST, the reduced one elsewhere) against the oracle.
    On lone_max the engine's own gradient from 600 nats on must not depend on the rung (the oracle's does not: X only
    prices the number of segments) -- a check that needs no oracle."""
    full = prec == FAST and shape in sl.FULL_SHAPES
    at = {}
    for X in sl.rungs(family, full):
        c = sl.case(shape, family, X, precision=prec)
        g, redone = run_rung(c, "%s %s %s %g" % (shape, NAME[prec], family, X), sl.reference(shape, family, X), shape, prec)
        at[X] = g
        if X == 0:
            assert redone == 0
        if X == 1500:
            assert redone == redo_expected_at_1500(shape, prec)
    if family == "lone_max":
        first = min(x for x in at if x >= 600)
        gden = max(1.0, np.abs(at[first]).max()) if shape == "stdseg480" else np.abs(at[first]).max()
        dev = max(np.abs(at[x] - at[first]).max() for x in at if x >= 600) / gden
        print("LADDER %s %s lone_max: the gradient moves by %.2e over the rungs from %g on" % (shape, NAME[prec], dev, first))
        assert dev <= 2 * bounds(shape, prec)[0]


# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def posterior_reference(shape, family, X):
    c = sl.case(shape, family, X)
    return tuple(post_ref.utterance(c, u) for u in range(len(c.Ts)))


@pytest.mark.parametrize("prec", [EXACT, FAST])
@pytest.mark.parametrize("family", sl.FAMILIES)
@pytest.mark.parametrize("shape", fs.POST_SHAPES)
def test_posteriors_across_the_ladder(shape, family, prec):
    """posteriors_batch (frame, end and segment posteriors) on the reduced ladder against tests/post_ref.py, as
    tests/test_gpu_posteriors.py compares them; a redo is counted at most once per call"""
    tol = POST_TOL[prec]
    for X in sl.rungs(family, False):
        c = sl.case(shape, family, X, precision=prec)
        ref = posterior_reference(shape, family, X)
        eng = c.engine(); b = c.batch(eng, with_labels=False)
        labs, _ = eng.viterbi_batch(b)
        out = eng.posteriors_batch(b, segments=labs)
        redone = eng.train_stats()
        dev = 0.0; zdev = 0.0
        for u, T in enumerate(c.Ts):
            g, occ, end, zx = ref[u]
            sp = post_ref.seg_post(g, labs[u], c.L, c.D)
            assert out["frame"][u].shape == (T, c.L) and out["end"][u].shape == (T,) and out["segments"][u].shape == sp.shape
            dev = max(dev, np.abs(out["frame"][u] - occ).max(), np.abs(out["end"][u] - end).max(), np.abs(out["segments"][u] - sp).max(),
                      np.abs(out["frame"][u].sum(1) - 1).max(), abs(out["end"][u][-1] - 1))
            zdev = max(zdev, abs(out["zx"][u] - zx) / max(1, abs(zx)))
        print("LADDER posteriors %s %s %s %g %s: max deviation %.2e (%.0e)  Zx %.2e" % (shape, NAME[prec], family, X, "redone" if redone else "linear", dev, tol, zdev))
        assert redone in (0, 1) and (X != 0 or redone == 0)
        assert dev <= tol and zdev <= max(1e-11, tol * 1e-2)
        b.close(); eng.close()


@pytest.mark.parametrize("family", sl.FAMILIES)
@pytest.mark.parametrize("shape", GROUP_SEG)
def test_node_value_hook_across_the_subnormal_range(shape, family):
    """scrf_forward_backward (getAlpha / getBeta / computeAlphaSum) runs the log-domain wavefront kernel k_dp_wave and
    answers from the workgroup kernel where that one gives up: alpha, beta and Zx against the oracle on the rungs from 705
    to 746 nats, at the bound of tests/test_gpu_errors.py's node-value test."""
    for X in sl.WINDOW:
        c = sl.case(shape, family, X)
        eng = c.engine(); b = c.batch(eng)
        dz = da = db = 0.0
        for u, T in enumerate(c.Ts):
            So, Mo = orc.seg_scores(c.ocfg, c.olay, c.lam, c.windows(u), T)
            rc, ad, al, apt, zx = orc.seg_forward(c.ocfg, So, Mo, T)
            rc2, be, sd = orc.seg_backward(c.ocfg, So, Mo, T)
            assert rc == 0 and rc2 == 0
            gad, gal, gbe, gzx = eng.forward_backward(b, u, T)
            dz = max(dz, abs(gzx - zx) / abs(zx))
            da = max(da, (np.abs(gal - al) / (1e-9 + 1e-11 * np.abs(al))).max())
            db = max(db, (np.abs(gbe - be) / (1e-9 + 1e-11 * np.abs(be))).max())
        print("LADDER hook %s %s %g: Zx %.2e (1e-11)  alpha %.2f  beta %.2f of the bound (rtol 1e-11, atol 1e-9)" % (shape, family, X, dz, da, db))
        assert dz <= 1e-11 and da <= 1.0 and db <= 1.0
        b.close(); eng.close()


@pytest.mark.parametrize("family", sl.FAMILIES)
@pytest.mark.parametrize("shape", ("mixed", "fused"))
def test_training_on_the_log_domain_wavefront_kernel(shape, family, monkeypatch):
    """SCRF_LINDP=0 (read when the engine is created): training runs k_dp_wave instead of the linear-domain recursion"""
    monkeypatch.setenv("SCRF_LINDP", "0")
    for X in sl.WINDOW:
        c = sl.case(shape, family, X, precision=FAST)
        run_rung(c, "%s FAST SCRF_LINDP=0 %s %g" % (shape, family, X), sl.reference(shape, family, X), shape, FAST)


@pytest.mark.parametrize("shape", GROUP)
def test_a_redone_batch_in_chunks_equals_one_chunk(shape):
    """heavy_out at 1500 nats (every chunk's first pass gives up) with a 64 KiB scratch budget against one chunk: numerator
    and Zx to the bit, the gradient to the order of its sums, one redo counted for the call either way"""
    out = []
    for scratch in (0, 1 << 16):
        c = sl.case(shape, "heavy_out", 1500, precision=FAST, scratch_bytes=scratch)
        eng = c.engine(); b = c.batch(eng)
        numer, zx = eng.fb_batch(b)
        assert eng.train_stats() == 1
        out.append((numer.copy(), zx.copy(), eng.get_grad()))
        b.close(); eng.close()
    np.testing.assert_array_equal(out[0][0], out[1][0])
    np.testing.assert_array_equal(out[0][1], out[1][1])
    np.testing.assert_allclose(out[0][2], out[1][2], rtol=1e-12, atol=1e-12 * np.abs(out[0][2]).max())
    e = deviations(shape, (out[1][2], out[1][0], out[1][1]), sl.reference(shape, "heavy_out", 1500))
    assert e[0] <= TOL[FAST][0] and e[1] <= TOL[FAST][1] and e[2] <= TOL[FAST][2], e


@pytest.mark.parametrize("prec", [EXACT, FAST])
def test_a_sparse_map_across_the_ladder(prec):
    """stdsparsetrans on the segmental model (the shape of tests/test_gpu_sparse.py: L = 5, D = 4, 40 indices, 6 pairs per
    window), heavy_out on the reduced ladder: one transition matrix per frame from the sparse score kernels, against
    tests/sparse_ref.py at that module's bound (1e-9 of max(1, |reference|))"""
    L, D, N, P, Ts = 5, 4, 40, 6, [9, 14, 6]
    model = scrf_amd.STDSEG_NO_DUR_NO_SEGTRANSFTR
    rng = np.random.RandomState(sl.SEED)
    lay = sr.SparseLayout(L, sfe=N - 1, tfe=N - 1, use_tf=True)
    Xw = [sr.random_windows(rng, orc.num_segs(T, D), P, N, messy=True) for T in Ts]
    labels = [orc.group_labels(rng.randint(0, L, T).astype(np.uint32), D, L) for T in Ts]
    lam0 = rng.uniform(-0.5, 0.5, lay.lambda_len)
    for X in sl.rungs("heavy_out", False):
        lam = lam0.copy()
        lam[lay.state_idx(0) + lay.nsf - 1] = sl.B
        for n in range(L):
            lam[lay.trans_idx(0, n) + lay.ntf - 1] = -float(X)
        eng = scrf_amd.Engine(scrf_amd.make_config(model_type=model, L=L, D=D, F=2 * P, sfe=N - 1, tfe=N - 1, use_trans_ftrs=True,
                                                   sparse=True, precision=prec))
        assert eng.lambda_len == lay.lambda_len
        eng.set_lambda(lam)
        b = eng.batch_from_windows(Xw, Ts, labels)
        numer, zx = eng.fb_batch(b)
        g = eng.get_grad()
        redone = eng.train_stats()
        rg = np.zeros(lay.lambda_len); rn = []; rz = []
        for u, T in enumerate(Ts):
            gu, nu, zu = sr.gradient(lay, lam, Xw[u], labels[u], T, D, model)
            rg += gu; rn.append(nu); rz.append(zu)
        e = [np.abs(a - r).max() / max(1.0, np.abs(r).max()) for a, r in ((g, rg), (zx, np.array(rz)), (numer, np.array(rn)))]
        print("LADDER sparse %s heavy_out %g %s: gradient %.2e  Zx %.2e  numerator %.2e (1e-9)" % (NAME[prec], X, "redone" if redone else "linear", *e))
        assert redone in (0, 1) and (X != 0 or redone == 0) and (X != 1500 or redone == 1)
        assert max(e) <= 1e-9, e
        b.close(); eng.close()
