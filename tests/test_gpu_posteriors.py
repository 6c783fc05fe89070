"""-m gpu: posterior output (scrf_posteriors_batch, scrf_seg_posteriors) against the numpy reference
tests/post_ref.py, which forms everything from the oracle's segment posteriors.

Bounds, absolute on values in [0, 1]: the project's per-tier bounds of tests/test_gpu_parity.py -- 1e-9 for EXACT and FAST,
1e-6 for FASTLIN (its window average is the exact mean, not the reference's float arithmetic), 1e-5 for FAST32.  Row sums
of the frame posteriors and the boundary posterior of the last frame lie within the same bound of 1 (the reference itself
stays within 2e-13).  Every test prints the largest deviation it saw before it asserts."""
import numpy as np
import pytest

import orc
import post_ref
import scrf_amd
from cases import Case
from post_ref import CASES
from spread_ladder import wide_spread_case      # heavy_out at 1500 nats on L = 4, D = 3

pytestmark = pytest.mark.gpu

EXACT, FAST, FAST32, FASTLIN = scrf_amd.PREC_EXACT, scrf_amd.PREC_FAST, scrf_amd.PREC_FAST32, scrf_amd.PREC_FASTLIN
TOL = {EXACT: 1e-9, FAST: 1e-9, FAST32: 1e-5, FASTLIN: 1e-6}
NAME = {EXACT: "EXACT", FAST: "FAST", FAST32: "FAST32", FASTLIN: "FASTLIN"}

# shape lists of tests/test_gpu_parity.py (copied: test modules are not imported)
FUSED_SHAPES = [
    dict(L=3, D=3, in_w=2, Ts=[1, 2, 3, 4, 7]),
    dict(L=50, D=5, in_w=45, Ts=[1, 13, 40, 77]),
    dict(L=7, D=32, in_w=5, Ts=[31, 32, 33, 100]),
    dict(L=48, D=25, in_w=39, Ts=[300, 57]),
]
MIXED_SHAPES = [
    dict(L=6, D=4, in_w=5, Ts=[9, 14, 3, 1], trans_ctx=1),
    dict(L=48, D=10, in_w=8, Ts=[40, 25], trans_ctx=1, lam_scale=0.05),
    dict(L=5, D=3, in_w=90, Ts=[12, 7], trans_ctx=1, lam_scale=0.05),
    dict(L=48, D=10, in_w=144, Ts=[30, 11], trans_ctx=2, lam_scale=0.02),
]
HYBRID_SHAPES = [
    dict(L=65, D=5, in_w=70, Ts=[1, 2, 9, 30], lam_scale=0.05),
    dict(L=130, D=12, in_w=66, Ts=[27, 1, 260], lam_scale=0.05),
    dict(L=200, D=40, in_w=60, Ts=[45, 130], lam_scale=0.05),
    dict(L=96, D=25, in_w=62, Ts=[60, 24], lam_scale=0.05),
    dict(L=70, D=6, in_w=90, Ts=[20, 7], lam_scale=0.05),
    dict(L=66, D=4, in_w=69, Ts=[9, 14, 3, 1, 11, 8], scratch_bytes=1 << 18, lam_scale=0.05),
]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def reference(c):
    return [post_ref.utterance(c, u) for u in range(len(c.Ts))]


def compare(c, eng, b, tol, ref=None, what=""):
    """every output of one call against the reference; returns (outputs, largest deviation)"""
    ref = ref or reference(c)
    labs, _ = eng.viterbi_batch(b)
    out = eng.posteriors_batch(b, segments=labs)
    dev = 0.0
    for u, T in enumerate(c.Ts):
        g, occ, end, zx = ref[u]
        sp = post_ref.seg_post(g, labs[u], c.L, c.D)
        assert out["frame"][u].shape == (T, c.L) and out["end"][u].shape == (T,) and out["segments"][u].shape == sp.shape
        d = max(np.abs(out["frame"][u] - occ).max(), np.abs(out["end"][u] - end).max(), np.abs(out["segments"][u] - sp).max(),
                np.abs(out["frame"][u].sum(1) - 1).max(), abs(out["end"][u][-1] - 1))
        dev = max(dev, d)
        assert abs(out["zx"][u] - zx) <= max(1e-11, tol * 1e-2) * max(1, abs(zx))
        # a segment's posterior cannot exceed the frame posterior of its label on any frame it covers
        for (e, dd, l), p in zip(post_ref.segments_of(labs[u], c.L), out["segments"][u]):
            assert p <= out["frame"][u][e - dd + 1:e + 1, l].min() + tol
    print("posteriors %s: max deviation %.3e (bound %.0e)" % (what, dev, tol))
    assert dev <= tol, dev
    return out, dev


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ci", range(len(CASES)))
def test_seg_posteriors_hook_equals_the_oracle(ci):
    c = Case(seed=100 + ci, **CASES[ci])
    eng = c.engine(); b = c.batch(eng, with_labels=False)
    dev = 0.0
    for u, T in enumerate(c.Ts):
        S, M = orc.seg_scores(c.ocfg, c.olay, c.lam, c.windows(u), T)
        rc, g, xi, zx = orc.seg_posteriors(c.ocfg, S, M, T)
        assert rc == 0
        gg = eng.seg_posteriors(b, u, T)
        dev = max(dev, np.abs(gg - g).max())
    print("seg_posteriors case %d: max deviation %.3e" % (ci, dev))
    assert dev <= 1e-9
    b.close(); eng.close()


CASES_MODE_FAST = [1, None, None, 1, 1, 1]   # batch forms known from the parity tests' own assertions (None: not pinned there)


@pytest.mark.parametrize("prec", [EXACT, FAST, FAST32, FASTLIN])
@pytest.mark.parametrize("ci", range(len(CASES)))
def test_posteriors_on_the_parity_cases(ci, prec):
    c = Case(seed=100 + ci, precision=prec, **CASES[ci])
    eng = c.engine(); b = c.batch(eng, with_labels=False)
    mode = eng.batch_fused_mode(b)
    # (under EXACT the form names the decode kernels only: the recursion runs on materialised windows, in the log domain)
    if prec in (FAST, FAST32) and CASES_MODE_FAST[ci] is not None:
        assert mode == CASES_MODE_FAST[ci]
    compare(c, eng, b, TOL[prec], what="case %d %s form %d" % (ci, NAME[prec], mode))
    assert eng.train_stats() == 0
    b.close(); eng.close()


@pytest.mark.parametrize("prec", [FAST, FAST32, FASTLIN])
@pytest.mark.parametrize("si", range(len(FUSED_SHAPES)))
def test_posteriors_on_the_fused_shapes(si, prec):
    c = Case(seed=300 + si, precision=prec, **FUSED_SHAPES[si])
    eng = c.engine(); b = c.batch(eng, with_labels=False)
    mode = eng.batch_fused_mode(b)
    if prec == FASTLIN:
        assert mode == 2 if si in (0, 3) else mode in (1, 2)   # 0 and 3 are shapes the FASTLIN parity test pins at form 2
    else:
        assert mode == 1
    compare(c, eng, b, TOL[prec], what="fused shape %d %s form %d" % (si, NAME[prec], mode))
    b.close(); eng.close()


@pytest.mark.parametrize("prec", [FAST, FASTLIN])
@pytest.mark.parametrize("si", range(len(MIXED_SHAPES)))
def test_posteriors_on_the_mixed_shapes(si, prec, monkeypatch):
    ref = None
    for mixed in ("1", "0"):
        monkeypatch.setenv("SCRF_FUSE_MIXED", mixed)
        c = Case(seed=830 + si, precision=prec, **MIXED_SHAPES[si])
        ref = ref or reference(c)
        eng = c.engine(); b = c.batch(eng, with_labels=False)
        mode = eng.batch_fused_mode(b)
        assert mode == (0 if mixed == "0" else (2 if prec == FASTLIN else 1))
        compare(c, eng, b, TOL[prec], ref, what="mixed shape %d %s form %d" % (si, NAME[prec], mode))
        b.close(); eng.close()


@pytest.mark.parametrize("si", range(len(HYBRID_SHAPES)))
def test_posteriors_on_the_hybrid_shapes(si, monkeypatch):
    ref = None
    for prec, hy, want in ((FAST, "1", 3), (FASTLIN, "1", 3), (FAST, "0", 0), (EXACT, "1", 0)):
        monkeypatch.setenv("SCRF_HYBRID", hy)
        c = Case(seed=870 + si, precision=prec, **HYBRID_SHAPES[si])
        ref = ref or reference(c)
        eng = c.engine(); b = c.batch(eng, with_labels=False)
        mode = eng.batch_fused_mode(b)
        assert mode == want
        compare(c, eng, b, TOL[prec], ref, what="hybrid shape %d %s form %d" % (si, NAME[prec], mode))
        b.close(); eng.close()


@pytest.mark.parametrize("prec", [EXACT, FAST])
def test_posteriors_of_the_frame_model_are_the_chain_posteriors(prec):
    """D = 1, stdframe: occ is the node posterior exp(alpha + beta - Zx) of CRF_NewLocalPosteriorBuilder::buildFtrSeq, here
    from a plain log-domain chain over the oracle's scores; every frame ends a segment"""
    c = Case(L=6, D=1, in_w=3, Ts=[4, 3, 4, 9, 1], trans_ctx=0, seed=5, frame_model=True, precision=prec)
    eng = c.engine(); b = c.batch(eng, with_labels=False)
    out, _ = compare(c, eng, b, TOL[prec], what="frame model %s" % NAME[prec])
    dev = 0.0
    for u, T in enumerate(c.Ts):
        S, M = orc.seg_scores(c.ocfg, c.olay, c.lam, c.windows(u), T)
        p, z = post_ref.frame_chain(S, M)
        dev = max(dev, np.abs(out["frame"][u] - p).max(), np.abs(out["end"][u] - 1).max())
        assert abs(out["zx"][u] - z) <= 1e-11 * max(1, abs(z))
    print("frame model %s against the chain: %.3e" % (NAME[prec], dev))
    assert dev <= TOL[prec]
    b.close(); eng.close()


@pytest.mark.parametrize("prec", [EXACT, FAST])
def test_posteriors_with_a_sparse_map(prec):
    """stdsparsetrans on the segmental model (built as in tests/test_gpu_sparse.py): the pass starts from S and M, so the
    sparse score kernels serve it unchanged"""
    import sparse_ref as sr
    rng = np.random.RandomState(31)
    L, D, N, P, Ts = 5, 3, 40, 6, [9, 14, 6, 1]
    lay = sr.SparseLayout(L, sfe=N - 1, tfe=N - 1, use_tf=True)
    X = [sr.random_windows(rng, orc.num_segs(T, D), P, N, messy=True) for T in Ts]
    lam = rng.uniform(-0.5, 0.5, lay.lambda_len)
    eng = scrf_amd.Engine(scrf_amd.make_config(model_type=scrf_amd.STDSEG_NO_DUR_NO_SEGTRANSFTR, L=L, D=D, F=2 * P, sfe=N - 1, tfe=N - 1,
                                               use_trans_ftrs=True, sparse=True, precision=prec))
    assert eng.lambda_len == lay.lambda_len
    eng.set_lambda(lam)
    b = eng.batch_from_windows(X, Ts)
    assert eng.batch_fused_mode(b) == 0
    labs, _ = eng.viterbi_batch(b)
    out = eng.posteriors_batch(b, segments=labs)
    ocfg = sr.ocfg(lay, scrf_amd.STDSEG_NO_DUR_NO_SEGTRANSFTR, D)
    dev = 0.0
    for u, T in enumerate(Ts):
        S, M = sr.scores(lay, lam, X[u], T, D)
        rc, g, xi, zx = orc.seg_posteriors(ocfg, S, M, T)
        assert rc == 0
        occ, end = post_ref.occupancy(g, T, D, L)
        dev = max(dev, np.abs(out["frame"][u] - occ).max(), np.abs(out["end"][u] - end).max(),
                  np.abs(out["segments"][u] - post_ref.seg_post(g, labs[u], L, D)).max(),
                  np.abs(out["frame"][u].sum(1) - 1).max(), abs(out["end"][u][-1] - 1))
    print("sparse map %s: max deviation %.3e" % (NAME[prec], dev))
    assert dev <= TOL[prec]
    b.close(); eng.close()


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(L=48, D=25, in_w=39, Ts=[300, 57], precision=FASTLIN),      # few wavefronts: frame segments
                                dict(L=70, D=3, in_w=4, Ts=[1, 2, 5, 9, 14], precision=FAST),      # two 64-output groups
                                dict(L=6, D=5, in_w=4, Ts=[1, 2, 4, 5, 6, 9, 17, 30, 3, 12], precision=FAST),
                                dict(L=5, D=4, in_w=3, Ts=[6, 9, 4], trans_ctx=1, precision=EXACT)])
def test_runs_and_output_selections_are_bit_identical(kw):
    c = Case(seed=41, **kw)
    eng = c.engine(); b = c.batch(eng, with_labels=False)
    labs, _ = eng.viterbi_batch(b)
    a = eng.posteriors_batch(b, segments=labs)
    a2 = eng.posteriors_batch(b, segments=labs)
    for k in ("zx", "frame_flat", "end_flat", "segments_flat"):
        assert np.array_equal(bits(a[k]), bits(a2[k])), k
    f = eng.posteriors_batch(b, frame=True, end=False)
    e = eng.posteriors_batch(b, frame=False, end=True)
    s = eng.posteriors_batch(b, frame=False, end=False, segments=labs)
    assert "end" not in f and "frame" not in e and "frame" not in s and "end" not in s
    assert np.array_equal(bits(f["frame_flat"]), bits(a["frame_flat"]))
    assert np.array_equal(bits(e["end_flat"]), bits(a["end_flat"]))
    assert np.array_equal(bits(s["segments_flat"]), bits(a["segments_flat"]))
    for o in (f, e, s):
        assert np.array_equal(bits(o["zx"]), bits(a["zx"]))
    b.close(); eng.close()


@pytest.mark.parametrize("kw", [dict(L=48, D=25, in_w=39, Ts=[300, 57, 130], precision=FASTLIN),     # the config-2 shape
                                dict(L=70, D=3, in_w=4, Ts=[40, 9, 1, 14], precision=FAST),            # two 64-output groups
                                dict(L=6, D=5, in_w=4, Ts=[90, 21, 4], trans_ctx=1, precision=FAST)])  # per-frame transition matrices
def test_the_walk_in_frame_segments_equals_the_walk_in_one_piece(kw, monkeypatch):
    """a launch of few utterances splits each walk into frame segments; every frame still receives the same terms in the
    same order, so the outputs are bit-identical.  The switch is read by scrf_create (per handle), and
    scrf_posterior_stats says which form a handle's launches took: the two runs below really differ in form, and each is
    also compared with the reference (the one-piece walk over utterances of T >= 4 D is what large batches run)."""
    res = []
    for split in ("1", "0"):
        monkeypatch.setenv("SCRF_POSTOCC_SPLIT", split)
        c = Case(seed=3, **kw)
        eng = c.engine(); b = c.batch(eng, with_labels=False)
        assert eng.posterior_stats() == (0, 0)
        out, _ = compare(c, eng, b, TOL[kw["precision"]], what="walk %s, L %d D %d" % ("in segments" if split == "1" else "in one piece", c.L, c.D))
        n_split, n_whole = eng.posterior_stats()
        assert (n_split > 0 and n_whole == 0) if split == "1" else (n_split == 0 and n_whole > 0), (split, n_split, n_whole)
        res.append(out)
        b.close(); eng.close()
    for k in ("frame_flat", "end_flat", "segments_flat", "zx"):
        assert np.array_equal(bits(res[0][k]), bits(res[1][k])), k


def test_chunking_is_invisible_and_the_log_domain_agrees(monkeypatch):
    """the shape of test_fused_path_chunking_and_log_domain_fallback: several chunks against one within 1e-13, the
    log-domain recursion (SCRF_LINDP=0) against the linear one within 1e-10"""
    kw = dict(L=6, D=5, in_w=4, Ts=[1, 2, 4, 5, 6, 9, 17, 30, 3, 12], seed=41, precision=FAST)
    outs = []
    for extra in (dict(), dict(scratch_bytes=1 << 15)):
        c = Case(**kw, **extra)
        eng = c.engine(); b = c.batch(eng, with_labels=False)
        labs, _ = eng.viterbi_batch(b)
        outs.append(eng.posteriors_batch(b, segments=labs))
        b.close(); eng.close()
    for k in ("frame_flat", "end_flat", "segments_flat", "zx"):
        d = np.abs(outs[0][k] - outs[1][k]).max()
        print("chunks vs one chunk, %s: %.3e" % (k, d))
        np.testing.assert_allclose(outs[0][k], outs[1][k], rtol=1e-13, atol=1e-13)
    monkeypatch.setenv("SCRF_LINDP", "0")
    c = Case(**kw)
    eng = c.engine(); b = c.batch(eng, with_labels=False)
    labs, _ = eng.viterbi_batch(b)
    o3 = eng.posteriors_batch(b, segments=labs)
    assert eng.train_stats() == 0
    for k in ("frame_flat", "end_flat", "segments_flat"):
        d = np.abs(outs[0][k] - o3[k]).max()
        print("log domain vs linear domain, %s: %.3e" % (k, d))
        assert d <= 1e-10
    b.close(); eng.close()


@pytest.mark.parametrize("prec", [EXACT, FAST])
def test_scores_spanning_more_than_700_nats_come_back_from_the_log_domain(prec):
    c = wide_spread_case(prec)
    ref = reference(c)
    eng = c.engine(); b = c.batch(eng, with_labels=False)
    compare(c, eng, b, 1e-9, ref, what="wide spread %s" % NAME[prec])
    assert eng.train_stats() == 1
    compare(c, eng, b, 1e-9, ref, what="wide spread %s, second call" % NAME[prec])
    assert eng.train_stats() == 2
    b.close(); eng.close()


@pytest.mark.parametrize("prec", [EXACT, FASTLIN])
def test_a_posterior_call_leaves_the_training_state_alone(prec):
    c = Case(L=6, D=4, in_w=5, Ts=[9, 14, 3], seed=7, precision=prec)
    eng = c.engine()
    b = c.batch(eng); bp = c.batch(eng, with_labels=False)
    eng.zero_grad()
    eng.fb_batch(b)
    g0, s0, l0 = eng.get_grad(), eng.batch_sums(), eng.get_lambda()
    eng.posteriors_batch(bp)
    eng.posteriors_batch(b)      # labels, if present, are ignored
    assert np.array_equal(bits(eng.get_grad()), bits(g0)) and np.array_equal(bits(eng.batch_sums()), bits(s0))
    assert np.array_equal(bits(eng.get_lambda()), bits(l0))
    eng.zero_grad()
    eng.fb_batch(b)
    assert np.array_equal(bits(eng.get_grad()), bits(g0))
    b.close(); bp.close(); eng.close()


def test_bad_queries_are_refused():
    c = Case(L=3, D=3, in_w=2, Ts=[4, 7], seed=100, precision=FAST)
    eng = c.engine(); b = c.batch(eng, with_labels=False)
    good = [np.array([0 + 3 * 1, 2 + 3 * 1], dtype=np.uint32), np.array([1 + 3 * 2, 0, 2 + 3 * 2], dtype=np.uint32)]
    eng.posteriors_batch(b, segments=good)
    for bad in ([good[0], np.array([1 + 3 * 2, 0, 2 + 3 * 2, 0], dtype=np.uint32)],       # runs past the utterance's 7 frames
                [np.array([0 + 3 * 3], dtype=np.uint32), good[1]],                          # duration 4 > D: label out of range
                [good[0], np.array([9], dtype=np.uint32)]):                                 # label value L * D
        with pytest.raises(scrf_amd.ScrfError) as ei:
            eng.posteriors_batch(b, segments=bad)
        assert ei.value.code == 1
    eng.posteriors_batch(b, segments=good)    # nothing is sticky
    with pytest.raises(ValueError):
        eng.posteriors_batch(b, segments=good[:1])     # one entry per utterance
    b.close(); eng.close()


@pytest.mark.parametrize("kw,name", [(dict(model_type=orc.STDSEG), "stdseg"), (dict(model_type=orc.STDSEG_NO_DUR, trans_share=(0, 9)), "stdseg_no_dur"),
                                     (dict(num_states=2), "stdseg_no_dur_no_segtransftr")])
def test_models_outside_the_posterior_pass_are_refused_by_name(kw, name):
    c = Case(L=4, D=3, in_w=3, Ts=[6, 5], seed=2, **kw)
    eng = c.engine(); b = c.batch(eng, with_labels=False)
    for call in (lambda: eng.posteriors_batch(b), lambda: eng.seg_posteriors(b, 0, c.Ts[0])):
        with pytest.raises(scrf_amd.ScrfError) as ei:
            call()
        assert ei.value.code == 1 and '"%s"' % name in str(ei.value)
    if "num_states" in kw:
        assert "crf_states" in str(ei.value)
    b.close(); eng.close()
