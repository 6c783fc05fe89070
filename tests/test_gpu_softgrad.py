"""-m gpu: training from transcripts (scrf_fb_transcript_batch) against the numpy reference
tests/softgrad_ref.py over the CPU oracle's scores and windows.  The gradient is measured relative to its largest component
under gpu_checks.TOL[tier][0] (1e-9 EXACT and FAST, 1e-6 on a FASTLIN handle, 1e-5 FAST32); log_num and zx relative to
max(1, |ref|) under gpu_checks.POST_TOL.  Every weight and every utterance of every call is compared, and each case prints
its largest deviation before it asserts.

Shapes, each the smallest at which one path can go wrong: L = 3, D = 3 with utterances of 1 frame, fewer than D, D and more
frames, as a frames batch (the fused form under the FAST tiers) and as a windows batch (the dense form); the same with
per-frame transition matrices (the XI route); the frame model; D = 10 with utterances shorter and longer than D; L = 70 (the
multi-wavefront recursion on a fusable batch; the hybrid form is the chunked test's L = 66 with a wide stream); K = 67
positions (past one wavefront of the sweep); one sparse-map case."""
import functools

import numpy as np
import pytest

import orc

import row_spread as rsp
import scrf_amd
import softgrad_ref as sg
import sparse_ref as sr
import transcript_ref as tr
from cases import Case
from gpu_checks import EXACT, FAST, FAST32, FASTLIN, NAME, POST_TOL, TOL, bits

pytestmark = pytest.mark.gpu

INVALID = 1
SHAPES = {
    "small": dict(L=3, D=3, in_w=4, Ts=[6, 5, 1, 9]),
    "ctx": dict(L=3, D=3, in_w=4, Ts=[6, 5, 1, 9], trans_ctx=1),
    "frame": dict(L=4, D=1, in_w=3, Ts=[7, 3], frame_model=True),
    "d10": dict(L=7, D=10, in_w=5, Ts=[23, 40, 4]),
    "wide": dict(L=70, D=2, in_w=3, Ts=[12, 9], lam_scale=0.1),
    "longk": dict(L=2, D=2, in_w=2, Ts=[70]),
}
SEED = {n: 700 + i for i, n in enumerate(sorted(SHAPES))}
MODES = (tr.ONE, tr.RUNS)


def case(name, **kw):
    return Case(seed=SEED[name], **dict(SHAPES[name], **kw))


def no_repeat(rng, K, L):
    ph = np.empty(K, dtype=np.int64)
    ph[0] = rng.randint(0, L)
    for i in range(1, K):
        ph[i] = (ph[i - 1] + 1 + rng.randint(0, L - 1)) % L
    return ph.astype(np.uint32)


@functools.lru_cache(maxsize=None)
def transcript_sets(name, mode):
    """((set name, one transcript per utterance), ...): every transcript fits.  random; K = 1 (RUNS: ONE fits K = 1 only
    when T <= D); K = T for the frame model under ONE; K = 67 for the long shape.  The best path's transcript is added by
    the test, from the engine's own decode."""
    c = case(name)
    rng = np.random.RandomState(800 + SEED[name] + 50 * mode)
    L, D = c.L, c.D
    if name == "longk":
        return (("K=67", [no_repeat(rng, 67, L) if mode == tr.RUNS else rng.randint(0, L, 67).astype(np.uint32)]),)
    sets = [("random", [tr.random_transcript(rng, T, L, D, mode) for T in c.Ts])]
    if mode == tr.RUNS:
        sets.append(("K=1", [rng.randint(0, L, 1).astype(np.uint32) for T in c.Ts]))
    elif name == "frame":
        sets.append(("K=T", [rng.randint(0, L, T).astype(np.uint32) for T in c.Ts]))
    return tuple((n, tuple(np.ascontiguousarray(p, dtype=np.uint32) for p in ts)) for n, ts in sets)


@functools.lru_cache(maxsize=None)
def _reference(name, mode, key):
    c = case(name)
    ts = [np.frombuffer(k, dtype=np.uint32) for k in key]
    g, ln, zx = sg.gradient(c, ts, mode)
    for a in (g, ln, zx):
        a.flags.writeable = False
    return g, ln, zx


def reference(name, mode, ts):
    """(gradient, log_num, zx) of a transcript set: computed once, shared, left unchanged"""
    return _reference(name, mode, tuple(np.ascontiguousarray(p, dtype=np.uint32).tobytes() for p in ts))


def path_transcripts(c, eng, b, mode):
    labs, _ = eng.viterbi_batch(b)
    out = []
    for u in range(len(c.Ts)):
        ph = (np.asarray(labs[u], dtype=np.int64) % c.L).astype(np.uint32)
        out.append(tr.collapse(ph).astype(np.uint32) if mode == tr.RUNS else ph)
    return out


def devs(c, ref, g, ln, zx, sums):
    og, oln, ozx = ref
    e_g = np.abs(g - og).max() / np.abs(og).max()
    e_s = max(np.abs(ln - oln).max() / max(1.0, np.abs(oln).max()), np.abs(zx - ozx).max() / max(1.0, np.abs(ozx).max()))
    want = np.array([oln.sum(), ozx.sum(), len(c.Ts)])
    e_b = np.abs(np.asarray(sums)[:3] - want).max() / max(1.0, np.abs(want).max())
    return e_g, e_s, e_b


def run_sets(name, kind, mode, prec, want_form=None):
    c = case(name, precision=prec)
    eng = c.engine()
    b = c.batch(eng, with_labels=False) if kind == "frames" else eng.batch_from_windows([c.windows(u) for u in range(len(c.Ts))], c.Ts)
    form = eng.batch_fused_mode(b)
    if want_form is not None:
        assert form in want_form, (form, want_form)
    sets = list(transcript_sets(name, mode))
    if name != "longk":
        sets.append(("best path", path_transcripts(c, eng, b, mode)))
    worst = (0.0, 0.0, 0.0)
    fails = []
    for sname, ts in sets:
        eng.zero_grad()
        s0 = np.asarray(eng.batch_sums())[:3].copy()
        ln, zx = eng.fb_transcript_batch(b, list(ts), mode)
        g = eng.get_grad()
        sums = np.asarray(eng.batch_sums())[:3] - s0
        d = devs(c, reference(name, mode, ts), g, ln, zx, sums)
        worst = tuple(max(a, b_) for a, b_ in zip(worst, d))
        if not (d[0] <= TOL[prec][0] and d[1] <= POST_TOL[prec] and d[2] <= POST_TOL[prec]):
            fails.append((sname, d))
    assert eng.train_stats() == 0 and eng.soft_stats() == (len(sets), len(sets), 0), (eng.train_stats(), eng.soft_stats())
    b.close(); eng.close()
    print("softgrad %s %s mode %d %s form %d: gradient %.3e (%.0e)  log_num/zx %.3e (%.0e)  batch sums %.3e" %
          (name, kind, mode, NAME[prec], form, worst[0], TOL[prec][0], worst[1], POST_TOL[prec], worst[2]))
    assert not fails, fails


@pytest.mark.parametrize("prec", [EXACT, FAST, FASTLIN, FAST32])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kind", ["frames", "windows"])
@pytest.mark.parametrize("name", ["small", "ctx"])
def test_small_shapes_on_every_tier_and_batch_kind(name, kind, mode, prec):
    # what batch_fused_mode reports for the batch: windows 0 (materialised); a frames batch of either shape is fusable -- 1
    # (under EXACT the training pass then takes the general path over the synthesised windows, under FAST / FAST32 the fused
    # form) and 2 on a FASTLIN handle (the linear-average form, which this pass runs as the FAST form)
    run_sets(name, kind, mode, prec, want_form=(0,) if kind == "windows" else ((2,) if prec == FASTLIN else (1,)))


@pytest.mark.parametrize("prec", [EXACT, FAST])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["frame", "d10", "wide", "longk"])
def test_the_other_shapes(name, mode, prec):
    # L = 70 with a narrow stream is still a fusable batch (1), run by the multi-wavefront recursion; the hybrid form (3) is
    # the chunked test's shape
    run_sets(name, "frames", mode, prec, want_form={"wide": (1,), "frame": (0,), "d10": (1,), "longk": (1,)}[name])


def test_the_fused_form_runs_under_FAST():
    c = case("small", precision=FAST)
    eng = c.engine(); b = c.batch(eng, with_labels=False)
    assert eng.batch_fused_mode(b) == 1
    b.close(); eng.close()


@pytest.mark.parametrize("prec", [EXACT, FAST])
def test_one_alignment_equals_fb_batch_on_that_segmentation(prec):
    """ONE mode with K * D = T: every segment has duration D, the transcript has one alignment, and the gradient is that of
    the batch labelled with exactly that segmentation -- both from the GPU, through different kernels"""
    L, D = 3, 3
    c = Case(L=L, D=D, in_w=4, Ts=[6, 9, 3], seed=31, precision=prec)
    rng = np.random.RandomState(32)
    ts = [rng.randint(0, L, T // D).astype(np.uint32) for T in c.Ts]
    labels = []
    for T, ph in zip(c.Ts, ts):
        lab = np.full(T, 0xffffffff, dtype=np.uint32)
        lab[D - 1::D] = ph + L * (D - 1)
        labels.append(lab)
    c.labels = labels
    eng = c.engine()
    bl = c.batch(eng, with_labels=True); b = c.batch(eng, with_labels=False)
    numer, zx0 = eng.fb_batch(bl)
    g0 = eng.get_grad()
    eng.zero_grad()
    ln, zx = eng.fb_transcript_batch(b, ts, tr.ONE)
    g = eng.get_grad()
    e_g = np.abs(g - g0).max() / np.abs(g0).max()
    e_s = max(np.abs(ln - numer).max() / max(1.0, np.abs(numer).max()), np.abs(zx - zx0).max() / max(1.0, np.abs(zx0).max()))
    print("one alignment %s: gradient %.3e (%.0e)  log_num/zx %.3e (%.0e)" % (NAME[prec], e_g, TOL[prec][0], e_s, POST_TOL[prec]))
    bl.close(); b.close(); eng.close()
    assert e_g <= TOL[prec][0] and e_s <= POST_TOL[prec]


@pytest.mark.parametrize("name", ["small", "ctx"])
def test_accumulation_determinism_and_labels_ignored(name):
    mode = tr.RUNS
    ts = list(transcript_sets(name, mode)[0][1])
    c = case(name, precision=FAST)
    eng = c.engine(); b = c.batch(eng, with_labels=False)
    ln, zx = eng.fb_transcript_batch(b, ts, mode)
    g1, s1 = eng.get_grad(), np.asarray(eng.batch_sums())[:3].copy()
    eng.fb_transcript_batch(b, ts, mode)
    g2, s2 = eng.get_grad(), np.asarray(eng.batch_sums())[:3].copy()
    assert np.array_equal(bits(g2), bits(2.0 * g1)) and np.array_equal(bits(s2), bits(2.0 * s1))
    assert np.allclose(s1, [ln.sum(), zx.sum(), len(c.Ts)], rtol=1e-14, atol=0)   # the device sums in an order of its own
    b.close(); eng.close()
    # a second engine: the same bytes; and a batch that carries labels gives them too
    eng = c.engine(); bl = c.batch(eng, with_labels=True)
    ln2, zx2 = eng.fb_transcript_batch(bl, ts, mode)
    assert np.array_equal(bits(eng.get_grad()), bits(g1)) and np.array_equal(bits(ln2), bits(ln)) and np.array_equal(bits(zx2), bits(zx))
    eng.zero_grad()
    eng.fb_batch(bl)   # the labels are still the batch's
    assert np.abs(eng.get_grad()).max() > 0
    bl.close(); eng.close()


@pytest.mark.parametrize("prec", [EXACT, FAST])
def test_chunked_under_a_small_scratch_budget(prec):
    kw = dict(L=66, D=4, in_w=69, Ts=[9, 14, 3, 1, 11, 8], lam_scale=0.05, seed=41)
    mode = tr.RUNS
    c1 = Case(precision=prec, **kw); cs = Case(precision=prec, scratch_bytes=1 << 18, **kw)
    rng = np.random.RandomState(42)
    ts = [tr.random_transcript(rng, T, c1.L, c1.D, mode) for T in c1.Ts]
    ref = sg.gradient(c1, ts, mode)
    out = []
    for c in (c1, cs):
        eng = c.engine(); b = c.batch(eng, with_labels=False)
        assert eng.batch_fused_mode(b) == (3 if prec == FAST else 0)   # a wide stream and L > 64: the hybrid form under FAST
        ln, zx = eng.fb_transcript_batch(b, ts, mode)
        out.append((eng.get_grad(), ln, zx, eng.soft_stats(), np.asarray(eng.batch_sums())[:3].copy()))
        b.close(); eng.close()
    assert out[0][3] == (1, 1, 0), out[0][3]
    assert out[1][3][0] == 1 and out[1][3][1] >= 3 and out[1][3][2] == 0, out[1][3]
    assert np.array_equal(bits(out[0][1]), bits(out[1][1]))   # log_num does not depend on the chunking
    for g, ln, zx, _, sums in out:
        d = devs(c1, ref, g, ln, zx, sums)
        print("chunked %s (%d chunks): gradient %.3e (%.0e)  log_num/zx %.3e" % (NAME[prec], _[1], d[0], TOL[prec][0], d[1]))
        assert d[0] <= TOL[prec][0] and d[1] <= POST_TOL[prec] and d[2] <= POST_TOL[prec], d


def test_refusals_leave_the_gradient_and_the_sums_alone():
    c = case("small", precision=FAST)
    eng = c.engine(); b = c.batch(eng, with_labels=False)
    good = list(transcript_sets("small", tr.RUNS)[0][1])
    eng.fb_transcript_batch(b, good, tr.RUNS)
    g0, s0 = eng.get_grad(), np.asarray(eng.batch_sums()).copy()
    stats = eng.soft_stats()
    u32 = lambda *v: np.array(v, dtype=np.uint32)
    bad = [("does not fit", tr.ONE, [u32(0), u32(1, 2), u32(0), u32(0, 1, 2)], ("utterance 0", "does not fit")),   # K = 1, T = 6 > D
           ("does not fit", tr.RUNS, [u32(0), u32(1, 2), u32(0, 1), u32(0, 1, 2)], ("utterance 2", "does not fit")),   # K = 2 > T = 1
           ("repeat", tr.RUNS, [u32(0, 1), u32(1, 2, 2), u32(0), u32(0, 1, 2)], ("utterance 1", "position 2")),
           ("q_k = L", tr.RUNS, [u32(0, 1), u32(1, 2), u32(0), u32(0, 3, 2)], ("utterance 3", "position 1")),
           ("mode", 2, good, ("unknown mode",))]
    for what, mode, ts, words in bad:
        with pytest.raises(scrf_amd.ScrfError) as ei:
            eng.fb_transcript_batch(b, ts, mode)
        assert ei.value.code == INVALID, (what, ei.value.code)
        for w in words:
            assert w in str(ei.value), (what, str(ei.value))
        assert np.array_equal(bits(eng.get_grad()), bits(g0)) and np.array_equal(bits(np.asarray(eng.batch_sums())), bits(s0)), what
    assert eng.soft_stats() == stats
    b.close(); eng.close()


def test_a_rung_that_is_redone_in_the_log_domain():
    """tests/row_spread.py at X = 2400 on a FAST handle: the transcript sweep's guard sends the whole pass to the log domain;
    the gradient then meets the EXACT bound, so nothing of the first pass is in it"""
    name, X = "fused3", 2400
    rs = rsp.RowSpread(name, X, precision=FAST)
    tname, mode, ts = rs.transcripts()[0]
    ref = sg.gradient(rs.case, ts, mode)
    eng = rs.engine(); b = rs.batch(eng)
    t0, s0 = eng.train_stats(), eng.soft_stats()
    ln, zx = eng.fb_transcript_batch(b, ts, mode)
    g = eng.get_grad()
    t1, s1 = eng.train_stats(), eng.soft_stats()
    d = devs(rs.case, ref, g, ln, zx, np.asarray(eng.batch_sums())[:3])
    print("redone rung %s X = %g (%s): gradient %.3e (%.0e)  log_num/zx %.3e" % (name, X, tname, d[0], TOL[EXACT][0], d[1]))
    b.close(); eng.close()
    assert t1 == t0 + 1 and s1[2] == s0[2] + 1 and s1[1] == s0[1] + 2, (t0, t1, s0, s1)
    assert d[0] <= TOL[EXACT][0] and d[1] <= POST_TOL[EXACT] and d[2] <= POST_TOL[EXACT], d


@pytest.mark.parametrize("prec", [EXACT, FAST])
@pytest.mark.parametrize("mode", MODES)
def test_a_sparse_map(mode, prec):
    """stdsparsetrans: pair windows over 12 indices, transition features, a windows batch (the sparse kernels' counts)"""
    L, D, N, P, Ts = 3, 2, 12, 3, [5, 3, 1]
    rng = np.random.RandomState(51)
    lay = sr.SparseLayout(L, sfe=N - 1, tfe=N - 1, use_tf=True)
    windows = [sr.random_windows(rng, orc.num_segs(T, D), P, N, sorted_unique=True) for T in Ts]
    lam = rng.uniform(-0.5, 0.5, lay.lambda_len)
    ts = [tr.random_transcript(rng, T, L, D, mode) for T in Ts]
    og, oln, ozx = sg.sparse_gradient(lay, lam, windows, Ts, D, ts, mode)
    cfg = scrf_amd.make_config(model_type=scrf_amd.STDSEG_NO_DUR_NO_SEGTRANSFTR, L=L, D=D, F=2 * P, sfe=N - 1, tfe=N - 1,
                               use_trans_ftrs=True, sparse=True, precision=prec)
    eng = scrf_amd.Engine(cfg)
    eng.set_lambda(lam)
    b = eng.batch_from_windows(windows, Ts)
    ln, zx = eng.fb_transcript_batch(b, ts, mode)
    g = eng.get_grad()
    b.close(); eng.close()
    e_g = np.abs(g - og).max() / np.abs(og).max()
    e_s = max(np.abs(ln - oln).max() / max(1.0, np.abs(oln).max()), np.abs(zx - ozx).max() / max(1.0, np.abs(ozx).max()))
    print("softgrad sparse mode %d %s: gradient %.3e (%.0e)  log_num/zx %.3e (%.0e)" % (mode, NAME[prec], e_g, TOL[prec][0], e_s, POST_TOL[prec]))
    assert e_g <= TOL[prec][0] and e_s <= POST_TOL[prec]
