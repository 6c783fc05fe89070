"""-m gpu: transcript scoring (scrf_transcript_batch) against the numpy reference tests/transcript_ref.py (form
1, the recursion) over the CPU oracle's scores.  The bounds are those of the posterior output per precision
tier: absolute on posteriors, row sums and end_post[T-1], relative to max(1, |ref|) on log_num and zx.  Every utterance and
every value of every call is compared.  (There is no T = 0 utterance among the cases: scrf_batch_create refuses an utterance
without frames, so a batch cannot hold one.)"""
import functools

import numpy as np
import pytest

import latprune_ref as lr
import orc
import post_ref
import scrf_amd
import sparse_ref as sr
import transcript_ref as tr
from cases import Case
from gpu_checks import all_devs
from scrf_amd import PREC_EXACT as EXACT, PREC_FAST as FAST, PREC_FAST32 as FAST32, PREC_FASTLIN as FASTLIN
from spread_ladder import wide_spread_case

pytestmark = pytest.mark.gpu

TOL = {EXACT: 1e-9, FAST: 1e-9, FAST32: 1e-5, FASTLIN: 1e-6}
NAME = {EXACT: "EXACT", FAST: "FAST", FAST32: "FAST32", FASTLIN: "FASTLIN"}
# the shapes of the lattice beam (T = 1, T < D, T = D, ring wrap at D = 10, per-frame M, the frame model (with one M: last), L = 70 / 66 > 64:
# the label reduce spans more than one wavefront of threads) and two of tests/test_gpu_align.py: K = 65 / 67 / 131 (the stride
# over k passes one wavefront) and K = 1030 (it passes 1024 threads)
SHAPES = lr.GPU_SHAPES[:6] + [
    dict(L=3, D=3, in_w=2, Ts=[66, 70, 131]),
    dict(L=2, D=2, in_w=2, Ts=[1100]),
] + lr.GPU_SHAPES[6:]   # what the beam's table gained later follows, so that no shape changes its index
LONG_K = {6: [65, 67, 131], 7: [1030]}
CHUNKED = 5   # L = 66: also runs under scratch_bytes = 1 << 18
MODES = (scrf_amd.ALIGN_ONE, scrf_amd.ALIGN_RUNS)
INVALID = 1


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def case(si, **kw):
    return Case(seed=600 + si, **dict(SHAPES[si], **kw))


def free_zx(c, u, w):
    if w.frame_model:
        return post_ref.frame_chain(w.S.reshape(w.T, w.L), np.broadcast_to(w.M.reshape(-1, w.L * w.L), (w.T, w.L * w.L)))[1]
    S, M = orc.seg_scores(c.ocfg, c.olay, c.lam, c.windows(u), w.T)
    rc, g, xi, zx = orc.seg_posteriors(c.ocfg, S, M, w.T)
    assert rc == 0
    return float(zx)


@functools.lru_cache(maxsize=None)
def reference(si):
    """per utterance (the oracle's fp64 scores, the free Zx); computed once per shape and not modified"""
    c = case(si)
    out = []
    for u in range(len(c.Ts)):
        w = tr.case_scores(c, u)
        w.S.flags.writeable = False; w.M.flags.writeable = False
        out.append((w, free_zx(c, u, w)))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def _ref_dp(si, u, mode, ph_bytes):
    return tr.dp(reference(si)[u][0], np.frombuffer(ph_bytes, dtype=np.uint32), mode)


def ref_dp(si, u, mode, ph):
    return _ref_dp(si, u, mode, np.ascontiguousarray(ph, dtype=np.uint32).tobytes())


def no_repeat(rng, K, L):
    """K random phones without equal neighbours"""
    ph = np.empty(K, dtype=np.int64)
    ph[0] = rng.randint(0, L)
    for i in range(1, K):
        ph[i] = (ph[i - 1] + 1 + rng.randint(0, L - 1)) % L
    return ph.astype(np.uint32)


def transcript_sets(si, mode):
    """named transcript sets (one transcript per utterance): seeded random admissible ones (ONE keeps a forced repeat, RUNS is
    free of equal neighbours), K = 1, K = T (all d = 1), K * D = T where D divides T (its ceiling elsewhere)"""
    c = case(si)
    rng = np.random.RandomState(900 + si + 50 * mode)
    L, D = c.L, c.D
    rand = []
    for u, T in enumerate(c.Ts):
        if si in LONG_K:
            K = LONG_K[si][u]
            if mode == tr.RUNS:
                ph = no_repeat(rng, K, L)
            else:
                ph = rng.randint(0, L, K).astype(np.uint32)
                i = int(rng.randint(0, K - 1))
                ph[i + 1] = ph[i]
        else:
            ph = tr.random_transcript(rng, T, L, D, mode)
        rand.append(ph)
    if mode == tr.ONE:
        assert any((p[1:] == p[:-1]).any() for p in rand if len(p) > 1)
    mk = (lambda K: no_repeat(rng, K, L)) if mode == tr.RUNS else (lambda K: rng.randint(0, L, K).astype(np.uint32))
    return [("random", rand), ("K=1", [mk(1) for T in c.Ts]), ("K=T", [mk(T) for T in c.Ts]),
            ("K*D=T", [mk((T + D - 1) // D) for T in c.Ts])]


def viterbi_transcript(eng, b, L, mode):
    labs, _ = eng.viterbi_batch(b)
    per_seg = [(np.asarray(l, dtype=np.int64) % L).astype(np.uint32) for l in labs]
    return per_seg if mode == tr.ONE else [tr.collapse(p).astype(np.uint32) for p in per_seg]


def check_against_reference(si, eng, b, transcripts, mode, tol, with_queries=True, what=""):
    """one transcript call (queries: the segments align_batch finds for the same transcripts) against form 1; returns (the
    engine's output, the largest deviation)"""
    ref = reference(si)
    segs = cost = None
    if with_queries:
        segs, cost = eng.align_batch(b, transcripts, mode)
    out = eng.transcript_batch(b, transcripts, mode, segments=segs)
    dev = 0.0
    for u, (w, zx) in enumerate(ref):
        r = ref_dp(si, u, mode, transcripts[u])
        T, K = w.T, len(transcripts[u])
        fits = tr.feasible(T, K, w.D, mode)
        d_zx = abs(out["zx"][u] - zx) / max(1.0, abs(zx))
        if not fits:
            assert r.A == -np.inf and out["log_num"][u] == -np.inf and out["logp"][u] == -np.inf, (what, u, out["log_num"][u])
            assert not out["frame"][u].any() and not out["end"][u].any(), (what, u)
            if with_queries:
                assert len(out["segments"][u]) == 0 and np.isinf(cost[u])
            devs = [d_zx]
        else:
            devs = [d_zx, abs(out["log_num"][u] - r.A) / max(1.0, abs(r.A)),
                    np.abs(out["frame"][u] - r.frame_post).max(), np.abs(out["end"][u] - r.end_post).max(),
                    np.abs(out["frame"][u].sum(axis=1) - 1.0).max(), abs(out["end"][u][T - 1] - 1.0)]
            assert out["logp"][u] <= tol * max(1.0, abs(zx)), (what, u, out["logp"][u])
            if with_queries:
                labs = [int(x) for x in segs[u]]
                want = r.queries(labs)
                devs.append(np.abs(out["segments"][u] - want).max())
                ends = np.cumsum([l // w.L + 1 for l in labs]) - 1
                # a queried segment is one of those that end at its frame
                assert (out["segments"][u] <= out["end"][u][ends] + tol).all(), (what, u)
                # the path the aligner found is one term of the sum.  Its cost is a float32 sum of float32-rounded weights, so
                # the margin below is a sanity margin and not a bound on anything
                assert out["log_num"][u] >= -np.float64(cost[u]) - 1e-5 * abs(np.float64(cost[u])), (what, u, out["log_num"][u], cost[u])
        for d in devs:
            assert d <= tol, (what, "utterance %d, K = %d" % (u, K), devs)
        dev = max(dev, max(devs))
    return out, dev


@pytest.mark.parametrize("prec", [EXACT, FAST])
@pytest.mark.parametrize("si", range(len(SHAPES)))
def test_every_output_equals_the_reference(si, prec):
    c = case(si, precision=prec)
    eng = c.engine(); b = c.batch(eng, with_labels=False)
    dev, n = 0.0, 0
    for mode in MODES:
        sets = transcript_sets(si, mode) + [("viterbi", viterbi_transcript(eng, b, c.L, mode))]
        for name, ts in sets:
            _, d = check_against_reference(si, eng, b, ts, mode, TOL[prec], what="shape %d %s mode %d %s" % (si, NAME[prec], mode, name))
            dev = max(dev, d); n += 1
    print("shape %d %s: max deviation %.3e over %d calls" % (si, NAME[prec], dev, n))
    calls, chunks, redone = eng.transcript_stats()
    assert calls == n and chunks == n and redone == 0   # the default budget: one chunk per call
    b.close(); eng.close()


@pytest.mark.parametrize("prec", [FASTLIN, FAST32])
@pytest.mark.parametrize("si", range(len(SHAPES)))
def test_the_other_tiers(si, prec):
    """every shape and every transcript set of the EXACT / FAST sweep above, at the tier's bound"""
    c = case(si, precision=prec)
    eng = c.engine(); b = c.batch(eng, with_labels=False)
    dev = 0.0
    for mode in MODES:
        for name, ts in transcript_sets(si, mode) + [("viterbi", viterbi_transcript(eng, b, c.L, mode))]:
            _, d = check_against_reference(si, eng, b, ts, mode, TOL[prec], what="shape %d %s mode %d %s" % (si, NAME[prec], mode, name))
            dev = max(dev, d)
    print("shape %d %s: max deviation %.3e" % (si, NAME[prec], dev))
    b.close(); eng.close()


def _code(fn):
    with pytest.raises(scrf_amd.ScrfError) as e:
        fn()
    return e.value.code, str(e.value)


@pytest.mark.parametrize("prec", [EXACT, FAST])
def test_transcripts_that_do_not_fit_leave_the_others_alone(prec):
    si = 3   # L = 7, D = 10, Ts = [9, 10, 11, 30]
    c = case(si, precision=prec)
    eng = c.engine(); b = c.batch(eng, with_labels=False)
    rng = np.random.RandomState(5)
    for mode in MODES:
        good = transcript_sets(si, mode)[0][1]
        full, _ = check_against_reference(si, eng, b, good, mode, TOL[prec], what="all fit")
        # K > T, K = 0, K * D = 20 < T = 30 (does not fit ONE, fits RUNS)
        mixed = [good[0], no_repeat(rng, 11, c.L), np.zeros(0, dtype=np.uint32), no_repeat(rng, 2, c.L)]
        out, _ = check_against_reference(si, eng, b, mixed, mode, TOL[prec], what="mixed")
        for k in ("frame", "end", "segments"):
            assert np.array_equal(bits(out[k][0]), bits(full[k][0])), k   # the one that fits is unchanged
        assert np.array_equal(bits(out["log_num"][:1]), bits(full["log_num"][:1])) and np.array_equal(bits(out["zx"]), bits(full["zx"]))
        assert out["log_num"][1] == -np.inf and out["log_num"][2] == -np.inf
        assert np.isinf(out["log_num"][3]) == (mode == scrf_amd.ALIGN_ONE)
    b.close(); eng.close()


def test_arguments_that_are_refused():
    si = 3
    c = case(si, precision=FAST)
    eng = c.engine(); b = c.batch(eng, with_labels=False)
    good = transcript_sets(si, tr.RUNS)[0][1]
    bad = [p.copy() for p in good]
    bad[2][-1] = c.L
    code, msg = _code(lambda: eng.transcript_batch(b, bad, scrf_amd.ALIGN_RUNS))
    assert code == INVALID and "utterance 2" in msg and "phone %d" % c.L in msg, msg
    code, msg = _code(lambda: eng.transcript_batch(b, good, 7))
    assert code == INVALID and "mode" in msg, msg
    rep = [p.copy() for p in good]
    rep[1] = np.array([3, 4, 4, 2], dtype=np.uint32)
    code, msg = _code(lambda: eng.transcript_batch(b, rep, scrf_amd.ALIGN_RUNS))
    assert code == INVALID and "utterance 1" in msg and "position 2" in msg and "SCRF_ALIGN_RUNS" in msg, msg
    segs, _ = eng.align_batch(b, good, scrf_amd.ALIGN_RUNS)
    past = [np.asarray(s, dtype=np.uint32) for s in segs]
    past[0] = np.concatenate([past[0], past[0][-1:]])   # one segment more than the utterance has frames for
    code, msg = _code(lambda: eng.transcript_batch(b, good, scrf_amd.ALIGN_RUNS, segments=past))
    assert code == INVALID and "utterance 0" in msg and "past the utterance" in msg, msg
    past[0] = np.array([c.L * c.D], dtype=np.uint32)
    code, msg = _code(lambda: eng.transcript_batch(b, good, scrf_amd.ALIGN_RUNS, segments=past))
    assert code == INVALID and "out of range" in msg, msg
    # nothing was launched for the refused calls, and the engine still answers; ONE takes the repeat
    assert eng.transcript_stats() == (0, 0, 0)
    check_against_reference(si, eng, b, good, scrf_amd.ALIGN_RUNS, TOL[FAST])
    out = eng.transcript_batch(b, rep, scrf_amd.ALIGN_ONE)
    assert np.isfinite(out["log_num"][1])
    b.close(); eng.close()


@pytest.mark.parametrize("kw,name", [(dict(model_type=orc.STDSEG), "stdseg"), (dict(model_type=orc.STDSEG_NO_DUR, trans_share=(0, 9)), "stdseg_no_dur"),
                                     (dict(num_states=3), "stdseg_no_dur_no_segtransftr")])
def test_models_transcript_scoring_is_not_built_for_are_refused_by_name(kw, name):
    c = Case(L=6, D=3, in_w=3, Ts=[6, 5], seed=2, **kw)
    eng = c.engine(); b = c.batch(eng, with_labels=False)
    code, msg = _code(lambda: eng.transcript_batch(b, [np.array([0, 1], dtype=np.uint32)] * 2))
    assert code == INVALID and "scrf_transcript_batch" in msg and '"%s"' % name in msg, msg
    if "num_states" in kw:
        assert "crf_states = 3" in msg
    b.close(); eng.close()


@pytest.mark.parametrize("prec", [EXACT, FAST])
def test_chunked_runs_equal_the_one_chunk_run_and_repeat_bit_for_bit(prec):
    si = CHUNKED
    c1 = case(si, precision=prec); cn = case(si, precision=prec, scratch_bytes=1 << 18)
    e1 = c1.engine(); b1 = c1.batch(e1, with_labels=False)
    en = cn.engine(); bn = cn.batch(en, with_labels=False)
    keys = ("log_num", "zx", "logp", "frame_flat", "end_flat")
    for mode in MODES:
        ts = transcript_sets(si, mode)[0][1]
        o1, _ = check_against_reference(si, e1, b1, ts, mode, TOL[prec], what="one chunk")
        calls0, chunks0, _ = en.transcript_stats()
        on, _ = check_against_reference(si, en, bn, ts, mode, TOL[prec], what="chunked")
        calls, chunks, redone = en.transcript_stats()
        assert calls == calls0 + 1 and chunks - chunks0 > 1 and redone == 0   # the small budget really splits the batch
        o2 = en.transcript_batch(bn, ts, mode, segments=en.align_batch(bn, ts, mode)[0])   # a second call on one engine
        o3 = en.transcript_batch(bn, ts, mode)                                              # ... and one without queries
        for k in keys + ("segments_flat",):
            assert np.array_equal(bits(on[k]), bits(o1[k])), (mode, k)
            assert np.array_equal(bits(o2[k]), bits(on[k])), (mode, k)
        for k in keys:
            assert np.array_equal(bits(o3[k]), bits(on[k])), (mode, k)
    assert e1.transcript_stats() == (2, 2, 0)
    b1.close(); e1.close(); bn.close(); en.close()


def test_a_transcript_the_linear_domain_loses_comes_back_from_the_log_domain():
    """the wide-spread case of tests/test_gpu_posteriors.py: label 0 at +1000, its transitions at -1500.  A transcript made of
    the disfavoured labels lies ~1000 nats under every row maximum: on the linear-domain scores each of its segments reads
    as exp(.) = 0.  An input the code must handle -- the call is redone in the log domain."""
    c = wide_spread_case(FAST)
    eng = c.engine(); b = c.batch(eng, with_labels=False)
    ts = [np.array([1, 2, 3], dtype=np.uint32), np.array([3, 1, 2, 1], dtype=np.uint32), np.array([2, 3], dtype=np.uint32)]
    for mode in MODES:
        redone0 = eng.transcript_stats()[2]
        segs, _ = eng.align_batch(b, ts, mode)
        out = eng.transcript_batch(b, ts, mode, segments=segs)
        assert eng.transcript_stats()[2] == redone0 + 1
        for u, T in enumerate(c.Ts):
            w = tr.case_scores(c, u)
            r = tr.dp(w, ts[u], mode)
            assert np.isfinite(r.A) and out["logp"][u] < -708.0   # every segment of the transcript underflows beside label 0
            zx = post_ref.utterance(c, u)[3]   # the oracle's log-domain recursion
            devs = all_devs(out, u, r, zx, [int(x) for x in segs[u]])
            assert max(devs) <= 1e-9, (mode, u, devs)
    b.close(); eng.close()


def test_a_sparse_map_and_a_batch_of_materialised_windows():
    rng = np.random.RandomState(31)
    L, D, N, P, Ts = 5, 3, 40, 6, [9, 14, 6, 1]
    lay = sr.SparseLayout(L, sfe=N - 1, tfe=N - 1, use_tf=True)
    X = [sr.random_windows(rng, orc.num_segs(T, D), P, N, messy=True) for T in Ts]
    lam = rng.uniform(-0.5, 0.5, lay.lambda_len)
    eng = scrf_amd.Engine(scrf_amd.make_config(model_type=scrf_amd.STDSEG_NO_DUR_NO_SEGTRANSFTR, L=L, D=D, F=2 * P, sfe=N - 1, tfe=N - 1,
                                               use_trans_ftrs=True, sparse=True, precision=FAST))
    eng.set_lambda(lam)
    b = eng.batch_from_windows(X, Ts)
    ocfg = sr.ocfg(lay, scrf_amd.STDSEG_NO_DUR_NO_SEGTRANSFTR, D)
    for mode in MODES:
        ts = [tr.random_transcript(rng, T, L, D, mode) for T in Ts]
        segs, _ = eng.align_batch(b, ts, mode)
        out = eng.transcript_batch(b, ts, mode, segments=segs)
        for u, T in enumerate(Ts):
            S, M = sr.scores(lay, lam, X[u], T, D)
            r = tr.dp(tr.Scores(S, M, T, L, D), ts[u], mode)
            rc, _, _, zx = orc.seg_posteriors(ocfg, S, M, T)
            assert rc == 0
            devs = all_devs(out, u, r, float(zx), [int(x) for x in segs[u]])
            assert max(devs) <= TOL[FAST], (mode, u, devs)
    b.close(); eng.close()
    si = 1   # dense, per-frame M: the same utterances given as window vectors
    c = case(si, precision=FAST)
    eng = c.engine()
    b = eng.batch_from_windows([c.windows(u) for u in range(len(c.Ts))], c.Ts)
    for mode in MODES:
        check_against_reference(si, eng, b, transcript_sets(si, mode)[0][1], mode, TOL[FAST], what="windows")
    b.close(); eng.close()
