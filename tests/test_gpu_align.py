"""-m gpu: batched forced alignment (scrf_align_batch) against the numpy reference tests/align_ref.py over the
CPU oracle's scores.  The rule fixes every bit (float32 min-plus over monotone left-to-right sums, a fixed tie rule), so
labels and costs are compared as raw bits: no tolerance, no excluded case."""
import functools

import numpy as np
import pytest

import align_ref as ar
import latprune_ref as lr
import orc
import scrf_amd
import sparse_ref as sr
from cases import Case

pytestmark = pytest.mark.gpu

# the shapes of the lattice beam (T = 1, T < D, T = D, ring wrap, per-frame M, the frame model with per-frame M and, last, with
# a single M, L > 64) and two for the
# workgroup kernel: transcripts of 65 .. 131 phones, and 1030 phones (the stride over k passes 1024 threads)
SHAPES = lr.GPU_SHAPES[:6] + [
    dict(L=3, D=3, in_w=2, Ts=[66, 70, 131]),
    dict(L=2, D=2, in_w=2, Ts=[1100]),
] + lr.GPU_SHAPES[6:]   # what the beam's table gained later follows, so that no shape changes its index
LONG_K = {6: [65, 67, 131], 7: [1030]}
CHUNKED = 5   # L = 66: also runs under scratch_bytes = 1 << 18
MODES = (scrf_amd.ALIGN_ONE, scrf_amd.ALIGN_RUNS)
INVALID = 1


def bits(x):
    return np.float32(x).tobytes()


def case(si, **kw):
    return Case(seed=600 + si, **dict(SHAPES[si], **kw))


@functools.lru_cache(maxsize=None)
def reference(si):
    """per utterance the oracle's float arc weights (ar.Weights); computed once per shape and not modified"""
    c = case(si)
    return tuple(ar.case_weights(c, u) for u in range(len(c.Ts)))


def seeded_transcripts(si):
    """per utterance the phones of a random admissible segmentation (adjacent equal phones occur)"""
    c = case(si)
    rng = np.random.RandomState(900 + si)
    out = []
    for u, T in enumerate(c.Ts):
        if si in LONG_K:
            ph = rng.randint(0, c.L, LONG_K[si][u]).astype(np.uint32)
            i = int(rng.randint(0, len(ph) - 1))
            ph[i + 1] = ph[i]
        else:
            ph = ar.random_transcript(rng, T, c.L, c.D)
        out.append(ph)
    assert any((p[1:] == p[:-1]).any() for p in out if len(p) > 1)
    return out


def viterbi_transcripts(eng, b, L):
    """(per-segment phones, collapsed phones) of the engine's own best paths, and the paths and costs themselves"""
    labs, cost = eng.viterbi_batch(b)
    per_seg = [(np.asarray(l, dtype=np.int64) % L).astype(np.uint32) for l in labs]
    return per_seg, [ar.collapse(p).astype(np.uint32) for p in per_seg], [list(l) for l in labs], cost.copy()


class ArcTable:
    """weights of an engine lattice (Engine.lattice_arcs) by (src, dst)"""

    def __init__(self, eng, b, u, T, L, frame_model):
        arcs, self.ns, self.fin = eng.lattice_arcs(b, u)
        key = arcs["src"].astype(np.int64) * self.ns + arcs["dst"]
        self.order = np.argsort(key)
        self.key, self.w = key[self.order], arcs["w"][self.order]
        self.T, self.L, self.frame_model = T, L, frame_model

    def weight(self, s, d):
        i = int(np.searchsorted(self.key, s * self.ns + d))
        assert self.key[i] == s * self.ns + d
        return np.float32(self.w[i])

    def end_state(self, t, lab):
        if self.frame_model:
            return 1 + t * self.L + lab
        return 1 + lab if t == 0 else 1 + self.L + (t - 1) * 2 * self.L + self.L + lab

    def path_cost(self, labels):
        """left-to-right float32 sum of the path's arc weights, the final arc and the final weight"""
        L = self.L
        c = np.float32(0.0)
        t, prev = -1, None
        for lab in labels:
            ph, d = int(lab) % L, int(lab) // L + 1
            ts, t = t + 1, t + d
            if self.frame_model:
                c = c + self.weight(0 if prev is None else self.end_state(t - 1, prev), self.end_state(t, ph))
            else:
                src = 0
                if prev is not None:
                    src = 1 + L + (ts - 1) * 2 * L + ph   # boundary state (ts, ph)
                    c = c + self.weight(self.end_state(ts - 1, prev), src)
                c = c + self.weight(src, self.end_state(t, ph))
            prev = ph
        assert t == self.T - 1
        c = c + self.weight(self.end_state(t, prev), self.fin)
        return np.float32(c + np.float32(0.0))


def check_against_reference(si, eng, b, transcripts, mode, tables=None):
    """one align call against form 1: labels and cost of every utterance bit for bit, the path tiles [0, T) and realises the
    transcript, and (with tables) its weights on the engine's lattice sum to the cost; returns (labels, costs)"""
    ref = reference(si)
    labs, cost = eng.align_batch(b, transcripts, mode)
    assert len(labs) == len(ref)
    for u, w in enumerate(ref):
        want_l, want_c = ar.dp(w, transcripts[u], mode)
        got = [int(x) for x in labs[u]]
        assert bits(cost[u]) == bits(want_c), (si, u, mode, cost[u], want_c)
        assert got == want_l, (si, u, mode, got, want_l)
        if ar.feasible(w.T, len(transcripts[u]), w.D, mode):
            assert sum(l // w.L + 1 for l in got) == w.T and all(l < w.L * w.D for l in got)
            assert ar.matches(got, w.L, transcripts[u], mode)
            if tables is not None:
                assert bits(tables[u].path_cost(got)) == bits(cost[u]), (si, u, mode)
        else:
            assert got == [] and np.isinf(cost[u]) and cost[u] > 0
    return [list(map(int, l)) for l in labs], cost.copy()


@pytest.mark.parametrize("si", range(len(SHAPES)))
def test_labels_and_costs_equal_the_reference_bit_for_bit(si):
    c = case(si)
    eng = c.engine(); b = c.batch(eng, with_labels=False)
    frame_model = c.ocfg.model_type == orc.STDFRAME
    tables = [ArcTable(eng, b, u, T, c.L, frame_model) for u, T in enumerate(c.Ts)]
    per_seg, collapsed, _, _ = viterbi_transcripts(eng, b, c.L)
    for tr in (seeded_transcripts(si), per_seg, collapsed):
        for mode in MODES:
            check_against_reference(si, eng, b, tr, mode, tables)
    calls, chunks, n_wave, n_group = eng.align_stats()
    assert calls == 6 and chunks == 6 and n_wave + n_group == 6   # the default budget: one chunk per call
    if si in LONG_K:
        assert n_group >= 2
    b.close(); eng.close()


@pytest.mark.parametrize("si", range(len(SHAPES)))
def test_aligning_the_viterbi_path_returns_it(si):
    c = case(si)
    eng = c.engine(); b = c.batch(eng, with_labels=False)
    per_seg, collapsed, vlabs, vcost = viterbi_transcripts(eng, b, c.L)
    for tr, mode in ((collapsed, scrf_amd.ALIGN_RUNS), (per_seg, scrf_amd.ALIGN_ONE)):
        labs, cost = eng.align_batch(b, tr, mode)
        assert cost.tobytes() == vcost.tobytes(), (mode, cost, vcost)
        for u in range(len(c.Ts)):
            # equal costs with other labels would be a tie between two paths: shown, not silenced
            assert [int(x) for x in labs[u]] == vlabs[u], "tie? mode %d utterance %d: aligned %s, viterbi %s, cost %r" % (
                mode, u, list(labs[u]), vlabs[u], cost[u])
    b.close(); eng.close()


def _code(fn):
    with pytest.raises(scrf_amd.ScrfError) as e:
        fn()
    return e.value.code, str(e.value)


def test_transcripts_that_do_not_fit_and_arguments_that_are_refused():
    si = 3   # L = 7, D = 10, Ts = [9, 10, 11, 30]
    c = case(si)
    eng = c.engine(); b = c.batch(eng, with_labels=False)
    good = seeded_transcripts(si)
    rng = np.random.RandomState(5)
    mixed = [good[0], rng.randint(0, c.L, 11).astype(np.uint32), np.zeros(0, dtype=np.uint32), rng.randint(0, c.L, 2).astype(np.uint32)]
    for mode in MODES:
        full_l, full_c = check_against_reference(si, eng, b, good, mode)
        labs, cost = check_against_reference(si, eng, b, mixed, mode)
        assert labs[0] == full_l[0] and bits(cost[0]) == bits(full_c[0])   # the feasible one is unchanged
        assert labs[1] == [] and labs[2] == [] and np.isinf(cost[1]) and np.isinf(cost[2])   # K > T, K = 0
        if mode == scrf_amd.ALIGN_ONE:
            assert labs[3] == [] and np.isinf(cost[3])   # K * D = 20 < T = 30
        else:
            assert len(labs[3]) >= 3 and np.isfinite(cost[3])
    bad = [p.copy() for p in good]
    bad[2][-1] = c.L
    code, msg = _code(lambda: eng.align_batch(b, bad, scrf_amd.ALIGN_RUNS))
    assert code == INVALID and "utterance 2" in msg
    code, msg = _code(lambda: eng.align_batch(b, good, 7))
    assert code == INVALID and "mode" in msg
    # nothing was launched for the refused calls, and the engine still answers
    assert eng.align_stats()[0] == 4
    check_against_reference(si, eng, b, good, scrf_amd.ALIGN_RUNS)
    b.close(); eng.close()


@pytest.mark.parametrize("kw,name", [(dict(model_type=orc.STDSEG), "stdseg"), (dict(model_type=orc.STDSEG_NO_DUR, trans_share=(0, 9)), "stdseg_no_dur"),
                                     (dict(num_states=3), "stdseg_no_dur_no_segtransftr")])
def test_models_alignment_is_not_built_for_are_refused_by_name(kw, name):
    c = Case(L=6, D=3, in_w=3, Ts=[6, 5], seed=2, **kw)
    eng = c.engine(); b = c.batch(eng, with_labels=False)
    code, msg = _code(lambda: eng.align_batch(b, [np.zeros(2, dtype=np.uint32)] * 2))
    assert code == INVALID and '"%s"' % name in msg, msg
    if "num_states" in kw:
        assert "crf_states = 3" in msg
    b.close(); eng.close()


def test_chunked_runs_equal_the_one_chunk_run_and_repeat_bit_for_bit():
    si = CHUNKED
    c1 = case(si); cn = case(si, scratch_bytes=1 << 18)
    e1 = c1.engine(); b1 = c1.batch(e1, with_labels=False)
    en = cn.engine(); bn = cn.batch(en, with_labels=False)
    tr = seeded_transcripts(si)
    for mode in MODES:
        l1, c1_ = check_against_reference(si, e1, b1, tr, mode)
        calls0, chunks0 = en.align_stats()[:2]
        ln, cn_ = check_against_reference(si, en, bn, tr, mode)
        calls, chunks = en.align_stats()[:2]
        assert calls == calls0 + 1 and chunks - chunks0 > 1   # the small budget really splits the batch
        assert ln == l1 and cn_.tobytes() == c1_.tobytes()
        l2, c2 = en.align_batch(bn, tr, mode)                 # a second call on one engine
        assert [list(map(int, x)) for x in l2] == ln and c2.tobytes() == cn_.tobytes()
    assert e1.align_stats()[:2] == (2, 2)
    b1.close(); e1.close(); bn.close(); en.close()


@pytest.mark.parametrize("si", [si for si in range(len(SHAPES)) if si not in LONG_K])
def test_the_workgroup_kernel_equals_the_wavefront_kernel(si, monkeypatch):
    tr = seeded_transcripts(si)
    res = {}
    for tag, env in (("wave", None), ("group", "0")):
        monkeypatch.delenv("SCRF_ALIGN_WAVE", raising=False)
        if env is not None:
            monkeypatch.setenv("SCRF_ALIGN_WAVE", env)
        c = case(si)
        eng = c.engine(); b = c.batch(eng, with_labels=False)
        _, collapsed, _, _ = viterbi_transcripts(eng, b, c.L)
        res[tag] = [check_against_reference(si, eng, b, t, mode) for t in (tr, collapsed) for mode in MODES]
        res[tag + "_stats"] = eng.align_stats()
        b.close(); eng.close()
    for (lw, cw), (lg, cg) in zip(res["wave"], res["group"]):
        assert lw == lg and cw.tobytes() == cg.tobytes()
    assert res["wave_stats"] == (4, 4, 4, 0) and res["group_stats"] == (4, 4, 0, 4)


def test_fast_decode_weights_give_the_exact_paths_bits(monkeypatch):
    """a fused batch (raw frames, segment recipe; the config-2 shape of test_fast_decode_is_bit_identical_to_exact_decode):
    the screened fast score path feeds the search the same float weights as the EXACT path"""
    kw = dict(seed=503, lam_scale=0.3, L=48, D=25, in_w=39, Ts=[300, 57])
    res = {}
    rng = np.random.RandomState(17)
    tr = [ar.random_transcript(rng, T, 48, 25) for T in kw["Ts"]]
    for tag, env in (("exact", {"SCRF_FAST_DECODE": "0"}), ("fast", {}), ("fix", {"SCRF_DECODE_BOUND_SCALE": "30"})):
        for k in ("SCRF_FAST_DECODE", "SCRF_DECODE_BOUND_SCALE"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        c = Case(**kw)
        eng = c.engine(); b = c.batch(eng, with_labels=False)
        assert eng.batch_is_fused(b)
        per_seg, collapsed, vlabs, vcost = viterbi_transcripts(eng, b, c.L)
        fix0 = eng.decode_stats()
        out = []
        for t, mode in ((tr, scrf_amd.ALIGN_RUNS), (tr, scrf_amd.ALIGN_ONE), (collapsed, scrf_amd.ALIGN_RUNS), (per_seg, scrf_amd.ALIGN_ONE)):
            labs, cost = eng.align_batch(b, t, mode)
            out.append(([list(map(int, l)) for l in labs], cost.copy()))
        assert out[2][0] == vlabs and out[3][0] == vlabs and out[2][1].tobytes() == vcost.tobytes() == out[3][1].tobytes()
        assert all(np.isfinite(o[1]).all() for o in out)
        res[tag] = (out, eng.decode_stats(), eng.align_stats())
        b.close(); eng.close()
    for tag in ("fast", "fix"):
        for (le, ce), (lf, cf) in zip(res["exact"][0], res[tag][0]):
            assert le == lf and ce.tobytes() == cf.tobytes(), tag
        assert res[tag][1][1] == 0, tag    # no chunk fell back to the EXACT path
        assert res[tag][2][2] >= 2, tag    # D = 25: the wavefront kernel's deepest variant took the random transcripts
    assert res["exact"][1] == (0, 0)
    # the fast score path ran: with the screen widened as in the decode test, the calls recomputed weights it listed
    # (at the default scale the list may be empty, which the counters cannot tell from the EXACT path)
    assert res["fix"][1][0] > res["fast"][1][0] >= 0 and res["fix"][1][0] > 0


def _sparse_case():
    """the stdsparsetrans segmental case of tests/test_gpu_sparse.py (copied: test modules are not imported)"""
    L, N, P, D, Ts = 5, 40, 6, 4, [9, 14, 6]
    rng = np.random.RandomState(3)
    lay = sr.SparseLayout(L, sfe=N - 1, tfe=N - 1, use_tf=True)
    X = [sr.random_windows(rng, orc.num_segs(T, D), P, N, messy=True, values=None) for T in Ts]
    lam = rng.uniform(-0.5, 0.5, lay.lambda_len)
    cfg = scrf_amd.make_config(model_type=scrf_amd.STDSEG_NO_DUR_NO_SEGTRANSFTR, L=L, D=D, F=2 * P, sfe=N - 1, tfe=N - 1,
                               use_trans_ftrs=True, sparse=True, state_bias_val=2.5, trans_bias_val=0.5)
    eng = scrf_amd.Engine(cfg)
    eng.set_lambda(lam)
    return eng, eng.batch_from_windows(X, Ts), Ts, L, D


def test_sparse_map_and_a_batch_of_materialised_windows():
    eng, b, Ts, L, D = _sparse_case()
    rng = np.random.RandomState(11)
    tr = [ar.random_transcript(rng, T, L, D) for T in Ts]
    lats = [eng.lattice_arcs(b, u) for u in range(len(Ts))]
    for mode in MODES:
        labs, cost = eng.align_batch(b, tr, mode)
        for u, T in enumerate(Ts):
            arcs, ns, fin = lats[u]
            assert bits(cost[u]) == bits(ar.compose(arcs, ns, fin, L, tr[u], mode)), (u, mode)   # form 2 on the engine's lattice
            assert np.isfinite(cost[u]) and ar.matches(labs[u], L, tr[u], mode)
            assert bits(ArcTable(eng, b, u, T, L, False).path_cost(labs[u])) == bits(cost[u])
    b.close(); eng.close()
    si = 1   # dense, per-frame M: the same utterances given as window vectors
    c = case(si)
    eng = c.engine()
    b = eng.batch_from_windows([c.windows(u) for u in range(len(c.Ts))], c.Ts)
    for mode in MODES:
        check_against_reference(si, eng, b, seeded_transcripts(si), mode)
    b.close(); eng.close()


@pytest.mark.parametrize("si", [0, 2, 3])
def test_aligned_segments_are_posterior_queries(si):
    c = case(si)
    eng = c.engine(); b = c.batch(eng, with_labels=False)
    for mode in MODES:
        labs, cost = eng.align_batch(b, seeded_transcripts(si), mode)
        assert np.isfinite(cost).all()
        post = eng.posteriors_batch(b, frame=False, end=False, segments=labs)
        conf = post["segments_flat"]
        assert conf.shape[0] == int(labs.off[-1]) > 0
        assert ((conf >= 0.0) & (conf <= 1.0)).all(), conf
    b.close(); eng.close()
