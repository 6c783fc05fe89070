"""-m gpu: batched N-best decoding (scrf_nbest_batch) against the numpy reference tests/nbest_ref.py over the CPU
oracle's scores.  The rule fixes every bit (sorted float32 lists over monotone left-to-right sums, a stable tie order), so labels,
counts and costs are compared as raw bits: no tolerance, no excluded case."""
import ctypes as C
import functools

import numpy as np
import pytest

import align_ref as ar
import nbest_ref as nr
import orc
import scrf_amd
import sparse_ref as sr
from cases import Case

pytestmark = pytest.mark.gpu

INVALID = 1

# (Case keywords, the n_best values)
CASES = [
    (dict(L=2, D=2, in_w=2, Ts=[1, 2, 3, 4, 5]), (1, 5, 40)),                                   # lists shorter than N
    (dict(L=3, D=3, in_w=2, Ts=[7]), (1, 2, 16)),
    (dict(L=4, D=1, in_w=3, Ts=[6], trans_ctx=1, frame_model=True), (8,)),                       # frame model
    (dict(L=3, D=4, in_w=3, Ts=[20], trans_ctx=1), (8,)),                                        # stdtrans map, per-frame M
    (dict(L=70, D=4, in_w=3, Ts=[12], lam_scale=0.1), (8,)),                                     # more lists than lanes
    (dict(L=2, D=66, in_w=2, Ts=[70]), (5,)),                                                    # more durations than lanes
    (dict(L=48, D=25, in_w=39, Ts=[300, 57], lam_scale=0.3), (16,)),                             # U = 2, the config-2 shape
    (dict(L=4, D=1, in_w=3, Ts=[1, 2, 6], frame_model=True), (1, 8)),                            # frame model, a single M
]
BIG = 6
CHUNKED = dict(L=66, D=4, in_w=69, Ts=[9, 14, 3, 1, 11, 8], lam_scale=0.05)


def bits(x):
    return np.float32(x).tobytes()


def case(ci, **kw):
    return Case(seed=1100 + ci, **dict(CASES[ci][0], **kw))


@functools.lru_cache(maxsize=None)
def weights(ci):
    """per utterance the oracle's float arc weights (ar.Weights); computed once per case and not modified"""
    c = case(ci)
    return tuple(ar.case_weights(c, u) for u in range(len(c.Ts)))


@functools.lru_cache(maxsize=None)
def reference(ci, N):
    return tuple(tuple((tuple(p), c) for p, c in nr.nbest(w, N)) for w in weights(ci))


def hyps(labs, hoff, cost):
    """per utterance [(labels, cost)] of an Engine.nbest_batch result"""
    return [[(tuple(int(x) for x in labs[i]), cost[i]) for i in range(int(hoff[u]), int(hoff[u + 1]))] for u in range(len(hoff) - 1)]


def check(got, want):
    assert len(got) == len(want)
    for u, (g, w) in enumerate(zip(got, want)):
        assert len(g) == len(w), (u, len(g), len(w))
        for r, ((gl, gc), (wl, wc)) in enumerate(zip(g, w)):
            assert bits(gc) == bits(wc), (u, r, gc, wc)
            assert gl == wl, (u, r, gl, wl)


def check_viterbi(eng, b, got):
    vl, vc = eng.viterbi_batch(b)
    for u, g in enumerate(got):
        assert g[0][0] == tuple(int(x) for x in vl[u]) and bits(g[0][1]) == bits(vc[u]), (u, g[0], list(vl[u]), vc[u])


@pytest.mark.parametrize("ci", range(len(CASES)))
def test_labels_counts_and_costs_equal_the_reference_bit_for_bit(ci):
    c = case(ci)
    eng = c.engine(); b = c.batch(eng, with_labels=False)
    for N in CASES[ci][1]:
        got = hyps(*eng.nbest_batch(b, N))
        check(got, reference(ci, N))
        check_viterbi(eng, b, got)
        for u, g in enumerate(got):
            assert len(set(p for p, _ in g)) == len(g)                      # pairwise distinct
            assert all(sum(l // c.L + 1 for l in p) == c.Ts[u] for p, _ in g)
            assert len(g) == min(N, nr.num_paths(c.Ts[u], c.L, c.D)) if c.Ts[u] <= 5 else len(g) == N
    calls, chunks, _ = eng.nbest_stats()
    assert calls == chunks == len(CASES[ci][1])   # the default budget: one chunk per call
    b.close(); eng.close()


def test_all_weights_zero_every_path_ties_and_the_tie_rule_alone_orders_them():
    c = Case(seed=1150, L=2, D=3, in_w=2, Ts=[5])
    c.lam[:] = 0.0
    w = ar.case_weights(c, 0)
    want = nr.nbest(w, 10)
    assert len(want) == 10 and all(bits(x) == bits(0.0) for _, x in want)
    eng = c.engine(); b = c.batch(eng, with_labels=False)
    got = hyps(*eng.nbest_batch(b, 10))
    check(got, [[(tuple(p), x) for p, x in want]])
    check_viterbi(eng, b, got)
    b.close(); eng.close()


def test_an_utterance_without_frames_never_reaches_the_search():
    """a T = 0 utterance would have 0 hypotheses (k_nbest writes an all-inf final list), but scrf_batch_create refuses it"""
    c = Case(seed=1151, L=2, D=2, in_w=2, Ts=[3])
    eng = c.engine()
    with pytest.raises(scrf_amd.ScrfError) as e:
        eng.batch_from_frames([c.frames[0], np.zeros((0, 2), dtype=np.float32)], None, c.recipes)
    assert e.value.code != 0 and "No features" in str(e.value)
    eng.close()


def test_a_small_scratch_budget_splits_the_batch_and_changes_no_byte():
    kw = dict(seed=1160, **CHUNKED)
    c1 = Case(**kw); cn = Case(scratch_bytes=1 << 18, **kw)
    want = [[(tuple(p), x) for p, x in nr.nbest(ar.case_weights(c1, u), 4)] for u in range(len(c1.Ts))]
    e1 = c1.engine(); b1 = c1.batch(e1, with_labels=False)
    en = cn.engine(); bn = cn.batch(en, with_labels=False)
    g1 = hyps(*e1.nbest_batch(b1, 4))
    gn = hyps(*en.nbest_batch(bn, 4))
    check(g1, want); check(gn, want)
    assert e1.nbest_stats()[:2] == (1, 1)
    calls, chunks, _ = en.nbest_stats()
    assert calls == 1 and chunks > 1   # the small budget really splits the batch
    check(hyps(*en.nbest_batch(bn, 4)), want)   # a second run on one engine
    check_viterbi(en, bn, gn)
    b1.close(); e1.close(); bn.close(); en.close()


def test_fast_decode_weights_give_the_exact_paths_bits(monkeypatch):
    """a fused batch (raw frames, segment recipe; the config-2 shape): the screened fast score path feeds the search the same
    float weights as the EXACT path"""
    res = {}
    for tag, env in (("exact", "0"), ("fast", None)):
        monkeypatch.delenv("SCRF_FAST_DECODE", raising=False)
        if env is not None:
            monkeypatch.setenv("SCRF_FAST_DECODE", env)
        c = case(BIG)
        eng = c.engine(); b = c.batch(eng, with_labels=False)
        assert eng.batch_is_fused(b)
        got = hyps(*eng.nbest_batch(b, 16))
        again = hyps(*eng.nbest_batch(b, 16))   # across two runs
        check(again, got)
        res[tag] = (got, eng.nbest_stats())
        b.close(); eng.close()
    check(res["fast"][0], res["exact"][0])
    check(res["fast"][0], reference(BIG, 16))
    assert res["exact"][1] == (2, 2, 0)
    assert res["fast"][1][0] == 2 and res["fast"][1][2] > 0   # the fast score path ran


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


class LatticeWeights:
    """nbest_ref's view of the float weights of an engine lattice (Engine.lattice_arcs) of a segmental model"""
    frame_model = False

    def __init__(self, arcs, T, L, D):
        self.T, self.L, self.D = T, L, D
        self.w = {(int(a["src"]), int(a["dst"])): np.float32(a["w"]) for a in arcs}

    def _end(self, t, lab):
        return 1 + lab if t == 0 else 1 + self.L + (t - 1) * 2 * self.L + self.L + lab

    def _bnd(self, t, lab):
        return 1 + self.L + (t - 1) * 2 * self.L + lab

    def seg(self, t, d, lab):
        ts = t - d + 1
        f = lambda l: self.w[(0 if ts == 0 else self._bnd(ts, int(l)), self._end(t, int(l)))]
        return np.array([f(l) for l in lab], dtype=np.float32) if np.ndim(lab) else f(lab)

    def boundary(self, t, p, lab):
        f = lambda l: self.w[(self._end(t - 1, int(p)), self._bnd(t, int(l)))]
        return np.array([f(l) for l in lab], dtype=np.float32) if np.ndim(lab) else f(lab)


def test_sparse_map_and_a_batch_of_materialised_windows():
    eng, b, Ts, L, D = _sparse_case()
    want = []
    for u, T in enumerate(Ts):
        arcs, ns, fin = eng.lattice_arcs(b, u)
        want.append([(tuple(p), x) for p, x in nr.nbest(LatticeWeights(arcs, T, L, D), 6)])
    got = hyps(*eng.nbest_batch(b, 6))
    check(got, want)
    check_viterbi(eng, b, got)
    b.close(); eng.close()
    ci = 3   # dense, per-frame M: the same utterance given as window vectors
    c = case(ci)
    eng = c.engine()
    b = eng.batch_from_windows([c.windows(u) for u in range(len(c.Ts))], c.Ts)
    check(hyps(*eng.nbest_batch(b, 8)), reference(ci, 8))
    b.close(); eng.close()


def test_hypotheses_chain_into_the_posterior_and_transcript_entry_points():
    c = Case(seed=1170, L=2, D=2, in_w=2, Ts=[4, 3])
    n_paths = [nr.num_paths(T, c.L, c.D) for T in c.Ts]
    N = 64
    assert N >= max(n_paths)
    eng = c.engine(); b = c.batch(eng, with_labels=False)
    got = hyps(*eng.nbest_batch(b, N))
    assert [len(g) for g in got] == n_paths
    U = len(c.Ts)
    # every hypothesis is a segment query of both entry points
    for r in range(max(n_paths)):
        segs = [np.asarray(got[u][min(r, len(got[u]) - 1)][0], dtype=np.uint32) for u in range(U)]
        post = eng.posteriors_batch(b, frame=False, end=False, segments=segs)
        assert ((post["segments_flat"] >= 0.0) & (post["segments_flat"] <= 1.0)).all()
        tr = [np.asarray(nr.collapsed(s, c.L), dtype=np.uint32) for s in segs]
        out = eng.transcript_batch(b, tr, scrf_amd.ALIGN_RUNS, frame=False, end=False, segments=segs)
        assert np.isfinite(out["logp"]).all() and ((out["segments_flat"] >= 0.0) & (out["segments_flat"] <= 1.0 + 1e-9)).all()
    # the distinct collapsed sequences partition the lattice: their probabilities sum to 1 (DESIGN.md 4.13's bound)
    seqs = []
    for g in got:
        s = []
        for p, _ in g:
            q = nr.collapsed(p, c.L)
            if q not in s:
                s.append(q)
        seqs.append(s)
    total = np.zeros(U)
    for r in range(max(len(s) for s in seqs)):
        tr = [np.asarray(s[r] if r < len(s) else [], dtype=np.uint32) for s in seqs]
        out = eng.transcript_batch(b, tr, scrf_amd.ALIGN_RUNS, frame=False, end=False)
        for u in range(U):
            assert (r < len(seqs[u])) == np.isfinite(out["logp"][u])
        total += np.exp(out["logp"])
    assert np.abs(total - 1.0).max() < 1e-9, total
    b.close(); eng.close()


def _code(fn):
    with pytest.raises(scrf_amd.ScrfError) as e:
        fn()
    return e.value.code, str(e.value)


@pytest.mark.parametrize("kw,name", [(dict(model_type=orc.STDSEG), "stdseg"), (dict(model_type=orc.STDSEG_NO_DUR, trans_share=(0, 9)), "stdseg_no_dur"),
                                     (dict(num_states=3), "stdseg_no_dur_no_segtransftr")])
def test_models_n_best_decoding_is_not_built_for_are_refused_by_name(kw, name):
    c = Case(L=6, D=3, in_w=3, Ts=[6, 5], seed=2, **kw)
    eng = c.engine(); b = c.batch(eng, with_labels=False)
    code, msg = _code(lambda: eng.nbest_batch(b, 4))
    assert code == INVALID and '"%s"' % name in msg and "N-best" in msg, msg
    if "num_states" in kw:
        assert "crf_states = 3" in msg
    assert eng.nbest_stats() == (0, 0, 0)
    b.close(); eng.close()


def _paths(eng, b, u0, n, cap):
    labs = np.empty(max(cap, 1), dtype=np.uint32); off = np.empty(4096, dtype=np.uint64); cost = np.empty(4096, dtype=np.float32)
    P = lambda a: a.ctypes.data_as(C.c_void_p)
    eng._chk(eng.lib.scrf_nbest_paths(eng.h, b.handle, C.c_uint32(u0), C.c_uint32(n), P(labs), C.c_uint64(cap), P(off), P(cost)))
    return labs, off, cost


def test_arguments_and_stale_results_are_refused_with_their_messages():
    c = Case(seed=1180, L=7, D=10, in_w=5, Ts=[9, 10, 11, 30])
    eng = c.engine(); b = c.batch(eng, with_labels=False); b2 = c.batch(eng, with_labels=False)
    code, msg = _code(lambda: eng.nbest_batch(b, 0))
    assert code == INVALID and "n_best" in msg and "got 0" in msg, msg
    code, msg = _code(lambda: eng.nbest_batch(b, 65536))
    assert code == INVALID and "n_best" in msg, msg
    # (10 + 2) * 7 * 600 * 4 bytes of lists + 16 wavefronts * 12 head ranks * 2 bytes
    code, msg = _code(lambda: eng.nbest_batch(b, 600))
    assert code == INVALID and "LDS" in msg and str(12 * 7 * 600 * 4 + 16 * 12 * 2) in msg and "163840" in msg, msg
    assert eng.nbest_stats() == (0, 0, 0)   # nothing was launched for the refused calls
    code, msg = _code(lambda: _paths(eng, b, 0, 4, 1 << 16))
    assert code == INVALID and "no valid result" in msg, msg
    labs, hoff, cost = eng.nbest_batch(b, 3)
    n_lab = int(labs.off[-1])
    l2, o2, c2 = _paths(eng, b, 1, 2, n_lab)   # a range: utterances 1 and 2
    h0, h1 = int(hoff[1]), int(hoff[3])
    assert o2[0] == 0 and [int(x) for x in o2[:h1 - h0 + 1]] == [int(labs.off[i]) - int(labs.off[h0]) for i in range(h0, h1 + 1)]
    assert c2[:h1 - h0].tobytes() == cost[h0:h1].tobytes()
    assert l2[:int(o2[h1 - h0])].tobytes() == labs.flat[int(labs.off[h0]):int(labs.off[h1])].tobytes()
    code, msg = _code(lambda: _paths(eng, b, 0, 4, n_lab - 1))   # too small a capacity: the count needed is named
    assert code == INVALID and "%d needed" % n_lab in msg, msg
    code, msg = _code(lambda: _paths(eng, b, 2, 3, n_lab))       # a bad range
    assert code == INVALID and "batch of 4" in msg, msg
    code, msg = _code(lambda: _paths(eng, b2, 0, 4, n_lab))      # another batch
    assert code == INVALID and "no valid result" in msg, msg
    eng.set_lambda(c.lam)                                        # new weights drop the result
    code, msg = _code(lambda: _paths(eng, b, 0, 4, n_lab))
    assert code == INVALID and "no valid result" in msg, msg
    eng.nbest_batch(b, 3)
    _paths(eng, b, 0, 4, n_lab)
    b.close()                                                    # destroying the batch drops it too; the engine still answers
    check(hyps(*eng.nbest_batch(b2, 3)), [[(tuple(p), x) for p, x in nr.nbest(ar.case_weights(c, u), 3)] for u in range(4)])
    b2.close(); eng.close()
