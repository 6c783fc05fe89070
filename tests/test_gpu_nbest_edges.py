"""-m gpu: scrf_nbest_batch where the kernels' own logic decides: equal costs within one lane of the merge, lists
longer than a wavefront, the largest footprint the host admits, the scan with several entries per thread, results that grow
over chunks ending on short lists, fast-decode weights in later chunks, and the tied input family.  The cases and what each
reaches are in tests/nbest_cases.py; tests/test_nbest_cases.py (no GPU) asserts that each edge really occurs.  Everything is
compared with tests/nbest_ref.py as raw bits: no tolerance, no excluded case."""
import ctypes as C

import numpy as np
import pytest

import family_shapes as fs
import nbest_cases as nc
import nbest_ref as nr
import align_ref as ar
import scrf_amd

pytestmark = pytest.mark.gpu

INVALID = 1
# (scratch bytes, chunks): found on the card and fixed here through the asserted chunk counts
SPLIT = (1 << 16, 29)                        # the split batch: 301 short utterances, N = 40
FUSED = {1: (1 << 16, 3), 3: (1 << 17, 2)}   # copies of the fused shape's four lengths (L = 7, D = 10, Ts 9 10 11 30), N = 8
MIXED = (1 << 15, 3)                         # the mixed shape (L = 6, D = 4, per-frame M, Ts 9 14 3 1), N = 16


def bits(x):
    return np.float32(x).tobytes()


def hyps(labs, hoff, cost):
    """per utterance [(labels, cost)] of an Engine.nbest_batch result"""
    return [[(tuple(int(x) for x in labs[i]), cost[i]) for i in range(int(hoff[u]), int(hoff[u + 1]))] for u in range(len(hoff) - 1)]


def check(got, want):
    """(tests/test_gpu_nbest.py's helper: test modules are not imported)"""
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


def run(eng, b, N, want, c):
    """one call compared with the reference, hypothesis 0 with viterbi_batch; paths distinct, their frames sum to T"""
    got = hyps(*eng.nbest_batch(b, N))
    check(got, want)
    check_viterbi(eng, b, got)
    for u, g in enumerate(got):
        assert len(set(p for p, _ in g)) == len(g)
        assert all(sum(l // c.L + 1 for l in p) == c.Ts[u] for p, _ in g)
    return got


def _code(fn):
    with pytest.raises(scrf_amd.ScrfError) as e:
        fn()
    return e.value.code, str(e.value)


@pytest.mark.parametrize("name", nc.ROW_NAMES)
def test_every_row_of_the_table_equals_the_reference_bit_for_bit(name, monkeypatch):
    row = nc.ROWS[name]
    res = {}
    for env in (("0", None) if name in nc.FAST_TOO else (None,)):
        monkeypatch.delenv("SCRF_FAST_DECODE", raising=False)
        if env is not None:
            monkeypatch.setenv("SCRF_FAST_DECODE", env)
        c = nc.make_case(name)
        eng = c.engine(); b = c.batch(eng, with_labels=False)
        if name == "lds_max":     # one hypothesis more than fits: refused before anything is launched
            N = row["ns"][0] + 1
            code, msg = _code(lambda: eng.nbest_batch(b, N))
            assert code == INVALID and "LDS" in msg and str(nc.lds_bytes(c.L, c.D, N)) in msg and str(nc.LDS_LIMIT) in msg, msg
            assert eng.nbest_stats() == (0, 0, 0)
        for N in row["ns"]:
            res[env, N] = run(eng, b, N, nc.reference(name, N), c)
        calls, chunks, fast = eng.nbest_stats()
        assert calls == chunks == len(row["ns"])
        if name in nc.FAST_TOO:
            assert eng.batch_is_fused(b) and (fast > 0) == (env is None), (env, fast)
        b.close(); eng.close()
    if name in nc.FAST_TOO:
        for N in row["ns"]:
            check(res[None, N], res["0", N])


def _paths(eng, b, u0, n, n_lab, n_hyp):
    labs = np.empty(max(n_lab, 1), dtype=np.uint32); off = np.empty(n_hyp + 1, dtype=np.uint64); cost = np.empty(max(n_hyp, 1), dtype=np.float32)
    P = lambda a: a.ctypes.data_as(C.c_void_p)
    eng._chk(eng.lib.scrf_nbest_paths(eng.h, b.handle, C.c_uint32(u0), C.c_uint32(n), P(labs), C.c_uint64(n_lab), P(off), P(cost)))
    return labs, off, cost


def check_offsets(labs, hoff, cost, want):
    """hyp_off, the label offsets and the costs of a whole result against the reference, as arrays"""
    counts = [len(h) for h in want]
    assert [int(x) for x in hoff] == [0] + [int(x) for x in np.cumsum(counts)]
    lens = [len(p) for h in want for p, _ in h]
    H = int(hoff[-1])
    assert [int(x) for x in labs.off[:H + 1]] == [0] + [int(x) for x in np.cumsum(lens)]
    assert len(cost) == H


@pytest.mark.parametrize("name", ["scan_even", "scan_odd"])
def test_the_scan_with_several_entries_per_thread(name):
    """one chunk of U * N > 1,024 (utterance, rank) entries: every thread of k_nbest_scan sums 2 (3) entries serially, with
    empty entries between full ones and, on the odd shape, a last range that is partly empty"""
    kw, N = nc.BATCHES[name]
    c = nc.make_batch_case(name)
    assert nc.scan_per(len(c.Ts), N) == (2 if name == "scan_even" else 3)
    want = nc.reference(name, N)
    eng = c.engine(); b = c.batch(eng, with_labels=False)
    labs, hoff, cost = eng.nbest_batch(b, N)
    check_offsets(labs, hoff, cost, want)
    got = hyps(labs, hoff, cost)
    check(got, want)
    check_viterbi(eng, b, got)
    assert eng.nbest_stats()[:2] == (1, 1)
    b.close(); eng.close()


def test_chunks_that_end_on_a_short_list_and_a_result_that_grows_chunk_by_chunk():
    """every utterance has fewer than N paths: the last (utterance, rank) entry of every chunk holds no hypothesis (the h_end
    sentinel of k_nbest_trace), every chunk holds short lists only, and the result arrays grow with every chunk"""
    kw, N = nc.BATCHES["split"]
    want = nc.reference("split", N)
    c1 = nc.make_batch_case("split"); cn = nc.make_batch_case("split", scratch_bytes=SPLIT[0])
    e1 = c1.engine(); b1 = c1.batch(e1, with_labels=False)
    en = cn.engine(); bn = cn.batch(en, with_labels=False)
    r1 = e1.nbest_batch(b1, N)
    rn = en.nbest_batch(bn, N)
    print("split batch: %s under the default budget, %s under %d bytes" % (e1.nbest_stats(), en.nbest_stats(), SPLIT[0]))
    assert e1.nbest_stats()[:2] == (1, 1)
    calls, chunks, _ = en.nbest_stats()
    assert calls == 1 and chunks == SPLIT[1] >= 4       # the result grows chunk by chunk; about ten utterances per chunk
    for labs, hoff, cost in (r1, rn):
        check_offsets(labs, hoff, cost, want)
        check(hyps(labs, hoff, cost), want)
    check(hyps(*en.nbest_batch(bn, N)), want)            # a second call on the split engine
    assert en.nbest_stats()[:2] == (2, 2 * chunks)
    check_viterbi(en, bn, hyps(*rn))
    # a range of utterances that straddles every chunk boundary but the ends, read back through scrf_nbest_paths
    labs, hoff, cost = rn
    u0, u1 = 2, len(c1.Ts) - 3
    h0, h1 = int(hoff[u0]), int(hoff[u1])
    a0, a1 = int(labs.off[h0]), int(labs.off[h1])
    l2, o2, c2 = _paths(en, bn, u0, u1 - u0, a1 - a0, h1 - h0)
    assert [int(x) for x in o2] == [int(labs.off[i]) - a0 for i in range(h0, h1 + 1)]
    assert c2[:h1 - h0].tobytes() == cost[h0:h1].tobytes()
    assert l2[:a1 - a0].tobytes() == labs.flat[a0:a1].tobytes()
    b1.close(); e1.close(); bn.close(); en.close()


def _fused_runs(monkeypatch, Ts, budget, scale=None):
    """the fused shape on the signed family, N = 8: (result, nbest_stats, decode_stats) of the EXACT run in one chunk and of the
    fast run under the budget"""
    out = {}
    for tag, env, sb in (("exact", "0", 0), ("fast", None, budget)):
        monkeypatch.delenv("SCRF_FAST_DECODE", raising=False)
        monkeypatch.delenv("SCRF_DECODE_BOUND_SCALE", raising=False)
        if env is not None:
            monkeypatch.setenv("SCRF_FAST_DECODE", env)
        if scale is not None and tag == "fast":
            monkeypatch.setenv("SCRF_DECODE_BOUND_SCALE", scale)
        c = fs.case("fused", "signed", Ts=Ts, scratch_bytes=sb)
        eng = c.engine(); b = c.batch(eng, with_labels=False)
        assert eng.batch_is_fused(b)
        got = hyps(*eng.nbest_batch(b, 8))
        check_viterbi(eng, b, got)
        out[tag] = (got, eng.nbest_stats(), eng.decode_stats())
        b.close(); eng.close()
    monkeypatch.delenv("SCRF_DECODE_BOUND_SCALE", raising=False)
    return out


@pytest.mark.parametrize("copies", [1, 3])
@pytest.mark.parametrize("scale", [None, "30"])
def test_fast_decode_weights_in_later_chunks(copies, scale, monkeypatch):
    """k_nbest reads the float weights at Wn + s_base * L with s_base relative to the chunk's first utterance: a split fast run
    (with three copies of the four lengths, later chunks hold several utterances) gives the EXACT run's and the reference's
    bytes; under SCRF_DECODE_BOUND_SCALE=30 the later chunks hold recomputed weights too"""
    Ts = fs.SHAPES["fused"][0]["Ts"] * copies
    c = fs.case("fused", "signed", Ts=Ts)
    want = [[(tuple(p), x) for p, x in nr.nbest(ar.case_weights(c, u), 8)] for u in range(len(Ts))]
    budget, n_chunks = FUSED[copies]
    out = _fused_runs(monkeypatch, Ts, budget, scale)
    print("fused x %d, bound scale %s: exact %s, fast under %d bytes %s, decode stats %s"
          % (copies, scale, out["exact"][1], budget, out["fast"][1], out["fast"][2]))
    assert out["exact"][1] == (1, 1, 0)
    calls, chunks, fast = out["fast"][1]
    assert calls == 1 and chunks == n_chunks > 1 and fast == chunks
    if copies > 1:
        assert chunks <= len(Ts) // 4     # the chunks after the first hold several utterances
    if scale is not None:
        assert out["fast"][2][0] > 0  # weights were listed and recomputed
    check(out["fast"][0], out["exact"][0])
    check(out["fast"][0], want)


def test_a_mixed_batch_in_chunks():
    """per-frame M (M + (f_base + t) L L with f_base relative to the chunk), the T = 1 utterance with its 6 paths last"""
    N = 16
    c1 = fs.case("mixed", "signed"); cn = fs.case("mixed", "signed", scratch_bytes=MIXED[0])
    assert c1.Ts[-1] == 1 and nr.num_paths(1, c1.L, c1.D) == 6
    want = [[(tuple(p), x) for p, x in nr.nbest(ar.case_weights(c1, u), N)] for u in range(len(c1.Ts))]
    assert [len(h) for h in want] == [N, N, N, 6]
    e1 = c1.engine(); b1 = c1.batch(e1, with_labels=False)
    en = cn.engine(); bn = cn.batch(en, with_labels=False)
    run(e1, b1, N, want, c1)
    run(en, bn, N, want, cn)
    print("mixed: %s in one chunk, %s under %d bytes" % (e1.nbest_stats(), en.nbest_stats(), MIXED[0]))
    assert e1.nbest_stats()[:2] == (1, 1)
    calls, chunks, _ = en.nbest_stats()
    assert calls == 1 and chunks == MIXED[1] > 1
    b1.close(); e1.close(); bn.close(); en.close()
