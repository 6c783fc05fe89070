"""No GPU: the tiled batches of tests/big_batch.py.  The tiled expected gradient equals the oracle run over the expanded
lists on a tiny shape; the restated plans give the values worked out by hand from scrf_engine.cpp; and every shape of
tests/test_gpu_big_batch.py crosses the byte size and the plan breakpoints it is there for by at least 5 %."""
import numpy as np
import pytest

import big_batch as bb
import orc
from cases import Case


def test_tiled_lists_hold_references_and_interleave_to_the_far_end():
    c = Case(L=3, D=3, in_w=2, Ts=[5, 1, 3], trans_ctx=1, seed=5)
    counts = [7, 2, 4]
    for order in ("spread", "roundrobin"):
        frames, labels, frames2, base = bb.tiled(c, counts, order)
        assert len(frames) == len(labels) == len(frames2) == len(base) == sum(counts)
        assert [int((base == i).sum()) for i in range(3)] == counts
        for u, i in enumerate(base):
            assert frames[u] is c.frames[i] and labels[u] is c.labels[i] and frames2[u] is c.frames2[i]
    assert list(bb.copy_order(counts, "roundrobin")) == [0, 1, 2, 0, 1, 2, 0, 2, 0, 2, 0, 0, 0]
    # spread: no base utterance is exhausted early -- each still occurs in the last third of the batch, and the last
    # copies of the GPU cases' batches are of different base utterances
    sp = bb.copy_order(counts, "spread")
    assert set(sp[-len(sp) // 3:]) == {0, 1, 2}
    for row in bb.CASES.values():
        o = bb.copy_order(row["counts"])
        n = len(o)
        # the last copy of base i sits at 1 - 1 / (2 counts[i]) of the batch: within its last 1 / (2 min(counts))
        assert len(set(o[-(n // (2 * min(row["counts"])) + 2):])) == len(row["counts"])
        assert len(set(o[-3:])) >= 2                              # and the very end alternates
    with pytest.raises(AssertionError):
        bb.Tiled(c, [2, 2, 2])                                    # the counts are to be unequal


@pytest.mark.parametrize("kw", [dict(L=3, D=3, in_w=2, Ts=[5, 1, 3], seed=5), dict(L=3, D=3, in_w=2, Ts=[4, 2, 6], trans_ctx=1, seed=6),
                                dict(L=2, D=3, in_w=2, Ts=[4, 3, 5], model_type=orc.STDSEG, seed=7),
                                dict(L=3, D=1, in_w=2, Ts=[4, 3, 5], trans_ctx=0, frame_model=True, seed=8)])
def test_tiled_expected_gradient_equals_the_oracle_over_the_expanded_lists(kw, oracle):
    c = Case(**kw)
    counts = [3, 1, 2]
    exp = bb.Expected(c)
    t = bb.Tiled(c, counts)
    import copy
    big = copy.copy(c)       # the same case over the expanded lists: the oracle sums utterance by utterance
    big.Ts, big.frames, big.labels, big.frames2 = [int(x) for x in t.Ts], t.frames, t.labels, t.frames2
    og, on, oz = big.oracle_gradient()
    assert np.abs(exp.gradient(counts) - og).max() <= 1e-13 * np.abs(og).max()    # two orders of summing 6 fp64 vectors
    assert np.array_equal(exp.numer[t.base], on) and np.array_equal(exp.zx[t.base], oz)


def test_nstate_case_expected_gradient(oracle):
    c = bb.NStateCase(P=3, K=2, F=3, Ts=[4, 1, 6], seed=3)
    exp = bb.Expected(c)
    og = np.zeros(c.olay.lambda_len)
    for u in (0, 1, 1, 2, 0, 0):
        rc, og, n, z = orc.nstate_build_gradient(c.ocfg, c.olay, c.lam, c.frames[u], c.labels[u], c.Ts[u], grad=og)
        assert rc == 0 and n == exp.numer[u] and z == exp.zx[u]
    assert np.abs(exp.gradient([3, 2, 1]) - og).max() <= 1e-13 * np.abs(og).max()


def test_layout_and_plans_by_hand():
    assert [bb.num_segs(T, 25) for T in (300, 257, 40, 7)] == [7200, 6125, 700, 28]
    assert bb.nseg([300, 7], [2, 3], 25) == 14484 and bb.nfr([300, 7], [2, 3]) == 621
    assert bb.num_segs(9, 4) == orc.num_segs(9, 4) and bb.num_segs(2, 4) == orc.num_segs(2, 4)
    # expf_rows_per_chunk: 4096 up to 1024 chunks of 4096 rows; then ceil(nseg / 1024) rounded up to 32
    assert bb.expf_rows_per_chunk(1) == 4096 and bb.expf_rows_per_chunk(bb.EXPF_BREAK) == 4096
    assert bb.expf_rows_per_chunk(bb.EXPF_BREAK + 1) == 4128
    assert bb.expf_rows_per_chunk(11968900) == 11712        # ceil(11968900 / 1024) = 11689 -> 11712
    # atb_rows_per_chunk: 64 up to 4096 chunks of 64 frames; then ceil(nfr / 4096) rounded up to 4
    assert bb.atb_rows_per_chunk(100) == 64 and bb.atb_rows_per_chunk(bb.ATB_BREAK) == 64
    assert bb.atb_rows_per_chunk(bb.ATB_BREAK + 1) == 68 and bb.atb_rows_per_chunk(502090) == 124
    # sl_rows_per_chunk: 64 up to 256 chunks of 64 frames; then ceil(nfr / 256) rounded up to 32
    assert bb.sl_rows_per_chunk(100) == 64 and bb.sl_rows_per_chunk(bb.SL_BREAK) == 64
    assert bb.sl_rows_per_chunk(bb.SL_BREAK + 1) == 96 and bb.sl_rows_per_chunk(201450) == 800


def test_lattice_arc_count_formula(oracle):
    import latprune_ref as lr
    c = Case(L=3, D=3, in_w=2, Ts=[1, 2, 3, 4, 7], seed=600)
    for u, T in enumerate(c.Ts):
        arcs, ns, fin = lr.oracle_lattice(c, u)
        assert arcs.shape[0] == bb.lattice_arcs(T, 3, 3), (T, arcs.shape[0])


def test_every_axis_a_case_crosses_what_it_is_there_for():
    for name, row in bb.CASES.items():
        ns, nf, nu = bb.case_sizes(name)
        sizes = bb.array_bytes(name)
        for a in row["arrays"]:
            print("%s: %s = %d bytes (%.3f x 2^32); nseg %d nfr %d utterances %d" % (name, a, sizes[a], sizes[a] / bb.TWO32, ns, nf, nu))
            assert sizes[a] >= bb.MARGIN * bb.TWO32, (name, a, sizes[a])
            assert sizes[a] // 8 < 1 << 31, (name, a)    # out of scope: more than 2^31 elements in one array
        if row["largest"]:
            print("%s: %s = %d bytes (below 2^32: see the test's docstring)" % (name, row["largest"], sizes[row["largest"]]))
            assert sizes[row["largest"]] < bb.TWO32
        for what, plan in row["crossings"]:
            v = ns if what == "nseg" else nf
            assert v >= bb.MARGIN * bb.BOUNDARY[plan], (name, plan, v)
        assert nf < 1 << 31
    # the plans really moved off their floors at these sizes
    assert bb.expf_rows_per_chunk(bb.case_sizes("fused")[0]) > 4096
    assert bb.expf_rows_per_chunk(bb.case_sizes("general")[0]) > 4096
    assert bb.expf_rows_per_chunk(bb.case_sizes("hybrid")[0]) > 4096
    assert bb.atb_rows_per_chunk(bb.case_sizes("fused")[1]) > 64
    assert bb.sl_rows_per_chunk(bb.case_sizes("stdseg_lin")[1]) > 64
    assert bb.need_bytes("fused") < 64 << 30 and bb.need_bytes("general") < 64 << 30
    # transcript scoring: each of the two cell arrays alone passes 2^32 bytes, every transcript fits in SCRF_ALIGN_ONE mode
    kw = bb.CASES["transcript"]["kw"]
    assert all(K <= T <= K * kw["D"] for T, K in zip(kw["Ts"], bb.TRANSCRIPT_K["transcript"]))
    assert [len(p) for p in bb.transcript_phones("transcript")] == bb.TRANSCRIPT_K["transcript"]
    assert bb.array_bytes("transcript")["cells"] == 8 * (270 * 1100 * 1030 + 240 * 1090 * 1020)
    assert bb.need_bytes("transcript") < 16 << 30
    # N-best: nfr * 48 * 64 * 4 bytes per back-pointer array pass 2^32 once nfr > 349,526; the lists fit a workgroup's LDS
    kw, N = bb.CASES["nbest"]["kw"], bb.NBEST_N["nbest"]
    nf = bb.case_sizes("nbest")[1]
    assert nf > bb.MARGIN * 349526 and bb.array_bytes("nbest")["bp"] == nf * 48 * 64 * 4
    assert (kw["D"] + 2) * kw["L"] * N * 4 + 16 * 48 * 2 <= 160 * 1024
    assert bb.need_bytes("nbest") >= 2 * bb.array_bytes("nbest")["bp"] and bb.need_bytes("nbest") < 32 << 30


def test_axis_b_passes_the_utterance_caps():
    n = sum(bb.MANY_COUNTS)
    assert n == 70000 and len(set(bb.MANY_COUNTS)) == 4
    assert n >= bb.MARGIN * bb.PLAN_CHUNK_CAP and n < 2 * bb.PLAN_CHUNK_CAP      # exactly two chunks of plan_chunk
    assert n >= 2 * bb.MARGIN * bb.SL_CHUNK_CAP                                   # at least three of the STDSEG linear path
    assert -(-n // bb.PLAN_CHUNK_CAP) == 2 and -(-n // bb.SL_CHUNK_CAP) == 3
