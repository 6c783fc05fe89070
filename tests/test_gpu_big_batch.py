"""-m gpu: batches of the size the engine is built for -- arrays past 2^32 bytes inside one chunk (axis A) and more utterances
than the chunk caps (axis B) -- against the CPU oracle.  Every batch is a few base utterances repeated many times
(tests/big_batch.py), so the expected gradient is sum_i counts[i] * g_i of the per-utterance oracle gradients and the
expected numerator, Zx, best path, N best paths, alignment, transcript score, posteriors and pruned arcs of every copy are those of its base utterance.
tests/test_big_batch.py (no GPU) asserts that each shape here crosses the byte size and the plan breakpoints it is there for.

Bounds, all taken from the suite and none measured on the code under test: gradient relative to max |g| 1e-9 EXACT / FAST,
1e-6 FASTLIN, 1e-5 FAST32 (tests/test_gpu_parity.py); Zx of every copy, relative, 1e-11 EXACT / FAST, 1e-8 FASTLIN, 1e-6
FAST32 (tests/test_gpu_score_staging.py, which holds the numerator to no bound of its own); the numerator of every copy,
relative to max(1, |numerator|), 1e-11 EXACT / FAST, 1e-6 FASTLIN, 1e-5 FAST32 (tests/test_gpu_input_ranges.py, and for
FASTLIN tests/test_gpu_parity.py::test_fb_batch_gradient_fastlin_precision: that tier takes the window average as the
exact mean where the oracle rounds it to float, which moves the labelled path's score by a few 1e-8 at any batch size);
posteriors 1e-9 / 1e-6 / 1e-5 absolute (tests/test_gpu_posteriors.py; transcript scoring against form 1 of tests/transcript_ref.py at the
same bounds, tests/test_gpu_transcript.py); best paths, alignments and pruned arcs bit for bit.  Position must not matter: all copies of a base utterance agree with its
first copy bit for bit where the path is deterministic per utterance (EXACT scalars, every decode output) and within 1e-12
relative on the FAST tiers (the cross-chunking bound of tests/test_gpu_parity.py:516); each test prints whether the FAST
tiers held bit for bit too.  A second fb_batch under the tiny scratch budget of the existing chunked tests (1 << 16) must
give the same scalars and the same gradient within rtol 1e-9 + 1e-10 max |g| (tests/test_gpu_parity.py:518): that run has
one chunk per utterance or a few, and large chunk-relative offsets at the far end of the batch.

The single chunk of axis A and the chunk counts of axis B are asserted from launch counts, as in
tests/test_gpu_chunk_plan.py.  Before an engine is created the card's free memory is checked against the case's computed
need; too little is a failure that names the need, not a skip.

Out of scope: more than 2^31 elements in one array (17 GB arrays; the benchmark's 1.4e9 elements stay below it), the 32-bit
entry-position cap of the sparse maps (plan_chunk: nseg * (F / 2) > 0xffffffff needs tens of GB of host windows), and more
than 2^31 frames."""
import numpy as np
import pytest

import align_ref as ar
import big_batch as bb
import family_shapes as fs
import latprune_ref as lr
import nbest_ref as nr
import orc
import post_ref
import scrf_amd
import transcript_ref as tref
from big_batch import EXACT, FAST, FAST32, FASTLIN, PREC_NAME

pytestmark = pytest.mark.gpu

ONE_CHUNK = 96 << 30      # scratch budget (only what a chunk needs is allocated)
TINY = 1 << 16            # tests/test_gpu_parity.py::test_chunking_is_invisible
SMALL_CELLS = 1 << 30     # transcript scoring on 1100-frame utterances: the cells of one utterance take 18 MB and a workgroup per
                          # utterance walks its frames one after the other, so a chunk per utterance would run 510 sweeps
                          # back to back; this budget holds a few dozen utterances per chunk
TINY_FUSED = 1 << 21      # the fused path's count slabs alone pass 1 << 16: the first rung of its ladder in
                          # tests/test_gpu_chunk_plan.py that holds more than one (short) utterance per chunk
GRAD_TOL = {EXACT: 1e-9, FAST: 1e-9, FASTLIN: 1e-6, FAST32: 1e-5}
ZX_TOL = {EXACT: 1e-11, FAST: 1e-11, FASTLIN: 1e-8, FAST32: 1e-6}
NUMER_TOL = {EXACT: 1e-11, FAST: 1e-11, FASTLIN: 1e-6, FAST32: 1e-5}
POST_TOL = {EXACT: 1e-9, FAST: 1e-9, FASTLIN: 1e-6, FAST32: 1e-5}
POSITION_TOL = 1e-12
RECURSIONS = ("k_dp_lin", "k_dp_lin_mw", "k_dp_wave", "k_fb", "k_fb_segtrans", "k_stdseg_fb", "k_sl_fb", "k_ns_fb")


class Ref:
    """a base case, its per-utterance oracle results (computed on first use, then left unchanged)"""

    def __init__(self, row_or_kw):
        self.case = bb.make_case(row_or_kw)
        self.exp = bb.Expected(self.case)
        self._utts = self._post = self._lat = None
        self._nbest = {}

    def utts(self):
        """per base utterance (arcs, n_states, final, best labels, best cost)"""
        if self._utts is None:
            self._utts = []
            for u in range(len(self.case.Ts)):
                S, M, arcs, ns, fin = fs.oracle_utterance(self.case, u)
                labs, cost = orc.best_path(arcs, ns, fin)
                arcs.flags.writeable = False
                self._utts.append((arcs, ns, fin, labs, cost))
        return self._utts

    def posteriors(self):
        if self._post is None:
            self._post = [post_ref.utterance(self.case, u) for u in range(len(self.case.Ts))]
        return self._post

    def nbest(self, N):
        """per base utterance ((labels, cost), ..) of the N-best reference"""
        if N not in self._nbest:
            self._nbest[N] = [[(tuple(p), c) for p, c in nr.nbest(ar.case_weights(self.case, u), N)] for u in range(len(self.case.Ts))]
        return self._nbest[N]

    def pruned(self, beam):
        """per base utterance (kept arcs, fp64 cost of the best path) under the beam"""
        out = []
        for arcs, ns, fin, _, _ in self.utts():
            fwd, bwd = lr.distances(arcs, ns, fin)
            out.append((arcs[lr.keep_mask(arcs, fwd, bwd, fin, beam)], fwd[fin]))
        return out


@pytest.fixture(scope="module")
def refs():
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = Ref(bb.CASES[name] if name in bb.CASES else bb.MANY[name[5:]])
        return cache[name]
    return get


def require_memory(name, need):
    import torch
    free, total = torch.cuda.mem_get_info()
    if free < need:
        pytest.fail("%s needs %.1f GB of device memory in one chunk; %.1f GB of %.1f GB are free" % (name, need / 1e9, free / 1e9, total / 1e9))


def fb_chunks(eng):
    got = {name: n for name, _, n in eng.kernel_timing() if name in RECURSIONS}
    assert got, eng.kernel_timing()
    return sum(got.values()), got


def check_scalars(what, t, ref, prec, numer, zx):
    on, oz = ref.exp.numer[t.base], ref.exp.zx[t.base]
    en = np.abs(numer - on).max() / max(1.0, np.abs(on).max())
    ez = np.abs(zx - oz).max() / np.abs(oz).max()
    k = len(t.counts)
    same_n, rel_n = bb.copies_vs_first(numer, t.base, k)
    same_z, rel_z = bb.copies_vs_first(zx, t.base, k)
    print("%s: numer vs oracle %.2e (bound %.0e), Zx vs oracle %.2e (bound %.0e); copies vs first copy: %s (numer %.1e, Zx %.1e)"
          % (what, en, NUMER_TOL[prec], ez, ZX_TOL[prec], "bit for bit" if same_n and same_z else "NOT bit for bit", rel_n, rel_z))
    assert en <= NUMER_TOL[prec] and ez <= ZX_TOL[prec], (what, en, ez)
    if prec == EXACT:
        assert same_n and same_z, (what, rel_n, rel_z)
    else:
        assert rel_n <= POSITION_TOL and rel_z <= POSITION_TOL, (what, rel_n, rel_z)


def run_fb(what, t, ref, prec, chunks=1, mode=None, tiny=TINY, need=0):
    """one fb_batch in `chunks` chunks (asserted) against the tiled oracle results, then the same batch under the tiny budget"""
    require_memory(what, need)
    og = ref.exp.gradient(t.counts)
    eng = t.engine(prec, ONE_CHUNK); b = t.batch(eng)
    try:
        if mode is not None:
            assert eng.batch_fused_mode(b) == mode, (what, eng.batch_fused_mode(b))
        eng.enable_timing(True)
        numer, zx = eng.fb_batch(b)
        g = eng.get_grad()
        n, by = fb_chunks(eng)
        err = np.abs(g - og).max() / np.abs(og).max()
        print("%s %s: %d utterances, %d chunk(s) %s, gradient vs sum counts * g_i %.2e (bound %.0e), redone in the log domain %d"
              % (what, PREC_NAME[prec], len(t.base), n, by, err, GRAD_TOL[prec], eng.train_stats()))
        assert (n >= -chunks) if chunks < 0 else (n == chunks), (what, n, by)
        assert err <= GRAD_TOL[prec], (what, err)
        check_scalars("%s %s" % (what, PREC_NAME[prec]), t, ref, prec, numer, zx)
        assert eng.train_stats() == 0
    finally:
        b.close(); eng.close()
    if not tiny:
        return
    eng = t.engine(prec, tiny); b = t.batch(eng)
    try:
        eng.enable_timing(True)
        n2, z2 = eng.fb_batch(b)
        g2 = eng.get_grad()
        nc, by = fb_chunks(eng)
        dn = np.abs(n2 - numer).max() / max(1.0, np.abs(numer).max()); dz = np.abs(z2 - zx).max() / np.abs(zx).max()
        dg = np.abs(g2 - g).max() / np.abs(g).max()
        print("%s %s under %d bytes of scratch: %d chunks, scalars vs the one-chunk run %.1e / %.1e, gradient %.2e"
              % (what, PREC_NAME[prec], tiny, nc, dn, dz, dg))
        assert nc > max(1, abs(chunks)), (what, nc)
        if prec == EXACT:
            assert np.array_equal(n2, numer) and np.array_equal(z2, zx)
        else:
            assert dn <= POSITION_TOL and dz <= POSITION_TOL, (what, dn, dz)
        np.testing.assert_allclose(g2, g, rtol=1e-9, atol=1e-10 * np.abs(g).max())
    finally:
        b.close(); eng.close()


def check_viterbi(what, t, ref, eng, b, chunks=1):
    """best paths of every copy: equal to the first copy's bit for bit, the first copy's equal to the oracle's; returns them"""
    eng.enable_timing(True)
    labs, cost = eng.viterbi_batch(b)
    fast = any(name == "k_scores_fused(decode)" for name, _, _ in eng.kernel_timing())
    nv = eng.last_timing()["viterbi"][1]
    n = nv // 2 if fast else nv
    same_l, _ = bb.blocks_vs_first(labs.flat, labs.off, t.base, len(t.counts))
    same_c, _ = bb.copies_vs_first(cost, t.base, len(t.counts))
    print("%s viterbi_batch: %d chunk(s) (%s decode), fixups %s; copies vs first copy: labels %s, costs %s"
          % (what, n, "fast" if fast else "exact", eng.decode_stats(), same_l, same_c))
    assert n == chunks, (what, nv, fast)
    assert same_l and same_c, what
    for i, (arcs, ns, fin, ol, oc) in enumerate(ref.utts()):
        u = int(t.first[i])
        assert list(labs[u]) == list(ol) and np.float32(cost[u]).tobytes() == np.float32(oc).tobytes(), (what, i)
    eng.enable_timing(False)
    return labs, cost


def check_posteriors(what, t, ref, eng, b, prec, chunks=1):
    s0 = sum(eng.posterior_stats())
    eng.enable_timing(True)
    out = eng.posteriors_batch(b)
    n = sum(eng.posterior_stats()) - s0 + sum(k for name, _, k in eng.kernel_timing() if name == "k_dp_wave")
    eng.enable_timing(False)
    off = t.frame_off()
    k = len(t.counts)
    same_f, dev_f = bb.blocks_vs_first(out["frame_flat"], off, t.base, k)
    same_e, dev_e = bb.blocks_vs_first(out["end_flat"], off, t.base, k)
    same_z, rel_z = bb.copies_vs_first(out["zx"], t.base, k)
    dev = 0.0
    for i, (g, occ, end, zx) in enumerate(ref.posteriors()):
        u = int(t.first[i])
        dev = max(dev, np.abs(out["frame"][u] - occ).max(), np.abs(out["end"][u] - end).max())
        assert abs(out["zx"][u] - zx) <= max(1e-11, POST_TOL[prec] * 1e-2) * max(1, abs(zx))
    print("%s posteriors_batch %s: %d chunk(s), vs oracle %.2e (bound %.0e); copies vs first copy: %s (frame %.1e, end %.1e, Zx %.1e)"
          % (what, PREC_NAME[prec], n, dev, POST_TOL[prec], "bit for bit" if same_f and same_e and same_z else "NOT bit for bit", dev_f, dev_e, rel_z))
    assert n == chunks, (what, n)
    assert dev <= POST_TOL[prec], (what, dev)
    if prec == EXACT:
        assert same_f and same_e and same_z
    else:   # values in [0, 1]: absolute
        assert dev_f <= POSITION_TOL and dev_e <= POSITION_TOL and rel_z <= POSITION_TOL, (what, dev_f, dev_e, rel_z)


def check_align(what, t, ref, eng, b, labs, chunks=1):
    """every copy aligned against the phones of its own best path, one segment per phone"""
    L = ref.case.ocfg.num_labs
    tr = scrf_amd.RaggedLabels((np.asarray(labs.flat) % L).astype(np.uint32), labs.off)
    s0 = eng.align_stats()[1]
    al, cost = eng.align_batch(b, tr, scrf_amd.ALIGN_ONE)
    n = eng.align_stats()[1] - s0
    same_l, _ = bb.blocks_vs_first(al.flat, al.off, t.base, len(t.counts))
    same_c, _ = bb.copies_vs_first(cost, t.base, len(t.counts))
    print("%s align_batch: %d search(es); copies vs first copy: labels %s, costs %s" % (what, n, same_l, same_c))
    assert n == chunks, (what, n)
    assert same_l and same_c, what
    for i in range(len(t.counts)):
        u = int(t.first[i])
        want_l, want_c = ar.dp(ar.case_weights(ref.case, i), tr[u], scrf_amd.ALIGN_ONE)
        assert [int(x) for x in al[u]] == want_l and np.float32(cost[u]).tobytes() == np.float32(want_c).tobytes(), (what, i)


def check_nbest(what, t, ref, eng, b, N, chunks=1):
    """the N best paths of every copy: labels, label counts and costs equal to the first copy's bit for bit, the first copy's
    equal to tests/nbest_ref.py on the base utterance"""
    s0 = eng.nbest_stats()
    labs, hoff, cost = eng.nbest_batch(b, N)
    s1 = eng.nbest_stats()
    n, k = s1[1] - s0[1], len(t.counts)
    hoff = np.asarray(hoff).astype(np.int64)
    loff = np.asarray(labs.off).astype(np.int64)
    same_l, _ = bb.blocks_vs_first(labs.flat, loff[hoff], t.base, k)
    same_n, _ = bb.blocks_vs_first(np.diff(loff), hoff, t.base, k)
    same_c, _ = bb.blocks_vs_first(cost, hoff, t.base, k)
    print("%s nbest_batch N = %d: %d chunk(s) (%d on fast-decode weights), %d hypotheses, %d labels; copies vs first copy: labels %s, lengths %s, costs %s"
          % (what, N, n, s1[2] - s0[2], int(hoff[-1]), int(loff[hoff[-1]]), same_l, same_n, same_c))
    assert s1[0] == s0[0] + 1 and n == chunks, (what, s0, s1)
    assert same_l and same_n and same_c, what
    for i, want in enumerate(ref.nbest(N)):
        u = int(t.first[i])
        h0, h1 = int(hoff[u]), int(hoff[u + 1])
        assert h1 - h0 == len(want), (what, i, h1 - h0, len(want))
        for r, (wl, wc) in enumerate(want):
            assert np.float32(cost[h0 + r]).tobytes() == np.float32(wc).tobytes(), (what, i, r, cost[h0 + r], wc)
            assert tuple(int(x) for x in labs[h0 + r]) == wl, (what, i, r)
    return n, s1[2] - s0[2]


def check_transcript(what, t, ref, eng, b, transcripts, prec, chunks=1):
    """every copy scored against its transcript (SCRF_ALIGN_ONE): equal to the first copy's bit for bit (zx, which the free
    recursion supplies, and logp within the position bound on the FAST tiers), the first copy's equal to form 1 of
    tests/transcript_ref.py on the oracle's scores within the tier's bound; returns the output"""
    c0, k0, r0 = eng.transcript_stats()
    out = eng.transcript_batch(b, transcripts, scrf_amd.ALIGN_ONE)
    c1, k1, r1 = eng.transcript_stats()
    n, k = k1 - k0, len(t.counts)
    off = t.frame_off()
    same_a, _ = bb.copies_vs_first(out["log_num"], t.base, k)
    same_f, _ = bb.blocks_vs_first(out["frame_flat"], off, t.base, k)
    same_e, _ = bb.blocks_vs_first(out["end_flat"], off, t.base, k)
    same_z, rel_z = bb.copies_vs_first(out["zx"], t.base, k)
    same_p, rel_p = bb.copies_vs_first(out["logp"], t.base, k)
    dev = 0.0
    for i in range(k):
        u = int(t.first[i])
        r = tref.dp(tref.case_scores(ref.case, i), transcripts[u], scrf_amd.ALIGN_ONE)
        zx = ref.posteriors()[i][3]
        T = r.frame_post.shape[0]
        devs = [abs(out["zx"][u] - zx) / max(1.0, abs(zx)), abs(out["log_num"][u] - r.A) / max(1.0, abs(r.A)),
                abs(out["logp"][u] - (r.A - zx)) / max(1.0, abs(r.A - zx)), np.abs(out["frame"][u] - r.frame_post).max(),
                np.abs(out["end"][u] - r.end_post).max(), np.abs(out["frame"][u].sum(axis=1) - 1.0).max(), abs(out["end"][u][T - 1] - 1.0)]
        assert np.isfinite(r.A) and max(devs) <= POST_TOL[prec], (what, i, devs)
        dev = max(dev, max(devs))
    print("%s transcript_batch %s: %d chunk(s), redone %d, vs form 1 %.2e (bound %.0e); copies vs first copy: log_num %s, frame %s, end %s, Zx %s (%.1e), logp %s (%.1e)"
          % (what, PREC_NAME[prec], n, r1 - r0, dev, POST_TOL[prec], same_a, same_f, same_e, same_z, rel_z, same_p, rel_p))
    assert c1 == c0 + 1 and r1 == r0, (what, c1 - c0, r1 - r0)
    assert (n > -chunks) if chunks < 0 else (n == chunks), (what, n)
    assert same_a and same_f and same_e, what
    if prec == EXACT:
        assert same_z and same_p, what
    else:
        assert rel_z <= POSITION_TOL and rel_p <= POSITION_TOL, (what, rel_z, rel_p)
    return out


def best_path_phones(labs, L):
    return scrf_amd.RaggedLabels((np.asarray(labs.flat) % L).astype(np.uint32), labs.off)


def check_pruned(what, t, ref, eng, b, beam, chunks=1, fetch_all=True):
    s0 = eng.lattice_prune_stats()[1]
    off, best = eng.lattice_prune_batch(b, beam)
    n = eng.lattice_prune_stats()[1] - s0
    k = len(t.counts)
    want = ref.pruned(beam)
    cnt = np.diff(off.astype(np.int64))
    same_n, _ = bb.copies_vs_first(cnt, t.base, k)
    same_b, _ = bb.copies_vs_first(best, t.base, k)
    same_a = None
    if fetch_all:
        same_a, _ = bb.blocks_vs_first(eng.pruned_arcs(b), off, t.base, k)
    print("%s lattice_prune_batch beam %g: %d chunk(s), %d arcs (%.3f x 2^32 bytes); copies vs first copy: counts %s, costs %s, arcs %s"
          % (what, beam, n, int(off[-1]), int(off[-1]) * 20 / bb.TWO32, same_n, same_b, same_a))
    assert n == chunks, (what, n)
    assert same_n and same_b and same_a in (None, True), what
    for i, (arcs, cost) in enumerate(want):
        for u in (int(t.first[i]), int(t.last[i])):      # the last copy sits at the far end of the arc array
            got = eng.pruned_arcs(b, u, 1)
            assert got.tobytes() == arcs.tobytes(), (what, i, u)
            assert np.float64(best[u]).tobytes() == np.float64(cost).tobytes(), (what, i, u)
    return int(off[-1])


def tiled_of(refs, name):
    ref = refs(name)
    return ref, bb.Tiled(ref.case, bb.CASES[name]["counts"])


# ---- axis A: one chunk whose arrays pass 2^32 bytes -------------------------------------------------------------------
@pytest.mark.parametrize("prec", [FAST, FASTLIN, FAST32])
def test_fused_training_pass_with_scores_past_4_gib(prec, refs):
    """L = 48, D = 25, 1970 utterances: S [nseg][48] fp64 is 4.60e9 bytes (1.07 x 2^32); nseg = 11,968,900 > 4096 * 1024 (the count
    contraction's rows per chunk grow to 11712) and nfr = 502,090 > 262,144 (the transition-bias contraction's rows per
    chunk grow to 124); the count kernel walks its tiles with the default cap of 512 workgroups."""
    ref, t = tiled_of(refs, "fused")
    run_fb("fused", t, ref, prec, mode=2 if prec == FASTLIN else 1, tiny=TINY if prec == FAST else 0, need=bb.need_bytes("fused"))


def test_fused_decode_and_posteriors_past_4_gib(refs):
    ref, t = tiled_of(refs, "fused")
    require_memory("fused", bb.need_bytes("fused"))
    eng = t.engine(FAST, ONE_CHUNK); b = t.batch(eng, with_labels=False)
    try:
        check_viterbi("fused", t, ref, eng, b)
        assert eng.decode_stats()[1] == 0       # the fast decode ran; no chunk went back to the EXACT path
        check_posteriors("fused", t, ref, eng, b, FAST)
    finally:
        b.close(); eng.close()


def test_general_path_with_scores_and_windows_past_4_gib(refs, monkeypatch):
    """EXACT, in_w = 9 (F = 97): the materialised windows X [nseg][97] float are 4.64e9 bytes and S 4.60e9 bytes, both past 2^32
    in one chunk."""
    monkeypatch.setenv("SCRF_FAST_DECODE", "0")     # read by scrf_create: viterbi_batch through the EXACT scores
    ref, t = tiled_of(refs, "general")
    need = bb.need_bytes("general")
    run_fb("general", t, ref, EXACT, need=need)
    eng = t.engine(EXACT, ONE_CHUNK); b = t.batch(eng, with_labels=False)
    try:
        labs, _ = check_viterbi("general", t, ref, eng, b)
        check_align("general", t, ref, eng, b, labs)
        check_transcript("general", t, ref, eng, b, best_path_phones(labs, ref.case.ocfg.num_labs), EXACT)
    finally:
        b.close(); eng.close()


@pytest.mark.parametrize("prec", [FAST, FASTLIN])
def test_mixed_path_with_transition_scores_past_4_gib(prec, refs):
    """L = 48, D = 10, a second stream of boundary context, 1100 utterances: M [nfr][48 * 48] fp64 is 5.12e9 bytes (1.19 x 2^32),
    and so are E, ET and XI.  (The transition-BIAS contraction and its atb_rows_per_chunk plan do not run with transition
    features; the fused case crosses that breakpoint.  Here nfr = 278,030 puts transframe_chunks past its base.)"""
    ref, t = tiled_of(refs, "mixed")
    run_fb("mixed", t, ref, prec, tiny=TINY if prec == FAST else 0, need=bb.need_bytes("mixed"))
    if prec == FAST:
        eng = t.engine(FAST, ONE_CHUNK); b = t.batch(eng, with_labels=False)
        try:
            check_posteriors("mixed", t, ref, eng, b, FAST)
        finally:
            b.close(); eng.close()


def test_hybrid_path_with_windows_past_4_gib(refs):
    """L = 65, D = 5, in_w = 70, 4200 utterances: the compact materialised rows X [nseg][216] float are 4.62e9 bytes."""
    ref, t = tiled_of(refs, "hybrid")
    run_fb("hybrid", t, ref, FAST, mode=3, need=bb.need_bytes("hybrid"))


def test_stdseg_linear_path_past_its_plan_breakpoint(refs):
    """nfr = 201,450 > 16,384: sl_rows_per_chunk grows to 800.  The D * nfr * La arrays are 32 MB here: 2^32 bytes would take
    26.8 M frames of this shape (La = 4, D = 5) inside the 32767 utterances of one chunk, which no longer runs in seconds."""
    ref, t = tiled_of(refs, "stdseg_lin")
    run_fb("stdseg_lin", t, ref, FAST, need=bb.need_bytes("stdseg_lin"))


@pytest.mark.parametrize("name", ["stdseg", "segtrans", "nstate", "frame"])
def test_other_exact_paths_on_long_tiled_batches(name, refs):
    """The family shapes on utterances of 300, 257, 40 and 7 frames, 85 .. 850 copies.  Their largest arrays (printed by
    tests/test_big_batch.py: 14 .. 58 MB) stay far below 2^32 bytes, which these narrow shapes would reach only at tens of
    millions of frames; what they cross is hundreds of thousands of frames and chunk-relative offsets in one chunk."""
    ref, t = tiled_of(refs, name)
    run_fb(name, t, ref, EXACT, need=bb.need_bytes(name))


def test_kept_arc_array_past_4_gib(refs):
    """beam 1e30 keeps every arc: 268 utterances, 234,308,448 arcs of 20 bytes = 4.69e9 bytes (1.09 x 2^32).  Only the first
    and the last copy of each base utterance are fetched."""
    ref, t = tiled_of(refs, "latprune")
    require_memory("latprune", bb.need_bytes("latprune") + 2 * bb.array_bytes("latprune")["arcs"])
    eng = t.engine(EXACT, ONE_CHUNK); b = t.batch(eng, with_labels=False)
    try:
        n = check_pruned("latprune", t, ref, eng, b, 1e30, fetch_all=False)
        assert n * 20 == bb.array_bytes("latprune")["arcs"]
    finally:
        b.close(); eng.close()


def test_transcript_cells_past_4_gib(refs):
    """L = 2, D = 2, 510 utterances of 1100 / 1090 frames with transcripts of 1030 / 1020 phones: aB and bE, [sum T K] fp64 each,
    are 4.58e9 bytes (1.07 x 2^32) apiece in one chunk, every workgroup strides 1024 threads over its positions, and the
    cells of the last utterances sit past 2^32 bytes from the chunk's first.  Then the same call under a budget of a tenth of
    that (SMALL_CELLS): several chunks, the same bytes."""
    ref, t = tiled_of(refs, "transcript")
    require_memory("transcript", bb.need_bytes("transcript"))
    phones = bb.transcript_phones("transcript")
    ts = [phones[i] for i in t.base]
    keys = ("log_num", "zx", "logp", "frame_flat", "end_flat")
    eng = t.engine(FAST, ONE_CHUNK); b = t.batch(eng, with_labels=False)
    try:
        one = check_transcript("transcript", t, ref, eng, b, ts, FAST)
    finally:
        b.close(); eng.close()
    eng = t.engine(FAST, SMALL_CELLS); b = t.batch(eng, with_labels=False)
    try:
        many = check_transcript("transcript under %d bytes of scratch" % SMALL_CELLS, t, ref, eng, b, ts, FAST, chunks=-4)
        for k in keys:
            assert np.array_equal(many[k].view(np.uint64), one[k].view(np.uint64)), k
    finally:
        b.close(); eng.close()


def test_nbest_back_pointers_past_4_gib(refs, monkeypatch):
    """L = 48, D = 2, N = 64, 1500 utterances, 371,840 frames: bp_b and bp_e, [nfr][48][64] 32-bit words each, are 4.57e9 bytes
    (1.06 x 2^32) apiece in one chunk; the back pointers of the last utterances sit past 2^32 bytes from the chunk's first."""
    monkeypatch.setenv("SCRF_FAST_DECODE", "0")
    ref, t = tiled_of(refs, "nbest")
    N = bb.NBEST_N["nbest"]
    print("nbest: bp_b = bp_e = %d bytes (%.3f x 2^32)" % (bb.array_bytes("nbest")["bp"], bb.array_bytes("nbest")["bp"] / bb.TWO32))
    require_memory("nbest", bb.need_bytes("nbest"))
    eng = t.engine(EXACT, ONE_CHUNK); b = t.batch(eng, with_labels=False)
    try:
        check_nbest("nbest", t, ref, eng, b, N, chunks=1)
    finally:
        b.close(); eng.close()


# ---- axis B: more utterances than the chunk caps ----------------------------------------------------------------------
def many_of(refs, name):
    ref = refs("many_" + name)
    return ref, bb.Tiled(ref.case, bb.MANY_COUNTS)


@pytest.mark.parametrize("prec", [EXACT, FAST, FASTLIN, FAST32])
@pytest.mark.parametrize("name", ["bias", "ctx"])
def test_70000_utterances_training_pass(name, prec, refs):
    """plan_chunk cuts at 65535 utterances: exactly two chunks under a budget that would hold all of them"""
    ref, t = many_of(refs, name)
    run_fb("70000 " + name, t, ref, prec, chunks=2, tiny={EXACT: TINY, FAST: TINY_FUSED}.get(prec, 0))


@pytest.mark.parametrize("name", ["bias", "ctx"])
def test_70000_utterances_decode_outputs(name, refs, monkeypatch):
    ref, t = many_of(refs, name)
    for fast_decode in ("1", "0"):
        monkeypatch.setenv("SCRF_FAST_DECODE", fast_decode)
        eng = t.engine(EXACT, ONE_CHUNK); b = t.batch(eng, with_labels=False)
        try:
            what = "70000 %s (SCRF_FAST_DECODE=%s)" % (name, fast_decode)
            labs, _ = check_viterbi(what, t, ref, eng, b, chunks=2)
            check_nbest(what, t, ref, eng, b, 3, chunks=2)     # 65,535 * 3 scan entries in the larger chunk
            if fast_decode == "1":
                continue
            check_align(what, t, ref, eng, b, labs, chunks=2)
            check_transcript(what, t, ref, eng, b, best_path_phones(labs, ref.case.ocfg.num_labs), EXACT, chunks=2)
            check_posteriors(what, t, ref, eng, b, EXACT, chunks=2)
            check_pruned(what, t, ref, eng, b, 2.0, chunks=2)
        finally:
            b.close(); eng.close()
    eng = t.engine(FAST, ONE_CHUNK); b = t.batch(eng, with_labels=False)
    try:
        check_posteriors("70000 " + name, t, ref, eng, b, FAST, chunks=2)
    finally:
        b.close(); eng.close()


def test_70000_utterances_stdseg_linear_path(refs):
    """the STDSEG linear path cuts at 32767 utterances: at least three chunks"""
    ref, t = many_of(refs, "stdseg")
    run_fb("70000 stdseg_lin", t, ref, FAST, chunks=-3, tiny=1 << 20)


@pytest.mark.parametrize("name", ["stdseg", "nstate"])
def test_70000_utterances_uncapped_chunkers(name, refs):
    """stdseg_plan_chunk (general form) and nstate_plan_chunk have no utterance cap: one chunk of 70000.  Every kernel behind
    them puts the utterance count into grid.x alone (limit 2^31 - 1), never into grid.y or grid.z, so none is needed."""
    ref, t = many_of(refs, name)
    run_fb("70000 " + name, t, ref, EXACT, chunks=1)
