"""-m gpu: where the chunk planners cut.  Every chunked path has a test that compares a chunked run with the one-chunk
run (test_chunking_is_invisible and its siblings); none of them sees whether the cuts moved.  Here one small case per
path runs under a ladder of scratch budgets and the vector of chunk counts must equal a recorded table: a scratch layout
whose size changes by a byte that matters moves a cut on some rung.

The counts are read from what the engine already reports: with timing enabled every path launches its recursion kernel
once per chunk (kernel_timing), the posterior walk counts one launch per linear-domain chunk (posterior_stats), the
lattice beam counts its chunks (lattice_prune_stats), and the Viterbi phase of last_timing counts one launch per exact
chunk.  Timing mode turns the two-lane split off, so the planner alone decides the counts."""
import numpy as np
import pytest

import latprune_ref as lr
import orc
import scrf_amd
import sparse_ref as sr
from cases import Case

pytestmark = pytest.mark.gpu

LADDER = tuple(1 << k for k in range(14, 22))


def launches(eng, kernel):
    return sum(n for name, _, n in eng.kernel_timing() if name == kernel)


def fb_chunks(c, kernel):
    """launches of `kernel` in one timed fb_batch of case c"""
    eng = c.engine(); b = c.batch(eng)
    eng.enable_timing(True)
    eng.fb_batch(b, want_scalars=False)
    n = launches(eng, kernel)
    b.close(); eng.close()
    return n


class NCase:
    """the n-state frame case of tests/test_gpu_nstate.py (copied: test modules are not imported)"""

    def __init__(self, P, K, F, Ts, seed=0, scratch_bytes=0):
        rng = np.random.RandomState(seed)
        self.frames = [rng.random_sample((T, F)).astype(np.float32) for T in Ts]
        kw = dict(model_type=orc.STDFRAME, L=P * K, D=1, F=F, use_trans_ftrs=True, tfs=0, tfe=F - 1, num_states=K)
        self.gcfg = scrf_amd.make_config(scratch_bytes=scratch_bytes, **kw)
        self.lam = rng.normal(0, 0.3, orc.Layout(orc.config(**kw)).lambda_len)
        self.labels = []
        for T in Ts:   # sequences the topology allows
            labs = np.zeros(T, dtype=np.uint32)
            c = int(rng.randint(0, P * K))
            for t in range(T):
                labs[t] = c
                if rng.rand() >= 0.4:
                    c = int(rng.randint(0, P)) * K if (c + 1) % K == 0 else c + 1
            self.labels.append(labs)
        self.recipes = [scrf_amd.StreamRecipe(F, 0, 0, 0)]

    def engine(self):
        e = scrf_amd.Engine(self.gcfg); e.set_lambda(self.lam); return e

    def batch(self, eng):
        return eng.batch_from_frames(self.frames, self.labels, self.recipes, None)


class SCase:
    """the segmental sparse case of tests/test_gpu_sparse.py over resident windows (copied likewise)"""

    def __init__(self, use_tf, Ts, scratch_bytes=0, L=5, N=40, P=6, D=4, seed=3):
        rng = np.random.RandomState(seed)
        self.Ts = list(Ts)
        lay = sr.SparseLayout(L, sfe=N - 1, tfe=N - 1, use_tf=use_tf)
        self.X = [sr.random_windows(rng, orc.num_segs(T, D), P, N, messy=True) for T in Ts]
        self.labels = [orc.group_labels(rng.randint(0, L, T).astype(np.uint32), D, L) for T in Ts]
        self.lam = rng.uniform(-0.5, 0.5, lay.lambda_len)
        self.cfg = scrf_amd.make_config(model_type=scrf_amd.STDSEG_NO_DUR_NO_SEGTRANSFTR, L=L, D=D, F=2 * P, sfe=N - 1, tfe=N - 1,
                                        use_trans_ftrs=use_tf, sparse=True, scratch_bytes=scratch_bytes,
                                        state_bias_val=2.5, trans_bias_val=0.5)

    def engine(self):
        e = scrf_amd.Engine(self.cfg); e.set_lambda(self.lam); return e

    def batch(self, eng):
        return eng.batch_from_windows(self.X, self.Ts, self.labels)


GENERAL = dict(L=5, D=4, in_w=3, Ts=[6, 9, 4, 12, 7], trans_ctx=1, seed=11)
FUSED = dict(L=6, D=5, in_w=4, Ts=[1, 2, 4, 5, 6, 9, 17, 30, 3, 12], seed=41)
HYBRID = dict(L=66, D=4, in_w=69, Ts=[9, 14, 3, 1, 11, 8], lam_scale=0.05, seed=5, precision=scrf_amd.PREC_FAST)
SEGTRANS = dict(L=4, D=3, in_w=3, Ts=[6, 9, 4, 12, 7], trans_share=(0, 26), seed=31, model_type=orc.STDSEG_NO_DUR)
STDSEG = dict(L=3, D=3, in_w=2, Ts=[5, 7, 3, 9, 4, 8], model_type=orc.STDSEG)
NSTATE = dict(P=3, K=2, F=3, Ts=[5, 7, 3, 9, 4, 8], seed=9)
SPARSE_TS = [9, 14, 6, 11, 3, 17, 8, 12]
LATTICE = dict(lr.GPU_SHAPES[5], seed=605)


def with_ts(kw, Ts, **more):
    return dict(kw, **more) if Ts is None else dict(kw, Ts=Ts, **more)


def posterior_chunks(kw, sb, Ts):
    """(linear-domain chunks, log-domain chunks) of one timed posteriors_batch"""
    c = Case(scratch_bytes=sb, **with_ts(kw, Ts))
    eng = c.engine(); b = c.batch(eng, with_labels=False)
    eng.enable_timing(True)
    eng.posteriors_batch(b)
    n = (sum(eng.posterior_stats()), launches(eng, "k_dp_wave"))
    b.close(); eng.close()
    return n


def lattice_chunks(sb, Ts):
    c = Case(scratch_bytes=sb, **with_ts(LATTICE, Ts))
    eng = c.engine(); b = c.batch(eng, with_labels=False)
    eng.lattice_prune_batch(b, lr.BEAMS[0])
    n = eng.lattice_prune_stats()[1]
    b.close(); eng.close()
    return n


def viterbi_chunks(sb, Ts):
    """exact chunks of one timed viterbi_batch (the caller turns the fast decode off)"""
    c = Case(scratch_bytes=sb, **with_ts(GENERAL, Ts))
    eng = c.engine(); b = c.batch(eng, with_labels=False)
    eng.enable_timing(True)
    eng.viterbi_batch(b)
    n = eng.last_timing()["viterbi"][1]
    b.close(); eng.close()
    return n


# path -> chunk count under scratch budget sb; Ts=None takes the path's own utterance list.  (The training pass runs the
# linear-domain recursion at SCRF_PREC_EXACT too: k_dp_lin is what fb_batch launches once per chunk on the general path;
# k_dp_wave is the label-less posterior pass at EXACT.)
PATHS = {
    "general_exact": lambda sb, Ts=None: fb_chunks(Case(scratch_bytes=sb, **with_ts(GENERAL, Ts)), "k_dp_lin"),
    "fused_fast": lambda sb, Ts=None: fb_chunks(Case(scratch_bytes=sb, precision=scrf_amd.PREC_FAST, **with_ts(FUSED, Ts)), "k_dp_lin"),
    "fused_fastlin": lambda sb, Ts=None: fb_chunks(Case(scratch_bytes=sb, precision=scrf_amd.PREC_FASTLIN, **with_ts(FUSED, Ts)), "k_dp_lin"),
    "hybrid": lambda sb, Ts=None: fb_chunks(Case(scratch_bytes=sb, **with_ts(HYBRID, Ts)), "k_dp_lin_mw"),
    "stdseg_no_dur": lambda sb, Ts=None: fb_chunks(Case(scratch_bytes=sb, **with_ts(SEGTRANS, Ts)), "k_fb_segtrans"),
    "stdseg_log": lambda sb, Ts=None: fb_chunks(Case(scratch_bytes=sb, seed=77, trans_share=(0, 1), **with_ts(STDSEG, Ts)), "k_stdseg_fb"),
    "stdseg_lin": lambda sb, Ts=None: fb_chunks(Case(scratch_bytes=sb, seed=78, precision=1, **with_ts(STDSEG, Ts)), "k_sl_fb"),
    "nstate": lambda sb, Ts=None: fb_chunks(NCase(scratch_bytes=sb, **with_ts(NSTATE, Ts)), "k_ns_fb"),
    "sparse": lambda sb, Ts=None: fb_chunks(SCase(False, Ts or SPARSE_TS, scratch_bytes=sb), "k_dp_lin"),
    "sparse_trans": lambda sb, Ts=None: fb_chunks(SCase(True, Ts or SPARSE_TS, scratch_bytes=sb), "k_dp_lin"),
    "posteriors_fast": lambda sb, Ts=None: posterior_chunks(dict(FUSED, precision=scrf_amd.PREC_FAST), sb, Ts)[0],
    "posteriors_exact": lambda sb, Ts=None: posterior_chunks(GENERAL, sb, Ts)[1],
    "lattice_beam": lambda sb, Ts=None: lattice_chunks(sb, Ts),
    "viterbi_exact": lambda sb, Ts=None: viterbi_chunks(sb, Ts),
}

# The utterance list each path starts from; a row of TABLE repeats it until the ladder moves the cuts.
BASE_TS = {"general_exact": GENERAL["Ts"], "fused_fast": FUSED["Ts"], "fused_fastlin": FUSED["Ts"], "hybrid": HYBRID["Ts"],
           "stdseg_no_dur": SEGTRANS["Ts"], "stdseg_log": STDSEG["Ts"], "stdseg_lin": STDSEG["Ts"], "nstate": NSTATE["Ts"],
           "sparse": SPARSE_TS, "sparse_trans": SPARSE_TS, "posteriors_fast": FUSED["Ts"], "posteriors_exact": GENERAL["Ts"],
           "lattice_beam": LATTICE["Ts"], "viterbi_exact": GENERAL["Ts"]}

# Recorded on the parent of the change that introduced this test (the change that derives every chunk's size from its
# carve).  A change that alters a scratch layout on purpose updates the rows it moves.
# path -> (repeats of the path's utterance list, k0 of the ladder 1 << k0 .. 1 << (k0 + 7), chunk counts along the ladder).
# The fused and hybrid paths carry fixed count slabs (1.3 MB and 100 MB here) that dwarf a short batch: their rows repeat
# the list and start the ladder higher until a rung gives an intermediate count.
TABLE = {
    "general_exact":    (1, 14, [5, 4, 2, 1, 1, 1, 1, 1]),
    "fused_fast":       (48, 20, [480, 5, 2, 1, 1, 1, 1, 1]),
    "fused_fastlin":    (48, 20, [480, 6, 2, 1, 1, 1, 1, 1]),
    "hybrid":           (96, 26, [576, 2, 1, 1, 1, 1, 1, 1]),
    "stdseg_no_dur":    (1, 14, [5, 3, 1, 1, 1, 1, 1, 1]),
    "stdseg_log":       (1, 14, [6, 3, 1, 1, 1, 1, 1, 1]),
    "stdseg_lin":       (4, 14, [12, 4, 2, 1, 1, 1, 1, 1]),
    "nstate":           (4, 14, [6, 3, 2, 1, 1, 1, 1, 1]),
    "sparse":           (1, 14, [8, 2, 1, 1, 1, 1, 1, 1]),
    "sparse_trans":     (1, 14, [8, 8, 3, 2, 1, 1, 1, 1]),
    "posteriors_fast":  (1, 14, [5, 4, 2, 1, 1, 1, 1, 1]),
    "posteriors_exact": (1, 14, [5, 3, 1, 1, 1, 1, 1, 1]),
    "lattice_beam":     (1, 14, [6, 6, 5, 5, 3, 1, 1, 1]),
    "viterbi_exact":    (1, 14, [4, 2, 1, 1, 1, 1, 1, 1]),
}


def test_the_table_covers_every_path_and_every_row_discriminates():
    assert sorted(TABLE) == sorted(PATHS) == sorted(BASE_TS)
    for name, (reps, k0, want) in TABLE.items():
        n_utts = reps * len(BASE_TS[name])
        assert len(want) == len(LADDER), name
        assert len(set(want)) >= 3, name
        assert any(1 < w < n_utts for w in want), name


@pytest.mark.parametrize("name", sorted(PATHS))
def test_chunk_counts_along_the_budget_ladder(name, monkeypatch):
    monkeypatch.setenv("SCRF_FAST_DECODE", "0")   # read by scrf_create; only the Viterbi row decodes
    reps, k0, want = TABLE[name]
    Ts = list(BASE_TS[name]) * reps
    got = [PATHS[name](sb << (k0 - 14), Ts) for sb in LADDER]
    print("%s: %s" % (name, got))
    assert got == want
