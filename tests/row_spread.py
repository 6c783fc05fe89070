"""Inputs that spread the STATE scores within a lattice row by a chosen number of nats, shared by tests/test_row_spread.py
(CPU: the conditions) and tests/test_gpu_transcript_spread.py (GPU: transcript scoring).

On the linear tiers the score stage leaves ES = exp(S - smax[row]) and transcript scoring reads a score back as
smax[row] + log(ES).  np.exp(-X) is a normal double up to X = 708.39, a subnormal one up to 745.13 and zero beyond.  The free
recursions may lose such a term: the label that holds the row maximum stands in the same sum.  A sum conditioned on a
transcript has no such neighbour when the row maximum sits on a label the transcript does not put there.

The design.  Raw feature column 0 is zero except for a 1.0 in one or two SPIKE frames of each utterance.  Window column 0 (the
first sample of the segment window; the frame itself in the frame model; index 0 of the sparse map) is the value of that
column at the segment's FIRST frame, so exactly the rows of the segments that start at a spike frame are "spiked".  The state
weights on window column 0 are

    top    W = 5400                  it holds the row maximum of every spiked row
    low    W - X                     every other state weight of `low` equals that of `top`: on a spiked row `low` lies X
                                     nats under `top` (to rounding), on every other row the two tie
    other  W - 400                   every further label: within 700 nats of `top` on a spiked row, whatever X is

so that at X <= 690 no label of a spiked row underflows and the linear form is exact, and from X = 746 on `low` reads as -inf
there.  No spike sits on frame 0, so the first segment of a path is never spiked.  The transcripts:

    ONE   [low] * K                  K = ceil(T / D) + 1: with a boundary on a spike frame a segment of `low` is spiked
    ONE   [third, low, .., low]      the same K, the first phone `third` = label 2 (L = 2: `top`)
    RUNS  [low]
    RUNS  [low, third]               the frame model only (D = 1: every frame starts a segment, so ONE has one alignment and
                                     nothing to lose but everything; ONE is not run there).  `third` pays P = 300 nats of state
                                     bias per frame, returned on window column 0, so that a long run of `third` -- the
                                     alignments that put `third` and not `low` on the spike frame 1 -- loses by P (T - 3) +
                                     400 - X nats

Every alignment that puts a boundary on a spike frame puts `low` on a spiked row and gains W - X >= 3000 nats over those that
do not: they carry all but e^-MARGIN of the mass (tests/test_row_spread.py measures the margin on the log-domain reference).
The alignments without such a boundary survive the linear form, so A stays finite and nothing tells the kernel that the
rest was lost.

The rungs from 705 to 728 carry no claim either way: exp(-X) is subnormal there with 50 to 24 bits left, log(ES) is off by
3e-16 to 1e-9, and whether the linear form meets a bound depends on the tier."""
import functools

import numpy as np

import orc
import scrf_amd
import sparse_ref as sr
import transcript_ref as tr
from cases import Case

W = 5400.0
OTHER = 400.0
P_FRAME = 300.0
MARGIN = 50.0
RUNGS = (0, 600, 690, 705, 712, 720, 728, 735, 740, 744.5, 746, 900, 2400)
REDUCED = (0, 690, 735, 746, 2400)
EXACT_UP_TO = 690        # the linear form equals the log form
WRONG_FROM = 735         # the unguarded linear form misses the FAST bound
GONE_FROM = 746          # exp(-X) == 0
SEED = 2300
TOP, LOW, THIRD = 0, 1, 2

# name -> (Case keywords, spike frames per utterance)
DENSE = {
    "fused3": (dict(L=3, D=3, in_w=2, Ts=[5, 7, 9, 6]), [[2], [3], [2, 6], [4]]),               # the fused score kernel
    "fused7": (dict(L=7, D=10, in_w=2, Ts=[9, 14, 11]), [[4], [3, 9], [6]]),                    # ... its D = 10 variant
    "ctx": (dict(L=2, D=4, in_w=2, Ts=[6, 13, 9], trans_ctx=1), [[2], [4, 9], [5]]),            # k_add_p_exp / k_exp_rows, per-frame M
    "wide66": (dict(L=66, D=4, in_w=2, Ts=[7, 12, 10]), [[3], [2, 7], [6]]),                    # the retire spans two wavefronts
    "frame": (dict(L=5, D=1, in_w=3, Ts=[14, 12, 13], frame_model=True), [[1], [1], [1]]),      # the frame model
}
# one spiked utterance among ordinary ones, wide enough that a budget of 1 << 18 bytes splits the batch (the L = 66 shape of
# tests/test_gpu_transcript.py's chunking test)
MIXED = {"mixed66": (dict(L=66, D=4, in_w=69, Ts=[9, 14, 6, 5, 11, 8], lam_scale=0.05), [[], [3, 9], [], [], [], []])}
SPARSE = dict(L=5, D=3, N=40, P=6, Ts=[9, 14, 6], spikes=[[4], [3, 9], [2]])
NAMES = tuple(DENSE) + ("sparse",)
ALL_TIERS = ("fused3", "ctx")     # the cases that also run under EXACT, FASTLIN and FAST32


class RowSpread:
    """one case at one rung: what the oracle and the engine need, the same for the dense and the sparse map"""

    def __init__(self, name, X, precision=0, scratch_bytes=0, spiked=True):
        self.name, self.X = name, float(X)
        if name == "sparse":
            self._sparse(precision, scratch_bytes, spiked)
        else:
            self._dense(precision, scratch_bytes, spiked)

    def _dense(self, precision, scratch_bytes, spiked):
        kw, spikes = (DENSE.get(self.name) or MIXED[self.name])
        c = Case(seed=SEED, precision=precision, scratch_bytes=scratch_bytes, **dict(dict(lam_scale=0.1), **kw))
        self.case, self.L, self.D, self.Ts, self.spikes = c, c.L, c.D, c.Ts, spikes
        self.frame_model = bool(kw.get("frame_model"))
        for u, f in enumerate(c.frames):
            f[:, 0] = 0.0
            if spiked:
                f[spikes[u], 0] = 1.0
        if c.frames2 is not None:   # the boundary-context stream repeats the edited frames
            n = c.trans_ctx
            c.frames2 = [np.concatenate([np.repeat(f[:1], n, 0), f, np.repeat(f[-1:], n, 0)]) for f in c.frames]
        lay, nsf, self.lam = c.olay, c.olay.num_state_funcs, c.lam
        self._weights(c.lam, lambda l: int(lay.state_idx[l]), nsf)

    def _sparse(self, precision, scratch_bytes, spiked):
        s = SPARSE
        rng = np.random.RandomState(SEED)
        self.case = None
        self.L, self.D, self.Ts, self.spikes, self.frame_model = s["L"], s["D"], s["Ts"], s["spikes"], False
        self.lay = sr.SparseLayout(self.L, sfe=s["N"] - 1, tfe=s["N"] - 1, use_tf=True)
        self.windows = []
        for u, T in enumerate(self.Ts):
            X = sr.random_windows(rng, orc.num_segs(T, self.D), s["P"], s["N"] - 1, sorted_unique=True)
            X[:, 0::2] += 1.0          # index 0 is the spike's alone
            if spiked:
                X[self.spiked_rows(u), 0] = 0.0   # the first pair of a spiked row: (index 0, value 1)
                X[self.spiked_rows(u), 1] = 1.0
            self.windows.append(X)
        self.lam = rng.uniform(-0.5, 0.5, self.lay.lambda_len)
        self._weights(self.lam, self.lay.state_idx, self.lay.nsf)
        self.gcfg = scrf_amd.make_config(model_type=scrf_amd.STDSEG_NO_DUR_NO_SEGTRANSFTR, L=self.L, D=self.D, F=2 * s["P"], sfe=s["N"] - 1,
                                         tfe=s["N"] - 1, use_trans_ftrs=True, sparse=True, precision=precision, scratch_bytes=scratch_bytes)

    def _weights(self, lam, state_idx, nsf):
        """the design's state weights, written into lam"""
        top, low = state_idx(TOP), state_idx(LOW)
        lam[low:low + nsf] = lam[top:top + nsf]
        for l in range(self.L):
            lam[state_idx(l)] = W - OTHER
        lam[top] = W
        lam[low] = W - self.X
        if self.frame_model:
            third = state_idx(THIRD)
            lam[third + nsf - 1] -= P_FRAME
            lam[third] += P_FRAME

    # ---- the design, stated apart from the weights
    def spiked_rows(self, u):
        """the rows of the segments that start at a spike frame"""
        T, D = self.Ts[u], self.D
        return [orc.seg_base(t, D) + d - 1 for t in range(T) for d in range(1, min(t + 1, D) + 1) if t - d + 1 in self.spikes[u]]

    def transcripts(self):
        """[(name, mode, one transcript per utterance)]"""
        if self.frame_model:
            return [("RUNS low third", tr.RUNS, [np.array([LOW, THIRD], dtype=np.uint32) for T in self.Ts])]
        Ks = [(T + self.D - 1) // self.D + 1 for T in self.Ts]
        first = THIRD if self.L > 2 else TOP
        return [("ONE low*K", tr.ONE, [np.full(K, LOW, dtype=np.uint32) for K in Ks]),
                ("ONE third low*", tr.ONE, [np.array([first] + [LOW] * (K - 1), dtype=np.uint32) for K in Ks]),
                ("RUNS low", tr.RUNS, [np.array([LOW], dtype=np.uint32) for T in self.Ts])]

    # ---- the oracle's side
    def scores(self, u):
        """tr.Scores of utterance u (fp64, log domain)"""
        T = self.Ts[u]
        if self.case is not None:
            return tr.case_scores(self.case, u)
        S, M = sr.scores(self.lay, self.lam, self.windows[u], T, self.D)
        return tr.Scores(S, M, T, self.L, self.D)

    # ---- the engine's side
    def engine(self):
        if self.case is not None:
            return self.case.engine()
        e = scrf_amd.Engine(self.gcfg)
        e.set_lambda(self.lam)
        return e

    def batch(self, eng, with_labels=False):
        if self.case is not None:
            return self.case.batch(eng, with_labels=with_labels)
        return eng.batch_from_windows(self.windows, self.Ts, self.labels() if with_labels else None)

    def labels(self):
        """training labels: the dense cases carry their own, the sparse one draws frame labels and groups them"""
        if self.case is not None:
            return self.case.labels
        rng = np.random.RandomState(SEED + 1)
        return [orc.group_labels(rng.randint(0, self.L, T).astype(np.uint32), self.D, self.L) for T in self.Ts]

    def oracle_numer_zx(self):
        """(numerators, Zx) of the labelled batch from the oracle"""
        if self.case is not None:
            return self.case.oracle_gradient()[1:]
        out = [sr.gradient(self.lay, self.lam, self.windows[u], self.labels()[u], T, self.D, scrf_amd.STDSEG_NO_DUR_NO_SEGTRANSFTR)[1:]
               for u, T in enumerate(self.Ts)]
        return np.array([o[0] for o in out]), np.array([o[1] for o in out])


def free_posteriors(w):
    """(gamma [N_seg, L], Zx) of the free lattice from the oracle's log-domain recursion (the frame model: a plain chain)"""
    if w.frame_model:
        import post_ref
        return post_ref.frame_chain(w.S.reshape(w.T, w.L), np.broadcast_to(w.M.reshape(-1, w.L * w.L), (w.T, w.L * w.L)))
    cfg = orc.config(L=w.L, D=w.D, F=2)
    M = np.ascontiguousarray(np.broadcast_to(w.M.reshape(-1, w.L * w.L), (w.T, w.L * w.L)))
    rc, g, xi, zx = orc.seg_posteriors(cfg, np.ascontiguousarray(w.S), M, w.T)
    assert rc == 0, rc
    return g, float(zx)


def free_zx(w):
    """Zx of the free lattice by a plain max-shifted forward recursion in numpy: takes scores of -inf, which the oracle refuses"""
    a = np.full((w.T, w.L), tr.NINF)
    for t in range(w.T):
        terms = []
        for d in range(1, min(t + 1, w.D) + 1):
            s = w.S[orc.seg_base(t, w.D) + d - 1]
            terms.append(s if d == t + 1 else s + tr.lse0(a[t - d][:, None] + w.Mt(t - d + 1)))
        a[t] = tr.lse0(terms)
    return float(tr.lse0(a[w.T - 1]))


@functools.lru_cache(maxsize=None)
def reference(name, X):
    """per utterance (the oracle's fp64 scores, the free gamma, the free Zx) at one rung; computed once and left unchanged"""
    rs = RowSpread(name, X)
    out = []
    for u in range(len(rs.Ts)):
        w = rs.scores(u)
        w.S.flags.writeable = False; w.M.flags.writeable = False
        g, zx = free_posteriors(w)
        g.flags.writeable = False
        out.append((w, g, zx))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def _ref_dp(name, X, u, mode, ph_bytes):
    return tr.dp(reference(name, X)[u][0], np.frombuffer(ph_bytes, dtype=np.uint32), mode)


def ref_dp(name, X, u, mode, ph):
    """form 1 on the oracle's log scores, cached"""
    return _ref_dp(name, X, u, mode, np.ascontiguousarray(ph, dtype=np.uint32).tobytes())
