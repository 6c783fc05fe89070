"""Big batches with an exact expected answer: a batch in which each of a few base utterances occurs many times.

tiled() builds the batch from a case of k base utterances (the lists hold references to the base arrays, nothing is
copied); expected() forms its gradient as sum_i counts[i] * g_i from the per-utterance oracle gradients g_i, summed in
float64 on the host, and the per-copy numerators and Zx as those of the base utterance.

Everything about a batch's size is computed here from the layout -- segments, frames, the bytes of the arrays that are to
pass 2^32, and the split-K plans, which restate three functions of asr-craft_amd/csrc/scrf_engine.cpp -- and nothing is read
from the engine.  CASES lists every shape of tests/test_gpu_big_batch.py with the boundaries it has to cross;
tests/test_big_batch.py (no GPU) asserts each crossing with a 5 % margin, so that a later change of a shape cannot quietly
fall back under a boundary."""
import copy

import numpy as np

import orc
import scrf_amd
from cases import Case

EXACT, FAST, FAST32, FASTLIN = scrf_amd.PREC_EXACT, scrf_amd.PREC_FAST, scrf_amd.PREC_FAST32, scrf_amd.PREC_FASTLIN
PREC_NAME = {EXACT: "EXACT", FAST: "FAST", FAST32: "FAST32", FASTLIN: "FASTLIN"}
TWO32 = 1 << 32
MARGIN = 1.05
BASE_TS = [300, 257, 40, 7]


# ---- layout ---------------------------------------------------------------------------------------------------------
def num_segs(T, D):
    return T * (T + 1) // 2 if T < D else D * (D + 1) // 2 + (T - D) * D


def nseg(Ts, counts, D):
    return sum(n * num_segs(T, D) for T, n in zip(Ts, counts))


def nfr(Ts, counts):
    return sum(n * T for T, n in zip(Ts, counts))


# ---- the plans (restated; the CPU test pins them on values worked out by hand) -----------------------------------------
def expf_rows_per_chunk(n_seg):
    """expf_rows_per_chunk (scrf_engine.cpp): about 1024 K-chunks of the state count contraction, multiples of 32 rows, at least 4096"""
    rpc = (n_seg + 1023) // 1024
    rpc = (rpc + 31) & ~31
    return max(rpc, 4096)


def atb_rows_per_chunk(n_fr):
    """atb_rows_per_chunk (scrf_engine.cpp): about 4096 K-chunks of the transition-bias contraction, multiples of 4 frames, at least 64"""
    rpc = ((n_fr + 4095) // 4096 + 3) & ~3
    return max(rpc, 64)


def sl_rows_per_chunk(n_fr):
    """sl_rows_per_chunk (scrf_engine.cpp): at most 256 K-chunks of the STDSEG linear path's contractions, multiples of 32 frames, at
    least 64"""
    rpc = ((n_fr + 255) // 256 + 31) & ~31
    return max(rpc, 64)


# first sizes at which each plan leaves its floor
EXPF_BREAK = 4096 * 1024         # segments: rows per chunk grow past 4096
ATB_BREAK = 64 * 4096            # frames: rows per chunk grow past 64
SL_BREAK = 64 * 256              # frames
TRANSFRAME_BREAK = 3 * 2048      # frames: transframe_chunks (scrf_engine.cpp) reaches its base of 4 and starts to search
PLAN_CHUNK_CAP = 65535           # utterances per chunk, plan_chunk (scrf_engine.cpp)
SL_CHUNK_CAP = 32767             # utterances per chunk, STDSEG linear path (stdseg_lin_pipe, scrf_engine.cpp)


# ---- tiling ---------------------------------------------------------------------------------------------------------
def copy_order(counts, order="spread"):
    """base index of every copy, in batch order.
    roundrobin: 0 1 .. k-1 0 1 .. while every base has copies left, the exhausted ones dropping out (the tail is the most
    frequent utterance alone).
    spread: copy j of base i sits at (j + 1/2) / counts[i] of the batch, ties by base index: every base occurs at an even
    rate from the first utterance to the last, so utterances of different lengths alternate up to the far end of every
    array."""
    counts = [int(n) for n in counts]
    if order == "roundrobin":
        left = list(counts)
        out = []
        while any(left):
            for i in range(len(left)):
                if left[i]:
                    out.append(i)
                    left[i] -= 1
        return np.array(out, dtype=np.int64)
    if order != "spread":
        raise ValueError("unknown order %r" % (order,))
    base = np.concatenate([np.full(n, i, dtype=np.int64) for i, n in enumerate(counts)])
    pos = np.concatenate([(np.arange(n) + 0.5) / n for n in counts])
    return base[np.lexsort((base, pos))]


class Tiled:
    """frames / labels / frames2: the batch's lists (references to the base arrays); base[u]: the base utterance of copy u"""

    def __init__(self, case, counts, order="spread"):
        assert len(counts) == len(case.Ts) and len(set(counts)) > 1, "one count per base utterance, not all equal"
        self.case, self.counts = case, [int(n) for n in counts]
        self.base = copy_order(counts, order)
        self.frames = [case.frames[i] for i in self.base]
        self.labels = [case.labels[i] for i in self.base]
        f2 = getattr(case, "frames2", None)
        self.frames2 = None if f2 is None else [f2[i] for i in self.base]
        self.Ts = np.array(case.Ts, dtype=np.int64)[self.base]
        self.first = np.array([int(np.argmax(self.base == i)) for i in range(len(counts))])
        self.last = np.array([len(self.base) - 1 - int(np.argmax(self.base[::-1] == i)) for i in range(len(counts))])

    def engine(self, precision=None, scratch_bytes=None):
        cfg = type(self.case.gcfg).from_buffer_copy(self.case.gcfg)
        if precision is not None:
            cfg.train_precision = precision
        if scratch_bytes is not None:
            cfg.scratch_bytes = scratch_bytes
        e = scrf_amd.Engine(cfg)
        e.set_lambda(self.case.lam)
        return e

    def batch(self, eng, with_labels=True):
        return eng.batch_from_frames(self.frames, self.labels if with_labels else None, self.case.recipes,
                                     [self.frames2] if self.frames2 is not None else None)

    def frame_off(self):
        return np.concatenate([[0], np.cumsum(self.Ts)])


def tiled(case, counts, order="spread"):
    """(frames, labels, frames2 or None, base) of the batch in which base utterance i of `case` occurs counts[i] times"""
    t = Tiled(case, counts, order)
    return t.frames, t.labels, t.frames2, t.base


# ---- expected results ---------------------------------------------------------------------------------------------------
class NStateCase:
    """the n-state frame model (the case of tests/test_gpu_nstate.py, with the attributes tiled() reads)"""

    def __init__(self, P, K, F, Ts, seed=0, scale=0.3):
        rng = np.random.RandomState(seed)
        self.P, self.K, self.L, self.D, self.F, self.Ts = P, K, P * K, 1, F, list(Ts)
        self.frames = [rng.random_sample((T, F)).astype(np.float32) for T in Ts]
        self.frames2 = None
        kw = dict(model_type=orc.STDFRAME, L=P * K, D=1, F=F, use_trans_ftrs=True, tfs=0, tfe=F - 1, num_states=K)
        self.ocfg = orc.config(**kw); self.olay = orc.Layout(self.ocfg)
        self.gcfg = scrf_amd.make_config(**kw)
        self.lam = rng.normal(0, scale, self.olay.lambda_len)
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


def utterance_gradient(c, u):
    """(gradient, numerator, Zx) of base utterance u alone, on the CPU oracle"""
    T = c.Ts[u]
    g = np.zeros(c.olay.lambda_len)
    if isinstance(c, NStateCase):
        rc, g, n, z = orc.nstate_build_gradient(c.ocfg, c.olay, c.lam, c.frames[u], c.labels[u], T, grad=g)
    else:
        fn = {orc.STDFRAME: orc.frame_build_gradient, orc.STDSEG: orc.stdseg_build_gradient,
              orc.STDSEG_NO_DUR: orc.segtrans_build_gradient}.get(c.ocfg.model_type, orc.seg_build_gradient)
        rc, g, n, z = fn(c.ocfg, c.olay, c.lam, c.windows(u), c.labels[u], T, grad=g)
    assert rc == 0, rc
    return g, n, z


class Expected:
    """per base utterance: gradient g[i], numerator, Zx (read-only)"""

    def __init__(self, c):
        r = [utterance_gradient(c, u) for u in range(len(c.Ts))]
        self.g = np.array([x[0] for x in r])
        self.numer = np.array([x[1] for x in r])
        self.zx = np.array([x[2] for x in r])
        for a in (self.g, self.numer, self.zx):
            a.flags.writeable = False

    def gradient(self, counts):
        """sum_i counts[i] * g_i in float64"""
        return (np.asarray(counts, dtype=np.float64)[:, None] * self.g).sum(0)


# ---- position must not matter ---------------------------------------------------------------------------------------
def copies_vs_first(values, base, k):
    """per-copy scalars against the first copy of the same base utterance: (all bit-equal?, largest relative difference)"""
    values = np.asarray(values)
    first = np.array([int(np.argmax(base == i)) for i in range(k)])
    ref = values[first][base]
    same = bool((values.view(np.uint8).reshape(len(values), -1) == ref.view(np.uint8).reshape(len(values), -1)).all())
    with np.errstate(invalid="ignore", divide="ignore"):
        rel = np.abs(values.astype(np.float64) - ref) / np.maximum(np.abs(ref.astype(np.float64)), 1e-300)
    rel = np.where(values == ref, 0.0, rel)
    return same, float(rel.max()) if rel.size else 0.0


def blocks_vs_first(flat, off, base, k):
    """ragged per-copy blocks (flat[off[u]:off[u + 1]]; rows of any width) against the first copy's block of the same base
    utterance, one gather per base utterance: (all bit-equal?, largest absolute difference)"""
    off = np.asarray(off, dtype=np.int64)
    same, dev = True, 0.0
    for i in range(k):
        us = np.nonzero(base == i)[0]
        n = off[us[0] + 1] - off[us[0]]
        if not (off[us + 1] - off[us] == n).all():
            return False, np.inf
        blk = flat[off[us][:, None] + np.arange(n)[None, :]]          # [copies, n, ...]
        if blk.dtype.names is not None:
            same = same and all(bool((blk[f] == blk[f][:1]).all()) for f in blk.dtype.names)
            continue
        eq = blk == blk[:1]
        if not eq.all():
            same = False
            dev = max(dev, float(np.abs(blk.astype(np.float64) - blk[:1]).max()))
    return same, dev


# ---- the GPU cases and what each has to cross -------------------------------------------------------------------------
def _case_row(kw, counts, arrays=(), crossings=(), largest=None, make=Case):
    return dict(kw=kw, counts=counts, arrays=arrays, crossings=crossings, largest=largest, make=make)


def case_sizes(name):
    """(n_seg, n_fr, n_utts) of CASES[name]"""
    row = CASES[name]
    kw = row["kw"]
    D = kw.get("D", 1)
    Ts = kw["Ts"]
    return nseg(Ts, row["counts"], D), nfr(Ts, row["counts"]), sum(row["counts"])


def array_bytes(name):
    """bytes of the arrays of CASES[name] that the table of tests/test_gpu_big_batch.py names: {array: bytes}"""
    row = CASES[name]
    kw = row["kw"]
    ns, nf, _ = case_sizes(name)
    L, D, W = kw.get("L"), kw.get("D", 1), kw.get("in_w")
    out = {}
    for a in row["arrays"] + ((row["largest"],) if row["largest"] else ()):
        if a == "S":                    # [nseg][L] fp64
            out[a] = ns * L * 8
        elif a == "X":                  # materialised windows [nseg][F] float
            out[a] = ns * orc.window_width(W, D, 0, 0, True) * 4
        elif a == "X_hybrid":           # [avg | max | min | onehot(d)], padded to 16 bytes (hybrid_row_floats, scrf_engine.cpp)
            out[a] = ns * ((3 * W + D + 3) & ~3) * 4
        elif a == "M":                  # [nfr][L * L] fp64
            out[a] = nf * L * L * 8
        elif a == "Sd":                 # STDSEG linear path: [D][nfr][La] fp64 (stdseg_lin_layout, scrf_engine.cpp)
            out[a] = D * nf * L * 8
        elif a == "M2":                 # STDSEG_NO_DUR: [nseg][L * L] fp64
            out[a] = ns * L * L * 8
        elif a == "TE":                 # n-state: [nfr][P * P] fp64 next to five [nfr][L] (nstate_layout, scrf_engine.cpp)
            out[a] = nf * max(kw["P"] * kw["P"], kw["P"] * kw["K"]) * 8
        elif a == "cells":              # transcript scoring: aB and bE, each [sum T * K] fp64 over the chunk's transcripts
            out[a] = 8 * sum(n * T * K for T, K, n in zip(kw["Ts"], TRANSCRIPT_K[name], row["counts"]))
        elif a == "bp":                 # N-best: bp_b and bp_e, each [nfr][L][N] 32-bit back pointers (chunk_layout, scrf_engine.cpp)
            out[a] = nf * L * NBEST_N[name] * 4
        elif a == "arcs":               # kept arcs, 20 bytes each: per frame t and duration d <= min(D, t + 1): L start or L * L
            out[a] = 20 * sum(n * lattice_arcs(T, L, D) for T, n in zip(kw["Ts"], row["counts"]))
        else:
            raise KeyError(a)
    return out


def lattice_arcs(T, L, D):
    """arcs of the full segmental lattice of one utterance (bias-only transitions): L per segment (its state -> end state),
    L * L boundary arcs per frame after the first, L final arcs"""
    return num_segs(T, D) * L + (T - 1) * L * L + L


def need_bytes(name, prec=EXACT):
    """device memory a case is checked against before its engine is created: the arrays of its one chunk as chunk_layout
    (chunk_layout, scrf_engine.cpp) takes them, rounded up generously (a bound for the free-memory check, not a plan)"""
    row = CASES[name]
    kw = row["kw"]
    ns, nf, nu = case_sizes(name)
    L = kw.get("L") or kw["P"] * kw["K"]
    D, W = kw.get("D", 1), kw.get("in_w") or kw.get("F")
    F = orc.window_width(W, D, 0, 0, True) + (3 * W if kw.get("trans_ctx") else 0)
    per_seg = 3 * L * 8 + F * 4 + 16                      # S, AD / R, float weights or gamma; X; row tables
    per_fr = 14 * L * 8 + 64
    if kw.get("trans_ctx") is not None or kw.get("trans_share") is not None:
        per_fr += 4 * L * L * 8                           # M, E, ET, XI
    if kw.get("model_type") == orc.STDSEG_NO_DUR:
        per_seg += 2 * L * L * 8
    if kw.get("model_type") == orc.STDSEG:
        per_seg += 3 * L * D * L * 8                      # MX [nseg][L * D][La] and its posteriors
    if name == "latprune":
        per_fr += 20 * (D * L + L * L)
    cells = 2 * array_bytes(name)["cells"] if "cells" in row["arrays"] else 0
    if "bp" in row["arrays"]:           # both back-pointer arrays next to the scores
        cells += 2 * array_bytes(name)["bp"]
    return int(1.25 * (ns * per_seg + nf * per_fr + cells)) + (2 << 30)


C48 = [950, 820, 150, 50]
CASES = {
    # axis A: one chunk; arrays past 2^32 bytes where a few seconds and the card allow it
    "fused": _case_row(dict(L=48, D=25, in_w=5, Ts=BASE_TS, seed=2101), C48, arrays=("S",),
                       crossings=(("nseg", "expf"), ("nfr", "atb"))),
    "general": _case_row(dict(L=48, D=25, in_w=9, Ts=BASE_TS, seed=2102), C48, arrays=("S", "X"), crossings=(("nseg", "expf"),)),
    "mixed": _case_row(dict(L=48, D=10, in_w=5, Ts=BASE_TS, trans_ctx=1, seed=2103, lam_scale=0.05), [520, 460, 90, 30], arrays=("M",),
                       crossings=(("nfr", "transframe"),)),
    "hybrid": _case_row(dict(L=65, D=5, in_w=70, Ts=BASE_TS, seed=2104, lam_scale=0.05), [2050, 1750, 300, 100], arrays=("X_hybrid",),
                        crossings=(("nseg", "expf"),)),
    # the paths below cannot pass 2^32 bytes in a few seconds (see the docstrings of their tests): taken to their plan
    # breakpoints and to the largest size that stays quick
    "stdseg_lin": _case_row(dict(L=4, D=5, in_w=3, Ts=BASE_TS, model_type=orc.STDSEG, seed=2105), [400, 300, 100, 50], largest="Sd",
                            crossings=(("nfr", "sl"),)),
    "stdseg": _case_row(dict(L=4, D=5, in_w=3, Ts=BASE_TS, model_type=orc.STDSEG, trans_share=(0, 1), seed=2106), [40, 30, 10, 5]),
    "segtrans": _case_row(dict(L=3, D=3, in_w=2, Ts=BASE_TS, model_type=orc.STDSEG_NO_DUR, trans_share=(0, 18), seed=2107),
                          [400, 300, 100, 50], largest="M2"),
    "nstate": _case_row(dict(P=3, K=2, F=3, Ts=BASE_TS, seed=2108), [400, 300, 100, 50], largest="TE", make=NStateCase),
    "frame": _case_row(dict(L=6, D=1, in_w=3, Ts=BASE_TS, trans_ctx=0, frame_model=True, seed=2109), [400, 300, 100, 50], largest="M"),
    "latprune": _case_row(dict(L=48, D=25, in_w=5, Ts=BASE_TS, seed=2101), [130, 110, 20, 8], arrays=("arcs",)),
    # transcript scoring: the long-K shape of tests/test_gpu_transcript.py, 510 utterances
    "transcript": _case_row(dict(L=2, D=2, in_w=2, Ts=[1100, 1090], seed=2110), [270, 240], arrays=("cells",)),
    # N-best decoding at N = 64: 1500 utterances, 371,840 frames
    "nbest": _case_row(dict(L=48, D=2, in_w=2, Ts=BASE_TS, seed=2111), [730, 570, 150, 50], arrays=("bp",)),
}
NBEST_N = {"nbest": 64}                           # list length (scrf_nbest_batch)
TRANSCRIPT_K = {"transcript": [1030, 1020]}       # phones per base utterance (SCRF_ALIGN_ONE: K <= T <= K * D)


def transcript_phones(name):
    """the seeded transcript of every base utterance of CASES[name]"""
    row = CASES[name]
    rng = np.random.RandomState(row["kw"]["seed"] + 1)
    return [rng.randint(0, row["kw"]["L"], K).astype(np.uint32) for K in TRANSCRIPT_K[name]]
BOUNDARY = {"expf": EXPF_BREAK, "atb": ATB_BREAK, "sl": SL_BREAK, "transframe": TRANSFRAME_BREAK}

# axis B: more utterances than the chunk caps
MANY_TS = [1, 2, 3, 5]
MANY_COUNTS = [17000, 17500, 17700, 17800]        # 70,000 utterances
MANY = {
    "bias": dict(L=6, D=4, in_w=3, Ts=MANY_TS, seed=2201),
    "ctx": dict(L=6, D=4, in_w=3, Ts=MANY_TS, trans_ctx=1, seed=2202),
    "stdseg": dict(L=4, D=4, in_w=3, Ts=MANY_TS, model_type=orc.STDSEG, seed=2203),
    "nstate": dict(P=3, K=2, F=3, Ts=MANY_TS, seed=2204),
}


def make_case(row_or_kw, make=Case):
    if "kw" in row_or_kw:
        return row_or_kw["make"](**row_or_kw["kw"])
    return (NStateCase if "P" in row_or_kw else make)(**row_or_kw)
