"""Cases, weight generators and references shared by tests/test_nbest_cases.py (CPU: the conditions) and
tests/test_gpu_nbest_edges.py (GPU: the kernels of scrf_nbest.hip).

Every row is built from the kernels' own constants: a wavefront of 64 lanes merges the lists (lane j % 64 owns lists j, j + 64, ..),
the fill loops step by 64, k_nbest_scan runs 1,024 threads over U * N entries, and a workgroup has 160 KiB of LDS.  grid_weights
makes exact ties abound: every weight is zero but the bias of every label and of every transition, each a small multiple of
0.5, so every score is such a multiple and the same at every frame; path costs are exact sums and collide across previous
labels, start frames and ranks at once."""
import functools

import numpy as np

import align_ref as ar
import family_shapes as fs
import nbest_ref as nr
from cases import Case

LDS_LIMIT = 160 * 1024     # bytes of dynamic LDS a workgroup of k_nbest may take (scrf_nbest_batch refuses more)
NB_WAVES = 16              # wavefronts of a workgroup of k_nbest, each with its own head ranks
LANES = 64
SCAN_THREADS = 1024        # k_nbest_scan: one workgroup
ENUMERABLE = 5000          # paths of an utterance up to which enumerate_all is run on the row itself


def lds_bytes(L, D, N):
    """dynamic LDS of k_nbest: the two end buffers and the boundary ring, (D + 2) L N floats, and per wavefront one 16-bit head
    rank per list, max(L, D + 1) of them rounded up to even (nbest_smem_bytes, scrf_nbest.hip)"""
    heads = (max(L, D + 1) + 1) & ~1
    return (D + 2) * L * N * 4 + NB_WAVES * heads * 2


def largest_n(L, D):
    """the largest n_best whose lists fit LDS_LIMIT"""
    heads = (max(L, D + 1) + 1) & ~1
    return (LDS_LIMIT - NB_WAVES * heads * 2) // ((D + 2) * L * 4)


def grid_weights(case, seed, step=0.5, span=4):
    """case.lam replaced: zero everywhere but the state bias weight of every label and the bias weight of every transition,
    each randint(-span, span + 1) * step.  With bias values of 1 every score is an exact multiple of step."""
    lay = case.olay
    NL = case.ocfg.num_labs
    rng = np.random.RandomState(seed)
    lam = np.zeros_like(case.lam)
    for l in range(NL):
        lam[lay.state_idx[l] + lay.num_state_funcs - 1] = rng.randint(-span, span + 1) * step
    seen = set()
    for p in range(NL):
        for n in range(NL):
            i = int(lay.trans_idx[p * NL + n]) + lay.num_trans_funcs - 1
            v = rng.randint(-span, span + 1) * step
            if i not in seen:
                seen.add(i)
                lam[i] = v
    case.lam = lam
    return case


def _row(gen, ns, kw=None, shape=None, seed=None, reaches="", span=4):
    return dict(gen=gen, ns=tuple(ns), kw=kw, shape=shape, seed=seed, reaches=reaches, span=span)


# name -> generator ("grid": grid_weights; "family": the tied family of family_shapes on one of its shapes; "large": N(0, 3000^2)
# weights), the n_best values, Case keywords or the shape, what the row reaches
ROWS = {
    "grid_labels": _row("grid", (1, 100), dict(L=70, D=3, in_w=2, Ts=[9]), seed=3101,
                        reaches="ties between lists j and j + 64 in the boundary merge; N > 64; 140,000 bytes of lists"),
    "grid_durs": _row("grid", (70,), dict(L=2, D=66, in_w=2, Ts=[70]), seed=3305,
                      reaches="ties between durations in one lane (1 + D = 67 lists); the ring wraps"),
    "grid_both": _row("grid", (8,), dict(L=66, D=66, in_w=2, Ts=[68]), seed=3369, reaches="both at once, near the LDS limit"),
    # 66 random biases always hold a label whose segments lower the cost, so the best paths use durations of 1 and the lists of
    # durations d and d + 64 never tie at their heads: with span = 0 every path costs 0 and both merges tie within a lane
    "grid_both_zero": _row("grid", (8,), dict(L=66, D=66, in_w=2, Ts=[68]), seed=3103, span=0,
                           reaches="both at once with every cost equal: the tie rule alone orders 66 labels and 67 durations"),
    "grid_long": _row("grid", (300,), dict(L=5, D=4, in_w=2, Ts=[12]), seed=3104, reaches="head ranks up to 299; N > 256"),
    "grid_frame": _row("grid", (100,), dict(L=70, D=1, in_w=2, Ts=[6], trans_ctx=1, frame_model=True), seed=3105,
                       reaches="the frame-model branch with ties over 70 lists"),
    "grid_final": _row("grid", (100,), dict(L=70, D=2, in_w=2, Ts=[1, 2]), seed=3106, reaches="NbFinal over 70 lists; lists shorter than N"),
    "tied_fused": _row("family", (16,), shape="fused", reaches="ties over time-dependent scores; the fused score path"),
    "tied_mw": _row("family", (16,), shape="mw", reaches="ties over time-dependent scores, 70 labels"),
    "tied_frame": _row("family", (16,), shape="frame", reaches="ties over time-dependent scores, frame model"),
    "tied_mixed": _row("family", (16,), shape="mixed", reaches="ties over time-dependent scores; per-frame M"),
    "tied_config2": _row("family", (16,), shape="config2", reaches="ties over time-dependent scores; the fused score path at L = 48, D = 25"),
    "large": _row("large", (16,), dict(L=7, D=10, in_w=5, Ts=[9, 10, 11, 30], lam_scale=3000), seed=3107,
                  reaches="sums at 1e4 .. 1e5, where the order of additions decides bits"),
    "lds_max": _row("grid", (largest_n(2, 2),), dict(L=2, D=2, in_w=2, Ts=[14]), seed=3108,
                    reaches="the largest list the host admits; one more is refused"),
}
ROW_NAMES = tuple(ROWS)
GRID_ROWS = tuple(n for n in ROW_NAMES if n.startswith("grid_"))
TIED_ROWS = tuple(n for n in ROW_NAMES if n.startswith("tied_"))
TIES_PRESENT = ("grid_labels", "grid_durs", "grid_both", "grid_both_zero", "grid_long", "grid_frame", "tied_fused", "tied_mixed")
FAST_TOO = ("tied_fused", "tied_config2")     # rows that also run with SCRF_FAST_DECODE=0

# batches of many short utterances (the default weights): the scan with several entries per thread, and chunks that end on a
# short list.  L = 2, D = 2: an utterance of 1, 2, 3 frames has 2, 6, 16 paths, one of 4 has 44.
SHORT_KW = dict(L=2, D=2, in_w=2)
BATCHES = {
    "scan_even": (dict(SHORT_KW, Ts=[1, 2, 3, 4, 5, 6] * 8, seed=3201), 40),             # 48 * 40 = 1,920 entries: 2 per thread
    "scan_odd": (dict(SHORT_KW, Ts=[1, 2, 3, 4, 5, 6] * 23 + [5], seed=3202), 22),      # 139 * 22 = 3,058 = 1,019 * 3 + 1
    "split": (dict(SHORT_KW, Ts=[1, 2, 3, 3, 2, 1, 1] * 43, seed=3203), 40),            # 301 utterances, all lists short
}


def count_paths(T, L, D):
    """nr.num_paths without the enumeration: P(0) = 1, P(t) = L * (P(t - 1) + .. + P(t - min(D, t)))"""
    P = [1]
    for t in range(1, T + 1):
        P.append(L * sum(P[t - d] for d in range(1, min(D, t) + 1)))
    return P[T]


def scan_per(U, N):
    """entries per thread of k_nbest_scan"""
    return -(-U * N // SCAN_THREADS)


def shape_of(name):
    row = ROWS[name]
    return fs.SHAPES[row["shape"]][0] if row["gen"] == "family" else row["kw"]


def make_case(name, **over):
    """a fresh Case of a row (over: keywords that replace the row's, for a small copy at the same generator)"""
    row = ROWS[name]
    if row["gen"] == "family":
        return fs.case(row["shape"], "tied", **over)
    c = Case(seed=row["seed"], **dict(row["kw"], **over))
    if row["gen"] == "grid":
        grid_weights(c, row["seed"], span=row["span"])
    return c


def small_copy(name):
    """the row's generator on L <= 3, D <= 3, at most two utterances of T <= 6"""
    kw = shape_of(name)
    Ts = sorted(set(min(T, 6) for T in kw["Ts"]))[-2:]
    return make_case(name, L=min(kw["L"], 3), D=min(kw["D"], 3), Ts=Ts)


def make_batch_case(name, **over):
    return Case(**dict(BATCHES[name][0], **over))


@functools.lru_cache(maxsize=None)
def weights(name):
    """per utterance the oracle's float arc weights (ar.Weights) of a row or a batch; computed once and not modified"""
    c = make_case(name) if name in ROWS else make_batch_case(name)
    return tuple(ar.case_weights(c, u) for u in range(len(c.Ts)))


@functools.lru_cache(maxsize=None)
def reference(name, N):
    """per utterance ((labels, cost), ..) of nr.nbest"""
    return tuple(tuple((tuple(p), c) for p, c in nr.nbest(w, N)) for w in weights(name))


def lane_tie_steps(w, N):
    """{kind: number of (merge, output step, column) at which two equal least heads lie in lists j and j + 64}, and whether
    the head-by-head merge gave the values of the stable sort at every merge"""
    count = {"boundary": 0, "end": 0, "final": 0}
    agree = [True]

    def on_merge(kind, t, cand, val):
        v, _, same = nr.merge_by_heads(cand, N)
        agree[0] = agree[0] and v.tobytes() == np.ascontiguousarray(val).tobytes()
        count[kind] += int(same.sum())
    nr.nbest(w, N, on_merge=on_merge)
    return count, agree[0]
