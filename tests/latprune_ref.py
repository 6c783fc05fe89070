"""numpy reference of the lattice beam over an ARC_DTYPE array, and the shapes its tests share.

With wd = float64(w): fwd[0] = 0, fwd[s] = min over arcs into s of fwd[src] + wd; bwd[final] = 0, bwd[s] = min over arcs out
of s of wd + bwd[dst]; an arc is kept iff (fwd[src] + wd) + bwd[dst] <= fwd[final] + beam, in fp64 with that association.
Every arc of these lattices has src < dst, so one sweep in state order per direction suffices."""
import numpy as np

import orc

BEAMS = [0.5, 2.0, 8.0, 1e-3]

# shapes of tests/test_gpu_latprune.py (the trim test of tests/test_latprune_ref.py runs them on the CPU oracle)
GPU_SHAPES = [
    dict(L=3, D=3, in_w=2, Ts=[1, 2, 3, 4, 7]),
    dict(L=2, D=4, in_w=3, Ts=[3, 4, 5, 12], trans_ctx=1),
    dict(L=5, D=1, in_w=4, Ts=[1, 6, 9], trans_ctx=2, frame_model=True),
    dict(L=7, D=10, in_w=5, Ts=[9, 10, 11, 30]),
    dict(L=70, D=2, in_w=3, Ts=[5, 2], lam_scale=0.1),
    dict(L=66, D=4, in_w=69, Ts=[9, 14, 3, 1, 11, 8], lam_scale=0.05),
    dict(L=4, D=1, in_w=3, Ts=[1, 2, 6], frame_model=True),   # bias-only transitions: the frame model with a single M
]


def distances(arcs, n_states, final):
    """(fwd, bwd) in fp64; computed once per utterance and reused for every beam"""
    assert (arcs["src"] < arcs["dst"]).all()
    src, dst = arcs["src"].astype(np.int64), arcs["dst"].astype(np.int64)
    wd = arcs["w"].astype(np.float64)
    fwd = np.full(n_states, np.inf); bwd = np.full(n_states, np.inf)
    fwd[0] = 0.0; bwd[final] = 0.0
    # arcs grouped by destination, states ascending: every arc into s leaves a state whose distance is final already
    order = np.argsort(dst, kind="stable")
    bounds = np.searchsorted(dst[order], np.arange(n_states + 1))
    for s in range(1, n_states):
        a = order[bounds[s]:bounds[s + 1]]
        if a.size:
            fwd[s] = np.min(fwd[src[a]] + wd[a])
    order = np.argsort(src, kind="stable")
    bounds = np.searchsorted(src[order], np.arange(n_states + 1))
    for s in range(n_states - 1, -1, -1):
        a = order[bounds[s]:bounds[s + 1]]
        if a.size and s != final:
            bwd[s] = np.min(wd[a] + bwd[dst[a]])
    return fwd, bwd


def through(arcs, fwd, bwd):
    """cost of the cheapest complete path through each arc, with the rule's association"""
    return (fwd[arcs["src"]] + arcs["w"].astype(np.float64)) + bwd[arcs["dst"]]


def keep_mask(arcs, fwd, bwd, final, beam):
    return through(arcs, fwd, bwd) <= fwd[final] + beam


def prune(arcs, n_states, final, beam):
    """boolean mask of the kept arcs"""
    fwd, bwd = distances(arcs, n_states, final)
    return keep_mask(arcs, fwd, bwd, final, beam)


def through_brute(arcs, n_states, final):
    """the same by enumerating every complete path 0 -> final (depth first; each path's weights summed left to right)"""
    out_arcs = [[] for _ in range(n_states)]
    for i, s in enumerate(arcs["src"]):
        out_arcs[int(s)].append(i)
    wd = arcs["w"].astype(np.float64)
    dst = arcs["dst"]
    best = np.full(arcs.shape[0], np.inf)
    path = []

    def walk(s, cost):
        if s == final:
            for i in path:
                if cost < best[i]:
                    best[i] = cost
            return
        for i in out_arcs[s]:
            path.append(i)
            walk(int(dst[i]), cost + wd[i])
            path.pop()

    walk(0, 0.0)
    return best


def oracle_lattice(c, u):
    """the CPU oracle's full lattice of utterance u of a cases.Case: (arcs, n_states, final)"""
    T = c.Ts[u]
    S, M = orc.seg_scores(c.ocfg, c.olay, c.lam, c.windows(u), T)
    if c.ocfg.model_type == orc.STDFRAME:
        return orc.frame_lattice_arcs(c.ocfg, S, M, T)
    return orc.seg_lattice_arcs(c.ocfg, S, M, T)


def is_trim(arcs, n_states, final):
    """every arc's source is reachable from 0 and its destination reaches final, over these arcs alone"""
    if arcs.shape[0] == 0:
        return False
    reach = np.zeros(n_states, dtype=bool); reach[0] = True
    for a in arcs[np.argsort(arcs["src"], kind="stable")]:   # src < dst: sources ascending visits every state after its inputs
        if reach[a["src"]]:
            reach[a["dst"]] = True
    coreach = np.zeros(n_states, dtype=bool); coreach[final] = True
    for a in arcs[np.argsort(-arcs["dst"].astype(np.int64), kind="stable")]:
        if coreach[a["dst"]]:
            coreach[a["src"]] = True
    return bool(reach[arcs["src"]].all() and coreach[arcs["dst"]].all())
