"""numpy reference of the posterior output (scrf_posteriors_batch): frame posteriors, boundary posteriors and segment
confidences from the oracle's segment posteriors gamma, and the frame model's node posteriors from a plain log-domain
chain.  gamma [N_seg, L]: row orc.seg_base(t, D) + d - 1 is the segment that ENDS at frame t with duration d."""
import numpy as np

import orc

# the six shapes of tests/test_gpu_parity.py (copied: test modules are not imported)
CASES = [
    dict(L=3, D=3, in_w=2, Ts=[1, 2, 3, 4, 7]),
    dict(L=2, D=4, in_w=3, Ts=[3, 4, 5, 12], trans_ctx=1),
    dict(L=5, D=1, in_w=4, Ts=[1, 6, 9], trans_ctx=2),
    dict(L=7, D=10, in_w=5, Ts=[9, 10, 11, 30]),
    dict(L=48, D=25, in_w=39, Ts=[60, 33]),
    dict(L=48, D=10, in_w=8, Ts=[40, 25], trans_ctx=1, lam_scale=0.05),
]


def occupancy(g, T, D, L):
    """occ [T, L]: sum of gamma over the segments that cover each frame; end [T]: sum over the segments ending there"""
    occ = np.zeros((T, L)); end = np.zeros(T)
    for t in range(T):
        base = orc.seg_base(t, D)
        for d in range(1, min(t + 1, D) + 1):
            row = g[base + d - 1]
            occ[t - d + 1:t + 1] += row
            end[t] += row.sum()
    return occ, end


def utterance(c, u):
    """(gamma, occ, end, zx) of utterance u of a cases.Case"""
    T = c.Ts[u]
    S, M = orc.seg_scores(c.ocfg, c.olay, c.lam, c.windows(u), T)
    rc, g, xi, zx = orc.seg_posteriors(c.ocfg, S, M, T)
    assert rc == 0, rc
    occ, end = occupancy(g, T, c.D, c.L)
    return g, occ, end, zx


def segments_of(labels, L):
    """(end frame, duration, label) of a path's segments: label value l + L * (d - 1), back to back from frame 0"""
    out = []
    e = -1
    for v in labels:
        d = int(v) // L + 1
        e += d
        out.append((e, d, int(v) % L))
    return out


def seg_post(g, labels, L, D):
    return np.array([g[orc.seg_base(e, D) + d - 1, l] for e, d, l in segments_of(labels, L)])


def lse(a, axis):
    m = a.max(axis=axis, keepdims=True)
    return (m + np.log(np.exp(a - m).sum(axis=axis, keepdims=True))).squeeze(axis)


def frame_chain(S, M):
    """D = 1: node posteriors exp(alpha + beta - Zx) [T, L] and Zx of the chain whose transition INTO frame t is M[t]"""
    T, L = S.shape
    al = np.zeros((T, L)); be = np.zeros((T, L))
    al[0] = S[0]
    for t in range(1, T):
        al[t] = S[t] + lse(al[t - 1][:, None] + M[t].reshape(L, L), 0)
    for t in range(T - 2, -1, -1):
        be[t] = lse(M[t + 1].reshape(L, L) + (S[t + 1] + be[t + 1])[None, :], 1)
    zx = lse(al[T - 1], 0)
    return np.exp(al + be - zx), float(zx)


def enumerate_paths(S, M, T, D, L):
    """gamma and Zx by enumeration of every (segmentation, labelling); the transition into a segment is scored with M of the
    segment's FIRST frame"""
    paths = []

    def rec(t, prev, score, segs):
        if t == T:
            paths.append((score, segs)); return
        for d in range(1, min(D, T - t) + 1):
            e = t + d - 1
            row = orc.seg_base(e, D) + d - 1
            for l in range(L):
                s = score + S[row, l]
                if prev is not None:
                    s += M[t, prev * L + l]
                rec(e + 1, l, s, segs + [(e, d, l)])
    rec(0, None, 0.0, [])
    sc = np.array([p[0] for p in paths]); mx = sc.max(); zx = mx + np.log(np.exp(sc - mx).sum())
    g = np.zeros((orc.num_segs(T, D), L))
    for s, segs in paths:
        p = np.exp(s - zx)
        for e, d, l in segs:
            g[orc.seg_base(e, D) + d - 1, l] += p
    return g, zx, len(paths)
