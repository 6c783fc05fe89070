"""numpy float32 reference of forced alignment (scrf_align_batch), in three independent forms.

The hypotheses are the paths of the full lattice (scrf_lattice_arcs, norm = 0) that realise a phone transcript q_0 .. q_{K-1}:
ONE = exactly K segments, segment k carrying q_k; RUNS = every q_k realised by one or more consecutive segments carrying q_k.
The cost of a path is its left-to-right float32 sum; float addition is monotone, so the minimum is defined bit for bit.

  dp(...)          form 1: the direct recursion with the tie rule (boundary: advance, then stay; end: the start arc, then t'
                   ascending), labels and cost
  compose(...)     form 2: the full lattice composed with the transcript acceptor, relaxed in state order; cost only
  enumerate_(...)  form 3: every admissible (segmentation, labelling), each path summed left to right; cost only
"""
import itertools

import numpy as np

import orc

ONE, RUNS = 0, 1
F32 = np.float32
INF = F32(np.inf)


def feasible(T, K, D, mode):
    return T > 0 and 0 < K <= T and (mode != ONE or K * D >= T)


def collapse(phones):
    """consecutive equal phones merged"""
    p = np.asarray(phones, dtype=np.int64)
    return p[np.concatenate([[True], p[1:] != p[:-1]])] if p.size else p


class Weights:
    """the float arc weights of one utterance from its fp64 scores S [N_seg, L] (frame model: [T, L]) and M [T, L * L] (or one
    row): float32(-1.0 * score), rounded once, as the lattice carries them"""

    def __init__(self, S, M, T, L, D, frame_model=False):
        self.S, self.T, self.L, self.D, self.frame_model = np.asarray(S), T, L, D, frame_model
        self.M = np.asarray(M).reshape(-1, L, L)

    def Mt(self, t):
        return self.M[t if self.M.shape[0] > 1 else 0]

    def seg(self, t, d, lab):
        """segment of duration d ending at t (lab: scalar or array)"""
        return (-1.0 * self.S[orc.seg_base(t, self.D) + d - 1, lab]).astype(F32)

    def boundary(self, t, p, lab):
        return (-1.0 * self.Mt(t)[p, lab]).astype(F32)

    def frame(self, t, p, c):
        return (-1.0 * (self.Mt(t)[p, c] + self.S[t, c])).astype(F32)


def dp(w, phones, mode):
    """form 1: (labels first to last as l + L * (d - 1), cost float32); ([], inf) when the transcript does not fit"""
    T, L, D = w.T, w.L, w.D
    q = np.asarray(phones, dtype=np.int64)
    K = q.shape[0]
    if not feasible(T, K, D, mode):
        return [], INF
    qp = np.concatenate([q[:1], q[:-1]])   # q_{k-1}; entry 0 is not used
    end = np.full((T, K), INF, F32)
    bnd = np.full((T, K), INF, F32)
    dur = np.zeros((T, K), dtype=np.int64)
    stay = np.zeros((T, K), dtype=bool)
    for t in range(T):
        if t >= 1:
            wA = w.frame(t, qp, q) if w.frame_model else w.boundary(t, qp, q)
            wS = w.frame(t, q, q) if w.frame_model else w.boundary(t, q, q)
            b = np.full(K, INF, F32)
            c = end[t - 1, :-1] + wA[1:]              # advance
            imp = c < b[1:]
            b[1:][imp] = c[imp]
            if mode == RUNS:                          # then stay
                c = end[t - 1] + wS
                imp = c < b
                b[imp] = c[imp]
                stay[t] = imp
            bnd[t] = b
        if w.frame_model:
            if t == 0:
                end[0, 0] = F32(0.0) + w.seg(0, 1, q[0])
            else:
                end[t] = bnd[t]
            dur[t] = 1
            continue
        best = np.full(K, INF, F32)
        if t < D:                                     # the start arc: duration t + 1
            c = F32(0.0) + w.seg(t, t + 1, q[0])
            if c < best[0]:
                best[0] = c
                dur[t, 0] = t + 1
        for tp in range(max(t - D + 1, 1), t + 1):    # t' ascending = d descending
            d = t - tp + 1
            c = bnd[tp] + w.seg(t, d, q)
            imp = c < best
            best[imp] = c[imp]
            dur[t][imp] = d
        end[t] = best
    cost = end[T - 1, K - 1] + (F32(0.0) if w.frame_model else F32(-0.0))
    if not cost < INF:
        return [], INF
    labels = []
    t, k = T - 1, K - 1
    while True:
        d = int(dur[t, k])
        labels.append(int(q[k]) + L * (d - 1))
        ts = t - d + 1
        if ts == 0:
            break
        if not stay[ts, k]:
            k -= 1
        t = ts - 1
    assert k == 0
    return labels[::-1], F32(cost + F32(0.0))


def compose(arcs, n_states, final, L, phones, mode):
    """form 2: cost of the best path of lattice o acceptor.  Acceptor states 0 .. K; j -> j + 1 on q_j; in RUNS a self loop on
    q_{j-1} at state j >= 1; final K.  olabel 0 is epsilon, the phone of a label is (olabel - 1) % L.  Every arc has src < dst, so
    one pass over the lattice states in order relaxes everything."""
    q = np.asarray(phones, dtype=np.int64)
    K = q.shape[0]
    if final < 0 or K == 0:
        return INF
    assert (arcs["src"] < arcs["dst"]).all()
    dist = np.full((n_states, K + 1), INF, F32)
    dist[0, 0] = F32(0.0)
    for a in arcs[np.argsort(arcs["src"], kind="stable")]:
        s, d, wt = int(a["src"]), int(a["dst"]), F32(a["w"])
        if a["olabel"] == 0:
            dist[d] = np.minimum(dist[d], dist[s] + wt)
            continue
        hit = q == (int(a["olabel"]) - 1) % L
        adv = dist[s, :-1] + wt
        dist[d, 1:][hit] = np.minimum(dist[d, 1:][hit], adv[hit])
        if mode == RUNS:
            st = dist[s, 1:] + wt
            dist[d, 1:][hit] = np.minimum(dist[d, 1:][hit], st[hit])
    c = dist[final, K]
    return F32(c + F32(0.0)) if c < INF else INF


def _compositions(n, k, cap):
    """ordered k-tuples of integers in 1 .. cap that sum to n"""
    if k == 0:
        if n == 0:
            yield ()
        return
    for first in range(1, min(cap, n - (k - 1)) + 1):
        for rest in _compositions(n - first, k - 1, cap):
            yield (first,) + rest


def enumerate_(w, phones, mode):
    """form 3: the minimum over every admissible (segmentation, labelling) of the path's left-to-right float32 sum"""
    T, L, D = w.T, w.L, w.D
    q = [int(p) for p in phones]
    K = len(q)
    best = INF
    if T == 0 or K == 0:
        return best
    for n in range(K, T + 1) if mode == RUNS else [K]:
        if n > T:
            continue
        for durs in _compositions(T, n, D):
            for runs in (_compositions(n, K, n) if mode == RUNS else [(1,) * K]):
                labs = list(itertools.chain.from_iterable([q[k]] * r for k, r in enumerate(runs)))
                c = F32(0.0)
                t = -1
                for i, (d, lab) in enumerate(zip(durs, labs)):
                    t += d
                    if w.frame_model:
                        c = c + (w.seg(0, 1, lab) if i == 0 else w.frame(t, labs[i - 1], lab))
                    else:
                        if i > 0:
                            c = c + w.boundary(t - d + 1, labs[i - 1], lab)
                        c = c + w.seg(t, d, lab)
                c = c + (F32(0.0) if w.frame_model else F32(-0.0))
                c = F32(c + F32(0.0))
                if c < best:
                    best = c
    return best


def case_weights(c, u):
    """Weights of utterance u of a cases.Case from the CPU oracle's scores"""
    T = c.Ts[u]
    S, M = orc.seg_scores(c.ocfg, c.olay, c.lam, c.windows(u), T)
    return Weights(S, M, T, c.ocfg.num_labs, c.ocfg.lab_max_dur, c.ocfg.model_type == orc.STDFRAME)


def random_transcript(rng, T, L, D):
    """the phones of a random admissible segmentation of T frames (one per segment); adjacent equal phones are likely (and
    forced once where there is room)"""
    n = 0
    left = T
    while left > 0:
        left -= int(rng.randint(1, min(D, left) + 1))
        n += 1
    ph = rng.randint(0, L, n)
    if n >= 2:
        i = int(rng.randint(0, n - 1))
        ph[i + 1] = ph[i]
    return ph.astype(np.uint32)


def matches(labels, L, phones, mode):
    """do the phones of a label sequence realise the transcript under the mode?"""
    ph = np.asarray(labels, dtype=np.int64) % L
    if mode == ONE:
        return ph.tolist() == [int(p) for p in phones]
    # RUNS: a greedy split exists iff the collapsed sequences agree and no run of the transcript is longer than the path's
    cl, cp = collapse(ph), collapse(phones)
    if cl.tolist() != cp.tolist():
        return False
    runs = lambda x: [len(list(g)) for _, g in itertools.groupby([int(v) for v in x])]
    return all(a >= b for a, b in zip(runs(ph), runs(phones)))
