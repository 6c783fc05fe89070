"""numpy fp64 reference of transcript scoring (scrf_transcript_batch), in three independent forms.

The hypotheses are those of forced alignment (tests/align_ref.py): the paths of the full lattice that realise a phone transcript
q_0 .. q_{K-1}, ONE = exactly K segments, RUNS = every q_k realised by one or more consecutive segments.  Here they are
SUMMED: the score of a path is the fp64 sum of its log scores (no float arc weights), A = log sum exp over the paths, and
g(t, d, k) = the posterior, given the transcript, that position k holds the segment ending at t with duration d.

  dp(...)          form 1: the recursion of DESIGN.md 4.17, vectorised over k (no liveness bounds: a cell that cannot lie on
                   a complete path gets posterior 0 from the other sweep by itself)
  compose(...)     form 2: the oracle's full lattice composed with the transcript acceptor, forward-backward in the log
                   semiring over the product, the arcs scored in fp64
  enumerate_(...)  form 3: every admissible (segmentation, labelling, run split), each path scored on its own

Each returns a Result: A, g [N_seg, K] (row orc.seg_base(t, D) + d - 1), frame_post [T, L], end_post [T]."""
import itertools

import numpy as np

import orc
from align_ref import ONE, RUNS, _compositions, collapse, feasible  # noqa: F401  (re-exported for the tests)

NINF = -np.inf


def lse0(a):
    """log sum exp over axis 0, max-shifted; all -inf gives -inf"""
    a = np.asarray(a, dtype=np.float64)
    m = a.max(axis=0)
    ms = np.where(np.isfinite(m), m, 0.0)
    with np.errstate(divide="ignore"):
        return np.where(np.isfinite(m), ms + np.log(np.exp(a - ms).sum(axis=0)), NINF)


class Scores:
    """the fp64 scores of one utterance: S [N_seg, L] (frame model: [T, L], D = 1) and M [T, L * L] (or one row)"""

    def __init__(self, S, M, T, L, D, frame_model=False):
        self.S, self.T, self.L, self.D, self.frame_model = np.asarray(S, dtype=np.float64), T, L, D, frame_model
        self.M = np.asarray(M, dtype=np.float64).reshape(-1, L, L)

    def Mt(self, t):
        return self.M[t if self.M.shape[0] > 1 else 0]

    def seg(self, t, d, lab):
        return self.S[orc.seg_base(t, self.D) + d - 1, lab]


def linear_view(w, float_smax=False):
    """the Scores of w as the linear-domain score stage leaves them and tr_score reads them back: per row
    smax + log(exp(S - smax)), -inf where exp gives 0; M untouched.  smax is the fp64 row maximum (k_exp_rows, k_add_p_exp)
    or, float_smax, the row maximum rounded to float (the fused score kernel)."""
    smax = w.S.max(axis=1, keepdims=True)
    if float_smax:
        smax = smax.astype(np.float32).astype(np.float64)
    with np.errstate(divide="ignore", under="ignore"):
        S = smax + np.log(np.exp(w.S - smax))
    return Scores(S, w.M, w.T, w.L, w.D, w.frame_model)


class Result:
    def __init__(self, w, phones, A, g):
        T, L, D = w.T, w.L, w.D
        q = np.asarray(phones, dtype=np.int64)
        self.A, self.g, self.L, self.D, self.q = A, g, L, D, q
        self.frame_post = np.zeros((T, L)); self.end_post = np.zeros(T)
        for t in range(T):
            for d in range(1, min(t + 1, D) + 1):
                row = g[orc.seg_base(t, D) + d - 1]
                if q.shape[0]:
                    self.frame_post[t - d + 1:t + 1] += np.bincount(q, weights=row, minlength=L)   # per label, its positions
                self.end_post[t] += row.sum()

    def queries(self, labels):
        """the posterior of every segment of a path (label value l + L * (d - 1), back to back from frame 0)"""
        out = []
        e = -1
        for v in labels:
            d, l = int(v) // self.L + 1, int(v) % self.L
            e += d
            out.append(self.g[orc.seg_base(e, self.D) + d - 1, self.q == l].sum())
        return np.array(out)


def _empty(w, phones):
    return Result(w, phones, NINF, np.zeros((orc.num_segs(w.T, w.D) if w.T else 0, len(phones))))


def dp(w, phones, mode):
    """form 1"""
    T, L, D = w.T, w.L, w.D
    q = np.asarray(phones, dtype=np.int64)
    K = q.shape[0]
    if not feasible(T, K, D, mode):
        return _empty(w, phones)
    aB = np.full((T, K), NINF); aE = np.full((T, K), NINF)
    for t in range(T):
        if t >= 1:
            Mt = w.Mt(t)
            adv = np.full(K, NINF)
            adv[1:] = aE[t - 1, :-1] + Mt[q[:-1], q[1:]]
            terms = [adv]
            if mode == RUNS:
                terms.append(aE[t - 1] + Mt[q, q])
            aB[t] = lse0(terms)
        terms = []
        if t < D:
            st = np.full(K, NINF)
            st[0] = w.seg(t, t + 1, q[0])
            terms.append(st)
        for d in range(min(t, D), 0, -1):
            terms.append(aB[t - d + 1] + w.seg(t, d, q))
        aE[t] = lse0(terms)
    A = aE[T - 1, K - 1]
    bE = np.full((T, K), NINF); bB = np.full((T, K), NINF)
    for t in range(T - 1, -1, -1):
        if t == T - 1:
            bE[t, K - 1] = 0.0
        else:
            Mn = w.Mt(t + 1)
            adv = np.full(K, NINF)
            adv[:-1] = bB[t + 1, 1:] + Mn[q[:-1], q[1:]]
            terms = [adv]
            if mode == RUNS:
                terms.append(bB[t + 1] + Mn[q, q])
            bE[t] = lse0(terms)
        bB[t] = lse0([w.seg(t + d - 1, d, q) + bE[t + d - 1] for d in range(1, min(D, T - t) + 1)])
    g = np.zeros((orc.num_segs(T, D), K))
    start = np.full(K, NINF); start[0] = 0.0
    with np.errstate(invalid="ignore"):
        for t in range(T):
            for d in range(1, min(t + 1, D) + 1):
                ab = start if t - d + 1 == 0 else aB[t - d + 1]
                x = ab + w.seg(t, d, q) + bE[t] - A
                g[orc.seg_base(t, D) + d - 1] = np.where(np.isnan(x), 0.0, np.exp(x))
    return Result(w, phones, float(A), g)


def arc_scores(w, arcs):
    """the fp64 log score of every arc of the oracle's full lattice, in its emission order, and the segment it stands for
    (t, d; d = 0 for an arc that is no segment).  Tied to the lattice: float32(-score) must be the arc's weight."""
    T, L, D = w.T, w.L, w.D
    sc, tt, dd = [], [], []
    for t in range(T):
        if w.frame_model:
            for cur in range(L):
                for prev in (range(L) if t else [None]):
                    sc.append(w.S[t, cur] + (w.Mt(t)[prev, cur] if t else 0.0)); tt.append(t); dd.append(1)
            continue
        if t >= 1:
            for lab in range(L):
                for p in range(L):
                    sc.append(w.Mt(t)[p, lab]); tt.append(t); dd.append(0)
        for lab in range(L):
            for d in range(1, min(t + 1, D) + 1):
                sc.append(w.seg(t, d, lab)); tt.append(t); dd.append(d)
    sc += [0.0] * L; tt += [T - 1] * L; dd += [0] * L   # into the final state
    sc = np.array(sc)
    assert sc.shape[0] == arcs.shape[0]
    assert ((-1.0 * sc).astype(np.float32) == arcs["w"]).all()
    return sc, np.array(tt), np.array(dd)


def compose(w, arcs, n_states, final, phones, mode):
    """form 2.  Acceptor states 0 .. K; j -> j + 1 on q_j; in RUNS a self loop on q_{j-1} at state j >= 1; final K.  olabel 0
    is epsilon, the phone of a label is (olabel - 1) % L.  Every arc has src < dst: one pass per direction."""
    T, L, D = w.T, w.L, w.D
    q = np.asarray(phones, dtype=np.int64)
    K = q.shape[0]
    if T == 0 or K == 0 or final < 0:
        return _empty(w, phones)
    sc, tt, dd = arc_scores(w, arcs)
    assert (arcs["src"] < arcs["dst"]).all()
    src, dst, ol = arcs["src"].astype(np.int64), arcs["dst"].astype(np.int64), arcs["olabel"].astype(np.int64)
    fwd = np.full((n_states, K + 1), NINF); fwd[0, 0] = 0.0
    bwd = np.full((n_states, K + 1), NINF); bwd[final, K] = 0.0
    hit = [(q == (o - 1) % L) if o else None for o in ol]
    for i in np.argsort(src, kind="stable"):
        s, d = src[i], dst[i]
        if ol[i] == 0:
            fwd[d] = np.logaddexp(fwd[d], fwd[s] + sc[i])
            continue
        h = hit[i]
        fwd[d, 1:][h] = np.logaddexp(fwd[d, 1:][h], (fwd[s, :-1] + sc[i])[h])
        if mode == RUNS:
            fwd[d, 1:][h] = np.logaddexp(fwd[d, 1:][h], (fwd[s, 1:] + sc[i])[h])
    A = fwd[final, K]
    if not np.isfinite(A):
        return _empty(w, phones)
    for i in np.argsort(-dst, kind="stable"):
        s, d = src[i], dst[i]
        if ol[i] == 0:
            bwd[s] = np.logaddexp(bwd[s], sc[i] + bwd[d])
            continue
        h = hit[i]
        bwd[s, :-1][h] = np.logaddexp(bwd[s, :-1][h], (sc[i] + bwd[d, 1:])[h])
        if mode == RUNS:
            bwd[s, 1:][h] = np.logaddexp(bwd[s, 1:][h], (sc[i] + bwd[d, 1:])[h])
    g = np.zeros((orc.num_segs(T, D), K))
    with np.errstate(invalid="ignore"):
        for i in np.nonzero(dd)[0]:
            s, d, h = src[i], dst[i], hit[i]
            x = fwd[s, :-1] + sc[i] + bwd[d, 1:] - A
            if mode == RUNS:
                x = np.logaddexp(x, fwd[s, 1:] + sc[i] + bwd[d, 1:] - A)
            p = np.where(h & ~np.isnan(x), np.exp(x), 0.0)
            g[orc.seg_base(tt[i], D) + dd[i] - 1] += p
    return Result(w, phones, float(A), g)


def enumerate_(w, phones, mode):
    """form 3"""
    T, L, D = w.T, w.L, w.D
    q = [int(p) for p in phones]
    K = len(q)
    if T == 0 or K == 0:
        return _empty(w, phones)
    paths = []
    for n in range(K, T + 1) if mode == RUNS else [K]:
        if n > T:
            continue
        for durs in _compositions(T, n, D):
            for runs in (_compositions(n, K, n) if mode == RUNS else [(1,) * K]):
                pos = list(itertools.chain.from_iterable([k] * r for k, r in enumerate(runs)))
                s = 0.0
                t = -1
                segs = []
                for i, (d, k) in enumerate(zip(durs, pos)):
                    t += d
                    if i > 0:
                        s += w.Mt(t - d + 1)[q[pos[i - 1]], q[k]]
                    s += w.seg(t, d, q[k])
                    segs.append((t, d, k))
                paths.append((s, segs))
    if not paths:
        return _empty(w, phones)
    sc = np.array([p[0] for p in paths])
    A = float(lse0(sc))
    g = np.zeros((orc.num_segs(T, D), K))
    for s, segs in paths:
        p = np.exp(s - A)
        for t, d, k in segs:
            g[orc.seg_base(t, D) + d - 1, k] += p
    return Result(w, phones, A, g)


def case_scores(c, u):
    """Scores of utterance u of a cases.Case from the CPU oracle's scores"""
    T = c.Ts[u]
    S, M = orc.seg_scores(c.ocfg, c.olay, c.lam, c.windows(u), T)
    return Scores(S, M, T, c.ocfg.num_labs, c.ocfg.lab_max_dur, c.ocfg.model_type == orc.STDFRAME)


def all_transcripts(L, T, D, mode):
    """every transcript that can fit T frames: ONE every phone string of every feasible length, RUNS every string without
    equal neighbours up to length T"""
    out = []
    for K in range(1, T + 1):
        if mode == ONE and K * D < T:
            continue
        for ph in itertools.product(range(L), repeat=K):
            if mode == RUNS and any(a == b for a, b in zip(ph, ph[1:])):
                continue
            out.append(np.array(ph, dtype=np.uint32))
    return out


def random_transcript(rng, T, L, D, mode):
    """the phones of a random admissible segmentation (align_ref.random_transcript: a forced repeat where there is room);
    collapsed in RUNS mode, where the sum refuses equal neighbours"""
    import align_ref
    ph = align_ref.random_transcript(rng, T, L, D)
    return collapse(ph).astype(np.uint32) if mode == RUNS else ph
