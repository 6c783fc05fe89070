"""numpy fp64 reference of the soft-alignment gradient (scrf_fb_transcript_batch):
d(A(q) - Zx)/d lambda = E[f | x, transcript] - E[f | x], per utterance and summed over a cases.Case.

  numerator state counts       transcript_ref.dp(...).g, summed over the positions that carry a label
  numerator transition counts  trans_posteriors(...): a forward/backward of its own over (frame, position) in terms of the
                               sums at a segment's END (aE) and START (bB), scalar loops with np.logaddexp -- no code shared
                               with transcript_ref.dp or with the kernels
  denominator                  the CPU oracle's gradient with every label SCRF_LAB_BAD: numer = 0 and grad = -E[f | x]
  posteriors -> weights        through the oracle layout's state_idx / trans_idx and the oracle's windows: a state count
                               multiplies the window's state columns (+ bias), a transition count at boundary t the first
                               window of node t, row seg_base(t, D) (+ bias)"""
import numpy as np

import orc
import post_ref
import transcript_ref
from transcript_ref import NINF, ONE, RUNS  # noqa: F401  (re-exported for the tests)


def trans_posteriors(w, phones, mode):
    """(A, N [T, L, L]): N[t, p, c] = the posterior, given the transcript, of a boundary at frame t >= 1 from label p into
    label c; N[0] = 0"""
    T, L, D = w.T, w.L, w.D
    q = [int(p) for p in phones]
    K = len(q)
    N = np.zeros((T, L, L))
    if not transcript_ref.feasible(T, K, D, mode):
        return NINF, N
    la = np.logaddexp
    aE = np.full((T, K), NINF); aB = np.full((T, K), NINF)
    aB[0, 0] = 0.0
    with np.errstate(invalid="ignore"):
        for t in range(T):
            for k in range(K):
                if t >= 1:
                    v = NINF
                    if k >= 1:
                        v = la(v, aE[t - 1, k - 1] + w.Mt(t)[q[k - 1], q[k]])
                    if mode == RUNS:
                        v = la(v, aE[t - 1, k] + w.Mt(t)[q[k], q[k]])
                    aB[t, k] = v
                v = NINF
                for d in range(1, min(t + 1, D) + 1):
                    v = la(v, aB[t - d + 1, k] + w.seg(t, d, q[k]))
                aE[t, k] = v
        A = aE[T - 1, K - 1]
        bE = np.full((T, K), NINF); bB = np.full((T, K), NINF)
        for t in range(T - 1, -1, -1):
            for k in range(K):
                if t == T - 1:
                    bE[t, k] = 0.0 if k == K - 1 else NINF
                else:
                    v = NINF
                    if k + 1 < K:
                        v = la(v, bB[t + 1, k + 1] + w.Mt(t + 1)[q[k], q[k + 1]])
                    if mode == RUNS:
                        v = la(v, bB[t + 1, k] + w.Mt(t + 1)[q[k], q[k]])
                    bE[t, k] = v
            for k in range(K):
                v = NINF
                for d in range(1, min(D, T - t) + 1):
                    v = la(v, w.seg(t + d - 1, d, q[k]) + bE[t + d - 1, k])
                bB[t, k] = v
        for t in range(1, T):
            for k in range(K):
                if k >= 1:
                    x = aE[t - 1, k - 1] + w.Mt(t)[q[k - 1], q[k]] + bB[t, k] - A
                    if x > NINF:
                        N[t, q[k - 1], q[k]] += np.exp(x)
                if mode == RUNS:
                    x = aE[t - 1, k] + w.Mt(t)[q[k], q[k]] + bB[t, k] - A
                    if x > NINF:
                        N[t, q[k], q[k]] += np.exp(x)
    return float(A), N


def state_counts(r):
    """[N_seg, L] from a transcript_ref.Result: per label the sum over its positions"""
    G = np.zeros((r.g.shape[0], r.L))
    for k, l in enumerate(r.q):
        G[:, int(l)] += r.g[:, k]
    return G


def counts_to_weights(c, u, G, N, out=None):
    """adds the weight-space image of state counts G [N_seg, L] and transition counts N [T, L, L] of utterance u"""
    cfg, lay = c.ocfg, c.olay
    L, D, T = cfg.num_labs, cfg.lab_max_dur, c.Ts[u]
    X = c.windows(u).astype(np.float64)
    g = np.zeros(lay.lambda_len) if out is None else out
    n_sf = (cfg.state_fidx_end - cfg.state_fidx_start + 1) if cfg.use_state_ftrs else 0
    n_tf = (cfg.trans_fidx_end - cfg.trans_fidx_start + 1) if cfg.use_trans_ftrs else 0
    Xs = X[:, cfg.state_fidx_start:cfg.state_fidx_start + n_sf]
    for l in range(L):
        i = int(lay.state_idx[l])
        g[i:i + n_sf] += G[:, l] @ Xs
        if cfg.use_state_bias:
            g[i + n_sf] += G[:, l].sum() * cfg.state_bias_val
    first = np.array([orc.seg_base(t, D) for t in range(T)], dtype=np.int64)   # row of the d = 1 window of node t
    Xt = X[first][:, cfg.trans_fidx_start:cfg.trans_fidx_start + n_tf]
    for p in range(L):
        for cl in range(L):
            i = int(lay.trans_idx[p * L + cl])
            g[i:i + n_tf] += N[:, p, cl] @ Xt
            if cfg.use_trans_bias:
                g[i + n_tf] += N[:, p, cl].sum() * cfg.trans_bias_val
    return g


def frame_free_counts(w):
    """the frame model's free posteriors from a chain of its own: (gamma [T, L], xi [T, L, L], Zx)"""
    T, L = w.T, w.L
    S = w.S.reshape(T, L)
    al = np.zeros((T, L)); be = np.zeros((T, L))
    al[0] = S[0]
    for t in range(1, T):
        al[t] = transcript_ref.lse0(al[t - 1][:, None] + w.Mt(t)) + S[t]
    for t in range(T - 2, -1, -1):
        be[t] = transcript_ref.lse0((w.Mt(t + 1) + (S[t + 1] + be[t + 1])[None, :]).T)
    zx = float(transcript_ref.lse0(al[T - 1]))
    xi = np.zeros((T, L, L))
    for t in range(1, T):
        xi[t] = np.exp(al[t - 1][:, None] + w.Mt(t) + (S[t] + be[t])[None, :] - zx)
    return np.exp(al + be - zx), xi, zx


def free_gradient(c, u):
    """(-E[f | x], Zx) of utterance u: the oracle's gradient with no label observed.  On the frame model the oracle, like the
    reference's computeExpF, forms no transition expectation behind an unlabelled frame: there the transition part comes from
    frame_free_counts, and the oracle's state part must agree with the chain's."""
    T = c.Ts[u]
    bad = np.full(T, orc.LAB_BAD, dtype=np.uint32)
    frame = c.ocfg.model_type == orc.STDFRAME
    fn = orc.frame_build_gradient if frame else orc.seg_build_gradient
    rc, g, numer, zx = fn(c.ocfg, c.olay, c.lam, c.windows(u), bad, T)
    assert rc == 0 and numer == 0.0, (rc, numer)
    if frame:
        gamma, xi, zx2 = frame_free_counts(transcript_ref.case_scores(c, u))
        L = c.ocfg.num_labs
        assert abs(zx - zx2) <= 1e-12 * max(1.0, abs(zx))
        state = counts_to_weights(c, u, gamma, np.zeros((T, L, L)))
        assert np.abs(g + state).max() <= 1e-12 * max(1.0, np.abs(state).max())
        g = -counts_to_weights(c, u, gamma, xi)
    return g, zx


def numerator(c, u, phones, mode):
    """(E[f | x, transcript] in weight space, A, the dp Result, N) of utterance u"""
    w = transcript_ref.case_scores(c, u)
    r = transcript_ref.dp(w, phones, mode)
    A, N = trans_posteriors(w, phones, mode)
    return counts_to_weights(c, u, state_counts(r), N), r.A, r, N


def gradient(c, transcripts, mode):
    """sum over the utterances of the Case: (grad, log_num [U], zx [U])"""
    g = np.zeros(c.olay.lambda_len)
    ln, zx = [], []
    for u in range(len(c.Ts)):
        gn, A, _, _ = numerator(c, u, transcripts[u], mode)
        gd, z = free_gradient(c, u)
        g += gn + gd
        ln.append(A); zx.append(z)
    return g, np.array(ln), np.array(zx)


def sparse_gradient(lay, lam, windows, Ts, D, transcripts, mode):
    """the same over the sparse feature map (tests/sparse_ref.py; stdseg_no_dur_no_segtransftr): (grad, log_num [U], zx [U]).
    The denominator is sparse_ref.gradient with no label observed, the counts go through its add_*_counts."""
    import sparse_ref as sr
    g = np.zeros(lay.lambda_len)
    unused = np.zeros(lay.lambda_len)
    ln, zxs = [], []
    for u, T in enumerate(Ts):
        X = windows[u]
        S, M = sr.scores(lay, lam, X, T, D)
        w = transcript_ref.Scores(S, M, T, lay.L, D)
        r = transcript_ref.dp(w, transcripts[u], mode)
        A, N = trans_posteriors(w, transcripts[u], mode)
        G = state_counts(r)
        for row in range(G.shape[0]):
            for c in range(lay.L):
                sr.add_state_counts(lay, X[row], g, unused, G[row, c], None, c)
        for t in range(1, T):
            xn = X[orc.seg_base(t, D)]
            for p in range(lay.L):
                for c in range(lay.L):
                    sr.add_trans_counts(lay, xn, g, unused, N[t, p, c], -1, -1, p, c)
        gd, numer, zx = sr.gradient(lay, lam, X, np.full(T, orc.LAB_BAD, dtype=np.uint32), T, D, orc.STDSEG_NO_DUR_NO_SEGTRANSFTR)
        assert numer == 0.0
        g += gd
        ln.append(r.A); zxs.append(zx)
    assert not unused.any()
    return g, np.array(ln), np.array(zxs)


def objective(c, u, phones, mode, lam):
    """A(lam) - Zx(lam) of utterance u (for finite differences in weight space)"""
    T = c.Ts[u]
    S, M = orc.seg_scores(c.ocfg, c.olay, lam, c.windows(u), T)
    w = transcript_ref.Scores(S, M, T, c.ocfg.num_labs, c.ocfg.lab_max_dur, c.ocfg.model_type == orc.STDFRAME)
    A = transcript_ref.dp(w, phones, mode).A
    if w.frame_model:
        zx = float(post_ref.frame_chain(w.S.reshape(T, w.L), np.broadcast_to(w.M.reshape(-1, w.L * w.L), (T, w.L * w.L)))[1])
    else:
        rc, _, _, _, zx = orc.seg_forward(c.ocfg, S, M, T)
        assert rc == 0
    return A - zx
