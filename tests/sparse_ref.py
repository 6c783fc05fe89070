"""CPU restatement of the sparse feature map CRF_StdSparseFeatureMap (CRF/src/ftrmaps/CRF_StdSparseFeatureMap.cpp of
the reference), for the tests.  Each window vector x of F floats is read as pairs (x[2k], x[2k+1]).  The scores feed
the oracle's DP (orc.seg_forward / seg_posteriors / *_lattice_arcs / best_path) unchanged.

Line numbers below are those of CRF_StdSparseFeatureMap.cpp.  Where the reference is undefined the engine's definition
is restated: an index float that is negative, NaN or >= 2^32 is out of range; the index range starts at 0."""
import math

import numpy as np

import orc

LAB_BAD = 0xFFFFFFFF


class SparseLayout:
    """The dense map's weight layout (CRF_StdFeatureMap::recalc, CRF_StdFeatureMap.cpp:472-517) with the index ranges
    [0, sfe] / [0, tfe]: numStateFuncs = sfe + 1 (+1 bias), numTransFuncs = tfe + 1 (+1 bias), per label c the block
    [state functions][for p: transition functions of (p -> c)]."""

    def __init__(self, L, sfe, tfe=0, use_sf=True, use_tf=False, use_sb=True, use_tb=True):
        self.L, self.sfe, self.tfe = L, sfe, tfe
        self.use_sf, self.use_tf, self.use_sb, self.use_tb = use_sf, use_tf, use_sb, use_tb
        self.nsfe = sfe + 1 if use_sf else 0
        self.ntfe = tfe + 1 if use_tf else 0
        self.nsf = self.nsfe + (1 if use_sb else 0)
        self.ntf = self.ntfe + (1 if use_tb else 0)
        self.stride = self.nsf + L * self.ntf
        self.lambda_len = L * self.stride

    def state_idx(self, c):
        return c * self.stride

    def trans_idx(self, p, c):
        return c * self.stride + self.nsf + p * self.ntf


def pair_index(xf, hi):
    """(QNUInt32) ftr_buf[fidx] (:66) and the range test (:67), or None when the pair is skipped."""
    xf = float(np.float32(xf))
    if math.isnan(xf) or xf < 0.0 or xf >= 4294967296.0:
        return None
    i = int(xf)   # truncation toward zero, as the C conversion
    return i if i <= hi else None


def state_value(lay, x, lam, clab):
    """computeStateArrayValue (:58-81): k ascending, each product value * lambda rounded then added, bias last and
    unscaled."""
    v = 0.0
    lc = lay.state_idx(clab)
    if lay.use_sf:
        for k in range(len(x) // 2):
            i = pair_index(x[2 * k], lay.sfe)
            if i is not None:
                v += float(np.float32(x[2 * k + 1])) * float(lam[lc + i])   # :70
    if lay.use_sb:
        v += float(lam[lc + lay.nsf - 1])                                   # :78
    return v


def trans_value(lay, x, lam, plab, clab):
    """computeTransMatrixValue (:96-120)."""
    v = 0.0
    lc = lay.trans_idx(plab, clab)
    if lay.use_tf:
        for k in range(len(x) // 2):
            i = pair_index(x[2 * k], lay.tfe)
            if i is not None:
                v += float(np.float32(x[2 * k + 1])) * float(lam[lc + i])   # :108
    if lay.use_tb:
        v += float(lam[lc + lay.ntf - 1])                                   # :116
    return v


def scores(lay, lam, X, T, D):
    """S [N_seg][L] over every window row, M [T][L*L] from the first window of each frame's node (the frame model: the
    frame itself, nodes/CRF_StdStateNode.cpp:68; stdseg_no_dur_no_segtransftr: ftrBuf, ...WithoutSegTransFtr.cpp:72)."""
    L = lay.L
    nseg = orc.num_segs(T, D)
    S = np.zeros((nseg, L))
    M = np.zeros((T, L * L))
    for r in range(nseg):
        for c in range(L):
            S[r, c] = state_value(lay, X[r], lam, c)
    for t in range(T):
        x = X[orc.seg_base(t, D)]
        for p in range(L):
            for c in range(L):
                M[t, p * L + c] = trans_value(lay, x, lam, p, c)
    return S, M


def add_state_counts(lay, x, ExpF, grad, gamma, t_clab, clab):
    """computeStateExpF (:142-170): expected += gamma * value, observed += value; a duplicate index counts twice."""
    lc = lay.state_idx(clab)
    if lay.use_sf:
        for k in range(len(x) // 2):
            i = pair_index(x[2 * k], lay.sfe)
            if i is not None:
                ExpF[lc + i] += gamma * float(np.float32(x[2 * k + 1]))
                if t_clab == clab:
                    grad[lc + i] += float(np.float32(x[2 * k + 1]))
    if lay.use_sb:
        ExpF[lc + lay.nsf - 1] += gamma
        if t_clab == clab:
            grad[lc + lay.nsf - 1] += 1.0


def add_trans_counts(lay, x, ExpF, grad, xi, t_plab, t_clab, plab, clab):
    """computeTransExpF (:193-223)."""
    lc = lay.trans_idx(plab, clab)
    match = plab == t_plab and clab == t_clab
    if lay.use_tf:
        for k in range(len(x) // 2):
            i = pair_index(x[2 * k], lay.tfe)
            if i is not None:
                ExpF[lc + i] += xi * float(np.float32(x[2 * k + 1]))
                if match:
                    grad[lc + i] += float(np.float32(x[2 * k + 1]))
    if lay.use_tb:
        ExpF[lc + lay.ntf - 1] += xi
        if match:
            grad[lc + lay.ntf - 1] += 1.0


def ocfg(lay, model_type, D):
    """An oracle config for the DP over restated S / M (the feature fields are not read there)."""
    return orc.config(model_type=model_type, L=lay.L, D=D, F=2)


def gradient(lay, lam, X, labels, T, D, model_type):
    """Observed minus expected counts of one utterance (the gradient builder's node loop, oracle posteriors), the
    numerator and log Z."""
    L = lay.L
    S, M = scores(lay, lam, X, T, D)
    cfg = ocfg(lay, model_type, D)
    rc, g, xi, zx = orc.seg_posteriors(cfg, S, M, T)
    assert rc == 0, rc
    ExpF = np.zeros(lay.lambda_len)
    grad = np.zeros(lay.lambda_len)
    numer = 0.0
    for t in range(T):
        base = orc.seg_base(t, D)
        lab = labels[t]
        a_lab, a_dur = (None, None) if lab == LAB_BAD else (lab % L, lab // L + 1)
        nxt = LAB_BAD
        for u in range(t + 1, T):
            if labels[u] != LAB_BAD:
                nxt = labels[u]
                break
        a_next = None if nxt == LAB_BAD else nxt % L
        for d in range(1, min(t + 1, D) + 1):
            for c in range(L):
                match = a_lab is not None and c == a_lab and d == a_dur
                add_state_counts(lay, X[base + d - 1], ExpF, grad, g[base + d - 1, c], c if match else None, c)
                if match:
                    numer += S[base + d - 1, c]
        if t + 1 < T:
            xn = X[orc.seg_base(t + 1, D)]
            for p in range(L):
                for c in range(L):
                    tp = a_lab if a_lab is not None else -1
                    tc = a_next if a_next is not None else -1
                    add_trans_counts(lay, xn, ExpF, grad, xi[t, p * L + c], tp, tc, p, c)
            if a_lab is not None and a_next is not None:
                numer += M[t + 1, a_lab * L + a_next]
    return grad - ExpF, numer, zx


def log_z(lay, lam, X, T, D, model_type):
    S, M = scores(lay, lam, X, T, D)
    rc, _, _, _, zx = orc.seg_forward(ocfg(lay, model_type, D), S, M, T)
    assert rc == 0, rc
    return zx


def densify(lay, X, which="state"):
    """The dense window over the index space [0, hi] that the map reads X as: pairs out of range dropped, duplicate
    indices summed (in float64, then rounded to float)."""
    hi = lay.sfe if which == "state" else lay.tfe
    out = np.zeros((X.shape[0], hi + 1), dtype=np.float64)
    for r in range(X.shape[0]):
        for k in range(X.shape[1] // 2):
            i = pair_index(X[r, 2 * k], hi)
            if i is not None:
                out[r, i] += float(np.float32(X[r, 2 * k + 1]))
    return out.astype(np.float32)


def random_windows(rng, nrows, npairs, nidx, sorted_unique=False, messy=False, values=None):
    """[nrows][2 npairs] float32 pair windows over the index space [0, nidx).  sorted_unique: ascending distinct
    indices; messy: unsorted, duplicates, fractional, out-of-range, negative and NaN index floats."""
    X = np.zeros((nrows, 2 * npairs), dtype=np.float32)
    for r in range(nrows):
        if sorted_unique:
            idx = np.sort(rng.choice(nidx, npairs, replace=False)).astype(np.float32)
        else:
            idx = rng.randint(0, nidx, npairs).astype(np.float32)
            if messy:
                idx[rng.rand(npairs) < 0.15] = nidx + rng.randint(0, 5)           # above the range
                idx[rng.rand(npairs) < 0.1] = -1.0 - rng.randint(0, 3)            # negative
                idx[rng.rand(npairs) < 0.1] += 0.75                               # truncated to the integer below
                if npairs >= 2:
                    idx[1] = idx[0]                                               # a duplicate pair
                if r % 7 == 3:
                    idx[-1] = np.nan
        v = (rng.randint(-8, 9, npairs) / 8.0) if values == "eighths" else rng.uniform(-1, 1, npairs)
        X[r, 0::2] = idx
        X[r, 1::2] = v.astype(np.float32)
    return X
