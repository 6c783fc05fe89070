"""Shapes, seeds and oracle helpers shared by tests/test_input_families.py (CPU: the conditions) and
tests/test_gpu_input_ranges.py (GPU: the kernels) -- the input families of cases.family_frames on the smallest shape that
still selects each kernel path."""
import functools

import numpy as np

import orc
from cases import FAMILIES, Case

FAMILY_NAMES = ("signed", "ranged", "offset", "tied")

# name -> (Case keywords, batch_fused_mode under FAST where the parity tests pin it)
SHAPES = {
    "mixed":     (dict(L=6, D=4, in_w=5, Ts=[9, 14, 3, 1], trans_ctx=1), 1),
    "fused":     (dict(L=7, D=10, in_w=5, Ts=[9, 10, 11, 30]), 1),
    "config2":   (dict(L=48, D=25, in_w=39, Ts=[60, 33]), 1),
    "twogroups": (dict(L=50, D=5, in_w=45, Ts=[1, 13, 40]), 1),
    "mw":        (dict(L=70, D=3, in_w=4, Ts=[1, 2, 5, 9, 14]), 1),
    "hybrid":    (dict(L=65, D=5, in_w=70, Ts=[1, 2, 9, 30]), 3),
    "frame":     (dict(L=6, D=1, in_w=3, Ts=[4, 3, 9], trans_ctx=0, frame_model=True), None),
    "stdseg_lin": (dict(L=4, D=5, in_w=3, Ts=[4, 5, 6, 15], model_type=orc.STDSEG), None),
    "stdseg_tf": (dict(L=4, D=5, in_w=3, Ts=[4, 5, 6, 15], model_type=orc.STDSEG, trans_share=(0, 1)), None),
    "no_dur":    (dict(L=3, D=3, in_w=2, Ts=[1, 2, 3, 4, 7], model_type=orc.STDSEG_NO_DUR, trans_share=(0, 18)), None),
    "nstate":    (dict(L=6, D=4, in_w=3, Ts=[3, 4, 5, 12], trans_ctx=1, num_states=3), None),
}
SHAPE_NAMES = tuple(SHAPES)
FUSED3 = ("fused", "config2", "twogroups")        # the three shapes whose decode takes the fused score kernel
FASTLIN_FORM2 = ("mixed", "fused", "config2", "twogroups")   # FASTLIN's own kernels (batch_fused_mode 2)
POST_SHAPES = ("mixed", "fused", "mw")            # posteriors and pruned lattices

# seeds fixed so that the tied cases' best paths run through the twin labels (tests/test_input_families.py asserts it)
SEEDS = {(s, f): 1300 + 10 * i + j for i, s in enumerate(SHAPE_NAMES) for j, f in enumerate(FAMILY_NAMES)}
SEEDS.update({("mw", "tied"): 4343, ("hybrid", "tied"): 13353})   # (68 and 63 other labels compete with the twins)


def case(shape, family, **kw):
    return Case(seed=SEEDS[(shape, family)], family=family, **dict(SHAPES[shape][0], **kw))


def oracle_utterance(c, u):
    """the oracle's (S, M, arcs, n_states, final) of utterance u, with the score and lattice functions of c's model"""
    T = c.Ts[u]
    mt = c.ocfg.model_type
    X = c.windows(u)
    if mt == orc.STDSEG:
        S, M = orc.stdseg_scores(c.ocfg, c.olay, c.lam, X, T)
        arcs, ns, fin = orc.stdseg_lattice_arcs(c.ocfg, S, M, T)
    elif mt == orc.STDSEG_NO_DUR:
        S, M = orc.segtrans_scores(c.ocfg, c.olay, c.lam, X, T)
        arcs, ns, fin = orc.segtrans_lattice_arcs(c.ocfg, S, M, T)
    elif mt == orc.STDFRAME:
        S, M = orc.seg_scores(c.ocfg, c.olay, c.lam, X, T)
        arcs, ns, fin = orc.frame_lattice_arcs(c.ocfg, S, M, T)
    else:
        S, M = orc.seg_scores(c.ocfg, c.olay, c.lam, X, T)
        arcs, ns, fin = orc.seg_lattice_arcs(c.ocfg, S, M, T)
    return S, M, arcs, ns, fin


@functools.lru_cache(maxsize=None)
def reference(shape, family):
    """computed once per (shape, family) and left unchanged: the case, per utterance (windows, S, M, arcs, n_states, final,
    best labels, best cost), and the oracle gradient (grad, numer, zx)"""
    c = case(shape, family)
    utts = []
    for u in range(len(c.Ts)):
        S, M, arcs, ns, fin = oracle_utterance(c, u)
        labs, cost = orc.best_path(arcs, ns, fin)
        X = c.windows(u)
        for a in (X, S, M, arcs):
            a.flags.writeable = False
        utts.append((X, S, M, arcs, ns, fin, labs, cost))
    g, numer, zx = c.oracle_gradient()
    for a in (g, numer, zx):
        a.flags.writeable = False
    return c, utts, (g, numer, zx)


def gradient_with_exact_mean(c):
    """the oracle gradient of a one-stream segmental case on windows whose average block is float32(exact float64 mean)
    instead of the reference's float running sum over the length: the features FASTLIN stands for"""
    W, D = c.in_w, c.D
    g = np.zeros(c.olay.lambda_len)
    for u, T in enumerate(c.Ts):
        X = c.windows(u).copy()
        cs = np.vstack([np.zeros((1, W)), np.cumsum(c.frames[u].astype(np.float64), 0)])
        r = 0
        for t in range(T):
            for d in range(1, min(D, t + 1) + 1):
                X[r, 5 * W:6 * W] = ((cs[t + 1] - cs[t + 1 - d]) / d).astype(np.float32)
                r += 1
        assert r == X.shape[0]
        rc, g, n, z = orc.seg_build_gradient(c.ocfg, c.olay, c.lam, X, c.labels[u], T, grad=g)
        assert rc == 0, rc
    return g


def uses_twin_labels(c, labs):
    """does a best path (labels l + L * (d - 1)) run through one of the tied labels?  (STDSEG: full labels carry the
    duration themselves)"""
    K = max(1, c.ocfg.num_states)
    NL = c.ocfg.num_labs
    return any(int(v) % NL < 2 * K for v in labs)


def nominal(family):
    return FAMILIES[family]


def case_like(c, **cfg):
    """a shallow copy of c whose engine configuration differs: precision=, scratch_bytes="""
    import copy
    r = copy.copy(c)
    r.gcfg = type(c.gcfg).from_buffer_copy(c.gcfg)
    if "precision" in cfg:
        r.gcfg.train_precision = cfg.pop("precision")
    if "scratch_bytes" in cfg:
        r.gcfg.scratch_bytes = cfg.pop("scratch_bytes")
    assert not cfg, cfg
    return r


def rescaled(c, k):
    """c with the frames multiplied by 2^k and the weights of the raw-feature columns by 2^-k (the one-hot duration
    weights and both biases stay): every product and every float window average scales exactly, so the scores keep
    their bits.  Returns (the rescaled case, the mask of the rescaled weights)."""
    import copy
    r = copy.copy(c)
    s = np.float32(2.0 ** k)
    r.frames = [f * s for f in c.frames]
    if c.frames2 is not None:
        r.frames2 = [f * s for f in c.frames2]
    lay, L, W = c.olay, c.L, c.in_w
    raw = np.zeros(lay.lambda_len, dtype=bool)
    for l in range(L):
        raw[lay.state_idx[l]:lay.state_idx[l] + 8 * W] = True
        for p in range(L):
            i = int(lay.trans_idx[p * L + l])
            raw[i:i + lay.num_trans_funcs - 1] = True      # a context stream's columns; the transition bias is the last
    r.lam = np.where(raw, c.lam * 2.0 ** -k, c.lam)
    return r, raw


def predicted_screen_count(c, factor, with_bias_value=True):
    """how many float arc weights the fast-decode screen of k_scores_fused sends to k_decode_fixup under
    SCRF_DECODE_BOUND_SCALE=factor, from the oracle's scores: w = float(-S) is listed when float(-S -+ B) != w with
    B = factor * 1.01 * 2^-53 * (F + 1 + 3 W + 8) * xm(u) * |state block of o|_1 and
    xm(u) = nextafter(max(1, |state bias value|, max|x| of utterance u)).  (The kernel's S differs from the oracle's by
    some 1e-15, B is 1e-11 and more: a prediction to within a few entries, not a bit-exact one.)  with_bias_value=False: what
    a screen that left the bias value out of xm would list."""
    lay, W = c.olay, c.in_w
    nsf = lay.num_state_funcs
    w1 = np.array([np.abs(c.lam[lay.state_idx[l]:lay.state_idx[l] + nsf]).sum() for l in range(c.L)])
    scale = factor * 1.01 * 2.0 ** -53 * (nsf + 3 * W + 8)
    n = 0
    for u, T in enumerate(c.Ts):
        S, M = orc.seg_scores(c.ocfg, c.olay, c.lam, c.windows(u), T)
        xm = np.nextafter(np.float32(max(1.0, abs(c.ocfg.state_bias_val) if with_bias_value else 1.0, np.abs(c.frames[u]).max())), np.float32(np.inf))
        v = -S
        B = float(xm) * scale * w1[None, :]
        w = v.astype(np.float32)
        n += int((((v - B).astype(np.float32) != w) | ((v + B).astype(np.float32) != w)).sum())
    return n
