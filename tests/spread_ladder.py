"""Weight families that spread the transition scores by a chosen number of nats, shared by tests/test_spread_ladder.py
(CPU: the conditions) and tests/test_gpu_spread_ladder.py (GPU: the kernels), on the shapes of tests/family_shapes.py.

The wavefront, linear-domain and STDSEG-linear recursions take the transition step on exp(M - max M).  np.exp(-X) is a
normal double up to X = 708.39, a subnormal one (fewer and fewer bits) up to 745.13 and zero beyond: the rungs below step
through all three regimes.  Each family puts the entries that carry posterior mass X nats below the matrix maximum in
another way; B = 1000 nats of state bias decide which labels carry mass.

lone_max   every transition bias is lowered by X except the one entry (q -> q) of the last label q, whose state bias is
           -B: the matrix maximum sits on a label without mass and every entry that carries mass lies X below it.  X then
           only prices the number of segments, so the posteriors stay spread over the other labels.
heavy_out  the state bias of label 0 (STDSEG: of every full label of phone 0) is +B and every transition OUT of those
           labels has the bias -X: the whole row of the labels that carry the mass is X below the rest.
heavy_in   the same with every transition INTO those labels at -X: one column of exp(M - max) is tiny, the rest is not."""
import functools

import numpy as np

import family_shapes as fs
import orc
from cases import Case

B = 1000.0
FAMILIES = ("lone_max", "heavy_out", "heavy_in")
FULL = (0, 600, 690, 705, 712, 720, 728, 735, 740, 742, 744.5, 746, 760, 900)
REDUCED = (0, 690, 735, 744.5, 900)
WINDOW = (705, 712, 720, 728, 735, 740, 742, 744.5, 746)      # the rungs around the subnormal range
SEED = 1700
NONE = 0xffffffff                                              # trans_idx of a transition the n-state topology lacks

SHAPES = {name: kw for name, (kw, _) in fs.SHAPES.items()}
SHAPES["stdseg480"] = dict(L=48, D=10, in_w=2, Ts=[12, 9], model_type=orc.STDSEG)   # 480 full labels: the TIMIT label space
SHAPE_NAMES = tuple(SHAPES)
FULL_SHAPES = ("mixed", "fused", "mw", "frame", "stdseg_lin")                       # the full ladder (under FAST)


def rungs(family, full):
    r = FULL if full else REDUCED
    return r + (1500,) if family == "heavy_out" else r


def heavy_labels(c):
    """label 0; under STDSEG every full label (duration, phone 0)"""
    if c.ocfg.model_type == orc.STDSEG:
        return [d0 * c.L for d0 in range(c.D)]
    return [0]


def designed_shift(c, family, X):
    """the design, stated apart from apply(): (lowered, set) boolean [NL, NL] masks over (previous, current) label -- the
    transition biases that are lowered by X and those that are set to -X -- and {label: state bias}"""
    NL = c.ocfg.num_labs
    lowered = np.zeros((NL, NL), dtype=bool); put = np.zeros((NL, NL), dtype=bool)
    if family == "lone_max":
        lowered[:] = True
        lowered[NL - 1, NL - 1] = False
        return lowered, put, {NL - 1: -B}
    hv = heavy_labels(c)
    if family == "heavy_out":
        put[hv, :] = True
    elif family == "heavy_in":
        put[:, hv] = True
    else:
        raise ValueError("unknown spread family %r" % (family,))
    return lowered, put, {l: B for l in hv}


def trans_bias_index(c, p, n):
    """index of the bias of transition p -> n in lambda (the last weight of its block), or None where the topology has none"""
    i = int(c.olay.trans_idx[p * c.ocfg.num_labs + n])
    return None if i == NONE else i + c.olay.num_trans_funcs - 1


def apply(c, family, X):
    """c with the family's weights at spread X (c.lam is replaced, not written into); every weight is touched once"""
    lay = c.olay
    NL = c.ocfg.num_labs
    lam = c.lam.copy()
    lowered, put, state = designed_shift(c, family, X)
    seen = set()
    for p in range(NL):
        for n in range(NL):
            i = trans_bias_index(c, p, n)
            if i is None or i in seen or not (lowered[p, n] or put[p, n]):
                continue
            seen.add(i)
            lam[i] = -float(X) if put[p, n] else lam[i] - X
    for l, v in state.items():
        lam[lay.state_idx[l] + lay.num_state_funcs - 1] = v
    c.lam = lam
    return c


def case(shape, family, X, **kw):
    return apply(Case(seed=SEED, lam_scale=0.1, **dict(SHAPES[shape], **kw)), family, X)


def wide_spread_case(prec):
    """heavy_out at 1500 nats on L = 4, D = 3: weights under which the scaled linear-domain and the wavefront recursions
    must give up where the reference's log-domain recursion succeeds -- the state bias of label 0 is +1000 (every frame's
    posterior mass sits on label 0 to 1000 nats) and every transition OUT of label 0 costs 1500 nats, so the whole
    transition row of the only label that carries mass lies more than 700 nats below the matrix maximum."""
    return apply(Case(L=4, D=3, in_w=3, Ts=[6, 9, 5], seed=17, precision=prec, lam_scale=0.1), "heavy_out", 1500)


def oracle_matrices(c):
    """the oracle's transition scores of every utterance, as [n, NL(previous), columns]: per frame, per window (STDSEG_NO_DUR)
    or per window over (previous full label, current phone) (STDSEG)"""
    out = []
    NL = c.ocfg.num_labs
    for u in range(len(c.Ts)):
        M = fs.oracle_utterance(c, u)[1]
        out.append(M if M.ndim == 3 else M.reshape(M.shape[0], NL, NL))
    return out


@functools.lru_cache(maxsize=None)
def reference(shape, family, X):
    """the oracle's (gradient, numerators, Zx) at one rung, computed once and left unchanged"""
    ref = case(shape, family, X).oracle_gradient()
    for a in ref:
        a.flags.writeable = False
    return ref
