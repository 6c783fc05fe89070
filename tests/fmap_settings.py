"""The feature map's settings off their defaults, on the shapes of tests/family_shapes.py: the table shared by
tests/test_fmap_settings.py (CPU: the conditions, from the oracle alone) and tests/test_gpu_fmap_settings.py (GPU: the kernels).

A row is (setting, shape): the overrides go to cases.Case(fmap=...), so the oracle and the engine get the same values.  Every
older case runs with both biases on, both bias values 1.0, all state columns from column 0 and transition columns that start
where the state columns end -- values under which a dropped factor, an off-by-one in a column count or a missing column
offset changes nothing."""
import functools

import numpy as np

import family_shapes as fs
import orc
from cases import Case
from family_shapes import FUSED3, SHAPE_NAMES, SHAPES

BIG = 40.0      # |state_bias_val| of big+ / big-; tests/test_fmap_settings.py holds the score spread under its cap at this value


def _dims(shape):
    """(Fs, F) of a shape: the width of stream 0's window (the state columns of the default map) and of the whole vector"""
    kw = SHAPES[shape][0]
    W, D = kw["in_w"], kw["D"]
    Fs = W if D == 1 else 8 * W + D
    c = kw.get("trans_ctx")
    return Fs, Fs + (0 if c is None else (2 * c + 1) * W)


def _vals(shape):
    return dict(state_bias_val=2.5, trans_bias_val=0.75 if shape == "nstate" else -0.5)   # n-state: the engine wants a value > 0


def _ssub(shape):
    return dict(sfs=1 if shape == "mixed" else 2, sfe=_dims(shape)[0] - 3)


def _tsub(shape):
    Fs, F = _dims(shape)
    return dict(tfs=Fs + 2, tfe=F - 3)


SUB = {
    "frame":     dict(sfs=1, sfe=1, tfs=0, tfe=1, state_bias_val=0.25, trans_bias_val=4.0),
    "stdseg_tf": dict(sfs=4, sfe=20, tfs=1, tfe=2, trans_bias_val=-2.0),
    "no_dur":    dict(sfs=2, tfs=3, tfe=10, use_state_bias=False),
    "nstate":    dict(sfs=1, state_bias_val=2.0, trans_bias_val=0.5),
}
NOT_NSTATE = tuple(s for s in SHAPE_NAMES if s != "nstate")

# setting -> (overrides of a shape, the shapes it runs on, batch_fused_mode under FAST: a number, "shape" = as
# family_shapes.SHAPES pins it, None = unpinned)
SETTINGS = {
    "vals":    (_vals, SHAPE_NAMES, "shape"),
    "nosb":    (lambda s: dict(use_state_bias=False), SHAPE_NAMES, "shape"),
    "notb":    (lambda s: dict(use_trans_bias=False), NOT_NSTATE, "shape"),
    "nobias":  (lambda s: dict(use_state_bias=False, use_trans_bias=False), NOT_NSTATE, "shape"),
    "nosf":    (lambda s: dict(use_state_ftrs=False, state_bias_val=2.5), SHAPE_NAMES, 0),
    "ssub":    (_ssub, ("fused", "mw", "hybrid", "mixed"), 0),
    "sdrop":   (lambda s: dict(sfe=8 * SHAPES[s][0]["in_w"] - 1), ("fused", "hybrid"), 0),     # no duration one-hot
    "tsub":    (_tsub, ("mixed",), 1),                                                        # (0 with SCRF_FUSE_MIXED=0)
    "overlap": (lambda s: dict(tfs=_dims(s)[0] - 4), ("mixed",), 0),
    "sub":     (lambda s: SUB[s], tuple(SUB), None),
    "big+":    (lambda s: dict(state_bias_val=BIG), FUSED3, 1),
    "big-":    (lambda s: dict(state_bias_val=-BIG), FUSED3, 1),
}
# the rows the engine refuses at scrf_create: the n-state topology is held by the transition bias
REFUSED = (("notb", "nstate"), ("nobias", "nstate"))
REFUSAL = "crf_states > 1 on a segmental model needs the transition bias"

# every row, and the `signed` twin of the vals rows: (setting, shape, family)
ROWS = tuple((st, sh, None) for st, (_, shapes, _m) in SETTINGS.items() for sh in shapes) + \
    tuple(("vals", sh, "signed") for sh in SHAPE_NAMES)
SEEDS = {(st, sh): 2100 + 20 * i + j for i, st in enumerate(SETTINGS) for j, sh in enumerate(SHAPE_NAMES)}


def row_id(row):
    return "%s-%s%s" % (row[0], row[1], "" if row[2] is None else "-" + row[2])


def overrides(setting, shape):
    return dict(SETTINGS[setting][0](shape))


def fast_mode(setting, shape):
    """batch_fused_mode the row must have under FAST, or None"""
    m = SETTINGS[setting][2]
    return SHAPES[shape][1] if m == "shape" else m


def has_bias_value(setting, shape):
    """does the row move a bias value off 1.0 (the rows the discrimination condition is about)?"""
    o = overrides(setting, shape)
    return o.get("state_bias_val", 1.0) != 1.0 or o.get("trans_bias_val", 1.0) != 1.0


def case(setting, shape, family=None, fmap=None, **kw):
    """the row's case; fmap= replaces the row's overrides (same seed: same frames and labels)"""
    return Case(seed=SEEDS[(setting, shape)], family=family, fmap=overrides(setting, shape) if fmap is None else fmap,
                **dict(SHAPES[shape][0], **kw))


@functools.lru_cache(maxsize=None)
def reference(setting, shape, family=None):
    """computed once per row and left unchanged, as family_shapes.reference: the case, per utterance (windows, S, M, arcs,
    n_states, final, best labels, best cost), and the oracle gradient (grad, numer, zx)"""
    c = case(setting, shape, family)
    utts = []
    for u in range(len(c.Ts)):
        S, M, arcs, ns, fin = fs.oracle_utterance(c, u)
        labs, cost = orc.best_path(arcs, ns, fin)
        X = c.windows(u)
        for a in (X, S, M, arcs):
            a.flags.writeable = False
        utts.append((X, S, M, arcs, ns, fin, labs, cost))
    g, numer, zx = c.oracle_gradient()
    for a in (g, numer, zx):
        a.flags.writeable = False
    return c, utts, (g, numer, zx)


def bias_masks(c):
    """(state-bias weights, transition-bias weights) of c's layout as boolean masks over lambda"""
    lay, cfg = c.olay, c.ocfg
    sb = np.zeros(lay.lambda_len, dtype=bool); tb = np.zeros(lay.lambda_len, dtype=bool)
    if cfg.use_state_bias:
        sb[lay.state_idx.astype(np.int64) + lay.num_state_funcs - 1] = True
    if cfg.use_trans_bias:
        ti = lay.trans_idx[lay.trans_idx != 0xffffffff].astype(np.int64)
        tb[ti + lay.num_trans_funcs - 1] = True
    return sb, tb


# (setting, shape) -> (lambda_len, num_state_funcs, num_trans_funcs), written out by hand from the map's definition: per
# label a block of [state columns][state bias] and, per previous label, [transition columns][transition bias]; STDSEG runs
# over L * D labels; the n-state map has L state blocks and P^2 + 2 L - P transition blocks (P = L / 3 phones)
EXPECT = {
    ("vals", "mixed"): (846, 45, 16),
    ("vals", "fused"): (406, 51, 1),
    ("vals", "config2"): (18528, 338, 1),
    ("vals", "twogroups"): (20800, 366, 1),
    ("vals", "mw"): (7420, 36, 1),
    ("vals", "hybrid"): (41015, 566, 1),
    ("vals", "frame"): (168, 4, 4),
    ("vals", "stdseg_lin"): (1000, 30, 1),
    ("vals", "stdseg_tf"): (1800, 30, 3),
    ("vals", "no_dur"): (240, 20, 20),
    ("vals", "nstate"): (314, 29, 10),
    ("nosb", "mixed"): (840, 44, 16),
    ("nosb", "fused"): (399, 50, 1),
    ("nosb", "config2"): (18480, 337, 1),
    ("nosb", "twogroups"): (20750, 365, 1),
    ("nosb", "mw"): (7350, 35, 1),
    ("nosb", "hybrid"): (40950, 565, 1),
    ("nosb", "frame"): (162, 3, 4),
    ("nosb", "stdseg_lin"): (980, 29, 1),
    ("nosb", "stdseg_tf"): (1780, 29, 3),
    ("nosb", "no_dur"): (237, 19, 20),
    ("nosb", "nstate"): (308, 28, 10),
    ("notb", "mixed"): (810, 45, 15),
    ("notb", "fused"): (357, 51, 0),
    ("notb", "config2"): (16224, 338, 0),
    ("notb", "twogroups"): (18300, 366, 0),
    ("notb", "mw"): (2520, 36, 0),
    ("notb", "hybrid"): (36790, 566, 0),
    ("notb", "frame"): (132, 4, 3),
    ("notb", "stdseg_lin"): (600, 30, 0),
    ("notb", "stdseg_tf"): (1400, 30, 2),
    ("notb", "no_dur"): (231, 20, 19),
    ("nobias", "mixed"): (804, 44, 15),
    ("nobias", "fused"): (350, 50, 0),
    ("nobias", "config2"): (16176, 337, 0),
    ("nobias", "twogroups"): (18250, 365, 0),
    ("nobias", "mw"): (2450, 35, 0),
    ("nobias", "hybrid"): (36725, 565, 0),
    ("nobias", "frame"): (126, 3, 3),
    ("nobias", "stdseg_lin"): (580, 29, 0),
    ("nobias", "stdseg_tf"): (1380, 29, 2),
    ("nobias", "no_dur"): (228, 19, 19),
    ("nosf", "mixed"): (582, 1, 16),
    ("nosf", "fused"): (56, 1, 1),
    ("nosf", "config2"): (2352, 1, 1),
    ("nosf", "twogroups"): (2550, 1, 1),
    ("nosf", "mw"): (4970, 1, 1),
    ("nosf", "hybrid"): (4290, 1, 1),
    ("nosf", "frame"): (150, 1, 4),
    ("nosf", "stdseg_lin"): (420, 1, 1),
    ("nosf", "stdseg_tf"): (1220, 1, 3),
    ("nosf", "no_dur"): (183, 1, 20),
    ("nosf", "nstate"): (146, 1, 10),
    ("ssub", "fused"): (378, 47, 1),
    ("ssub", "mw"): (7140, 32, 1),
    ("ssub", "hybrid"): (40755, 562, 1),
    ("ssub", "mixed"): (828, 42, 16),
    ("sdrop", "fused"): (336, 41, 1),
    ("sdrop", "hybrid"): (40690, 561, 1),
    ("tsub", "mixed"): (702, 45, 12),
    ("overlap", "mixed"): (990, 45, 20),
    ("sub", "frame"): (120, 2, 3),
    ("sub", "stdseg_tf"): (1560, 18, 3),
    ("sub", "no_dur"): (132, 17, 9),
    ("sub", "nstate"): (308, 28, 10),
    ("big+", "fused"): (406, 51, 1),
    ("big+", "config2"): (18528, 338, 1),
    ("big+", "twogroups"): (20800, 366, 1),
    ("big-", "fused"): (406, 51, 1),
    ("big-", "config2"): (18528, 338, 1),
    ("big-", "twogroups"): (20800, 366, 1),
}
