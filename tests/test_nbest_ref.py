"""not-gpu: the N-best reference (tests/nbest_ref.py).  The list recursion and the enumeration of every path
agree bit for bit in their sorted costs, on the oracle's scores as they are, quantised to 0.5 (ties abound) and scaled by 1e4
(small weights are absorbed); the paths are distinct, every cost is the path's own sum, hypothesis 0 is the oracle's best
path, and an N above the path count returns every path."""
import functools

import numpy as np
import pytest

import align_ref as ar
import nbest_ref as nr
import orc
from cases import Case

# T <= 6, L <= 3, D <= 3: one transition matrix, one per frame, the frame model (one M and one per frame)
SMALL = [
    dict(L=3, D=3, in_w=2, Ts=[1, 2, 3, 4, 6]),
    dict(L=2, D=2, in_w=3, Ts=[1, 2, 5, 6], trans_ctx=1),
    dict(L=3, D=1, in_w=2, Ts=[1, 4, 6], trans_ctx=1, frame_model=True),
    dict(L=2, D=1, in_w=2, Ts=[2, 5], frame_model=True),
    dict(L=2, D=3, in_w=2, Ts=[3, 5, 6]),
    dict(L=3, D=2, in_w=2, Ts=[4, 5, 6], trans_ctx=1),
]
NS = (1, 2, 3, 5, 8, 40)
# (case, utterance, variant): the scores as they are for the first utterance of a case, then "ties" and "absorb" in turn
COMBOS = [(ci, u, (None, "ties", "absorb")[k]) for ci, kw in enumerate(SMALL) for u in range(len(kw["Ts"])) for k in ((0, 1, 2) if u == 0 else (1 + u % 2,))]


def bits(x):
    return np.float32(x).tobytes()


@functools.lru_cache(maxsize=None)
def weights(ci, u, kind):
    c = Case(seed=800 + ci, **SMALL[ci])
    return nr.variant(ar.case_weights(c, u), kind)


@functools.lru_cache(maxsize=None)
def every_path(ci, u, kind):
    return tuple((tuple(l), c) for l, c in nr.enumerate_all(weights(ci, u, kind)))


def test_there_are_about_forty_combinations_of_every_kind():
    assert 30 <= len(COMBOS) <= 50
    for kind in (None, "ties", "absorb"):
        assert sum(1 for c in COMBOS if c[2] == kind) >= 6
    assert any(SMALL[ci].get("frame_model") for ci, _, _ in COMBOS) and any("trans_ctx" in SMALL[ci] for ci, _, _ in COMBOS)


@pytest.mark.parametrize("ci,u,kind", COMBOS)
def test_recursion_and_enumeration_agree_bit_for_bit(ci, u, kind):
    w = weights(ci, u, kind)
    allp = every_path(ci, u, kind)
    assert len(allp) == nr.num_paths(w.T, w.L, w.D) == len(set(p for p, _ in allp))
    want = sorted(allp, key=lambda pc: pc[1])
    by_path = dict(allp)
    for N in NS:
        got = nr.nbest(w, N)
        assert len(got) == min(N, len(allp)), (N, len(got))
        assert [bits(c) for _, c in got] == [bits(c) for _, c in want[:len(got)]], (N, got, want[:len(got)])
        assert len(set(tuple(p) for p, _ in got)) == len(got)                       # pairwise distinct
        for p, c in got:
            assert bits(c) == bits(nr.path_cost(w, p)) == bits(by_path[tuple(p)])   # the path's own sum
            assert sum(l // w.L + 1 for l in p) == w.T
    if kind == "ties":
        costs = [c for _, c in allp]
        assert len(set(bits(c) for c in costs)) < len(costs) or len(costs) < 20   # the quantised scores do tie


@pytest.mark.parametrize("ci,u,kind", COMBOS)
def test_hypothesis_zero_is_the_oracles_best_path(ci, u, kind):
    w = weights(ci, u, kind)
    c = Case(seed=800 + ci, **SMALL[ci])
    if w.frame_model:
        arcs, ns, fin = orc.frame_lattice_arcs(c.ocfg, w.S, w.M.reshape(w.M.shape[0], -1), w.T)
    else:
        arcs, ns, fin = orc.seg_lattice_arcs(c.ocfg, w.S, w.M.reshape(w.M.shape[0], -1), w.T)
    labs, cost = orc.best_path(arcs, ns, fin)
    for N in (1, 5):
        p0, c0 = nr.nbest(w, N)[0]
        assert bits(c0) == bits(cost), (N, c0, cost)
        assert p0 == [int(x) for x in labs], (N, p0, labs)


@pytest.mark.parametrize("T,L,D,n", [(1, 3, 3, 3), (2, 2, 2, 6), (5, 2, 3, 152)])
def test_an_n_above_the_path_count_returns_every_path(T, L, D, n):
    ci, u = {(1, 3, 3): (0, 0), (2, 2, 2): (1, 1), (5, 2, 3): (4, 1)}[(T, L, D)]
    w = weights(ci, u, None)
    assert (w.T, w.L, w.D) == (T, L, D) and nr.num_paths(T, L, D) == n
    got = nr.nbest(w, n + 7)
    assert len(got) == n
    assert sorted(tuple(p) for p, _ in got) == sorted(p for p, _ in every_path(ci, u, None))
    c = [float(x) for _, x in got]
    assert c == sorted(c)
