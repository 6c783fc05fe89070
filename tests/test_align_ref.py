"""not-gpu: the forced-alignment reference (tests/align_ref.py).  Its three forms -- the direct recursion, the
composition of the oracle's full lattice with the transcript acceptor, the enumeration of every admissible path -- agree bit
for bit; transcripts that do not fit give inf; aligning the oracle's own best path reproduces its cost."""
import numpy as np
import pytest

import align_ref as ar
import latprune_ref as lr
import orc
from cases import Case

# L <= 3, D <= 3, T <= 7: one transition matrix, one per frame, the frame model
SMALL = [
    dict(L=3, D=3, in_w=2, Ts=[1, 2, 3, 4, 7]),
    dict(L=2, D=2, in_w=3, Ts=[3, 5, 6], trans_ctx=1),
    dict(L=3, D=1, in_w=2, Ts=[1, 4, 6], trans_ctx=1, frame_model=True),
    dict(L=2, D=3, in_w=2, Ts=[6, 7]),
]


def bits(x):
    return np.float32(x).tobytes()


def transcripts(rng, T, L, D):
    """random admissible ones, one of every length 1 .. min(T, 4) and two that cannot fit"""
    out = [ar.random_transcript(rng, T, L, D) for _ in range(3)]
    out += [rng.randint(0, L, k).astype(np.uint32) for k in range(1, min(T, 4) + 1)]
    out += [rng.randint(0, L, T + 1).astype(np.uint32), np.zeros(0, dtype=np.uint32)]
    return out


@pytest.mark.parametrize("ci", range(len(SMALL)))
def test_the_three_forms_agree_bit_for_bit(ci):
    c = Case(seed=700 + ci, **SMALL[ci])
    rng = np.random.RandomState(70 + ci)
    L, D = c.L, c.D
    n = n_inf = 0
    for u, T in enumerate(c.Ts):
        w = ar.case_weights(c, u)
        arcs, ns, fin = lr.oracle_lattice(c, u)
        for ph in transcripts(rng, T, L, D):
            for mode in (ar.ONE, ar.RUNS):
                labs, c1 = ar.dp(w, ph, mode)
                c2 = ar.compose(arcs, ns, fin, L, ph, mode)
                c3 = ar.enumerate_(w, ph, mode)
                assert bits(c1) == bits(c2) == bits(c3), (u, ph, mode, c1, c2, c3)
                if ar.feasible(T, len(ph), D, mode):
                    assert np.isfinite(c1) and ar.matches(labs, L, ph, mode), (u, ph, mode, labs)
                    assert sum(l // L + 1 for l in labs) == T   # the path tiles [0, T)
                    n += 1
                else:
                    assert labs == [] and np.isinf(c1) and c1 > 0
                    n_inf += 1
    assert n > 10 and n_inf > 3, (n, n_inf)


def test_one_mode_needs_enough_duration():
    c = Case(seed=704, L=2, D=2, in_w=2, Ts=[7])
    w = ar.case_weights(c, 0)
    arcs, ns, fin = lr.oracle_lattice(c, 0)
    for K in (1, 2, 3):   # K * D < T
        ph = np.zeros(K, dtype=np.uint32)
        assert ar.dp(w, ph, ar.ONE) == ([], ar.INF)
        assert np.isinf(ar.compose(arcs, ns, fin, 2, ph, ar.ONE)) and np.isinf(ar.enumerate_(w, ph, ar.ONE))
        assert np.isfinite(ar.dp(w, ph, ar.RUNS)[1])
    assert np.isfinite(ar.dp(w, np.zeros(4, dtype=np.uint32), ar.ONE)[1])


@pytest.mark.parametrize("si", range(len(lr.GPU_SHAPES)))
def test_aligning_the_best_path_reproduces_its_cost(si):
    c = Case(seed=600 + si, **lr.GPU_SHAPES[si])
    L = c.L
    for u in range(len(c.Ts)):
        arcs, ns, fin = lr.oracle_lattice(c, u)
        labs, cost = orc.best_path(arcs, ns, fin)
        w = ar.case_weights(c, u)
        ph = np.asarray(labs, dtype=np.int64) % L
        l1, c1 = ar.dp(w, ph, ar.ONE)
        l2, c2 = ar.dp(w, ar.collapse(ph), ar.RUNS)
        assert bits(c1) == bits(cost) and bits(c2) == bits(cost), (u, cost, c1, c2)
        assert ar.matches(l1, L, ph, ar.ONE) and ar.matches(l2, L, ar.collapse(ph), ar.RUNS)
