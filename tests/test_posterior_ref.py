"""not-gpu: the numpy reference of the posterior output (tests/post_ref.py) against an enumeration of every
(segmentation, labelling) on the utterances small enough for one, and its sum-to-one properties on the six parity shapes.
It checks the checker the GPU tests (tests/test_gpu_posteriors.py) compare the engine with."""
import numpy as np
import pytest

import orc
import post_ref
from cases import Case


def n_paths(T, D, L):
    """(segmentation, labelling) pairs of an utterance"""
    w = [1] + [0] * T
    for t in range(1, T + 1):
        w[t] = sum(w[t - d] * L for d in range(1, min(D, t) + 1))
    return w[T]


@pytest.mark.parametrize("ci", [0, 1, 2])
def test_reference_equals_enumeration_on_small_utterances(ci):
    c = Case(seed=100 + ci, **post_ref.CASES[ci])
    done = 0
    for u, T in enumerate(c.Ts):
        if T > 7 or n_paths(T, c.D, c.L) > 300000:
            continue
        S, M = orc.seg_scores(c.ocfg, c.olay, c.lam, c.windows(u), T)
        g, occ, end, zx = post_ref.utterance(c, u)
        gb, zb, n = post_ref.enumerate_paths(S, M, T, c.D, c.L)
        assert n == n_paths(T, c.D, c.L)
        assert abs(zb - zx) <= 1e-12 * max(1, abs(zx))
        assert np.abs(gb - g).max() <= 1e-13
        ob, eb = post_ref.occupancy(gb, T, c.D, c.L)
        assert np.abs(ob - occ).max() <= 1e-13 and np.abs(eb - end).max() <= 1e-13
        done += 1
    assert done >= 2


@pytest.mark.parametrize("ci", range(len(post_ref.CASES)))
def test_reference_rows_sum_to_one(ci):
    c = Case(seed=100 + ci, **post_ref.CASES[ci])
    for u, T in enumerate(c.Ts):
        g, occ, end, zx = post_ref.utterance(c, u)
        assert (g >= 0).all()
        assert np.abs(occ.sum(1) - 1).max() <= 1e-12
        assert abs(end[-1] - 1) <= 1e-12
        assert (end <= 1 + 1e-12).all()


def test_frame_chain_is_the_occupancy_at_duration_one():
    """D = 1: the occupancy formed from gamma is the node posterior exp(alpha + beta - Zx) of a plain chain -- for the
    segmental model with maximum duration 1 and for the frame model"""
    for c in (Case(seed=102, **post_ref.CASES[2]),
              Case(L=6, D=1, in_w=3, Ts=[4, 3, 4, 9], trans_ctx=0, seed=5, frame_model=True)):
        for u, T in enumerate(c.Ts):
            S, M = orc.seg_scores(c.ocfg, c.olay, c.lam, c.windows(u), T)
            g, occ, end, zx = post_ref.utterance(c, u)
            p, z = post_ref.frame_chain(S, M)
            assert abs(z - zx) <= 1e-12 * max(1, abs(zx))
            assert np.abs(p - occ).max() <= 1e-13
            assert np.abs(end - 1).max() <= 1e-12


def test_segment_queries_follow_the_viterbi_label_convention():
    L, D = 3, 4
    labs = [1 + L * 0, 2 + L * 2, 0 + L * 3]          # durations 1, 3, 4
    assert post_ref.segments_of(labs, L) == [(0, 1, 1), (3, 3, 2), (7, 4, 0)]
    T = 8
    g = np.arange(orc.num_segs(T, D) * L, dtype=float).reshape(-1, L)
    sp = post_ref.seg_post(g, labs, L, D)
    assert sp[1] == g[orc.seg_base(3, D) + 2, 2]
