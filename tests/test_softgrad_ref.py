"""not-gpu: the reference of the soft-alignment gradient (tests/softgrad_ref.py) checked against forms that
share nothing with it: central finite differences of A - Zx in WEIGHT space (through the oracle's scores at lambda +- h),
enumeration of every path of a transcript, the boundary posterior of transcript scoring, and the partition of the lattice by
the transcripts.

The finite-difference bound: the largest |fd - grad| over every weight of every case below, at h = 1e-6, was 1.53e-9 when
this test was written (noise eps |f| / h ~ 1e-16 * 10 / 1e-6 = 1e-9 plus the O(h^2) term); the assertion is at 100 times
that.  It moves with libm and the seed, which is what the factor is for."""
import itertools

import numpy as np
import pytest

import softgrad_ref as sg
import transcript_ref as tr
from cases import Case

FD_H = 1e-6
FD_BOUND = 1.6e-7   # 100 x the 1.53e-9 measured

FD_CASES = {
    "stdstate": dict(L=3, D=3, in_w=2, Ts=[6, 5], seed=11),
    "trans_ctx": dict(L=3, D=3, in_w=2, Ts=[6, 5], trans_ctx=1, seed=12),
    "frame": dict(L=3, D=1, in_w=2, Ts=[5], frame_model=True, seed=13),
    "frame_trans_ctx": dict(L=3, D=1, in_w=2, Ts=[5], frame_model=True, trans_ctx=1, seed=14),
}


@pytest.mark.parametrize("mode", [tr.ONE, tr.RUNS])
@pytest.mark.parametrize("name", sorted(FD_CASES))
def test_gradient_equals_finite_differences_in_weight_space(name, mode):
    c = Case(**FD_CASES[name])
    rng = np.random.RandomState(5 + mode)
    worst = 0.0
    for u, T in enumerate(c.Ts):
        ph = tr.random_transcript(rng, T, c.L, c.D, mode)
        gn, A, r, N = sg.numerator(c, u, ph, mode)
        gd, zx = sg.free_gradient(c, u)
        g = gn + gd
        fd = np.zeros_like(g)
        for i in range(g.shape[0]):
            lp = c.lam.copy(); lp[i] += FD_H
            lm = c.lam.copy(); lm[i] -= FD_H
            fd[i] = (sg.objective(c, u, ph, mode, lp) - sg.objective(c, u, ph, mode, lm)) / (2 * FD_H)
        assert np.abs(g).max() > 0.1   # the comparison is not one of zeros
        worst = max(worst, float(np.abs(fd - g).max()))
    print("%s mode %d: max |fd - grad| = %.3e" % (name, mode, worst))
    assert worst <= FD_BOUND


def enumerate_boundaries(w, phones, mode):
    """N [T, L, L] by enumeration of every (segmentation, run split) of the transcript, each path scored on its own"""
    T, L, D = w.T, w.L, w.D
    q = [int(p) for p in phones]
    K = len(q)
    paths = []
    for n in (range(K, T + 1) if mode == tr.RUNS else [K]):
        for durs in tr._compositions(T, n, D):
            for runs in (tr._compositions(n, K, n) if mode == tr.RUNS else [(1,) * K]):
                pos = list(itertools.chain.from_iterable([k] * r for k, r in enumerate(runs)))
                s, t, bnd = 0.0, -1, []
                for i, (d, k) in enumerate(zip(durs, pos)):
                    t += d
                    if i > 0:
                        s += w.Mt(t - d + 1)[q[pos[i - 1]], q[k]]
                        bnd.append((t - d + 1, q[pos[i - 1]], q[k]))
                    s += w.seg(t, d, q[k])
                paths.append((s, bnd))
    A = float(tr.lse0(np.array([p[0] for p in paths])))
    N = np.zeros((T, L, L))
    for s, bnd in paths:
        for t, p, c in bnd:
            N[t, p, c] += np.exp(s - A)
    return A, N


SMALL = [dict(L=2, D=2, in_w=2, Ts=[4, 6]), dict(L=3, D=3, in_w=2, Ts=[5, 6]), dict(L=3, D=2, in_w=2, Ts=[6, 3], trans_ctx=1),
         dict(L=3, D=1, in_w=2, Ts=[5, 2], frame_model=True, trans_ctx=1)]


@pytest.mark.parametrize("mode", [tr.ONE, tr.RUNS])
@pytest.mark.parametrize("si", range(len(SMALL)))
def test_transition_numerator_equals_enumeration_and_the_boundary_posterior(si, mode):
    c = Case(seed=40 + si, **SMALL[si])
    rng = np.random.RandomState(70 + si + 10 * mode)
    for u, T in enumerate(c.Ts):
        w = tr.case_scores(c, u)
        for ph in (tr.random_transcript(rng, T, c.L, c.D, mode), tr.random_transcript(rng, T, c.L, c.D, mode)):
            A, N = sg.trans_posteriors(w, ph, mode)
            A2, N2 = enumerate_boundaries(w, ph, mode)
            assert abs(A - A2) <= 1e-12 * max(1.0, abs(A2))
            assert np.abs(N - N2).max() <= 1e-12
            r = tr.dp(w, ph, mode)
            assert (N[0] == 0).all()
            for t in range(1, T):   # a boundary at t = a segment ends at t - 1
                assert abs(N[t].sum() - r.end_post[t - 1]) <= 1e-12


@pytest.mark.parametrize("mode", [tr.ONE, tr.RUNS])
@pytest.mark.parametrize("kw", [dict(L=2, D=2, in_w=2, Ts=[4]), dict(L=2, D=2, in_w=2, Ts=[4], trans_ctx=1),
                                dict(L=2, D=1, in_w=2, Ts=[4], frame_model=True)], ids=["stdstate", "trans_ctx", "frame"])
def test_the_transcripts_partition_the_lattice(kw, mode):
    """sum over every transcript q of P(q | x) E[f | x, q] = E[f | x]"""
    c = Case(seed=90, **kw)
    T = c.Ts[0]
    gd, zx = sg.free_gradient(c, 0)
    tot, mass = np.zeros_like(gd), 0.0
    for ph in tr.all_transcripts(c.L, T, c.D, mode):
        gn, A, _, _ = sg.numerator(c, 0, ph, mode)
        if np.isfinite(A):
            tot += np.exp(A - zx) * gn
            mass += np.exp(A - zx)
    assert abs(mass - 1.0) <= 1e-10
    assert np.abs(tot + gd).max() <= 1e-10
