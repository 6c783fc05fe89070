"""not-gpu: the transcript-scoring reference (tests/transcript_ref.py).  Its three forms -- the recursion, the
oracle's full lattice composed with the transcript acceptor in the log semiring, the enumeration of every admissible path --
agree; the posteriors are normalised; the transcripts partition the lattice (sum over q of exp(A(q)) = exp(Zx)) and mixing the
transcript-conditioned posteriors by P(q | x) gives back the free ones; transcripts that do not fit give -inf and zeros."""
import numpy as np
import pytest

import latprune_ref as lr
import orc
import post_ref
import transcript_ref as tr
from cases import Case

# small enough to enumerate: T <= 6, L <= 3, D <= 3; one transition matrix, one per frame, the frame model
SMALL = [
    dict(L=3, D=3, in_w=2, Ts=[1, 2, 3, 4, 6]),
    dict(L=2, D=2, in_w=3, Ts=[3, 5, 6], trans_ctx=1),
    dict(L=3, D=1, in_w=2, Ts=[1, 4, 6], trans_ctx=1, frame_model=True),
    dict(L=2, D=3, in_w=2, Ts=[5, 6]),
]
# (shape, utterance) pairs whose every transcript is summed: L = 2, T = 5, D = 3 has 60 (ONE) and 10 (RUNS)
PARTITION = [(3, 0), (0, 3), (1, 1), (2, 1)]


def transcripts(rng, T, L, D, mode):
    """random admissible ones, one of every length 1 .. min(T, 4) and two that cannot fit"""
    out = [tr.random_transcript(rng, T, L, D, mode) for _ in range(3)]
    out += [rng.randint(0, L, k).astype(np.uint32) for k in range(1, min(T, 4) + 1)]
    out += [rng.randint(0, L, T + 1).astype(np.uint32), np.zeros(0, dtype=np.uint32)]
    if mode == tr.RUNS:
        out = [tr.collapse(p).astype(np.uint32) for p in out]
    return out


def free_posteriors(c, u):
    """(occ [T, L], end [T], Zx) of the free lattice"""
    T = c.Ts[u]
    if c.ocfg.model_type == orc.STDFRAME:
        S, M = orc.seg_scores(c.ocfg, c.olay, c.lam, c.windows(u), T)
        occ, zx = post_ref.frame_chain(np.asarray(S).reshape(T, c.L), np.asarray(M).reshape(T, c.L * c.L))
        return occ, np.ones(T), zx
    g, occ, end, zx = post_ref.utterance(c, u)
    return occ, end, zx


@pytest.mark.parametrize("ci", range(len(SMALL)))
def test_the_three_forms_agree(ci):
    c = Case(seed=900 + ci, **SMALL[ci])
    rng = np.random.RandomState(90 + ci)
    L, D = c.L, c.D
    n = n_inf = 0
    for u, T in enumerate(c.Ts):
        w = tr.case_scores(c, u)
        arcs, ns, fin = lr.oracle_lattice(c, u)
        for mode in (tr.ONE, tr.RUNS):
            for ph in transcripts(rng, T, L, D, mode):
                r1 = tr.dp(w, ph, mode)
                r2 = tr.compose(w, arcs, ns, fin, ph, mode)
                r3 = tr.enumerate_(w, ph, mode)
                if not tr.feasible(T, len(ph), D, mode):
                    for r in (r1, r2, r3):
                        assert r.A == -np.inf and not r.g.any() and not r.frame_post.any() and not r.end_post.any(), (u, ph, mode)
                    n_inf += 1
                    continue
                for r in (r2, r3):
                    assert abs(r.A - r1.A) <= 1e-12 * max(1.0, abs(r1.A)), (u, ph, mode, r1.A, r.A)
                    assert np.abs(r.g - r1.g).max() <= 1e-12
                    assert np.abs(r.frame_post - r1.frame_post).max() <= 1e-12
                    assert np.abs(r.end_post - r1.end_post).max() <= 1e-12
                assert np.abs(r1.frame_post.sum(axis=1) - 1.0).max() <= 1e-12
                assert abs(r1.end_post[T - 1] - 1.0) <= 1e-12
                n += 1
    assert n > 10 and n_inf > 3, (n, n_inf)


@pytest.mark.parametrize("ci,u", PARTITION)
@pytest.mark.parametrize("mode", [tr.ONE, tr.RUNS])
def test_the_transcripts_partition_the_lattice(ci, u, mode):
    c = Case(seed=900 + ci, **SMALL[ci])
    T, L, D = c.Ts[u], c.L, c.D
    w = tr.case_scores(c, u)
    occ, end, zx = free_posteriors(c, u)
    qs = tr.all_transcripts(L, T, D, mode)
    if (L, T, D) == (2, 5, 3):
        assert len(qs) == (60 if mode == tr.ONE else 10)
    tot = 0.0
    mix_occ = np.zeros((T, L)); mix_end = np.zeros(T)
    for ph in qs:
        r = tr.dp(w, ph, mode)
        p = np.exp(r.A - zx)
        tot += p
        mix_occ += p * r.frame_post
        mix_end += p * r.end_post
    assert abs(tot - 1.0) <= 1e-12, tot
    # total probability: the free posteriors are the mixture of the transcript-conditioned ones
    assert np.abs(mix_occ - occ).max() <= 1e-12
    assert np.abs(mix_end - end).max() <= 1e-12


def test_queries_follow_the_positions():
    c = Case(seed=903, **SMALL[3])
    w = tr.case_scores(c, 0)   # T = 5, D = 3
    ph = np.array([1, 0, 1], dtype=np.uint32)
    for mode in (tr.ONE, tr.RUNS):
        r = tr.dp(w, ph, mode)
        labs = [1 + 2 * 1, 0 + 2 * 0, 1 + 2 * 1]   # durations 2, 1, 2
        sp = r.queries(labs)
        # label 1 sits at positions 0 and 2: the query adds both, and is bounded by the boundary posterior
        assert sp[0] == r.g[orc.seg_base(1, 3) + 1, [0, 2]].sum() and sp[1] == r.g[orc.seg_base(2, 3), 1]
        assert (sp <= r.end_post[[1, 2, 4]] + 1e-15).all() and (sp > 0).all()


def test_one_mode_needs_enough_duration():
    c = Case(seed=904, L=2, D=2, in_w=2, Ts=[6])
    w = tr.case_scores(c, 0)
    for K in (1, 2):   # K * D < T
        ph = (np.arange(K) % 2).astype(np.uint32)
        assert tr.dp(w, ph, tr.ONE).A == -np.inf and tr.enumerate_(w, ph, tr.ONE).A == -np.inf
        assert np.isfinite(tr.dp(w, ph, tr.RUNS).A)
    assert np.isfinite(tr.dp(w, np.array([0, 1, 0], dtype=np.uint32), tr.ONE).A)
