"""The input families of cases.family_frames (signed, rescaled per utterance, offset, tied) on the CPU oracle alone: the
conditions tests/test_gpu_input_ranges.py leans on.  The families are well formed; the oracle succeeds on every shape with
scores a few nats apart (so the GPU's scaled linear-domain recursion never has to give up); the tied cases' best paths
really run through the twin labels; and FASTLIN's 1e-6 gradient bound has room on every family: the exact mean in
place of the reference's float average moves the oracle gradient by at most 1e-7 of its largest component."""
import numpy as np
import pytest

import family_shapes as fs
from cases import FAMILIES, TIED_VALUES, Case
from family_shapes import FAMILY_NAMES, SHAPE_NAMES, SHAPES

SPREAD_CAP = 100.0     # nats; measured on these shapes: at most 16


def neg_zero(x):
    return bool((np.signbit(x) & (x == 0)).any())


@pytest.mark.parametrize("family", FAMILY_NAMES)
def test_families_are_well_formed(family):
    kw = SHAPES["mixed"][0]
    a, b, other = Case(seed=5, family=family, **kw), Case(seed=5, family=family, **kw), Case(seed=6, family=family, **kw)
    assert len(a.frames) == len(kw["Ts"])
    for u, T in enumerate(kw["Ts"]):
        x = a.frames[u]
        assert x.dtype == np.float32 and x.shape == (T, kw["in_w"])
        assert np.isfinite(x).all() and not neg_zero(x)
        assert x.tobytes() == b.frames[u].tobytes()
        # the context stream is rebuilt from the family's frames: first and last frame repeated
        c = kw["trans_ctx"]
        assert np.array_equal(a.frames2[u], np.concatenate([np.repeat(x[:1], c, 0), x, np.repeat(x[-1:], c, 0)]))
    assert any(a.frames[u].tobytes() != other.frames[u].tobytes() for u in range(len(kw["Ts"])))
    assert np.array_equal(a.lam, b.lam) and all(np.array_equal(p, q) for p, q in zip(a.labels, b.labels))
    F = a.F
    allx = np.concatenate([f.ravel() for f in a.frames])
    if family == "signed":
        assert (allx < 0).any() and (allx > 0).any() and 1.0 < np.abs(allx).max() <= FAMILIES[family]
    elif family == "offset":
        assert allx.min() >= 8.0 and allx.max() < 9.0
    elif family == "tied":
        assert set(np.unique(allx)) <= set(TIED_VALUES)
    # the weights follow the data: N(0, 3 / (nominal max|x| sqrt(F))) unless the caller says otherwise
    if family != "tied":     # (tied raises two state biases by 2)
        assert 0.8 < a.lam.std() * FAMILIES[family] * np.sqrt(F) / 3.0 < 1.25
    assert Case(seed=5, family=family, lam_scale=0.3, **kw).lam.std() > 0.2


def test_the_default_family_is_the_values_of_every_older_test():
    kw = SHAPES["mixed"][0]
    c = Case(seed=5, **kw)
    rng = np.random.RandomState(5)
    for u, T in enumerate(kw["Ts"]):
        assert c.frames[u].tobytes() == rng.random_sample((T, kw["in_w"])).astype(np.float32).tobytes()
    assert abs(c.lam.std() - 0.3) < 0.03


@pytest.mark.parametrize("shape", [s for s in SHAPE_NAMES if len(SHAPES[s][0]["Ts"]) >= 4])
def test_ranged_spans_a_factor_of_32_within_one_batch(shape):
    c = fs.case(shape, "ranged")
    m = [float(np.abs(f).max()) for f in c.frames]
    print("ranged %s: max|x| per utterance %s" % (shape, " ".join("%.3g" % v for v in m)))
    assert max(m) >= 32.0 * min(m)
    assert max(m) <= FAMILIES["ranged"]


@pytest.mark.parametrize("shape", SHAPE_NAMES)
def test_tied_has_windows_whose_extremum_is_attained_twice(shape):
    c = fs.case(shape, "tied")
    D = c.D
    n = 0
    for x in c.frames:
        for t in range(x.shape[0]):
            for d in range(2, min(D, t + 1) + 1):
                w = x[t - d + 1:t + 1]
                n += int(((w == w.max(0)).sum(0) >= 2).any() or ((w == w.min(0)).sum(0) >= 2).any())
    assert n >= 1 or D == 1


@pytest.mark.parametrize("family", FAMILY_NAMES)
@pytest.mark.parametrize("shape", SHAPE_NAMES)
def test_the_oracle_is_sound_and_scores_stay_a_few_nats_apart(shape, family):
    c, utts, (g, numer, zx) = fs.reference(shape, family)     # oracle_gradient asserts rc == 0 per utterance
    assert np.isfinite(g).all() and np.isfinite(numer).all() and np.isfinite(zx).all() and np.abs(g).max() > 0
    spread = max(float(S.max() - S.min()) for (_, S, *_rest) in utts)
    print("%s %s: score spread %.2f nats, max|x| %.3g" % (shape, family, spread, max(np.abs(f).max() for f in c.frames)))
    assert spread < SPREAD_CAP
    for u, (X, S, M, arcs, ns, fin, labs, cost) in enumerate(utts):
        assert labs is not None and np.isfinite(cost) and np.isfinite(arcs["w"]).all()
        assert not neg_zero(X)


@pytest.mark.parametrize("shape", SHAPE_NAMES)
def test_tied_best_paths_run_through_the_twin_labels(shape):
    c, utts, _ = fs.reference(shape, "tied")
    hit = [fs.uses_twin_labels(c, labs) for (*_x, labs, cost) in utts]
    print("tied %s: best path through a twin label in %d of %d utterances" % (shape, sum(hit), len(hit)))
    assert 2 * sum(hit) >= len(hit)


@pytest.mark.parametrize("shape", ["mixed", "fused", "mw", "nstate"])
def test_tied_twin_labels_score_alike(shape):
    """the twin's state scores are the first label's bit for bit, and so are the transition scores with either as previous
    or as current label: every path through one has a path of equal cost through the other"""
    c, utts, _ = fs.reference(shape, "tied")
    L, K = c.L, max(1, c.ocfg.num_states)
    ok = (c.olay.trans_idx != 0xffffffff).reshape(L, L)
    twin = lambda l: l - K if K <= l < 2 * K else l
    for (X, S, M, *_r) in utts:
        assert np.array_equal(S[:, K:2 * K], S[:, :K])
        Mm = M.reshape(M.shape[0], L, L)
        for p in range(L):
            for q in range(L):
                if ok[p, q] and ok[twin(p), twin(q)]:
                    assert np.array_equal(Mm[1:, p, q], Mm[1:, twin(p), twin(q)])


@pytest.mark.parametrize("family", FAMILY_NAMES)
@pytest.mark.parametrize("shape", ["fused", "config2"])
def test_the_fastlin_bound_has_room(shape, family):
    """FASTLIN takes the window average as the exact mean.  With float32(exact float64 mean) in the oracle's average block the
    oracle gradient moves by (measured) 3e-9 .. 2.6e-8 of its largest component: 1e-7 here leaves the GPU bound of 1e-6 a
    margin of about 40 for the tier's own reordered sums."""
    c, _, (g0, _, _) = fs.reference(shape, family)
    g1 = fs.gradient_with_exact_mean(c)
    dev = np.abs(g1 - g0).max() / np.abs(g0).max()
    print("exact mean against float average, %s %s: %.2e" % (shape, family, dev))
    assert dev <= 1e-7


@pytest.mark.parametrize("shape", fs.FUSED3)
def test_the_widened_decode_screen_has_entries_to_recompute(shape):
    """what the rescaling test of tests/test_gpu_input_ranges.py asserts of the screen's counts, from the oracle's scores: under
    SCRF_DECODE_BOUND_SCALE=30 the signed case lists some weights, and with the frames times 16 (weights over 16) at least
    as many -- with room for the kernel's own rounding on both sides (factors 28.9 and 31.1 bracket the kernel's count)"""
    c = fs.case(shape, "signed")
    r4, raw = fs.rescaled(c, 4)
    assert raw.any() and not raw.all()
    lo0, hi0 = fs.predicted_screen_count(c, 28.9), fs.predicted_screen_count(c, 31.1)
    lo4, hi4 = fs.predicted_screen_count(r4, 28.9), fs.predicted_screen_count(r4, 31.1)
    print("%s signed: screen count %d .. %d, frames times 16: %d .. %d" % (shape, lo0, hi0, lo4, hi4))
    assert 1 <= lo0 <= hi0 <= lo4 <= hi4
