"""CPU checks of the sparse feature map restatement (tests/sparse_ref.py) against the oracle's dense map and against
finite differences of log Z."""
import numpy as np
import pytest

import orc
import sparse_ref as sr

MODELS = [(orc.STDFRAME, 1), (orc.STDSEG_NO_DUR_NO_SEGTRANSFTR, 3)]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.mark.parametrize("model,D", MODELS)
@pytest.mark.parametrize("use_tf", [False, True])
def test_restatement_equals_dense_bitwise(model, D, use_tf):
    # sorted, unique, in-range pairs, start 0, bias value 1: both sums add the same products in the same order (the
    # dense one also adds exact zeros)
    rng = np.random.RandomState(3 + use_tf)
    L, N, P, T = 4, 23, 6, 7
    lay = sr.SparseLayout(L, sfe=N - 1, tfe=N - 1, use_tf=use_tf)
    nseg = orc.num_segs(T, D)
    X = sr.random_windows(rng, nseg, P, N, sorted_unique=True)
    lam = rng.uniform(-1, 1, lay.lambda_len)
    S, M = sr.scores(lay, lam, X, T, D)
    cfg = orc.config(model_type=model, L=L, D=D, F=N, use_trans_ftrs=use_tf)
    olay = orc.Layout(cfg)
    assert olay.lambda_len == lay.lambda_len
    So, Mo = orc.seg_scores(cfg, olay, lam, sr.densify(lay, X), T)
    assert np.array_equal(_bits(S), _bits(So))
    assert np.array_equal(_bits(M), _bits(Mo))


@pytest.mark.parametrize("model,D", MODELS)
@pytest.mark.parametrize("use_tf", [False, True])
def test_gradient_matches_finite_differences(model, D, use_tf):
    rng = np.random.RandomState(11 + D)
    L, N, P, T = 3, 6, 3, 5
    lay = sr.SparseLayout(L, sfe=N - 1, tfe=N - 1, use_tf=use_tf)
    X = sr.random_windows(rng, orc.num_segs(T, D), P, N, messy=True)
    lam = rng.uniform(-0.5, 0.5, lay.lambda_len)
    if model == orc.STDFRAME:
        labels = rng.randint(0, L, T).astype(np.uint32)
    else:
        labels = orc.group_labels(rng.randint(0, L, T).astype(np.uint32), D, L)
    g, numer, zx = sr.gradient(lay, lam, X, labels, T, D, model)
    assert abs(zx - sr.log_z(lay, lam, X, T, D, model)) <= 1e-12 * abs(zx)
    # log likelihood = numer - zx: its derivative is the gradient; the numerator is linear in lambda
    h = 1e-5
    for i in range(lay.lambda_len):
        e = np.zeros(lay.lambda_len); e[i] = h
        dz = (sr.log_z(lay, lam + e, X, T, D, model) - sr.log_z(lay, lam - e, X, T, D, model)) / (2 * h)
        _, n_p, _ = sr.gradient(lay, lam + e, X, labels, T, D, model)
        dn = (n_p - numer) / h
        assert abs((dn - dz) - g[i]) <= 1e-6 * max(1.0, abs(g[i])), (i, dn - dz, g[i])


@pytest.mark.parametrize("model,D", MODELS)
@pytest.mark.parametrize("use_tf", [False, True])
def test_gradient_matches_dense_oracle(model, D, use_tf):
    # values in eighths: the duplicates' sums are exact in float, so the densified windows carry the same counts
    rng = np.random.RandomState(5 + D)
    L, N, P, T = 4, 9, 5, 8
    lay = sr.SparseLayout(L, sfe=N - 1, tfe=N - 1, use_tf=use_tf)
    X = sr.random_windows(rng, orc.num_segs(T, D), P, N, messy=True, values="eighths")
    lam = rng.uniform(-0.5, 0.5, lay.lambda_len)
    cfg = orc.config(model_type=model, L=L, D=D, F=N, use_trans_ftrs=use_tf)
    olay = orc.Layout(cfg)
    if model == orc.STDFRAME:
        labels = rng.randint(0, L, T).astype(np.uint32)
        rc, og, on, oz = orc.frame_build_gradient(cfg, olay, lam, sr.densify(lay, X), labels, T)
    else:
        labels = orc.group_labels(rng.randint(0, L, T).astype(np.uint32), D, L)
        rc, og, on, oz = orc.seg_build_gradient(cfg, olay, lam, sr.densify(lay, X), labels, T)
    assert rc == 0
    g, numer, zx = sr.gradient(lay, lam, X, labels, T, D, model)
    assert abs(zx - oz) <= 1e-12 * abs(oz)
    assert abs(numer - on) <= 1e-12 * max(1.0, abs(on))
    assert np.abs(g - og).max() <= 1e-10 * max(1.0, np.abs(og).max())


def test_unsorted_duplicate_and_out_of_range_pairs_by_hand():
    L, N = 2, 5
    lay = sr.SparseLayout(L, sfe=N - 1, tfe=N - 1, use_tf=True)
    lam = np.arange(lay.lambda_len, dtype=np.float64) * 0.5 + 1.0
    x = np.array([3, 0.5, 1, 2.0, 3, 0.25, 7, 9.0, -1, 3.0, 2.9, 1.5, np.nan, 1.0, 4, -2.0], dtype=np.float32)
    # kept: (3, .5) (1, 2) (3, .25) (2, 1.5) (4, -2); dropped: index 7 > sfe, -1, NaN
    s = lay.state_idx(1)
    want = 0.0
    for i, v in ((3, 0.5), (1, 2.0), (3, 0.25), (2, 1.5), (4, -2.0)):
        want += v * lam[s + i]
    want += lam[s + lay.nsf - 1]
    assert sr.state_value(lay, x, lam, 1) == want
    assert want == 0.5 * (1 + 0.5 * (s + 3)) + 2 * (1 + 0.5 * (s + 1)) + 0.25 * (1 + 0.5 * (s + 3)) + \
        1.5 * (1 + 0.5 * (s + 2)) - 2 * (1 + 0.5 * (s + 4)) + (1 + 0.5 * (s + 5))
    tw = lay.trans_idx(1, 0)
    assert sr.trans_value(lay, x, lam, 1, 0) == 0.5 * lam[tw + 3] + 2 * lam[tw + 1] + 0.25 * lam[tw + 3] + \
        1.5 * lam[tw + 2] - 2 * lam[tw + 4] + lam[tw + lay.ntf - 1]
    # counts: a duplicated index counts twice, the bias once with unit value
    ExpF = np.zeros(lay.lambda_len); grad = np.zeros(lay.lambda_len)
    sr.add_state_counts(lay, x, ExpF, grad, 0.25, 1, 1)
    assert grad[s + 3] == 0.75 and grad[s + 1] == 2.0 and grad[s + 2] == 1.5 and grad[s + 4] == -2.0 and grad[s + 0] == 0
    assert grad[s + lay.nsf - 1] == 1.0 and ExpF[s + lay.nsf - 1] == 0.25 and ExpF[s + 3] == 0.25 * 0.5 + 0.25 * 0.25
    assert sr.pair_index(np.float32(4.9), 4) == 4 and sr.pair_index(np.float32(5.0), 4) is None
    assert sr.pair_index(np.float32(-0.5), 4) is None and sr.pair_index(np.float32(2.0 ** 32), 2 ** 40) is None
