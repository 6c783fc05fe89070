"""Sparse feature maps (stdsparse / stdsparsetrans) on the device against the CPU restatement (tests/sparse_ref.py)
and the oracle's DP, lattice and best path."""
import numpy as np
import pytest

import orc
import scrf_amd
import sparse_ref as sr

MODELS = [(scrf_amd.STDFRAME, 1), (scrf_amd.STDSEG_NO_DUR_NO_SEGTRANSFTR, 4)]
TIERS = [scrf_amd.PREC_EXACT, scrf_amd.PREC_FAST, scrf_amd.PREC_FAST32, scrf_amd.PREC_FASTLIN]


class SCase:
    def __init__(self, model, D, use_tf, L=5, N=40, P=6, Ts=(9, 14, 6), seed=0, frames=False, precision=0,
                 scratch_bytes=0, values=None):
        self.model, self.D, self.use_tf, self.L, self.N, self.P, self.Ts = model, D, use_tf, L, N, P, list(Ts)
        self.frames_in = frames
        rng = np.random.RandomState(seed)
        self.lay = sr.SparseLayout(L, sfe=N - 1, tfe=N - 1, use_tf=use_tf)
        self.F = 2 * P
        if frames:   # raw pair frames; windows synthesised by the engine (first-frame windows for the segmental model)
            self.frames = [sr.random_windows(rng, T, P, N, messy=True, values=values) for T in self.Ts]
        else:
            self.X = [sr.random_windows(rng, orc.num_segs(T, D), P, N, messy=True, values=values) for T in self.Ts]
        if model == scrf_amd.STDFRAME:
            self.labels = [rng.randint(0, L, T).astype(np.uint32) for T in self.Ts]
        else:
            self.labels = [orc.group_labels(rng.randint(0, L, T).astype(np.uint32), D, L) for T in self.Ts]
        self.lam = rng.uniform(-0.5, 0.5, self.lay.lambda_len)
        self.cfg = scrf_amd.make_config(model_type=model, L=L, D=D, F=self.F, sfe=N - 1, tfe=N - 1, use_trans_ftrs=use_tf,
                                        sparse=True, precision=precision, scratch_bytes=scratch_bytes,
                                        state_bias_val=2.5, trans_bias_val=0.5)   # not applied by a sparse map

    def engine(self):
        eng = scrf_amd.Engine(self.cfg)
        assert eng.lambda_len == self.lay.lambda_len
        eng.set_lambda(self.lam)
        return eng

    def batch(self, eng, labels=None):
        labels = self.labels if labels is None else labels
        if self.frames_in:
            return eng.batch_from_frames(self.frames, labels, recipes=[scrf_amd.StreamRecipe(self.F, 0, 0, 0)])
        return eng.batch_from_windows(self.X, self.Ts, labels)

    def windows(self, eng, b, u):
        if not self.frames_in:
            return self.X[u]
        X = eng.windows(b, u, self.Ts[u])
        assert np.array_equal(X.view(np.uint32), orc.windows(self.frames[u], self.D, extract_seg=False).view(np.uint32))
        return X

    def oracle_arcs(self, S, M, T):
        ocfg = sr.ocfg(self.lay, self.model, self.D)
        if self.model == scrf_amd.STDFRAME:
            return orc.frame_lattice_arcs(ocfg, S, M, T)
        return orc.seg_lattice_arcs(ocfg, S, M, T)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def test_refused_configurations():
    def create(**kw):
        base = dict(model_type=scrf_amd.STDSEG_NO_DUR_NO_SEGTRANSFTR, L=4, D=3, F=8, sfe=20, sparse=True)
        base.update(kw)
        with pytest.raises(scrf_amd.ScrfError) as e:
            scrf_amd.Engine(scrf_amd.make_config(**base))
        return str(e.value)
    assert "stdseg" in create(model_type=scrf_amd.STDSEG, L=6, D=3)
    assert "stdseg_no_dur" in create(model_type=scrf_amd.STDSEG_NO_DUR)
    assert "crf_featuremap must be \"stdstate\" for \"stdseg_no_dur_no_transftr\"" in create(model_type=scrf_amd.STDSEG_NO_DUR_NO_TRANSFTR)
    assert "crf_states = 1" in create(num_states=2)
    assert "even" in create(F=7)
    assert "index start 0" in create(sfs=1)
    assert "index start 0" in create(use_trans_ftrs=True, tfs=2)


@pytest.mark.gpu
@pytest.mark.parametrize("model,D", MODELS)
def test_accepted_configurations(model, D):
    for mt in (scrf_amd.STDSPARSE, scrf_amd.STDSPARSETRANS):
        cfg = scrf_amd.make_config(model_type=model, L=4, D=D, F=8, sfe=99, tfe=49, use_trans_ftrs=mt == scrf_amd.STDSPARSETRANS,
                                   map_type=mt)
        eng = scrf_amd.Engine(cfg)
        lay = sr.SparseLayout(4, 99, 49, use_tf=mt == scrf_amd.STDSPARSETRANS)
        assert eng.lambda_len == lay.lambda_len and eng.num_state_funcs() == lay.nsf and eng.num_trans_funcs() == lay.ntf
        assert eng.state_idx(3, 7) == lay.state_idx(3) + 7 and eng.trans_idx(2, 1, 5) == lay.trans_idx(2, 1) + 5
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("model,D", MODELS)
@pytest.mark.parametrize("use_tf", [False, True])
@pytest.mark.parametrize("frames", [False, True])
def test_scores_arcs_viterbi_bitwise(model, D, use_tf, frames):
    c = SCase(model, D, use_tf, frames=frames, seed=1 + use_tf + 2 * frames)
    eng = c.engine()
    b = c.batch(eng)
    assert eng.batch_is_fused(b) == 0
    labs, cost = eng.viterbi_batch(b)
    for u, T in enumerate(c.Ts):
        X = c.windows(eng, b, u)
        S, M = eng.scores(b, u, T)
        rS, rM = sr.scores(c.lay, c.lam, X, T, D)
        assert np.array_equal(_bits(S), _bits(rS))
        assert np.array_equal(_bits(M), _bits(rM))
        arcs, ns, fin = eng.lattice_arcs(b, u)
        oarcs, ons, ofin = c.oracle_arcs(rS, rM, T)
        assert (ns, fin) == (ons, ofin)
        assert arcs.tobytes() == oarcs.tobytes()
        ol, oc = orc.best_path(oarcs, ons, ofin)
        assert list(labs[u]) == list(ol) and np.float32(cost[u]) == np.float32(oc)
    b.close(); eng.close()


def _restated(c, eng, b):
    g = np.zeros(c.lay.lambda_len); numer = []; zx = []
    for u, T in enumerate(c.Ts):
        gu, nu, zu = sr.gradient(c.lay, c.lam, c.windows(eng, b, u), c.labels[u], T, c.D, c.model)
        g += gu; numer.append(nu); zx.append(zu)
    return g, np.array(numer), np.array(zx)


def _close(a, b, rel):
    return np.abs(a - b).max() <= rel * max(1.0, np.abs(b).max())


@pytest.mark.gpu
@pytest.mark.parametrize("model,D", MODELS)
@pytest.mark.parametrize("use_tf", [False, True])
@pytest.mark.parametrize("prec", TIERS)
def test_gradient_every_tier(model, D, use_tf, prec):
    c = SCase(model, D, use_tf, precision=prec, frames=prec == scrf_amd.PREC_FAST, seed=7)
    eng = c.engine()
    b = c.batch(eng)
    numer, zx = eng.fb_batch(b)
    g = eng.get_grad()
    rg, rn, rz = _restated(c, eng, b)
    assert _close(numer, rn, 1e-9) and _close(zx, rz, 1e-9)
    assert _close(g, rg, 1e-9)
    b.close(); eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("model,D", MODELS)
def test_wide_index_space_and_many_pairs(model, D):
    # > 64 pairs per window (several pair groups per wavefront) and > 8192 indices (several counter windows of the sort)
    c = SCase(model, D, True, L=3, N=20000, P=70, Ts=(5, 7), seed=9)
    eng = c.engine()
    b = c.batch(eng)
    numer, zx = eng.fb_batch(b)
    rg, rn, rz = _restated(c, eng, b)
    assert _close(eng.get_grad(), rg, 1e-9) and _close(zx, rz, 1e-9)
    S, M = eng.scores(b, 1, 7)
    rS, rM = sr.scores(c.lay, c.lam, c.X[1], 7, D)
    assert np.array_equal(_bits(S), _bits(rS)) and np.array_equal(_bits(M), _bits(rM))
    b.close(); eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("use_tf", [False, True])
def test_exact_reproducible_and_chunked(use_tf):
    model, D = scrf_amd.STDSEG_NO_DUR_NO_SEGTRANSFTR, 4
    Ts = [9, 14, 6, 11, 3, 17, 8, 12]
    c = SCase(model, D, use_tf, Ts=Ts, seed=3)
    eng = c.engine()
    b = c.batch(eng)
    runs = []
    for _ in range(2):
        eng.zero_grad()
        eng.fb_batch(b)
        runs.append(eng.get_grad())
    assert runs[0].tobytes() == runs[1].tobytes()
    b.close(); eng.close()
    small = SCase(model, D, use_tf, Ts=Ts, seed=3, scratch_bytes=96 * 1024)   # several chunks
    eng2 = small.engine()
    b2 = small.batch(eng2)
    eng2.fb_batch(b2)
    assert _close(eng2.get_grad(), runs[0], 1e-12)
    b2.close(); eng2.close()


@pytest.mark.gpu
def test_bad_label_leaves_gradient_untouched():
    c = SCase(scrf_amd.STDSEG_NO_DUR_NO_SEGTRANSFTR, 4, True, seed=4)
    eng = c.engine()
    b = c.batch(eng)
    eng.fb_batch(b)
    g0 = eng.get_grad()
    bad = [l.copy() for l in c.labels]
    bad[1][5] = c.L * c.D + 3
    bb = c.batch(eng, bad)
    with pytest.raises(scrf_amd.ScrfError) as e:
        eng.fb_batch(bb)
    assert e.value.code == 5
    assert eng.get_grad().tobytes() == g0.tobytes()
    b.close(); bb.close(); eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("model,D", MODELS)
@pytest.mark.parametrize("use_tf", [False, True])
def test_sparse_equals_dense_on_densified_windows(model, D, use_tf):
    c = SCase(model, D, use_tf, seed=5, values="eighths")   # duplicate sums exact in float
    eng = c.engine()
    b = c.batch(eng)
    eng.fb_batch(b)
    g = eng.get_grad()
    cfg = scrf_amd.make_config(model_type=model, L=c.L, D=D, F=c.N, use_trans_ftrs=use_tf)
    dense = scrf_amd.Engine(cfg)
    dense.set_lambda(c.lam)
    db = dense.batch_from_windows([sr.densify(c.lay, X) for X in c.X], c.Ts, c.labels)
    dense.fb_batch(db)
    assert _close(g, dense.get_grad(), 1e-9)
    b.close(); db.close(); eng.close(); dense.close()


@pytest.mark.gpu
@pytest.mark.parametrize("model,D", MODELS)
@pytest.mark.parametrize("prec", [scrf_amd.PREC_EXACT, scrf_amd.PREC_FAST])
def test_buckets_of_several_count_segments(model, D, prec):
    # index space 3: hundreds of entries per index bucket, so each bucket is cut into several count segments (>= 128
    # entries each) for the state and the transition counts, and k_sp_counts_reduce adds more than one segment
    Ts = (160, 120) if model == scrf_amd.STDFRAME else (90, 80)
    c = SCase(model, D, True, L=3, N=3, P=8, Ts=Ts, seed=12, precision=prec)
    eng = c.engine()
    b = c.batch(eng)
    state_rows = np.concatenate(c.X)
    trans_rows = np.concatenate([X[[orc.seg_base(t, D) for t in range(T)]] for X, T in zip(c.X, Ts)])
    for rows in (state_rows, trans_rows):
        per_bucket = np.zeros(c.N)
        for x in rows:
            for k in range(c.P):
                i = sr.pair_index(x[2 * k], c.N - 1)
                if i is not None:
                    per_bucket[i] += 1
        assert per_bucket.min() > 2 * 128, per_bucket
    numer, zx = eng.fb_batch(b)
    rg, rn, rz = _restated(c, eng, b)
    assert _close(numer, rn, 1e-9) and _close(zx, rz, 1e-9)
    assert _close(eng.get_grad(), rg, 1e-9)
    b.close(); eng.close()
