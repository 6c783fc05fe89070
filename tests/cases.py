"""Shared construction of test cases: the same seeded inputs for the oracle and the engine."""
import numpy as np

import orc
import scrf_amd
from scrf_amd import synth


def nstate_segment_labels(rng, L, K, T, D):
    """A random segmentation whose labels follow the K-states-per-phone topology (stay, advance, or end state -> a
    start state), in the segment-end labelling of the label stream: label + L*(dur-1) on a segment's last frame."""
    out = np.full(T, 0xffffffff, dtype=np.uint32)
    c = int(rng.randint(0, L))
    t = -1
    while t + 1 < T:
        d = int(rng.randint(1, min(D, T - 1 - t) + 1))
        t += d
        out[t] = c + L * (d - 1)
        if rng.rand() >= 0.3:
            c = int(rng.randint(0, L // K)) * K if (c + 1) % K == 0 else c + 1
    return out


# input families (None: U[0, 1), the values every older test runs on): name -> nominal max |x|
FAMILIES = {"signed": 8.0, "ranged": 64.0, "offset": 9.0, "tied": 2.0}
TIED_VALUES = (-1.0, -0.5, 0.5, 1.0, 2.0)


def family_frames(rng, family, Ts, in_w):
    """float32 frames of one batch under an input family, finite and without a negative zero:
    signed  N(0, 2^2): sign changes inside every window
    ranged  N(0, 1) * 4^((u mod 4) - 1): scales 1/4, 1, 4 and 16 side by side in one batch
    offset  8 + U[0, 1): a large common part (cancellation in differences of sums)
    tied    values of TIED_VALUES, whole frames repeated in runs of 1 .. 3: exact ties in every running extremum"""
    out = []
    for u, T in enumerate(Ts):
        if family == "signed":
            x = rng.normal(0.0, 2.0, (T, in_w))
        elif family == "ranged":
            x = rng.normal(0.0, 1.0, (T, in_w)) * 4.0 ** ((u % 4) - 1)
        elif family == "offset":
            x = 8.0 + rng.random_sample((T, in_w))
        elif family == "tied":
            x = rng.choice(TIED_VALUES, (T, in_w))
            t = 0
            while t < T:
                n = int(rng.randint(1, 4))
                x[t:t + n] = x[t]
                t += n
        else:
            raise ValueError("unknown input family %r" % (family,))
        out.append(x.astype(np.float32) + np.float32(0.0))   # (-0.0) + 0.0 = +0.0
    return out


def tie_twin_labels(lam, lay, L, K=1):
    """phone 1 becomes a twin of phone 0 (K = 1: label 1 of label 0): every weight indexed by one of its labels equals the
    weight indexed the same way by the label of phone 0 -- the state block, and every transition block with it as previous
    or as current label -- and the state bias of both is raised by 2, so that best paths run through them: any best
    path through either then has a twin of equal cost."""
    nsf, ntf = lay.num_state_funcs, lay.num_trans_funcs
    if L < 2 * K:
        return
    twin = lambda l: l - K if K <= l < 2 * K else l
    for l in range(K, 2 * K):
        lam[lay.state_idx[l]:lay.state_idx[l] + nsf] = lam[lay.state_idx[l - K]:lay.state_idx[l - K] + nsf]
    for p in range(L):
        for c in range(L):
            i, j = int(lay.trans_idx[p * L + c]), int(lay.trans_idx[twin(p) * L + twin(c)])
            if i != j and i != 0xffffffff and j != 0xffffffff:
                lam[i:i + ntf] = lam[j:j + ntf]
    if lay.cfg.use_state_bias:
        for l in range(2 * K):
            lam[lay.state_idx[l] + nsf - 1] += 2.0


# feature-map settings a Case takes through fmap= (orc.config and scrf_amd.make_config name them alike)
FMAP_KEYS = frozenset(("sfs", "sfe", "tfs", "tfe", "use_state_ftrs", "use_state_bias", "use_trans_bias", "state_bias_val", "trans_bias_val"))


class Case:
    """L labels, max duration D, raw frame width in_w, utterance lengths Ts.
    trans_ctx=None: `stdstate` map (bias-only transitions); trans_ctx=c: `stdtrans` map whose
    transition features are a second stream of boundary context (c frames each side), like the
    TIMIT demo's ftr2 stream (demo/segmental-timit-demo.cfg.in:21-24).
    family: one of FAMILIES instead of frames in [0, 1) (family_frames); lam_scale then defaults to
    3 / (nominal max |x| * sqrt(F)), which keeps scores to a few nats, and `tied` also ties two labels (tie_twin_labels).
    fmap: feature-map settings (FMAP_KEYS) that replace what the keywords above imply, in both configurations; the frames,
    labels and the random stream of the weights do not depend on it (only the number of weights drawn does)."""

    def __init__(self, L, D, in_w, Ts, trans_ctx=None, seed=0, lam_scale=None, frame_model=False,
                 scratch_bytes=0, precision=0, l1_norm=False, model_type=None, trans_share=None,
                 num_states=1, conform_labels=True, exact_avg=False, family=None, fmap=None):
        self.L, self.D, self.in_w, self.Ts = L, D, in_w, list(Ts)
        self.trans_ctx = trans_ctx
        self.family = family
        rng = np.random.RandomState(seed)
        if family is None:
            self.frames = [rng.random_sample((T, in_w)).astype(np.float32) for T in Ts]
        else:
            self.frames = family_frames(rng, family, Ts, in_w)
        if exact_avg:
            # frame values m * lcm(1..D) / 2^k, m in 0..4: every running float sum over <= D frames and its quotient by
            # the length is exact in float, so the reference's float window average IS the exact mean (D <= 10)
            assert D <= 10
            lcm = int(np.lcm.reduce(np.arange(1, D + 1)))
            scale = 2.0 ** -int(np.ceil(np.log2(5 * lcm)))
            self.frames = [(rng.randint(0, 5, (T, in_w)) * (lcm * scale)).astype(np.float32) for T in Ts]
        if l1_norm:   # rows L1-normalised like softmax posteriors (SURVEY 8d, config 3/4 inputs)
            self.frames = [(f / f.sum(1, keepdims=True)).astype(np.float32) for f in self.frames]
        if frame_model:
            self.labels = [rng.randint(0, L, T).astype(np.uint32) for T in Ts]
        elif num_states > 1 and conform_labels:
            self.labels = [nstate_segment_labels(rng, L, num_states, T, D) for T in Ts]
        else:
            self.labels = [synth.group_labels(synth.frame_labels(rng, T, L, D), D, L) for T in Ts]
        Fs = orc.window_width(in_w, D, 0, 0, True)
        self.recipes = [scrf_amd.StreamRecipe(in_w, 0, 0, 1)]
        self.frames2 = None
        mt = orc.STDFRAME if frame_model else orc.STDSEG_NO_DUR_NO_SEGTRANSFTR
        if model_type is not None:
            mt = model_type
        if trans_ctx is None and trans_share is not None:
            # transition features = columns [lo, hi] of the segment's own window vector (single stream)
            self.F = Fs
            kw = dict(model_type=mt, L=L, D=D, F=Fs, use_trans_ftrs=True, tfs=trans_share[0], tfe=trans_share[1])
        elif trans_ctx is None:
            self.F = Fs
            kw = dict(model_type=mt, L=L, D=D, F=Fs)
        else:
            c = trans_ctx
            Ft = orc.window_width(in_w, D, c, c, False)
            self.F = Fs + Ft
            self.frames2 = [np.concatenate([np.repeat(f[:1], c, 0), f, np.repeat(f[-1:], c, 0)]) for f in self.frames]
            self.recipes.append(scrf_amd.StreamRecipe(in_w, c, c, 0))
            kw = dict(model_type=mt, L=L, D=D, F=self.F, sfe=Fs - 1, use_trans_ftrs=True, tfs=Fs)
        self.Fs = Fs
        if num_states > 1:
            kw["num_states"] = num_states
        if mt == orc.STDSEG:   # the feature map and the weight layout run over all labels: nLabs = nActualLabs * D
            kw["L"] = L * D
        if fmap is not None:   # feature-map overrides, the same for the oracle and the engine
            assert set(fmap) <= FMAP_KEYS, sorted(set(fmap) - FMAP_KEYS)
            kw.update(fmap)
        self.ocfg = orc.config(**kw)
        self.olay = orc.Layout(self.ocfg)
        self.gcfg = scrf_amd.make_config(scratch_bytes=scratch_bytes, precision=precision, **kw)
        if lam_scale is None:
            lam_scale = 0.3 if family is None else 3.0 / (FAMILIES[family] * np.sqrt(self.F))
        self.lam = rng.normal(0, lam_scale, self.olay.lambda_len)
        if family == "tied":
            tie_twin_labels(self.lam, self.olay, self.ocfg.num_labs, max(1, num_states))

    def windows(self, u):
        """oracle window vectors of utterance u: [N_seg, F]"""
        T = self.Ts[u]
        X = np.zeros((orc.num_segs(T, self.D), self.F), dtype=np.float32)
        orc.windows(self.frames[u], self.D, 0, 0, True, out=X, out_col=0)
        if self.trans_ctx is not None:
            c = self.trans_ctx
            orc.windows(self.frames2[u], self.D, c, c, False, out=X, out_col=self.Fs)
        return X

    def engine(self):
        e = scrf_amd.Engine(self.gcfg)
        e.set_lambda(self.lam)
        return e

    def batch(self, eng, with_labels=True):
        return eng.batch_from_frames(self.frames, self.labels if with_labels else None, self.recipes,
                                     [self.frames2] if self.frames2 is not None else None)

    def oracle_gradient(self):
        """sum over utterances of buildGradient (one stream): grad, numer[], zx[]"""
        g = np.zeros(self.olay.lambda_len)
        numer, zx = [], []
        for u, T in enumerate(self.Ts):
            if self.ocfg.model_type == orc.STDFRAME:
                rc, g, n, z = orc.frame_build_gradient(self.ocfg, self.olay, self.lam, self.windows(u), self.labels[u], T, grad=g)
            elif self.ocfg.model_type == orc.STDSEG:
                rc, g, n, z = orc.stdseg_build_gradient(self.ocfg, self.olay, self.lam, self.windows(u), self.labels[u], T, grad=g)
            elif self.ocfg.model_type == orc.STDSEG_NO_DUR:
                rc, g, n, z = orc.segtrans_build_gradient(self.ocfg, self.olay, self.lam, self.windows(u), self.labels[u], T, grad=g)
            else:
                rc, g, n, z = orc.seg_build_gradient(self.ocfg, self.olay, self.lam, self.windows(u), self.labels[u], T, grad=g)
            assert rc == 0, rc
            numer.append(n); zx.append(z)
        return g, np.array(numer), np.array(zx)
