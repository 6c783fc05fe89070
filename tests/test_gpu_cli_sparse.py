"""-m gpu: crf_featuremap=stdsparse / stdsparsetrans through the CRFTrain / CRFFstDecode front-ends, against the dense
map on the densified twin of the same ASCII stream."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "asr-craft_amd", "bin")
L, N, P = 4, 12, 4


def _write_streams(tmp_path):
    """A sparse pair stream (unsorted, duplicate indices, values in eighths so the twin's sums are exact), its densified
    twin over the index space [0, N) and the labels."""
    rng = np.random.RandomState(2)
    sp, dn, lb = (str(tmp_path / n) for n in ("sparse.ascii", "dense.ascii", "lab.ascii"))
    with open(sp, "w") as fs, open(dn, "w") as fd, open(lb, "w") as fl:
        for u, T in enumerate([7, 9, 6]):
            lab = rng.randint(0, L, T)
            for t in range(T):
                idx = rng.randint(0, N, P)
                val = rng.randint(-8, 9, P) / 8.0
                d = np.zeros(N)
                for i, v in zip(idx, val):
                    d[i] += v
                fs.write("%d %d %s\n" % (u, t, " ".join("%d %g" % (i, v) for i, v in zip(idx, val))))
                fd.write("%d %d %s\n" % (u, t, " ".join("%g" % v for v in d)))
                fl.write("%d %d %d\n" % (u, t, lab[t]))
    return sp, dn, lb


def _flags(ftr, fmap, sparse):
    f = ["ftr1_file=" + ftr, "ftr1_format=ascii", "crf_label_size=%d" % L, "crf_model_type=stdframe",
         "label_maximum_duration=1", "crf_featuremap=" + fmap, "crf_state_bias_value=1", "crf_trans_bias_value=1"]
    if sparse:   # the index ranges: CRFTrain's default end is the window width - 1
        f += ["crf_stateftr_end=%d" % (N - 1), "crf_transftr_end=%d" % (N - 1)]
    return f


@pytest.mark.parametrize("fmap,dense_map", [("stdsparse", "stdstate"), ("stdsparsetrans", "stdtrans")])
def test_crftrain_and_fstdecode_sparse_equals_dense_twin(tmp_path, fmap, dense_map):
    sp, dn, lb = _write_streams(tmp_path)
    outs = {}
    for tag, ftr, m, sparse in (("sparse", sp, fmap, True), ("dense", dn, dense_map, False)):
        os.makedirs(str(tmp_path / tag))   # its own weight directory: a .done.train there ends a repeated run
        out = str(tmp_path / tag / "w.out")
        r = subprocess.run([os.path.join(BIN, "CRFTrain")] + _flags(ftr, m, sparse) + [
            "hardtarget_file=" + lb, "out_weight_file=" + out, "crf_epochs=3", "crf_lr=0.05", "crf_bunch_size=1",
            "threads=1", "crf_utt_rpt=1", "crf_train_order=seq"], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        outs[tag] = out
    ws, wd = np.loadtxt(outs["sparse"]), np.loadtxt(outs["dense"])
    assert ws.shape == wd.shape and np.abs(wd).max() > 0
    # the weight file keeps 6 significant digits: equal files, or a last-digit rounding apart
    np.testing.assert_allclose(ws, wd, rtol=1e-5, atol=1e-9)
    assert np.abs(ws - wd).max() <= 1e-6 * np.abs(wd).max() or open(outs["sparse"]).read() == open(outs["dense"]).read()
    # decode both inputs with the dense run's weights: the same scores, the same bytes
    dec = {}
    for tag, ftr, m, sparse in (("sparse", sp, fmap, True), ("dense", dn, dense_map, False)):
        d = str(tmp_path / ("dec_%s.txt" % tag))
        r = subprocess.run([os.path.join(BIN, "CRFFstDecode")] + _flags(ftr, m, sparse) + [
            "weight_file=" + outs["dense"], "crf_output_labelfile=" + d], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        dec[tag] = open(d, "rb").read()
    assert dec["sparse"] == dec["dense"] and len(dec["dense"]) > 0


@pytest.mark.parametrize("model,extra,msg", [
    ("stdseg", ["label_maximum_duration=2", "crf_label_size=8"], "crf_states=1"),
    ("stdseg_no_dur", ["label_maximum_duration=2"], "crf_states=1"),
    ("stdframe", ["crf_states=2", "crf_label_size=8"], "crf_states=1"),
    ("stdseg_no_dur_no_transftr", ["label_maximum_duration=2"], "crf_featuremap must be \"stdstate\""),
])
def test_crftrain_refuses_sparse_on_other_models(tmp_path, model, extra, msg):
    sp, _, lb = _write_streams(tmp_path)
    flags = [f for f in _flags(sp, "stdsparse", True) if not f.startswith("crf_model_type")]
    flags = [f for f in flags if not any(f.split("=")[0] == e.split("=")[0] for e in extra)]
    r = subprocess.run([os.path.join(BIN, "CRFTrain")] + flags + extra + [
        "crf_model_type=" + model, "hardtarget_file=" + lb, "out_weight_file=" + str(tmp_path / "w.out"), "crf_epochs=1"],
        capture_output=True, text=True, timeout=300)
    assert r.returncode != 0
    assert msg in r.stdout + r.stderr
