"""-m gpu: CRFTrain crf_objective_function=softexpf on the bundled fixture (tests/golden/crftrain_test.*: the frame model, 48
labels, three utterances) against a Python loop of Engine.fb_transcript_batch + sgd_step over the same bunches: the printed
average log-likelihood per epoch and the final weights at rtol 2e-4 / atol 2e-6 (the bounds tests/test_gpu_cli.py uses for
weight files: they keep six digits); and the refusals."""
import os
import re
import subprocess

import numpy as np
import pytest

import scrf_amd
import transcript_ref as tr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
BIN = os.path.join(ROOT, "asr-craft_amd", "bin")
LR, EPOCHS = 0.1, 2


def fixture():
    f1 = np.loadtxt(os.path.join(G, "crftrain_test.ascii"))
    f2 = np.loadtxt(os.path.join(G, "crftrain_test.ftr2.ascii"))
    lb = np.loadtxt(os.path.join(G, "crftrain_test.lab.ascii"))
    return [(np.concatenate([f1[f1[:, 0] == u, 2:], f2[f1[:, 0] == u, 2:]], axis=1).astype(np.float32), lb[f1[:, 0] == u, 2].astype(np.uint32))
            for u in range(3)]


def train_flags(out, *more):
    return [os.path.join(BIN, "CRFTrain"), "ftr1_file=" + os.path.join(G, "crftrain_test.ascii"), "ftr1_format=ascii",
            "ftr2_file=" + os.path.join(G, "crftrain_test.ftr2.ascii"), "ftr2_format=ascii", "crf_label_size=48", "crf_model_type=stdframe",
            "label_maximum_duration=1", "crf_featuremap=stdstate", "hardtarget_file=" + os.path.join(G, "crftrain_test.lab.ascii"),
            "out_weight_file=" + out, "crf_epochs=%d" % EPOCHS, "crf_lr=%g" % LR, "crf_bunch_size=1", "threads=1", "crf_utt_rpt=1",
            "crf_train_order=seq", "crf_precision=exact"] + list(more)


def python_loop(mode):
    """the same run: per utterance zero_grad, fb_transcript_batch, sgd_step; returns (weights, summed log_num - zx per epoch)"""
    utts = fixture()
    eng = scrf_amd.Engine(scrf_amd.make_config(model_type=scrf_amd.STDFRAME, L=48, D=1, F=6, precision=scrf_amd.PREC_EXACT))
    eng.set_lambda(np.zeros(eng.lambda_len))
    tot = []
    for _ in range(EPOCHS):
        s = 0.0
        for X, lab in utts:
            ph = tr.collapse(lab).astype(np.uint32) if mode == scrf_amd.ALIGN_RUNS else lab
            b = eng.batch_from_windows([X], [X.shape[0]])
            eng.zero_grad()
            ln, zx = eng.fb_transcript_batch(b, [ph], mode)
            s += float(ln[0] - zx[0])
            eng.sgd_step(np.float32(LR))
            b.close()
        tot.append(s)
    lam = eng.get_lambda()
    eng.close()
    return lam, tot


@pytest.mark.parametrize("repeat", [1, 0])
def test_crftrain_softexpf_equals_the_python_loop(tmp_path, repeat):
    out = str(tmp_path / "w.out")
    r = subprocess.run(train_flags(out, "crf_objective_function=softexpf", "crf_align_repeat=%d" % repeat), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    for k in range(EPOCHS):
        assert os.path.exists(out + ".i%d.out" % k) and os.path.exists(out + ".i%d.avg.out" % k)
    assert os.path.exists(out) and os.path.exists(out + ".avg.out")
    lam, tot = python_loop(scrf_amd.ALIGN_RUNS if repeat else scrf_amd.ALIGN_ONE)
    avg = [float(v) for v in re.findall(r"Iter-Avg LogLi: (\S+)", r.stdout)]
    assert len(avg) == 3 * EPOCHS, r.stdout
    print("epoch averages: CRFTrain %s, python %s" % ([avg[2], avg[5]], [t / 3 for t in tot]))
    np.testing.assert_allclose([avg[2], avg[5]], [t / 3 for t in tot], rtol=2e-4, atol=2e-6)
    np.testing.assert_allclose(np.loadtxt(out), lam, rtol=2e-4, atol=2e-6)
    assert np.abs(lam).max() > 0
    assert tot[1] > tot[0] and avg[5] > avg[2]   # the objective rises
    if not repeat:
        # one segment per phone on the frame model with every frame labelled: one alignment, i.e. the expf objective
        (tmp_path / "expf").mkdir()
        oute = str(tmp_path / "expf" / "w.out")
        r = subprocess.run(train_flags(oute), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        np.testing.assert_allclose(np.loadtxt(out), np.loadtxt(oute), rtol=2e-4, atol=2e-6)


@pytest.mark.parametrize("env,more,words", [({"WORLD_SIZE": "2", "RANK": "0"}, [], ("softexpf", "one process", "WORLD_SIZE=2")),
                                             ({}, ["crf_train_method=lbfgs"], ("softexpf", "crf_train_method=sg")),
                                             ({}, ["crf_align_repeat=2"], ("crf_align_repeat=2",))])
def test_refusals_come_before_any_weight_file(tmp_path, env, more, words):
    out = str(tmp_path / "w.out")
    r = subprocess.run(train_flags(out, "crf_objective_function=softexpf", *more), capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, **env))
    assert r.returncode != 0
    for w in words:
        assert w in r.stderr, r.stderr
    assert os.listdir(str(tmp_path)) == []
