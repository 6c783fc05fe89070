"""not-gpu: CRFTrain's two sources built over the stub of the C ABI (the command of tests/test_host_multirank.py), without the
soft-objective unit crf_softgrad.cpp: crf_objective_function=softexpf is refused with the "not linked" message, before any
file is read or written; the expf objective is still taken up to the first file it opens."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "asr-craft_amd", "host")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("stubbin") / "CRFTrain_stub")
    subprocess.run(["g++", "-O1", "-ffp-contract=off", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + HOST,
                    os.path.join(HOST, "CRFTrain_main.cpp"), os.path.join(HOST, "crf_amd.cpp"),
                    os.path.join(ROOT, "tests", "host", "scrf_stub.cpp"), "-o", out], check=True, timeout=600)
    return out


def flags(tmp_path):
    return ["ftr1_file=" + str(tmp_path / "none.ascii"), "ftr1_format=ascii", "hardtarget_file=" + str(tmp_path / "none.lab"),
            "out_weight_file=" + str(tmp_path / "w.out"), "crf_label_size=4"]


def test_softexpf_without_the_unit_is_refused(exe, tmp_path):
    r = subprocess.run([exe] + flags(tmp_path) + ["crf_objective_function=softexpf"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0
    assert "crf_objective_function=softexpf: the soft-objective unit is not linked into this binary" in r.stderr
    assert os.listdir(str(tmp_path)) == []


def test_the_other_objectives_keep_their_answers(exe, tmp_path):
    r = subprocess.run([exe] + flags(tmp_path) + ["crf_objective_function=ferr"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "expf only" in r.stderr
    r = subprocess.run([exe] + flags(tmp_path) + ["crf_objective_function=expf", "crf_align_repeat=0"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "crf_align_repeat needs crf_objective_function=softexpf" in r.stderr
