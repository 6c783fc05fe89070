"""not-gpu: the host side of N-best decoding (asr-craft_amd/host/crf_nbest.cpp) under AddressSanitizer and
UndefinedBehaviorSanitizer, as a stand-alone program (tests/host/nbest_args_check.cpp, its own main) linked against the ABI
stub: the sizes of every buffer it hands the ABI (the stand-ins write each to its full extent), the collapse / unique logic,
the per-rank transcript assembly with short utterances, and its argument checks.  Nothing is loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "asr-craft_amd", "host")


def test_the_host_unit_is_clean_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "nbest_args_check")
    subprocess.run(["g++", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-ffp-contract=off", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + HOST,
                    os.path.join(ROOT, "tests", "host", "nbest_args_check.cpp"), os.path.join(HOST, "crf_nbest.cpp"),
                    os.path.join(HOST, "crf_amd.cpp"), os.path.join(ROOT, "tests", "host", "scrf_stub.cpp"), "-o", exe], check=True, timeout=900)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "nbest_args_check OK" in r.stdout, r.stdout + r.stderr
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr
