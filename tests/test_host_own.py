"""-m "not gpu": the engine's owning types (asr-craft_amd/csrc/scrf_own.h: DevArray, PinnedArray, Event, Stream).

The header touches the HIP runtime through a dozen calls only, so tests/host/own_types.cpp compiles it with g++ against a
counting stand-in (tests/host/fakehip) under AddressSanitizer and UBSan, as a program of its own: nothing stays live after any
sequence of reserve, reserve_keep, move and destruction with a failure injected at every creating call; reserve_keep keeps the
live elements; a failed reserve leaves an empty array; borrowed memory and streams are never released.  The same failures go
through scrf_create's allocation sequence in miniature, which leaves through scrf_destroy's path.  The program's second mode
runs that check on the delete-only path scrf_create used to take on raw pointers, where it must fail: the check can."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "asr-craft_amd", "csrc")
HOST = os.path.join(ROOT, "tests", "host")


@pytest.fixture(scope="module")
def own_types(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("own") / "own_types")
    subprocess.run(["g++", "-std=c++17", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + os.path.join(HOST, "fakehip"), "-I" + CSRC, os.path.join(HOST, "own_types.cpp"), "-o", exe],
                   check=True, timeout=300)
    return exe


def test_nothing_stays_live(own_types):
    r = subprocess.run([own_types], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("own_types OK")


def test_the_check_fails_on_the_delete_only_path(own_types):
    r = subprocess.run([own_types, "delete-only"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1, r.stdout + r.stderr
    assert "delete-only: 18 live after a failed create" in r.stdout
    assert "CHECK(left == 0) failed" in r.stderr


def test_header_uses_the_runtime_through_the_listed_calls_only():
    import re
    src = open(os.path.join(CSRC, "scrf_own.h")).read()
    code = re.sub(r"//[^\n]*", "", src)
    allowed = {"hipMalloc", "hipFree", "hipHostMalloc", "hipHostFree", "hipEventCreate", "hipEventCreateWithFlags", "hipEventDestroy",
               "hipStreamCreateWithFlags", "hipStreamDestroy", "hipMemcpyAsync", "hipStreamSynchronize"}
    called = set(re.findall(r"\b(hip[A-Z]\w*)\s*\(", code)) - {"hipEvent_t", "hipStream_t"}   # (the conversion operators)
    assert called == allowed
    assert re.findall(r"#include\s*[<\"](hip[^>\"]*)[>\"]", code) == ["hip/hip_runtime.h"]
