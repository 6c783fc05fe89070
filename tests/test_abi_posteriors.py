"""not-gpu: the posterior output is part of the C ABI and of the host interface: include/scrf_abi.h declares the two entry
points and the built library exports them; CRF_NewLocalPosteriorBuilder keeps the reference's constructor and buildFtrSeq
signature (tests/host/posterior_conformance.cpp, static_asserts); the new product files do not reach for the oracle."""
import os
import re
import subprocess

import scrf_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_posterior_entry_points_are_declared_and_exported():
    src = open(os.path.join(ROOT, "include", "scrf_abi.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\bint\s+scrf_posteriors_batch\s*\(\s*scrf_handle\s+\w+,\s*scrf_batch\s+\w+,\s*double\s*\*\s*\w+,\s*double\s*\*\s*\w+,"
                     r"\s*double\s*\*\s*\w+,\s*const\s+uint32_t\s*\*\s*\w+,\s*const\s+uint64_t\s*\*\s*\w+,\s*double\s*\*\s*\w+\s*\)\s*;", src)
    assert re.search(r"\bint\s+scrf_seg_posteriors\s*\(\s*scrf_handle\s+\w+,\s*scrf_batch\s+\w+,\s*uint32_t\s+\w+,\s*double\s*\*\s*\w+\s*\)\s*;", src)
    if not os.path.exists(scrf_amd.lib_path()):
        import __graft_entry__ as g
        g.build()
    lib = scrf_amd.load_library()
    assert hasattr(lib, "scrf_posteriors_batch") and hasattr(lib, "scrf_seg_posteriors")
    assert hasattr(scrf_amd.Engine, "posteriors_batch") and hasattr(scrf_amd.Engine, "seg_posteriors")


def test_posterior_builder_keeps_the_reference_shaped_signatures():
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                        "-I" + os.path.join(ROOT, "asr-craft_amd", "host"),
                        os.path.join(ROOT, "tests", "host", "posterior_conformance.cpp")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr


def test_the_posterior_unit_is_part_of_the_host_library_and_apart_from_crf_amd_cpp():
    """tests/test_host_multirank.py links crf_amd.cpp against a stub of the ABI symbols it uses: the posterior entry
    point must be called from a translation unit of its own"""
    host = os.path.join(ROOT, "asr-craft_amd", "host")
    assert "scrf_posteriors_batch" in open(os.path.join(host, "crf_posteriors.cpp")).read()
    assert not re.search(r"scrf_posteriors_batch|scrf_seg_posteriors", open(os.path.join(host, "crf_amd.cpp")).read())
    assert "crf_posteriors.cpp" in open(os.path.join(host, "Makefile")).read()
    assert "scrf_post.hip" in open(os.path.join(ROOT, "asr-craft_amd", "csrc", "Makefile")).read()


def test_the_new_product_files_never_reference_the_oracle():
    for rel in ("asr-craft_amd/csrc/scrf_post.hip", "asr-craft_amd/host/crf_posteriors.cpp", "tools/time_posteriors.py"):
        txt = open(os.path.join(ROOT, rel), errors="ignore").read()
        assert not re.search(r"oracle|orc_|libscrf_oracle|import orc", txt), rel
