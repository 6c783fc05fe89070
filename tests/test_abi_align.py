"""not-gpu: forced alignment is part of the C ABI, the library and the engine; its host unit is a translation unit of its
own (tests/test_host_multirank.py links crf_amd.cpp against a stub of the ABI); the new product files never reach for the
oracle."""
import os
import re

import scrf_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_align_entry_points_are_declared_and_exported():
    src = open(os.path.join(ROOT, "include", "scrf_abi.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\bint\s+scrf_align_batch\s*\(\s*scrf_handle\s+\w+,\s*scrf_batch\s+\w+,\s*const\s+uint32_t\s*\*\s*\w+,\s*const\s+uint64_t\s*\*\s*\w+\s*,"
                     r"\s*int\s+\w+,\s*uint32_t\s*\*\s*\w+,\s*uint64_t\s+\w+,\s*uint64_t\s*\*\s*\w+,\s*float\s*\*\s*\w+\s*\)\s*;", src)
    assert re.search(r"\bint\s+scrf_align_stats\s*\(\s*scrf_handle\s+\w+(,\s*uint64_t\s*\*\s*\w+){4}\s*\)\s*;", src)
    assert re.search(r"SCRF_ALIGN_ONE\s*=\s*0\s*,\s*SCRF_ALIGN_RUNS\s*=\s*1", src)
    if not os.path.exists(scrf_amd.lib_path()):
        import __graft_entry__ as g
        g.build()
    lib = scrf_amd.load_library()
    assert hasattr(lib, "scrf_align_batch") and hasattr(lib, "scrf_align_stats")
    assert hasattr(scrf_amd.Engine, "align_batch") and hasattr(scrf_amd.Engine, "align_stats")
    assert (scrf_amd.ALIGN_ONE, scrf_amd.ALIGN_RUNS) == (0, 1)


def test_the_align_unit_is_part_of_the_host_library_and_apart_from_crf_amd_cpp():
    host = os.path.join(ROOT, "asr-craft_amd", "host")
    assert "scrf_align_batch" in open(os.path.join(host, "crf_align.cpp")).read()
    assert not re.search(r"scrf_align_batch|scrf_align_stats|crf_amd_alignments", open(os.path.join(host, "crf_amd.cpp")).read())
    assert "crf_align.cpp" in open(os.path.join(host, "Makefile")).read()
    assert "scrf_align.hip" in open(os.path.join(ROOT, "asr-craft_amd", "csrc", "Makefile")).read()


def test_the_new_product_files_never_reference_the_oracle():
    for rel in ("asr-craft_amd/csrc/scrf_align.hip", "asr-craft_amd/host/crf_align.cpp", "tools/time_align.py"):
        txt = open(os.path.join(ROOT, rel), errors="ignore").read()
        assert not re.search(r"oracle|orc_|libscrf_oracle|import orc", txt), rel
