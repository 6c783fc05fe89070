"""not-gpu: N-best decoding is part of the C ABI, the library and the engine; its kernels and its host unit are units of their
own in the Makefiles (tests/test_host_multirank.py links crf_amd.cpp against a stub of the ABI); the new product files never
reach for the oracle."""
import os
import re

import scrf_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_nbest_entry_points_are_declared_and_exported():
    src = open(os.path.join(ROOT, "include", "scrf_abi.h")).read()
    assert re.search(r"#define\s+SCRF_ABI_VERSION\s+1\b", src)
    # the declarations follow a comment that states the rule
    doc = src[src.index("N-best decoding"):src.index("scrf_nbest_stats(")]
    for cite in ("ShortestPath(lat, n)", "boundary(t,l)[0..N)", "end(t,l)[0..N)", "final[0..N)", "(cost, p, r)", "monotone", "pairwise distinct",
                 "scrf_viterbi_batch's result", "byte for byte", "scrf_set_lambda", "160 KiB"):
        assert cite in doc, cite
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    u64p = r"\s*uint64_t\s*\*\s*\w+\s*"
    assert re.search(r"\bint\s+scrf_nbest_batch\s*\(\s*scrf_handle\s+\w+,\s*scrf_batch\s+\w+,\s*uint32_t\s+\w+\s*," + u64p + "," + u64p + r"\)\s*;", src)
    assert re.search(r"\bint\s+scrf_nbest_paths\s*\(\s*scrf_handle\s+\w+,\s*scrf_batch\s+\w+,\s*uint32_t\s+\w+,\s*uint32_t\s+\w+,\s*uint32_t\s*\*\s*\w+,"
                     r"\s*uint64_t\s+\w+\s*," + u64p + r",\s*float\s*\*\s*\w+\s*\)\s*;", src)
    assert re.search(r"\bint\s+scrf_nbest_stats\s*\(\s*scrf_handle\s+\w+(,\s*uint64_t\s*\*\s*\w+){3}\s*\)\s*;", src)
    if not os.path.exists(scrf_amd.lib_path()):
        import __graft_entry__ as g
        g.build()
    lib = scrf_amd.load_library()
    assert hasattr(lib, "scrf_nbest_batch") and hasattr(lib, "scrf_nbest_paths") and hasattr(lib, "scrf_nbest_stats")
    assert hasattr(scrf_amd.Engine, "nbest_batch") and hasattr(scrf_amd.Engine, "nbest_stats")


def test_the_new_units_are_in_the_makefiles_and_apart_from_crf_amd_cpp():
    host = os.path.join(ROOT, "asr-craft_amd", "host")
    unit = open(os.path.join(host, "crf_nbest.cpp")).read()
    assert "scrf_nbest_batch" in unit and "scrf_nbest_paths" in unit and "scrf_transcript_batch" in unit and "crf_amd_nbest" in unit
    assert "crf_amd_nbest" in open(os.path.join(host, "crf_amd.h")).read()
    assert not re.search(r"scrf_nbest_batch|scrf_nbest_paths|scrf_nbest_stats|crf_amd_nbest", open(os.path.join(host, "crf_amd.cpp")).read())
    assert "crf_nbest.cpp" in open(os.path.join(host, "Makefile")).read()
    assert "scrf_nbest.hip" in open(os.path.join(ROOT, "asr-craft_amd", "csrc", "Makefile")).read()
    kern = open(os.path.join(ROOT, "asr-craft_amd", "csrc", "scrf_nbest.hip")).read()
    for k in ("k_nbest", "k_nbest_count", "k_nbest_scan", "k_nbest_trace"):
        assert re.search(r"__global__[^;{]*\b%s\s*\(" % k, kern), k
    assert not re.search(r"\batomic", kern.split("#include", 1)[1])   # no atomics


def test_the_new_product_files_never_reference_the_oracle():
    for rel in ("asr-craft_amd/csrc/scrf_nbest.hip", "asr-craft_amd/host/crf_nbest.cpp", "tools/time_nbest.py"):
        txt = open(os.path.join(ROOT, rel), errors="ignore").read()
        assert not re.search(r"oracle|orc_|libscrf_oracle|import orc", txt), rel
