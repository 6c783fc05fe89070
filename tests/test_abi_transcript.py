"""not-gpu: transcript scoring is part of the C ABI, the library and the engine; its host unit is a translation unit of its
own (tests/test_host_multirank.py links crf_amd.cpp against a stub of the ABI); the new product files never reach for the
oracle."""
import os
import re

import scrf_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_transcript_entry_points_are_declared_and_exported():
    src = open(os.path.join(ROOT, "include", "scrf_abi.h")).read()
    assert re.search(r"#define\s+SCRF_ABI_VERSION\s+1\b", src)
    # each declaration follows a comment that states the rule and cites the reference
    doc = src[src.index("transcript scoring"):src.index("scrf_transcript_stats(")]
    for cite in ("CRF_LatticeBuilder.cpp:129-165", ":374-386", "CRF_NewGradBuilderSoft.cpp:44-58", "getAlignmentGammas", "computeAlignedAlphaBeta",
                 "aB(t,k)", "aE(t,k)", "bE(t,k)", "bB(t,k)", "g(t,d,k)"):
        assert cite in doc, cite
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    dp, cu32, cu64 = r"\s*double\s*\*\s*\w+\s*", r"\s*const\s+uint32_t\s*\*\s*\w+\s*", r"\s*const\s+uint64_t\s*\*\s*\w+\s*"
    assert re.search(r"\bint\s+scrf_transcript_batch\s*\(\s*scrf_handle\s+\w+,\s*scrf_batch\s+\w+," + cu32 + "," + cu64 + r",\s*int\s+\w+\s*,"
                     + dp + "," + dp + "," + dp + "," + dp + "," + cu32 + "," + cu64 + "," + dp + r"\)\s*;", src)
    assert re.search(r"\bint\s+scrf_transcript_stats\s*\(\s*scrf_handle\s+\w+(,\s*uint64_t\s*\*\s*\w+){3}\s*\)\s*;", src)
    if not os.path.exists(scrf_amd.lib_path()):
        import __graft_entry__ as g
        g.build()
    lib = scrf_amd.load_library()
    assert hasattr(lib, "scrf_transcript_batch") and hasattr(lib, "scrf_transcript_stats")
    assert hasattr(scrf_amd.Engine, "transcript_batch") and hasattr(scrf_amd.Engine, "transcript_stats")


def test_the_transcript_unit_is_part_of_the_host_library_and_apart_from_crf_amd_cpp():
    host = os.path.join(ROOT, "asr-craft_amd", "host")
    unit = open(os.path.join(host, "crf_transcript.cpp")).read()
    assert "scrf_transcript_batch" in unit and "crf_amd_transcript_scores" in unit
    assert "crf_amd_transcript_scores" in open(os.path.join(host, "crf_amd.h")).read()
    assert not re.search(r"scrf_transcript_batch|scrf_transcript_stats|crf_amd_transcript_scores", open(os.path.join(host, "crf_amd.cpp")).read())
    assert "crf_transcript.cpp" in open(os.path.join(host, "Makefile")).read()
    assert "scrf_transcript.hip" in open(os.path.join(ROOT, "asr-craft_amd", "csrc", "Makefile")).read()


def test_the_new_product_files_never_reference_the_oracle():
    for rel in ("asr-craft_amd/csrc/scrf_transcript.hip", "asr-craft_amd/host/crf_transcript.cpp", "tools/time_transcript.py"):
        txt = open(os.path.join(ROOT, rel), errors="ignore").read()
        assert not re.search(r"oracle|orc_|libscrf_oracle|import orc", txt), rel
