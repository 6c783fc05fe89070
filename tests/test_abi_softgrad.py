"""not-gpu: training from transcripts is part of the C ABI, the library and the engine; its kernels are a unit
of their own in the Makefile; CRFTrain's two sources, which tests/test_host_multirank.py links against a stub of the ABI, do
not name the new entry points; the new product file never reaches for the oracle."""
import os
import re

import scrf_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_entry_points_are_declared_and_exported():
    src = open(os.path.join(ROOT, "include", "scrf_abi.h")).read()
    doc = src[src.index("training from transcripts"):src.index("scrf_soft_stats(")]
    for cite in ("CRF_NewGradBuilderSoft.cpp:30-116", ":44-58", ":99-110", "xa(t,k)", "xs(t,k)", "end_post[t-1]", "SCRF_PREC_FASTLIN",
                 "does not fit", "same bytes", "scrf_train_stats"):
        assert cite in doc, cite
    assert "scrf_fb_transcript_batch" in src[src.index("HIP-event time of every kernel"):src.index("scrf_kernel_timing(")]
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\bint\s+scrf_fb_transcript_batch\s*\(\s*scrf_handle\s+\w+,\s*scrf_batch\s+\w+,\s*const\s+uint32_t\s*\*\s*\w+,"
                     r"\s*const\s+uint64_t\s*\*\s*\w+\s*,\s*int\s+\w+,\s*double\s*\*\s*\w+\s*,\s*double\s*\*\s*\w+\s*\)\s*;", src)
    assert re.search(r"\bint\s+scrf_soft_stats\s*\(\s*scrf_handle\s+\w+(,\s*uint64_t\s*\*\s*\w+){3}\s*\)\s*;", src)
    if not os.path.exists(scrf_amd.lib_path()):
        import __graft_entry__ as g
        g.build()
    lib = scrf_amd.load_library()
    assert hasattr(lib, "scrf_fb_transcript_batch") and hasattr(lib, "scrf_soft_stats")
    assert hasattr(scrf_amd.Engine, "fb_transcript_batch") and hasattr(scrf_amd.Engine, "soft_stats")


def test_the_kernels_are_a_unit_of_their_own_without_atomics():
    assert "scrf_softnum.hip" in open(os.path.join(ROOT, "asr-craft_amd", "csrc", "Makefile")).read()
    kern = open(os.path.join(ROOT, "asr-craft_amd", "csrc", "scrf_softnum.hip")).read()
    for k in ("k_soft_state", "k_soft_trans", "k_soft_add_r", "k_soft_add_xi", "k_soft_pos_sums", "k_soft_trans_table"):
        assert re.search(r"__global__[^;{]*\b%s\s*\(" % k, kern), k
    assert not re.search(r"\batomic", kern.split("#include", 1)[1])
    eng = open(os.path.join(ROOT, "asr-craft_amd", "csrc", "scrf_engine.cpp")).read()
    for k in ("k_soft_state", "k_soft_trans", "k_soft_add_r", "k_soft_add_xi", "k_soft_trans_table"):
        assert '"%s"' % k in eng, k   # listed by scrf_kernel_timing


def test_the_host_unit_is_in_its_makefile_and_fills_the_hook_slot():
    host = os.path.join(ROOT, "asr-craft_amd", "host")
    mk = open(os.path.join(host, "Makefile")).read()
    lib_rule = [l for l in mk.splitlines() if l.lstrip().startswith("$(CXX)") and "-shared" in l][0]
    assert "crf_softgrad.cpp" in lib_rule and mk.count("crf_softgrad.cpp") >= 2   # compiled into the host library, and a prerequisite
    unit = open(os.path.join(host, "crf_softgrad.cpp")).read()
    assert "scrf_fb_transcript_batch" in unit and re.search(r"crf_amd_soft_fb\s*=\s*\w+", unit)
    hdr = open(os.path.join(host, "crf_amd.h")).read()
    assert re.search(r"extern\s+crf_amd_soft_fb_fn\s+crf_amd_soft_fb\s*;", hdr)
    assert "the soft-objective unit is not linked into this binary" in hdr
    assert re.search(r"crf_amd_soft_fb_fn\s+crf_amd_soft_fb\s*=\s*nullptr", open(os.path.join(host, "crf_amd.cpp")).read())
    assert not re.search(r"oracle|orc_|libscrf_oracle", unit)


def test_the_trainer_sources_do_not_name_the_new_entry_points():
    host = os.path.join(ROOT, "asr-craft_amd", "host")
    for f in ("crf_amd.cpp", "CRFTrain_main.cpp"):
        assert not re.search(r"scrf_fb_transcript_batch|scrf_soft_stats", open(os.path.join(host, f)).read()), f


def test_the_new_product_files_never_reference_the_oracle():
    for rel in ("asr-craft_amd/csrc/scrf_softnum.hip", "asr-craft_amd/csrc/scrf_softnum.h"):
        txt = open(os.path.join(ROOT, rel), errors="ignore").read()
        assert not re.search(r"oracle|orc_|libscrf_oracle|import orc", txt), rel
