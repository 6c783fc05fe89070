"""-m "not gpu": the SCRF_* environment knobs (asr-craft_amd/csrc/scrf_knobs.h).

scrf_create reads every knob once, through scrf_knobs_read, into one struct on the engine handle.  The header is host-only,
so tests/host/knobs_probe.cpp compiles it alone with g++, feeds scrf_knobs_read a getter backed by its own argv and
prints the struct: the defaults and every parse rule are checked here without a GPU.  Two checks on the source tree keep
the arrangement: no other getenv in csrc (but wait_collective's operational timeout), and one list of names, the
header's table = DESIGN.md's "Knobs" table."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "asr-craft_amd", "csrc")

DEFAULTS = dict(
    lanes=1, fuse=1, side=1, dtab=1, fuse_mixed=1, comm_overlap=1, lindp=1, stdseg_lin=1, postocc_split=1, fast_decode=1,
    align_wave=1, batch_pool=1, pool_on=1, pool_up=1, hybrid=1, hybrid_on=1, hybrid_first=0, decode_bound_scale=1.0,
    postz_split=1, expf_dma=1, expf_big=0, expf_ws=1, expf_blocks=512, dplin_ereg=1, dplin_tail=1, dplin_mv=-1,
    dplin_mv_sweeps=3, scores_mfma_ws=1, expf_db=1, expf_mfma_ws=1, expm_tile=1, viterbi_vec=1, trans_chunks=0, rtab=1,
    scores_dma=1, fbw_waves=0, comm_timeout_s=300.0)
# default on, "0" (or anything atoi reads as 0) turns it off
ON_OFF = dict(
    SCRF_FUSE="fuse", SCRF_SIDE="side", SCRF_DTAB="dtab", SCRF_FUSE_MIXED="fuse_mixed", SCRF_COMM_OVERLAP="comm_overlap",
    SCRF_LINDP="lindp", SCRF_STDSEG_LIN="stdseg_lin", SCRF_POSTOCC_SPLIT="postocc_split", SCRF_FAST_DECODE="fast_decode",
    SCRF_ALIGN_WAVE="align_wave", SCRF_POSTZ_SPLIT="postz_split", SCRF_EXPF_DMA="expf_dma", SCRF_EXPF_WS="expf_ws",
    SCRF_DPLIN_EREG="dplin_ereg", SCRF_DPLIN_TAIL="dplin_tail", SCRF_SCORES_MFMA_WS="scores_mfma_ws", SCRF_EXPF_DB="expf_db",
    SCRF_EXPF_MFMA_WS="expf_mfma_ws", SCRF_EXPM_TILE="expm_tile", SCRF_VITERBI_VEC="viterbi_vec", SCRF_RTAB="rtab",
    SCRF_SCORES_DMA="scores_dma")


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("knobs") / "knobs_probe")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I" + CSRC, os.path.join(ROOT, "tests", "host", "knobs_probe.cpp"),
                    "-o", exe], check=True, timeout=300)

    def run(**env):
        out = subprocess.run([exe] + ["%s=%s" % kv for kv in env.items()], capture_output=True, text=True, check=True, timeout=60).stdout
        fields, names = {}, []
        for ln in out.splitlines():
            k, v = ln.split()
            if k == "name":
                names.append(v)
            else:
                fields[k] = float(v)
        return fields, names
    return run


def changed(probe, **env):
    """the fields that differ from the defaults under env"""
    f, _ = probe(**env)
    assert sorted(f) == sorted(DEFAULTS)
    return {k: v for k, v in f.items() if v != DEFAULTS[k]}


def test_empty_environment_gives_the_defaults(probe):
    f, names = probe()
    assert f == {k: float(v) for k, v in DEFAULTS.items()}
    assert len(names) == len(set(names)) and all(n.startswith("SCRF_") for n in names)
    # one field per name (pool_on / pool_up / hybrid_on / hybrid_first are views of two of them)
    assert len(names) == len(DEFAULTS) - 4


@pytest.mark.parametrize("name", sorted(ON_OFF))
def test_switches_are_on_unless_the_value_is_zero(probe, name):
    field = ON_OFF[name]
    big = {"expf_big": 1.0} if name == "SCRF_SIDE" else {}   # SCRF_EXPF_BIG's default follows the side stream
    assert changed(probe, **{name: "0"}) == {field: 0.0, **big}
    assert changed(probe, **{name: "off"}) == {field: 0.0, **big}   # atoi("off") == 0, as before
    assert changed(probe, **{name: "1"}) == {}
    assert changed(probe, **{name: "7"}) == {}


def test_lanes_is_one_or_two(probe):
    assert changed(probe, SCRF_LANES="2") == {"lanes": 2.0}
    assert changed(probe, SCRF_LANES="5") == {"lanes": 2.0}
    assert changed(probe, SCRF_LANES="1") == {}
    assert changed(probe, SCRF_LANES="0") == {}
    assert changed(probe, SCRF_LANES="-3") == {}


def test_batch_pool_0_1_2(probe):
    assert changed(probe, SCRF_BATCH_POOL="0") == {"batch_pool": 0.0, "pool_on": 0.0}
    assert changed(probe, SCRF_BATCH_POOL="1") == {}
    assert changed(probe, SCRF_BATCH_POOL="2") == {"batch_pool": 2.0, "pool_up": 0.0}   # pool on, uploads on the engine stream


def test_hybrid_0_1_2(probe):
    assert changed(probe, SCRF_HYBRID="0") == {"hybrid": 0.0, "hybrid_on": 0.0}
    assert changed(probe, SCRF_HYBRID="1") == {}
    assert changed(probe, SCRF_HYBRID="2") == {"hybrid": 2.0, "hybrid_first": 1.0}


def test_decode_bound_scale_only_widens(probe):
    assert changed(probe, SCRF_DECODE_BOUND_SCALE="0.5") == {}        # max(1.0, 0.5)
    assert changed(probe, SCRF_DECODE_BOUND_SCALE="30") == {"decode_bound_scale": 30.0}
    assert changed(probe, SCRF_DECODE_BOUND_SCALE="1.5") == {"decode_bound_scale": 1.5}


def test_dplin_mv_unset_0_1_and_sweeps(probe):
    assert probe()[0]["dplin_mv"] == -1.0   # automatic
    assert changed(probe, SCRF_DPLIN_MV="0") == {"dplin_mv": 0.0}
    assert changed(probe, SCRF_DPLIN_MV="1") == {"dplin_mv": 1.0}
    assert changed(probe, SCRF_DPLIN_MV="4") == {"dplin_mv": 1.0}
    assert changed(probe, SCRF_DPLIN_MV_SWEEPS="8") == {"dplin_mv_sweeps": 8.0}
    assert changed(probe, SCRF_DPLIN_MV_SWEEPS="3") == {}


def test_expf_blocks_is_unsigned(probe):
    assert changed(probe, SCRF_EXPF_BLOCKS="64") == {"expf_blocks": 64.0}
    assert changed(probe, SCRF_EXPF_BLOCKS="-1") == {"expf_blocks": float(2 ** 32 - 1)}   # (uint32_t)atoi, as before: no cap


def test_expf_big_defaults_to_side_stream_off(probe):
    assert probe()[0]["expf_big"] == 0.0
    assert changed(probe, SCRF_SIDE="0") == {"side": 0.0, "expf_big": 1.0}
    assert changed(probe, SCRF_SIDE="1") == {}
    assert changed(probe, SCRF_EXPF_BIG="0", SCRF_SIDE="0") == {"side": 0.0}
    assert changed(probe, SCRF_EXPF_BIG="1") == {"expf_big": 1.0}
    assert changed(probe, SCRF_EXPF_BIG="1", SCRF_SIDE="1") == {"expf_big": 1.0}
    assert changed(probe, SCRF_EXPF_BIG="0") == {}


def test_trans_chunks_and_fbw_waves_keep_the_raw_integer(probe):
    assert changed(probe, SCRF_TRANS_CHUNKS="0") == {}     # not forced
    assert changed(probe, SCRF_TRANS_CHUNKS="12") == {"trans_chunks": 12.0}
    # the range check [1, FBW_WAVES] stays with the constant, in the launch plan: the struct carries what was given
    assert changed(probe, SCRF_FBW_WAVES="4") == {"fbw_waves": 4.0}
    assert changed(probe, SCRF_FBW_WAVES="99") == {"fbw_waves": 99.0}
    assert changed(probe, SCRF_FBW_WAVES="0") == {}
    src = open(os.path.join(CSRC, "scrf_dp_plan.h")).read()
    assert "kn.fbw_waves >= 1 && kn.fbw_waves <= FBW_WAVES" in src


def test_comm_timeout_is_listed(probe):
    assert changed(probe, SCRF_COMM_TIMEOUT_S="5") == {"comm_timeout_s": 5.0}
    assert changed(probe, SCRF_COMM_TIMEOUT_S="-1") == {}
    assert "SCRF_COMM_TIMEOUT_S" in probe()[1]


def strip_comments(text):
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return re.sub(r"//[^\n]*", "", text)


def test_getenv_only_in_the_header_and_wait_collective():
    hits = {}
    for fn in sorted(os.listdir(CSRC)):
        if fn.endswith((".h", ".hip", ".cpp")):
            n = len(re.findall(r"\bgetenv\b", strip_comments(open(os.path.join(CSRC, fn)).read())))
            if n:
                hits[fn] = n
    assert hits == {"scrf_knobs.h": 1, "scrf_engine.cpp": 1}
    eng = open(os.path.join(CSRC, "scrf_engine.cpp")).read()
    body = eng[eng.index("static int wait_collective("):]
    body = body[:body.index("\n}\n")]
    assert 'getenv("SCRF_COMM_TIMEOUT_S")' in body
    # and the engine reads the table exactly once, in scrf_create
    assert len(re.findall(r"\bscrf_knobs_read\b", eng)) == 1
    create = eng[eng.index('extern "C" int scrf_create('):]
    assert "scrf_knobs_read(scrf_env)" in create[:create.index("\n}\n")]


def test_design_md_lists_the_same_names(probe):
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    sec = design[design.index("### 4.16 Knobs"):]
    sec = sec[:sec.index("\n## ")]
    rows = [ln for ln in sec.splitlines() if ln.startswith("| `SCRF_")]
    first = [re.match(r"\| `(SCRF_[A-Z0-9_]+)` \|", ln).group(1) for ln in rows]
    assert len(first) == len(set(first))
    assert set(first) == set(probe()[1])
    assert all(ln.count("|") == 6 for ln in rows)   # name, default, values, what, where
    assert "read once, at `scrf_create`" in sec
