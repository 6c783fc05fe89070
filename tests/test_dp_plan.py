"""-m "not gpu": which kernel form the launchers of the recursions, the walks and the searches pick (asr-craft_amd/csrc/scrf_dp_plan.h).

launch_exp_m, launch_dp_wave, launch_dp_lin, launch_atb, launch_fb, launch_viterbi, launch_viterbi_fast, launch_fb_segtrans,
launch_post_occ, launch_align_wave, launch_sl_fb and launch_sl_trans_counts take their choice from the host-only header, so
tests/host/dp_plan_probe.cpp, which compiles that header alone with g++, answers for them.  The sweep plans every call over L
in LS, D 1..41, m_per_frame, use_tf, use_tb, the utterance counts N_UTTS, 256 and 64 CUs, the t_max list of the fused test
(k_post_occ) and La in LAS (k_sl_*), under the default knobs and each knob set of KNOB_SETS, twice: by the plain probe and by
one built with AddressSanitizer and UBSan.

Checked on every line whose shape the guarding predicate (or the engine's LDS check) admits (ok=1): the LDS request fits a
workgroup, the threads, DMAX >= D, the grid against the utterances, the wavefronts per workgroup, the rules of each template
argument; and the set of instantiations the sweep emits is INSTANTIATIONS below.  launch_viterbi is guarded by no check
(its lines say ok=0): its LDS request passes 160 KB once (D + 2) L > 40 960, e.g. L = 1024 from D = 39 on.

tests/golden/dp_plan_parent.txt records, per knob set and section, the SHA-256 of the same sweep through the launchers and
predicates of the commit before the header existed (compiled with g++ against stand-in launch calls): the probe reproduces
it, so the header picks what that code picked."""
import hashlib
import os
import re
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "asr-craft_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "host", "dp_plan_probe.cpp")
GOLDEN = os.path.join(ROOT, "tests", "golden", "dp_plan_parent.txt")

LS = (1, 3, 4, 16, 32, 33, 47, 48, 49, 52, 63, 64, 65, 96, 128, 129, 192, 193, 200, 208, 209, 256, 257, 512, 1024)
N_UTTS = (1, 11, 12, 13, 95, 96, 97, 128, 129, 256, 257, 383, 384, 385, 1024, 3072, 3073, 8192, 65535)
LAS = (1, 16, 17, 48, 64, 65)
SECTIONS = ("exp_m", "dp_wave", "dp_lin", "atb", "fb", "viterbi", "viterbi_fast", "fb_segtrans", "post_occ", "align_wave", "sl_fb", "sl_atb", "support")
KNOB_SETS = ({}, {"SCRF_DPLIN_MV": "0"}, {"SCRF_DPLIN_MV": "1"}, {"SCRF_DPLIN_MV_SWEEPS": "1"}, {"SCRF_DPLIN_EREG": "0"}, {"SCRF_DPLIN_TAIL": "0"},
             {"SCRF_EXPM_TILE": "0"}, {"SCRF_VITERBI_VEC": "0"}, {"SCRF_FBW_WAVES": "4"})
KNOB_IDS = [" ".join("%s=%s" % kv for kv in k.items()) or "default" for k in KNOB_SETS]
LDS_LIMIT = 160 * 1024


def t_maxes(D):
    return (1, 2 * D - 1, 2 * D, 4 * D - 1, 4 * D, 1000)


def _expected():
    out = {"k_exp_m", "k_fb", "k_viterbi", "k_fb_segtrans_w", "k_sl_fb"}
    out |= {"k_exp_m_tile<%d>" % ne for ne in (4, 9, 16)}
    out |= {"k_dp_wave<%d,%d>" % (dm, mpf) for dm in (1, 4, 10, 16, 25, 32) for mpf in (0, 1)}
    out |= {"k_dp_lin<%d,%d,0>" % (dm, mpf) for dm in (1, 4, 10, 16, 25, 32, 40) for mpf in (0, 1)} | {"k_dp_lin<25,0,48>"}
    out |= {"k_dp_lin_mv<%d,%d>" % (dm, mpf) for dm in (10, 16, 25, 32, 40) for mpf in (0, 1)}
    for dm in (10, 25, 40):     # k_dp_lin_mw: per-frame matrices, the column from L2, 128 rows of it in registers ...
        out |= {"k_dp_lin_mw<%d,%s>" % (dm, f) for f in ("1,0,0", "0,0,0", "0,128,0")}
    out |= {"k_dp_lin_mw<%d,0,%d,0>" % (dm, lr) for dm in (10, 25) for lr in (192, 208)} | {"k_dp_lin_mw<40,0,128,1>"}     # ... all of it, or a tail from L2
    out |= {"k_atb<%d>" % lt for lt in (1, 2, 3, 4)} | {"k_sl_atb<%d>" % nt for nt in (1, 2, 3, 4)}
    out |= {"k_viterbi_fast<%d,%d>" % (dm, lv) for dm in (12, 25, 40) for lv in (0, 48, 64)}
    out |= {"k_post_occ<%d,%d>" % (dm, rw) for dm in (8, 16, 25, 32, 40) for rw in (48, 64)}
    out |= {"k_align_wave<%d>" % dm for dm in (4, 12, 40)}
    return frozenset(out)


# every instantiation a shape the engine admits can reach.  A new or vanished one is an edit of this list.
# (k_fb_segtrans, the column-wise kernel, is planned only where two D x L images pass 150 KB; its own three then pass the
# 160 KB the engine checks, so no admitted layout gets it: test_every_planned_launch_fits_its_shape asserts that too)
INSTANTIATIONS = _expected()
assert len(INSTANTIATIONS) == 5 + 3 + 12 + 15 + 10 + 14 + 4 + 4 + 9 + 10 + 3


def build(tmp, name, extra=()):
    exe = str(tmp / name)
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-I" + CSRC, *extra, SRC, "-o", exe], check=True, timeout=300)
    return exe


@pytest.fixture(scope="module")
def probes(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("dp_plan")
    return build(tmp, "dp_plan_probe"), build(tmp, "dp_plan_probe_san", ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))


def run(exe, *args, **knobs):
    r = subprocess.run([exe] + [str(a) for a in args] + ["%s=%s" % kv for kv in knobs.items()], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-2000:])
    return r.stdout


@pytest.fixture(scope="module")
def sweeps(probes):
    """per knob set {section: text}; the sanitized probe must print the same bytes and nothing on stderr"""
    def both(job):
        ki, s = job
        out = run(probes[0], "sweep", s, **KNOB_SETS[ki])
        return out, hashlib.sha256(out.encode()).digest() == hashlib.sha256(run(probes[1], "sweep", s, **KNOB_SETS[ki]).encode()).digest()
    jobs = [(ki, s) for ki in range(len(KNOB_SETS)) for s in SECTIONS]
    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as ex:
        outs = list(ex.map(both, jobs))
    res = [dict() for _ in KNOB_SETS]
    for (ki, s), (out, same) in zip(jobs, outs):
        assert same, (KNOB_IDS[ki], s)
        res[ki][s] = out
    return res


FIELD = re.compile(r"(\w+)=(\S+)")


def parse(text):
    """probe lines -> dicts of the named fields: integers, except kernel, grid (a tuple), walk and the a/b lists (text)"""
    res = []
    for ln in text.splitlines():
        l = {}
        for k, v in FIELD.findall(ln):
            if k == "grid":
                l[k] = tuple(int(x) for x in v.split("/"))
            elif k == "kernel" or "/" in v:
                l[k] = v
            else:
                l[k] = int(v)
        m = re.search(r"<([\d,]+)>", l.get("kernel", ""))
        l["targs"] = tuple(int(x) for x in m.group(1).split(",")) if m else ()
        res.append(l)
    return res


def ceil_div(a, b):
    return -(-a // b)


def check_section(s, lines, knobs, seen, not_admitted):
    """the assertions of one section's lines; the instantiations of admitted shapes go to seen, the others' to not_admitted"""
    for l in lines:
        if s == "support":
            continue
        k, ta, grid = l["kernel"], l["targs"], l.get("grid")
        L, D, n = l.get("L"), l.get("D"), l.get("n_utts")
        if s == "viterbi":      # no check guards it: the threads hold for every L, the LDS does not
            assert l["threads"] % 64 == 0 and 64 <= l["threads"] <= 1024 and l["threads"] >= min(L, 1024), l
            assert l["lds"] == 4 * (2 * L + D * L), l
            seen.add(k)
            continue
        if s == "exp_m":        # (guarded by nothing: it serves every L)
            ne = ta[0] if ta else 0
            assert grid == (l["n_mat"], 1, 1) and l["threads"] == 256 and l["lds"] == 0, l
            assert (ne > 0) == (L <= 64 and knobs.get("SCRF_EXPM_TILE") != "0"), l
            if ne:
                assert ne * 256 >= L * L, l
            seen.add(k)
            continue
        if not l["ok"]:
            not_admitted.add(k)
            continue
        seen.add(k)
        assert l["lds"] <= LDS_LIMIT, l
        assert l["threads"] % 64 == 0 and 64 <= l["threads"] <= 1024, l
        wpb = l["threads"] // 64
        if s == "dp_wave":
            assert ta[0] >= D and ta[1] == l["mpf"], l
            assert wpb in (12, 8, 4, 2, 1) and grid == (2 * ceil_div(n, wpb), 1, 1), l
            assert l["lds"] == 8 * ((0 if l["mpf"] else L * L) + wpb * D * L), l
        elif s == "dp_lin":
            assert ta[0] >= D and ta[1] == l["mpf"], l
            if k.startswith("k_dp_lin<"):
                assert L <= 64 and wpb in (12, 11, 10, 9, 8, 4, 2, 1) and grid == (2 * ceil_div(n, wpb), 1, 1), l
                assert (ta[2] == 48) == (L == 48 and ta[0] == 25 and not l["mpf"]) and ta[2] in (0, 48), l
                assert l["lds"] == 8 * ((0 if l["mpf"] else L * L) + wpb * (D * L + 128)), l
                assert knobs.get("SCRF_DPLIN_MV") != "1" or D < 2, l
            elif k.startswith("k_dp_lin_mv<"):
                assert L <= 64 and D >= 2 and wpb == 4 and grid == (2 * n, 1, 1) and knobs.get("SCRF_DPLIN_MV") != "0", l
                if "SCRF_DPLIN_MV" not in knobs:
                    assert l["mpf"] and 2 * n <= int(knobs.get("SCRF_DPLIN_MV_SWEEPS", 3)) * l["n_cu"], l
            else:
                lr, tail = ta[2], ta[3]
                assert L > 64 and wpb == ceil_div(L, 64) and grid == (2 * n, 1, 1), l
                assert lr in (0, 128, 192, 208) and not (tail and lr != 128), l
                if lr > 0 and not tail:
                    assert lr >= L, l
                if lr == 128 and lr < L:
                    assert tail, l
                if lr:
                    assert not l["mpf"] and knobs.get("SCRF_DPLIN_EREG") != "0", l
                if tail:
                    assert knobs.get("SCRF_DPLIN_TAIL") != "0" and ta[0] == 40, l
        elif s == "atb":
            assert grid == (ceil_div(l["n_chunks"], 4), ceil_div(L, 64) ** 2, 1) and 16 * ta[0] >= min(L, 64) and l["threads"] == 256, l
        elif s == "fb":
            assert k == "k_fb" and l["threads"] == (256 if L <= 256 else 1024), l
        elif s == "viterbi_fast":
            dm, lv = ta
            assert dm >= D and l["lds"] <= 64 * 1024 and wpb == 4 and grid == (ceil_div(n, 4), 1, 1), l
            assert lv in (0, 48, 64) and (lv > 0) == (L % 4 == 0 and knobs.get("SCRF_VITERBI_VEC") != "0"), l
            if lv:
                assert L % 4 == 0 and lv >= L, l
        elif s == "fb_segtrans":
            assert k == "k_fb_segtrans_w" and grid == (n, 1, 1) and l["lds"] == 16 * D * L and l["lds"] <= 150 * 1024, l
            assert wpb == (4 if "SCRF_FBW_WAVES" in knobs else 8 if n > 256 else 16), l
        elif s == "post_occ":
            dm, rw = ta
            assert dm >= D and rw == (48 if L <= 48 else 64) and l["gy"] == ceil_div(L, 64) and l["sum_groups"] == int(L > 64), l
            calls = [(u, t) for u in N_UTTS for t in t_maxes(D)]
            walk = [tuple(int(x) for x in e.split("/")) for e in l["walk"].split(",")]
            assert len(walk) == len(calls), l
            for (u, t_max), (gx, nz, seg_len) in zip(calls, walk):
                assert gx == u and nz >= 1, (l, u, t_max)
                if nz > 1:
                    assert l["split_ok"] and u * l["gy"] <= 512 and t_max >= 4 * D, (l, u, t_max)
                    assert nz * seg_len >= t_max and seg_len >= 2 * D and (nz - 1) * seg_len < t_max, (l, u, t_max)
                else:
                    assert seg_len >= 2 ** 29, (l, u, t_max)     # one piece: longer than any utterance
        elif s == "align_wave":
            assert ta[0] >= D and wpb == 4 and grid == (ceil_div(n, 4), 1, 1) and l["lds"] == 4 * 4 * 64 * (D + 1), l
        elif s == "sl_fb":
            assert grid == (2 * n, 1, 1) and l["threads"] == 512 and L <= 512 and l["lds"] <= 150 * 1024, l
        elif s == "sl_atb":
            assert 16 * ta[0] >= l["La"] and grid == (l["n_chunks"] * D * ceil_div(ceil_div(L, 16), 3), 1, 1) and l["threads"] == 64, l


def check_support(lines):
    for l in lines:
        L, D = l["L"], l["D"]
        assert l["dp_wave"] == int(L <= 64 and D <= 32) and l["dplin"] == int(L <= 64 and D <= 40), l
        assert l["dplin_mw"] == int(64 < L <= 256 and D <= 40) and l["atb"] == int(L <= 256) and l["align_wave"] == int(D <= 40), l
        assert not (l["dplin"] and l["dplin_mw"]) and l["dp_wave"] <= l["dplin"], l
        if l["viterbi_fast"]:
            assert L <= 64 and 2 <= D <= 40 and not l["use_tf"], l
        assert l["post_occ_groups"] == ceil_div(L, 64) and l["lat_sweep_smem"] == 8 * (D + 2) * L, l
        sl = [int(x) for x in l["stdseg_lin"].split("/")]
        for La, ok in zip(LAS, sl):
            assert ok <= int(not l["use_tf"] and l["use_tb"] and L <= 512 and La <= 64), l


@pytest.fixture(scope="module")
def checked(sweeps):
    """per knob set (seen, not_admitted), every line checked; a section a knob set leaves as the default has it is checked once"""
    res = []
    for ki, by in enumerate(sweeps):
        seen, rest = set(), set()
        for s in SECTIONS:
            if ki and by[s] == sweeps[0][s]:
                continue
            lines = parse(by[s])
            assert lines, (KNOB_IDS[ki], s)
            check_section(s, lines, KNOB_SETS[ki], seen, rest)
            if s == "support":
                check_support(lines)
        res.append((seen, rest))
    return res


def test_every_planned_launch_fits_its_shape(checked):
    for ki, (seen, rest) in enumerate(checked):
        assert seen <= INSTANTIATIONS, (KNOB_IDS[ki], sorted(seen - INSTANTIATIONS))
    assert "k_fb_segtrans" in checked[0][1] and "k_fb_segtrans" not in checked[0][0]
    print("default knobs: %d instantiations" % len(checked[0][0]))


def test_the_sweep_emits_exactly_the_recorded_instantiations(checked):
    ids = {k: i for i, k in enumerate(KNOB_IDS)}
    union = set().union(*(seen for seen, _ in checked))
    for name in sorted(union ^ INSTANTIATIONS):
        print("differs:", name)
    assert union == INSTANTIATIONS
    count = lambda p: sum(n.startswith(p) for n in union)
    assert (count("k_dp_lin<"), count("k_dp_lin_mv<"), count("k_dp_lin_mw<")) == (15, 10, 14)
    # what each knob adds to or takes from the default set (a knob set's `seen` holds the sections it changes)
    dflt = checked[0][0]
    assert {n for n in dflt if n.startswith("k_dp_lin_mv")} == {"k_dp_lin_mv<%d,1>" % dm for dm in (10, 16, 25, 32, 40)}
    assert not any(n.startswith("k_dp_lin_mv") for n in checked[ids["SCRF_DPLIN_MV=0"]][0])
    assert count("k_dp_lin_mv<") == sum(n.startswith("k_dp_lin_mv<") for n in checked[ids["SCRF_DPLIN_MV=1"]][0])
    assert {n for n in checked[ids["SCRF_DPLIN_EREG=0"]][0] if n.startswith("k_dp_lin_mw")} == {"k_dp_lin_mw<%d,%d,0,0>" % (dm, mpf) for dm in (10, 25, 40) for mpf in (0, 1)}
    assert "k_dp_lin_mw<40,0,128,1>" in dflt and "k_dp_lin_mw<40,0,128,1>" not in checked[ids["SCRF_DPLIN_TAIL=0"]][0]
    assert checked[ids["SCRF_EXPM_TILE=0"]][0] == {"k_exp_m"}
    assert checked[ids["SCRF_VITERBI_VEC=0"]][0] == {"k_viterbi_fast<%d,0>" % dm for dm in (12, 25, 40)}
    assert checked[ids["SCRF_FBW_WAVES=4"]][0] == {"k_fb_segtrans_w"}


def test_the_probe_reproduces_the_choice_of_the_code_before_the_header(sweeps):
    want = {}
    for ln in open(GOLDEN):
        if ln.strip() and not ln.startswith("#"):
            knob, section, n_lines, digest = ln.split()
            want[(knob, section)] = (int(n_lines), digest)
    assert len(want) == len(KNOB_SETS) * len(SECTIONS)
    bad = []
    for ki, by in enumerate(sweeps):
        for s in SECTIONS:
            got = (by[s].count("\n"), hashlib.sha256(by[s].encode()).hexdigest())
            if got != want[(KNOB_IDS[ki], s)]:
                bad.append((KNOB_IDS[ki], s, "lines: %d, recorded %d" % (got[0], want[(KNOB_IDS[ki], s)][0])))
    assert not bad, bad


LAUNCHERS = {"scrf_dp.hip": ("launch_exp_m", "launch_dp_wave", "launch_atb"), "scrf_dplin.hip": ("launch_dp_lin",),
             "scrf_kernels.hip": ("launch_fb", "launch_viterbi", "launch_viterbi_fast"), "scrf_segtrans.hip": ("launch_fb_segtrans",),
             "scrf_post.hip": ("launch_post_occ",), "scrf_align.hip": ("launch_align_wave",),
             "scrf_stdseg_lin.hip": ("launch_sl_fb", "launch_sl_trans_counts")}
MOVED = ("dp_wave_supported", "dplin_supported", "dplin_mw_supported", "atb_supported", "viterbi_fast_supported", "align_wave_supported",
         "stdseg_lin_supported", "fb_block_threads", "fb_smem_bytes", "fb_segtrans_smem_bytes", "align_group_smem_bytes", "lat_sweep_smem_bytes",
         "transcript_smem_bytes", "nbest_smem_bytes", "post_occ_groups", "dp_waves_per_block")
MOVED_CONSTANTS = ("DP_WPB", "DPV_NW", "VF_WAVES", "FBW_WAVES", "AL_WAVES", "SL_NT")


def test_the_launchers_hold_no_threshold_of_their_own():
    """the launchers take every form from the plan: no macro ladder, no comparison against a size, no knob read, no LDS formula;
    the predicates and the shared constants are defined in the header only, and the segment rule once"""
    for fn, names in LAUNCHERS.items():
        src = open(os.path.join(CSRC, fn)).read()
        assert not re.search(r"_GO\d?\(|_LAUNCH\d?\(", src), fn
        for name in names:
            m = re.search(r"^(?:static )?(?:void|uint32_t) %s\(.*?^}" % name, src, re.S | re.M)
            assert m, name
            body = m.group(0)
            assert "_plan(" in body, name
            assert not re.search(r"(<=|>=)\s*\w|\s[<>]\s", body), name
            assert not re.search(r"lay\.[LD]\s*[<>%]|sizeof|\bkn\.|\b(150|156|1024)\b", body), name
    plan = open(os.path.join(CSRC, "scrf_dp_plan.h")).read()
    for fn in sorted(os.listdir(CSRC)):
        if fn == "scrf_dp_plan.h" or not fn.endswith((".h", ".hip", ".cpp")):
            continue
        src = open(os.path.join(CSRC, fn)).read()
        for name in MOVED:
            assert not re.search(r"^\w[\w \*]*\b%s\(.*\)\s*[;{]" % name, src, re.M), (fn, name)
        for name in MOVED_CONSTANTS:
            assert not re.search(r"#define\s+%s\b" % name, src), (fn, name)
    for name in MOVED:
        assert len(re.findall(r"^inline \w+ %s\(" % name, plan, re.M)) == 1, name
    for name in MOVED_CONSTANTS:
        assert len(re.findall(r"#define\s+%s\b" % name, plan)) == 1, name
    assert "hip" not in re.sub(r"//[^\n]*", "", plan).replace("__HIPCC__", "").lower()
    # one segment rule: k_post_z's plan and k_post_occ's both call it
    fused = open(os.path.join(CSRC, "scrf_fused_plan.h")).read()
    assert len(re.findall(r"\bwalk_segments\(", plan)) == 2 and len(re.findall(r"\bwalk_segments\(", fused)) == 1
    assert "4 * 256" not in fused and plan.count("4 * 256") == 1
    assert "dp_cu_count()" in open(os.path.join(CSRC, "scrf_dplin.hip")).read()


def test_single_calls_match_the_sweep(probes, sweeps):
    by = sweeps[0]
    for args in (("dp_lin", 48, 25, 0, 8192, 256), ("dp_lin", 200, 40, 0, 128, 64), ("dp_lin", 64, 10, 1, 128, 256), ("dp_wave", 64, 32, 0, 13),
                 ("viterbi_fast", 48, 25, 0, 97), ("fb_segtrans", 96, 10, 257), ("align_wave", 12, 385), ("sl_fb", 512, 10, 48, 1),
                 ("sl_atb", 200, 25, 17, 13), ("atb", 129, 1024), ("exp_m", 49, 12), ("fb", 257, 10), ("viterbi", 1024, 41), ("support", 64, 40, 0, 1)):
        line = run(probes[0], *args)
        assert line.count("\n") == 1 and line in by[args[0]], args
    got = parse(run(probes[0], "post_occ", 48, 25, 1, 256, 1000))[0]
    want = [l for l in parse(by["post_occ"]) if (l["L"], l["D"], l["split_ok"]) == (48, 25, 1)]
    assert len(want) == 1 and got["kernel"] == want[0]["kernel"]
    assert got["walk"] == want[0]["walk"].split(",")[N_UTTS.index(256) * 6 + 5]
