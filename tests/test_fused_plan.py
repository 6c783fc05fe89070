"""-m "not gpu": which instantiations the launchers of scrf_fused.hip pick (asr-craft_amd/csrc/scrf_fused_plan.h).

Every launch_* of the fused kernels takes its choice from the host-only header, so tests/host/fused_plan_probe.cpp, which
compiles that header alone with g++, answers for them.  The sweep plans every call over L in LS, D 1..41, W 1..210, both
use_sb, both precisions, la, both alignments of R, the tile counts N_TILES and, for the walks, N_UTTS x t_max(D), under the
default knobs and each knob set of KNOB_SETS, twice: by the plain probe and by one built with AddressSanitizer and UBSan.
The probe folds the axes that move only the grid into lists (and stops if such an axis moves anything else), so a line
stands for every call of its cross product.

Checked on every line: the LDS request fits a workgroup; where fused_supported is 1 every launch has a plan and
fused_la_supported implies fused_supported; the sizes against the shape; the count kernel's columns, slots and knob
conditions; the segments of k_post_z and k_lin_z5; and the set of instantiations the sweep emits is INSTANTIATIONS below.
D = 41 is past what any fused kernel holds (DMAX <= 40): there fused_supported must be 0, and the DMAX >= D check applies
to D <= 40.

tests/golden/fused_plan_parent.txt records, per knob set and section, the SHA-256 of the same sweep through the selection
code of the commit before the header existed (its helpers and macro ladders, compiled with g++ against stub launchers):
the probe reproduces it, so the header picks what that code picked."""
import hashlib
import os
import re
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "asr-craft_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "host", "fused_plan_probe.cpp")
GOLDEN = os.path.join(ROOT, "tests", "golden", "fused_plan_parent.txt")

LS = (1, 6, 7, 47, 48, 49, 63, 64, 65, 96, 200, 256)
N_TILES = (0, 1, 3, 255, 256, 257, 511, 512, 513, 100000)
N_UTTS = (1, 8, 64, 256, 512, 513, 2048)
D_MAX, W_MAX = 41, 210
SECTIONS = ("support", "scores", "counts", "post_z", "lin_z", "lin_z5", "pframe", "ztf")
KNOB_SETS = ({}, {"SCRF_EXPF_WS": "0"}, {"SCRF_EXPF_DMA": "0"}, {"SCRF_EXPF_BIG": "1"}, {"SCRF_SIDE": "0"}, {"SCRF_EXPF_BLOCKS": "3"},
             {"SCRF_POSTZ_SPLIT": "0"}, {"SCRF_SCORES_DMA": "0"}, {"SCRF_DTAB": "0"}, {"SCRF_RTAB": "0"})
KNOB_IDS = [" ".join("%s=%s" % kv for kv in k.items()) or "default" for k in KNOB_SETS]


def t_maxes(D):
    return (1, 2 * D - 1, 2 * D, 4 * D - 1, 4 * D, 1000)


def _expected():
    out = set()
    for dm in (12, 25, 40):     # k_scores_fused: fp64, f32, la and decode, each staged through registers or by LDS-DMA
        for f32, dec, la in ((0, 0, 0), (1, 0, 0), (0, 0, 1), (0, 1, 0)):
            out |= {"k_scores_fused<%d,%d,%d,%d,%d>" % (dm, f32, dec, la, dma) for dma in (0, 1)}
    for dm in (8, 16, 25, 32, 40):
        out |= {"k_lin_z<%d>" % dm, "k_lin_z5<%d>" % dm}
        out |= {"k_post_z<%d,%d,%d,%d>" % (dm, la, rw, sp) for la, rw in ((0, 64), (1, 48), (1, 64)) for sp in (0, 1)}
    out |= {"k_pframe<%d>" % ks for ks in (4, 10, 16, 20)}
    out |= {"k_ztf<%d,%d>" % (nt, mt) for nt in (1, 2, 3, 4, 5) for mt in (1, 4)}
    depths = ((12, 19), (25, 16), (25, 19), (40, 13), (40, 16), (40, 19))
    for dm, ks in depths:
        out |= {"k_expf_fused<%d,%d,%d,%d>" % (nt, dm, f32, ks) for nt in (4, 7, 10) for f32 in (0, 1)}
        for g0 in (0, 1):
            for dma in (0, 1):
                out.add("k_expf_fused_ws_n<4,%d,%d,%d,76,%d>" % (dm, ks, g0, dma))
                out |= {"k_expf_fused_ws<%d,%d,%d,%d,76,%d>" % (nt, dm, ks, g0, dma) for nt in (6, 7)}
    for dm, ks in ((12, 25), (25, 21), (25, 25), (40, 21), (40, 25)):     # the tall tiles
        out |= {"k_expf_fused_ws_n<4,%d,%d,1,100,%d>" % (dm, ks, dma) for dma in (0, 1)}
    return frozenset(out)


# every instantiation the launchers can reach: 24 score kernels, 5 + 5 k_lin_z / k_lin_z5, 30 k_post_z, 4 k_pframe, 10 k_ztf,
# 36 single-role count kernels, 24 + 48 wave-specialised ones on 76-row tiles (the 4-slot forms under the register cap) and
# 10 on 100-row tiles (only with SCRF_EXPF_BIG=1 or SCRF_SIDE=0).  A new or vanished one is an edit of this list.
# launch_expf_fused's switch names these and no others (test_the_count_switch_names_exactly_the_reachable_forms): no 10-slot
# wave-specialised kernel (two images of 13 column tiles are 182 KB: the plan z-blocks or leaves the shape to the single-role
# kernel before it gets there), no 21-step tall form at D <= 12 (whole frames of D <= 12 always fill more than 84 of 100 rows).
INSTANTIATIONS = _expected()
assert len(INSTANTIATIONS) == 24 + 5 + 5 + 30 + 4 + 10 + 36 + 24 + 48 + 10


def build(tmp, name, extra=()):
    exe = str(tmp / name)
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-I" + CSRC, *extra, SRC, "-o", exe], check=True, timeout=300)
    return exe


@pytest.fixture(scope="module")
def probes(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("fused_plan")
    return build(tmp, "fused_plan_probe"), build(tmp, "fused_plan_probe_san", ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))


def run(exe, *args, **knobs):
    r = subprocess.run([exe] + [str(a) for a in args] + ["%s=%s" % kv for kv in knobs.items()], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-2000:])
    return r.stdout


def parse(out):
    """probe lines -> dicts: section, the named fields (integers; kernel a string; a folded field stays text: entries()), W_lo / W_hi"""
    res = []
    for ln in out.splitlines():
        w = ln.split()
        l = {"section": w[0]}
        for kv in w[1:]:
            k, v = kv.split("=")
            if k == "W":
                l["W_lo"], l["W_hi"] = (int(x) for x in v.split(".."))
            elif k == "kernel":
                l[k] = v
            elif "," in v or "/" in v:
                l[k] = v
            else:
                l[k] = int(v)
        res.append(l)
    return res


def entries(v):
    """a folded field's entries, each a tuple of its numbers"""
    return [tuple(int(x) for x in e.split("/")) for e in str(v).split(",")]


def folded(vals):
    return ",".join("/".join(str(x) for x in (v if isinstance(v, tuple) else (v,))) for v in vals)


@pytest.fixture(scope="module")
def sweeps(probes):
    """per knob set {section: text}; the sanitized probe must print the same bytes and nothing on stderr"""
    def both(job):
        ki, s = job
        out = run(probes[0], "sweep", s, **KNOB_SETS[ki])
        return out, hashlib.sha256(out.encode()).digest() == hashlib.sha256(run(probes[1], "sweep", s, **KNOB_SETS[ki]).encode()).digest()
    jobs = [(ki, s) for ki in range(len(KNOB_SETS)) for s in sorted(SECTIONS, key=lambda s: s not in ("counts", "scores"))]     # (the long ones first)
    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as ex:
        outs = list(ex.map(both, jobs))
    res = [dict() for _ in KNOB_SETS]
    for (ki, s), (out, same) in zip(jobs, outs):
        assert same, (KNOB_IDS[ki], s)
        res[ki][s] = out
    return res


def lds_limit():
    m = re.search(r"#define SCRF_LDS_BYTES \((\d+) \* 1024\)", open(os.path.join(CSRC, "scrf_common.h")).read())
    return int(m.group(1)) * 1024


def ceil_div(a, b):
    return -(-a // b)


def planned_widths(lines, key_fields):
    """{key: [W -> has a plan]} of a section's lines"""
    res = {}
    for l in lines:
        a = res.setdefault(tuple(l[k] for k in key_fields), [False] * (W_MAX + 1))
        for W in range(l["W_lo"], l["W_hi"] + 1):
            a[W] = l["kernel"] != "none"
    return res


def check_scores(lines, knobs, limit, seen):
    for l in lines:
        if l["kernel"] == "none":
            continue
        D = l["D"]
        assert l["lds"] <= limit and l["threads"] == 512, l
        assert l["tb"] >= 1 and l["tb"] * D <= 256, l
        if D <= 40:
            assert l["dmax"] >= D, l
        assert (l["f32"], l["dec"], l["la"]) == ((0, 0, 0), (1, 0, 0), (0, 0, 1), (0, 1, 0))[l["mode"]], l
        # the LDS-DMA form: SCRF_SCORES_DMA with both launch tables
        assert l["dma"] == int(all(knobs.get(k) != "0" for k in ("SCRF_SCORES_DMA", "SCRF_DTAB", "SCRF_RTAB"))), l
        assert l["grid"] == folded((ceil_div(L, 48), int(L <= 48 and not l["dec"])) for L in LS), l
        seen.add("k_scores_fused<%d,%d,%d,%d,%d>" % (l["dmax"], l["f32"], l["dec"], l["la"], l["dma"]))


def check_counts(lines, knobs, limit, seen):
    big = knobs.get("SCRF_EXPF_BIG") == "1" or knobs.get("SCRF_SIDE") == "0"
    cap = int(knobs.get("SCRF_EXPF_BLOCKS", 512))
    assert cap <= 512
    gy_want = folded(ceil_div(L, 48) for L in LS)
    # [L][aligned]: DMA only with an even L, an aligned R and SCRF_EXPF_DMA; never in the single-role kernel
    dma_ws = folded(int(L % 2 == 0 and al == 1 and knobs.get("SCRF_EXPF_DMA") != "0") for L in LS for al in (0, 1))
    dma_plain = folded(0 for L in LS for al in (0, 1))
    # blocks: the tiles up to SCRF_EXPF_BLOCKS (<= 512), the wave-specialised form up to 256
    gx_ws, gx_plain = folded(min(n, cap, 256) for n in N_TILES), folded(min(n, cap) for n in N_TILES)
    for l in lines:
        if l["kernel"] == "none":
            continue
        D, W = l["D"], l["W_lo"]
        assert l["W_lo"] == l["W_hi"] or l["ws"], l      # (the single-role kernel's LDS grows with every W)
        ws = l["kernel"] in ("ws", "ws_n")
        assert ws == bool(l["ws"]) and l["lds"] <= limit, l
        if D <= 40:
            assert l["dmax"] >= D, l
        assert l["frames"] * D <= l["rows"] and 4 * l["nks"] >= l["frames"] * D and l["frames"] >= 1, l
        assert l["rows"] in (76, 100) and (l["tile_list"] == 2) == (l["rows"] != 76), l
        assert l["n_ct"] <= 13 and l["xs"] >= 16 * l["n_ct"] and l["xs"] in (80, 144, 208), l
        assert l["gy"] == gy_want, l
        for W in range(l["W_lo"], l["W_hi"] + 1):
            if ws:
                cols = W if l["nz"] > 1 else (3 - l["g0"]) * W
                assert l["ncol"] == (3 - l["g0"]) * W and l["ndur"] == D + l["use_sb"] and l["nz"] in (1, 3 - l["g0"]), l
            else:
                cols = 3 * W + D + l["use_sb"]
                assert l["ncol"] == cols and l["ndur"] == 0 and l["nz"] == 1 and l["g0"] == 0, l
            assert 16 * (l["n_ct"] - 1) < cols <= 16 * l["n_ct"], l
        if ws:
            assert l["nt"] >= ceil_div(3 * l["n_ct"], 4) and (l["kernel"] == "ws_n") == (l["nt"] <= 4) and l["threads"] == 512, l
            assert not l["f32"] and not l["call_f32"] and knobs.get("SCRF_EXPF_WS") != "0", l
            assert l["g0"] == l["call_la"], l
            assert l["gx"] == gx_ws and l["dma"] == dma_ws, l
            if l["rows"] == 100:
                assert l["g0"] == 1 and l["n_ct"] <= 5 and l["nz"] == 1 and big, l
            names = ["%s<%d,%d,%d,%d,%d,%d>" % ("k_expf_fused_ws_n" if l["nt"] <= 4 else "k_expf_fused_ws", l["nt"], l["dmax"], l["nks"], l["g0"], l["rows"], d)
                     for d in set(e[0] for e in entries(l["dma"]))]
        else:
            assert l["nt"] == ceil_div(3 * (l["xs"] // 16), 4) and l["threads"] == 256 and l["f32"] == l["call_f32"], l
            assert l["rows"] == 76 and l["nfmax"] == l["frames"] + D - 1, l
            assert l["gx"] == gx_plain and l["dma"] == dma_plain, l
            names = ["k_expf_fused<%d,%d,%d,%d>" % (l["nt"], l["dmax"], l["f32"], l["nks"])]
        if D <= 40:
            seen.update(names)


def check_walks(sections, knobs, seen):
    for l in sections["post_z"] + sections["lin_z5"] + sections["lin_z"]:
        L, D = l["L"], l["D"]
        if D <= 40:
            assert l["dmax"] >= D, l
        assert l["gy"] == ceil_div(L, 64), l
        calls = [(u, t) for u in N_UTTS for t in t_maxes(D)] if l["section"] != "lin_z" else [(u, 0) for u in N_UTTS]
        grid = entries(l["grid"])
        assert len(grid) == len(calls), l
        for (n_utts, t_max), g in zip(calls, grid):
            assert g[0] == n_utts, l
            if l["section"] == "lin_z":
                continue
            if l["section"] == "post_z":
                gx, nz, split, seg_len, clear = g
                assert split == int(nz > 1) and (seg_len == 0) == (nz == 1), (l, g)
                if knobs.get("SCRF_POSTZ_SPLIT") == "0":
                    assert nz == 1, (l, g)
            else:
                gx, nz, seg_len, clear = g
                assert nz * seg_len >= t_max, (l, g)
            assert clear == int(nz > 1) and nz >= 1, (l, g)
            if nz > 1:
                assert nz * seg_len >= t_max and seg_len >= 2 * D and (nz - 1) * seg_len < t_max, (l, g)
        if l["section"] == "post_z":
            assert l["la"] == l["call_la"] and (l["rw"] == 48) == bool(l["la"] and L <= 48) and l["rw"] in (48, 64), l
            if D <= 40:
                seen.update("k_post_z<%d,%d,%d,%d>" % (l["dmax"], l["la"], l["rw"], sp) for sp in set(g[2] for g in grid))
        elif D <= 40:
            seen.add("k_%s<%d>" % (l["section"], l["dmax"]))


def check_frames(sections, seen):
    for l in sections["pframe"] + sections["ztf"]:
        n_out = (6 if l["call_la"] else 5) * l["L"]
        if l["kernel"] == "none":
            assert l["W_lo"] > 80, l
            continue
        grid = entries(l["grid"])
        assert l["W_hi"] <= 80 and len(grid) == len(N_TILES) - 1, l
        if l["section"] == "pframe":
            assert 4 * l["ks"] >= l["W_hi"] and l["gy"] * 64 >= n_out > (l["gy"] - 1) * 64, l
            for n, (gx, fpw) in zip(N_TILES[1:], grid):
                assert fpw >= 64 and fpw % 32 == 0 and gx * fpw >= n > (gx - 1) * fpw, (l, n)
            seen.add("k_pframe<%d>" % l["ks"])
        else:
            mt = 1 if l["narrow"] else 4
            assert l["mt"] == mt and 16 * l["nt"] >= l["W_hi"] and l["gy"] * 16 * mt >= n_out > (l["gy"] - 1) * 16 * mt, l
            assert [g[0] for g in grid] == list(N_TILES[1:]), l
            seen.add("k_ztf<%d,%d>" % (l["nt"], l["mt"]))


def parse_section(text):
    """parse, with the call's arguments f32 / la (before W=, or before kernel= where a line has no W) renamed call_f32 / call_la:
    the plan has fields of the same names"""
    out = []
    for ln in text.splitlines():
        head, sep, tail = ln.partition(" W=" if " W=" in ln else " kernel=")
        out.append(re.sub(r" (f32|la)=", r" call_\1=", head) + sep + tail)
    return parse("\n".join(out))


@pytest.fixture(scope="module")
def parsed(sweeps):
    return [{s: parse_section(t) for s, t in by.items()} for by in sweeps]


SEEN = {}   # knob set -> the instantiations its sweep emitted, once its lines are checked


@pytest.mark.parametrize("ki", range(len(KNOB_SETS)), ids=KNOB_IDS)
def test_every_planned_launch_fits_its_shape(parsed, ki):
    limit = lds_limit()
    assert limit == 160 * 1024
    knobs, sec = KNOB_SETS[ki], parsed[ki]
    seen = set()
    check_scores(sec["scores"], knobs, limit, seen)
    check_counts(sec["counts"], knobs, limit, seen)
    check_walks(sec, knobs, seen)
    check_frames(sec, seen)
    assert seen <= INSTANTIATIONS, sorted(seen - INSTANTIATIONS)
    # wherever fused_supported is 1, every launch has a plan; fused_la_supported implies fused_supported
    has_scores = planned_widths(sec["scores"], ("D", "mode"))
    has_counts = planned_widths(sec["counts"], ("D", "use_sb", "call_f32", "call_la"))
    ws_counts = {}
    for l in sec["counts"]:
        a = ws_counts.setdefault((l["D"], l["use_sb"], l["call_f32"], l["call_la"]), [False] * (W_MAX + 1))
        for W in range(l["W_lo"], l["W_hi"] + 1):
            a[W] = l["kernel"] in ("ws", "ws_n") and l["g0"] == 1
    n_fused = n_la = 0
    for l in sec["support"]:
        D, sb, f32 = l["D"], l["use_sb"], l["call_f32"]
        assert l["la"] <= l["fused"] and not (f32 and l["la"]), l
        if l["la"]:
            assert l["L"] <= 64, l
        if not l["fused"]:
            continue
        assert 2 <= D <= 40, l
        for W in range(l["W_lo"], l["W_hi"] + 1):
            assert has_scores[(D, 1 if f32 else 0)][W] and has_scores[(D, 3)][W] and has_counts[(D, sb, f32, 0)][W], (l, W)
            if l["la"]:
                assert has_scores[(D, 2)][W] and ws_counts[(D, sb, 0, 1)][W], (l, W)
        n_fused += l["W_hi"] - l["W_lo"] + 1
        n_la += (l["W_hi"] - l["W_lo"] + 1) * l["la"]
    assert n_fused > 0
    SEEN[ki] = seen
    print("%s: %d supported shapes (%d with the linear average), %d instantiations, largest LDS request %d bytes" %
          (KNOB_IDS[ki], n_fused, n_la, len(seen), max(l["lds"] for l in sec["scores"] + sec["counts"] if l["kernel"] != "none")))


def test_the_sweep_emits_exactly_the_recorded_instantiations(parsed):
    seen = []
    for ki, sec in enumerate(parsed):
        if ki not in SEEN:      # (run alone: the test above has not filled it)
            s = SEEN[ki] = set()
            check_scores(sec["scores"], KNOB_SETS[ki], 1 << 30, s)
            check_counts(sec["counts"], KNOB_SETS[ki], 1 << 30, s)
            check_walks(sec, KNOB_SETS[ki], s)
            check_frames(sec, s)
        seen.append(SEEN[ki])
    union = set().union(*seen)
    for name in sorted(union ^ INSTANTIATIONS):
        print("differs:", name)
    assert union == INSTANTIATIONS
    ids = {k: i for i, k in enumerate(KNOB_IDS)}
    # what each knob adds to or takes from the default set
    tall = {n for n in INSTANTIATIONS if ",100," in n}
    assert seen[0] & tall == set() and tall <= seen[ids["SCRF_EXPF_BIG=1"]] and tall <= seen[ids["SCRF_SIDE=0"]]
    assert not any(n.startswith("k_expf_fused_ws") for n in seen[ids["SCRF_EXPF_WS=0"]])
    assert not any(n.startswith("k_expf_fused_ws") and n.endswith(",1>") for n in seen[ids["SCRF_EXPF_DMA=0"]])
    assert not any(n.startswith("k_post_z") and n.endswith(",1>") for n in seen[ids["SCRF_POSTZ_SPLIT=0"]])
    for k in ("SCRF_SCORES_DMA=0", "SCRF_DTAB=0", "SCRF_RTAB=0"):
        assert not any(n.startswith("k_scores_fused") and n.endswith(",1>") for n in seen[ids[k]]), k
        assert {n for n in seen[0] if n.startswith("k_scores_fused")} == {n[:-3] + ",1>" for n in seen[ids[k]] if n.startswith("k_scores_fused")}


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


def test_the_launchers_hold_no_threshold_of_their_own():
    """scrf_fused.hip takes every form from the plan: no macro ladder, no comparison against a size, and the helpers and the
    tile geometry are defined in the header only"""
    src = open(os.path.join(CSRC, "scrf_fused.hip")).read()
    assert "_GO(" not in src and "_GO3(" not in src
    for m in re.finditer(r"^(?:static )?void (launch_\w+)\(.*?^}", src, re.S | re.M):
        body = m.group(0)
        if m.group(1) in ("launch_tile_tables", "launch_dur_table", "launch_avg_prefix", "launch_add_p_exp"):
            continue        # no form to pick
        assert not re.search(r"(<=|>=)\s*\w", body), m.group(1)
        assert not re.search(r"\b(76|100|156|1024)\b", body), m.group(1)
        assert not re.search(r"lay\.D\s*[<>]|\bW\s*[<>]\s*\d|sizeof\(float\)|\bkn\.", body), m.group(1)
    for name in ("FU_ROWS", "FE_ROWS", "FW_ROWS_BIG", "FU_GC", "FU_XS", "FU_WS", "FU_DS", "FE_RS", "FE_RSF", "PF_MT", "FU_EXPT_N", "FU_NT", "FE_NT", "FW_NT"):
        assert not re.search(r"#define\s+%s\b" % name, src), name
    eng = open(os.path.join(CSRC, "scrf_engine.cpp")).read() + open(os.path.join(CSRC, "scrf_kernels.h")).read()
    for name in ("fused_supported", "fused_scores_tb", "fused_expf_plan", "fused_expf_blocks", "lin_z5_segments", "pframe_supported", "fu_sample_step"):
        assert not re.search(r"^\w[\w \*]*\b%s\(.*\)\s*[;{]" % name, src + eng, re.M), name


def test_the_count_switch_names_exactly_the_reachable_forms():
    """the (NT, DMAX, NKS) keys launch_expf_fused's switch names, per count kernel, are those of INSTANTIATIONS"""
    src = open(os.path.join(CSRC, "scrf_fused.hip")).read()
    body = re.search(r"^void launch_expf_fused\(.*?^}", src, re.S | re.M).group(0)
    depths = [(int(dm), int(ks)) for dm, ks in re.findall(r"FE_CASE\(GO, N, (\d+), (\d+)\)", body)]
    assert depths
    named = {(go, int(nt), dm, ks) for go, nt in re.findall(r"FE_DEPTHS\((launch_\w+), (\d+)\)", body) for dm, ks in depths}
    named |= {(go, int(nt), int(dm), int(ks)) for go, nt, dm, ks in re.findall(r"FE_CASE\((launch_\w+), (\d+), (\d+), (\d+)\)", body)}
    want = set()
    for name in INSTANTIATIONS:
        a = [int(x) for x in name[name.index("<") + 1:-1].split(",")]
        if name.startswith("k_expf_fused<"):
            want.add(("launch_expf_fused_t", a[0], a[1], a[3]))
        elif name.startswith("k_expf_fused_ws"):
            want.add(("launch_expf_ws_t" if a[4] == 76 else "launch_expf_big_t", a[0], a[1], a[2]))
    assert named == want, sorted(named ^ want)


def test_single_calls_match_the_sweep(probes, parsed):
    sec = parsed[0]
    for L, D, W, mode in ((47, 25, 39, 0), (64, 10, 13, 2), (200, 25, 39, 1), (48, 40, 40, 3)):
        got = parse(run(probes[0], "scores", L, D, W, mode))[0]
        want = [l for l in sec["scores"] if l["D"] == D and l["mode"] == mode and l["W_lo"] <= W <= l["W_hi"]]
        assert len(want) == 1
        for k, v in got.items():
            if k == "grid":
                assert entries(v)[0] == entries(want[0]["grid"])[LS.index(L)]
            elif k not in ("W_lo", "W_hi"):
                assert v == want[0][k], (k, got, want[0])
    for L, D, sb, W, f32, la, al, nt in ((47, 25, 1, 39, 0, 1, 1, 257), (64, 10, 1, 13, 0, 0, 1, 513), (48, 25, 0, 144, 0, 0, 0, 3), (6, 30, 1, 20, 1, 0, 1, 1)):
        got = parse_section(run(probes[0], "counts", L, D, sb, W, f32, la, al, nt))[0]
        want = [l for l in sec["counts"] if (l["D"], l["use_sb"], l["call_f32"], l["call_la"]) == (D, sb, f32, la) and l["W_lo"] <= W <= l["W_hi"]]
        assert len(want) == 1
        li = LS.index(L)
        assert (got["gy"], got["dma"], got["gx"]) == (entries(want[0]["gy"])[li][0], entries(want[0]["dma"])[2 * li + al][0], entries(want[0]["gx"])[N_TILES.index(nt)][0])
        for k, v in got.items():
            if k not in ("W_lo", "W_hi", "gy", "dma", "gx"):
                assert v == want[0][k], (k, got, want[0])
