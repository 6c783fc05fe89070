"""-m "not gpu": which instantiations launch_scores_mfma and launch_expf_mfma pick (asr-craft_amd/csrc/scrf_mfma_plan.h).

The two launchers of scrf_mfma.hip take their choice from the host-only header, so tests/host/mfma_plan_probe.cpp, which
compiles that header alone with g++, answers for them.  The sweep runs every call over n_out 1..640, nfe / nfun 1..800,
both precisions and both row maps, under the default knobs, with each of the three knobs of the choice off and with both
count knobs off, twice: by the plain probe and by one built with AddressSanitizer and UBSan.  Checked on every call: the launches tile [0, n_out) without
gap or overlap, a launch's overhang lies in its last tile only, the feature tiles cover nfun, MT <= MTW, the wave-specialised
and double-buffered forms appear only where the kernels exist, the LDS request fits a workgroup; and the set of instantiations
the sweep emits is INSTANTIATIONS below, which tests/test_mfma_forms.py holds the GPU case table against."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "asr-craft_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "host", "mfma_plan_probe.cpp")

N_OUT_MAX, NF_MAX = 640, 800
# the default, each knob of the choice off, and both count knobs off: the one-pair 8-wave f64 kernel needs the two together
KNOB_SETS = ({}, {"SCRF_SCORES_MFMA_WS": "0"}, {"SCRF_EXPF_MFMA_WS": "0"}, {"SCRF_EXPF_DB": "0"}, {"SCRF_EXPF_MFMA_WS": "0", "SCRF_EXPF_DB": "0"})
INT_FIELDS = ("f32", "nt", "mw", "ntw", "has_xrow", "nw", "kc", "mt", "mtw", "db", "o_base", "gy", "o_step", "gx", "lds", "wide_tiles")


def inst(l):
    """the instantiation of a launch, as the tests name it"""
    if l["call"] == "scores":
        if l["kernel"] == "single":
            return "k_scores_mfma<F32=%d,NT=%d>" % (l["f32"], l["nt"])
        return "k_scores_mfma_ws<MW=%d,NTW=%d>" % (l["mw"], l["ntw"])
    if l["kernel"] == "ws":
        return "k_expf_mfma_ws<XROW=%d,MT=%d>" % (l["has_xrow"], l["mt"])
    if l["kernel"] == "split":
        return "k_expf_mfma<XROW=%d,NW=%d,KC=%d,F32=%d,SPLIT>" % (l["has_xrow"], l["nw"], l["kc"], l["f32"])
    return "k_expf_mfma<XROW=%d,NW=%d,KC=%d,F32=%d,MT=%d,DB=%d,MTW=%d>" % (l["has_xrow"], l["nw"], l["kc"], l["f32"], l["mt"], l["db"], l["mtw"])


def _expected():
    out = set()
    for f32 in (0, 1):
        out |= {"k_scores_mfma<F32=%d,NT=%d>" % (f32, nt) for nt in (1, 2, 3)}
        for x in (0, 1):
            out.add("k_expf_mfma<XROW=%d,NW=4,KC=16,F32=%d,SPLIT>" % (x, f32))
            for nw, kc in ((1, 32), (2, 64), (3, 64), (4, 64)):      # the narrow forms: one image pair, 48 outputs wide
                out |= {"k_expf_mfma<XROW=%d,NW=%d,KC=%d,F32=%d,MT=%d,DB=0,MTW=3>" % (x, nw, kc, f32, mt) for mt in (1, 2, 3)}
            mtw = 3 if f32 else 4                                       # the 8-wave form: 64 outputs wide in f64
            for db in (0, 1):                                           # DB=0 only under SCRF_EXPF_DB=0
                out |= {"k_expf_mfma<XROW=%d,NW=8,KC=32,F32=%d,MT=%d,DB=%d,MTW=%d>" % (x, f32, mt, db, mtw) for mt in range(1, mtw + 1)}
    out |= {"k_scores_mfma_ws<MW=4,NTW=3>", "k_scores_mfma_ws<MW=2,NTW=7>"}
    out |= {"k_expf_mfma_ws<XROW=%d,MT=%d>" % (x, mt) for x in (0, 1) for mt in (1, 2, 3, 4)}
    return frozenset(out)


# every instantiation the launchers can reach: 6 + 2 single-role and wave-specialised score kernels, 4 split count
# kernels, 48 narrow, 28 8-wave (of which the 8 f64 ones with DB=1 only under SCRF_EXPF_MFMA_WS=0 and the 14 with DB=0 only
# under SCRF_EXPF_DB=0, f64 then with SCRF_EXPF_MFMA_WS=0 too) and 8 role-split count kernels.  A new or vanished one is an
# edit of this list.
INSTANTIATIONS = _expected()
assert len(INSTANTIATIONS) == 6 + 2 + 4 + 48 + 28 + 8


def parse(out):
    """probe lines -> launches (dicts: call, n_out, nf_lo, nf_hi, call_f32, call_xrow, kernel, the integer fields)"""
    res = []
    for ln in out.splitlines():
        w = ln.split()
        n_head = 5 if w[0] == "scores" else 6
        l = dict(call=w[0], n_out=int(w[1]), nf_lo=int(w[2]), nf_hi=int(w[3]), call_f32=int(w[4]), call_xrow=int(w[5]) if w[0] == "counts" else 0)
        for kv in w[n_head:]:
            k, v = kv.split("=")
            l[k] = v if k == "kernel" else int(v)
        res.append(l)
    return res


def build(tmp, name, extra=()):
    exe = str(tmp / name)
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I" + CSRC, *extra, SRC, "-o", exe], check=True, timeout=300)
    return exe


@pytest.fixture(scope="module")
def probes(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("mfma_plan")
    return build(tmp, "mfma_plan_probe"), build(tmp, "mfma_plan_probe_san", ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))


def run(exe, *args, **knobs):
    r = subprocess.run([exe] + [str(a) for a in args] + ["%s=%s" % kv for kv in knobs.items()], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-2000:])
    return r.stdout


@pytest.fixture(scope="module")
def sweeps(probes):
    """per knob set the parsed sweep; the sanitized probe must print the same bytes and nothing on stderr"""
    res = []
    for knobs in KNOB_SETS:
        out = run(probes[0], "sweep", N_OUT_MAX, NF_MAX, **knobs)
        assert run(probes[1], "sweep", N_OUT_MAX, NF_MAX, **knobs) == out, knobs
        res.append(parse(out))
    return res


def lds_limit():
    m = re.search(r"#define SCRF_LDS_BYTES \((\d+) \* 1024\)", open(os.path.join(CSRC, "scrf_common.h")).read())
    return int(m.group(1)) * 1024


def calls(launches):
    """launches grouped by call: {(call, n_out, nf_lo, nf_hi, f32, xrow): [launch, ..]} in the order of launching"""
    by = {}
    for l in launches:
        by.setdefault((l["call"], l["n_out"], l["nf_lo"], l["nf_hi"], l["call_f32"], l["call_xrow"]), []).append(l)
    return by


def check_call(key, ls, knobs, limit):
    """every property of one call's launches (for each feature count of its run nf_lo..nf_hi)"""
    call, n_out, nf_lo, nf_hi, f32, xrow = key
    at = 0
    for i, l in enumerate(ls):
        assert all(isinstance(l[k], int) and l[k] >= 0 for k in INT_FIELDS if k in l), (key, l)
        # consecutive, no gap, no overlap: a launch starts where the one before it stops owning outputs
        assert l["o_base"] == at, (key, "o_base", l["o_base"], at)
        assert l["gy"] >= 1 and l["o_step"] >= 1 and l["gx"] >= 1
        if l["kernel"] == "single":
            width = 16 * l["nt"]
        elif call == "counts" and l["kernel"] != "split":
            width = 16 * l["mt"]
        else:       # the wave-specialised score tiles and the split count form compute whole tiles
            width = l["o_step"]
        assert width <= l["o_step"]
        end = l["o_base"] + l["gy"] * l["o_step"]
        # every tile but the last is whole and inside n_out; the outputs a launch computes reach to its end or to n_out
        assert l["o_base"] + (l["gy"] - 1) * l["o_step"] < n_out, (key, "a tile wholly past n_out", l)
        if l["gy"] > 1:
            assert width == l["o_step"], (key, "thin tiles in a launch of several", l)
        computed_end = l["o_base"] + (l["gy"] - 1) * l["o_step"] + width
        if i + 1 < len(ls):
            assert end <= n_out and computed_end == end, (key, "a launch that is not the last leaves outputs uncomputed or hangs over", l)
        else:
            assert computed_end >= n_out, (key, "outputs left over", l)
            # no whole 16-output tile past n_out (the split form: whole wavefronts of its one 192-wide tile may idle)
            assert computed_end - n_out < (l["o_step"] if l["kernel"] == "split" else 16), (key, "a whole tile past n_out", l)
        at = end
        assert l["f32"] == f32
        assert l["lds"] <= limit, (key, l["lds"])
        if call == "scores":
            assert l["gx"] == 1
            if l["kernel"] == "single":
                assert l["nt"] in (1, 2, 3) and l["o_step"] == 48 and l["lds"] == 0
            else:
                assert l["kernel"] == "ws" and (l["mw"], l["ntw"], l["o_step"]) in ((4, 3, 96), (2, 7, 112))
                assert not f32 and nf_lo >= 192 and n_out >= 96 and knobs.get("SCRF_SCORES_MFMA_WS") != "0"
        else:
            assert l["has_xrow"] == xrow and l["kernel"] in ("plain", "db", "ws", "split")
            assert 1 <= l["mt"] <= l["mtw"], (key, l)
            if l["kernel"] == "split":
                assert nf_hi <= 48 and n_out >= 192 and (l["nw"], l["kc"], l["o_step"], l["gx"], l["db"]) == (4, 16, 192, 1, 0)
                assert l["gx"] * 48 >= nf_hi
            else:
                assert l["gx"] * 48 * l["nw"] >= nf_hi and (l["gx"] - 1) * 48 * l["nw"] < nf_lo, (key, l)
                assert (l["nw"], l["kc"]) in ((1, 32), (2, 64), (3, 64), (4, 64), (8, 32))
                assert l["nw"] == min(8, -(-nf_hi // 48)) if nf_hi <= 192 else l["nw"] == 8
                assert l["o_step"] == 16 * l["mtw"] and l["mtw"] == (4 if l["nw"] == 8 and not f32 else 3)
                assert (l["db"] == 1) == (l["kernel"] == "db")
                if l["kernel"] in ("ws", "db"):
                    assert l["nw"] == 8
                if l["kernel"] == "ws":
                    assert not f32 and knobs.get("SCRF_EXPF_MFMA_WS") != "0"
                if l["kernel"] == "db":
                    assert knobs.get("SCRF_EXPF_DB") != "0"
                if l["nw"] == 8:      # the knobs decide among the three 8-wave forms, and only they
                    want = "ws" if not f32 and knobs.get("SCRF_EXPF_MFMA_WS") != "0" else "db" if knobs.get("SCRF_EXPF_DB") != "0" else "plain"
                    assert l["kernel"] == want, (key, l["kernel"], want)
            wide = (-(-nf_hi // 384)) * (-(-n_out // (48 if f32 else 64))) if nf_lo > 192 else 0
            assert l["wide_tiles"] == wide, (key, l["wide_tiles"], wide)
    assert at >= n_out


def test_the_sweep_runs_every_call_once(sweeps):
    for launches in sweeps:
        by = calls(launches)
        runs = {}
        for (call, n_out, lo, hi, f32, xrow) in by:
            runs.setdefault((call, n_out, f32, xrow), []).append((lo, hi))
        assert len(runs) == N_OUT_MAX * 2 * 3      # scores, counts without and with a row map; both precisions
        for k, r in runs.items():
            r.sort()
            assert r[0][0] == 1 and r[-1][1] == NF_MAX and all(a[1] + 1 == b[0] for a, b in zip(r, r[1:])), (k, r)


@pytest.mark.parametrize("ki", range(len(KNOB_SETS)), ids=[" ".join("%s=%s" % kv for kv in k.items()) or "default" for k in KNOB_SETS])
def test_every_call_tiles_its_outputs_and_features(sweeps, ki):
    limit = lds_limit()
    assert limit == 160 * 1024
    by = calls(sweeps[ki])
    for key, ls in by.items():
        check_call(key, ls, KNOB_SETS[ki], limit)
    print("%d runs of calls, %d launches, largest LDS request %d bytes" % (len(by), len(sweeps[ki]), max(l["lds"] for l in sweeps[ki])))


def test_the_sweep_emits_exactly_the_recorded_instantiations(sweeps):
    seen = [set(inst(l) for l in launches) for launches in sweeps]
    union = set().union(*seen)
    for name in sorted(union ^ INSTANTIATIONS):
        print("differs:", name)
    assert union == INSTANTIATIONS
    # what each knob adds to the default set, and nothing else
    assert seen[1] == seen[0] - {"k_scores_mfma_ws<MW=4,NTW=3>", "k_scores_mfma_ws<MW=2,NTW=7>"}
    assert seen[2] - seen[0] == {"k_expf_mfma<XROW=%d,NW=8,KC=32,F32=0,MT=%d,DB=1,MTW=4>" % (x, mt) for x in (0, 1) for mt in (1, 2, 3, 4)}
    assert seen[3] - seen[0] == {"k_expf_mfma<XROW=%d,NW=8,KC=32,F32=1,MT=%d,DB=0,MTW=3>" % (x, mt) for x in (0, 1) for mt in (1, 2, 3)}
    assert seen[4] - seen[3] == {"k_expf_mfma<XROW=%d,NW=8,KC=32,F32=0,MT=%d,DB=0,MTW=4>" % (x, mt) for x in (0, 1) for mt in (1, 2, 3, 4)}


def test_the_launchers_hold_no_threshold_of_their_own():
    """scrf_mfma.hip takes the form from the plan: the numbers of the choice occur in the header only"""
    src = open(os.path.join(CSRC, "scrf_mfma.hip")).read()
    a = src.index("void launch_scores_mfma(")
    body = src[a:src.index("#undef SCORES_ARGS")]
    assert "scrf_scores_mfma_plan(" in body and not re.search(r"\b(192|96|112|48)\b", body)
    a = src.index("void launch_expf_mfma(")
    body = src[a:]
    assert "scrf_expf_mfma_plan(" in body and not re.search(r"\b(192|384|48|47)\b", body)
    assert "kn." not in src[src.index("static void launch_scores_mfma_ws("):].replace("h->kn", "")
    for name in ("SM_NO", "SW_NO", "EM_MTF", "EW_IMG", "SW_IMG", "EM_SPLIT_NO"):
        assert not re.search(r"#define\s+%s\b" % name, src), name


def test_single_calls_match_the_sweep(probes, sweeps):
    by = calls(sweeps[0])
    for call, n_out, nf, f32, xrow in (("scores", 121, 200, 0, 0), ("counts", 121, 200, 0, 1), ("counts", 196, 40, 1, 0), ("scores", 56, 5, 1, 0)):
        args = (n_out, nf, f32) + ((xrow,) if call == "counts" else ())
        got = parse(run(probes[0], call, *args))
        want = [ls for k, ls in by.items() if k[0] == call and k[1] == n_out and k[2] <= nf <= k[3] and k[4] == f32 and k[5] == xrow]
        assert len(want) == 1
        strip = lambda l: {k: v for k, v in l.items() if k not in ("nf_lo", "nf_hi")}
        assert [strip(l) for l in got] == [strip(l) for l in want[0]]
