"""-m gpu: CRFFstDecode crf_lat_beam=B on a tiny segmental model trained by CRFTrain: the lattice dump and
the MLF path consume the beam-pruned machines, the label file and the decoded words do not change, the summary line
counts what the files hold, and the flag is refused where no lattice would survive or be consumed."""
import os
import re
import subprocess

import numpy as np
import pytest

import orc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "asr-craft_amd", "bin")
L, D, W = 3, 3, 2
TS = [3, 5, 8, 6]


@pytest.fixture(scope="module")
def tiny(tmp_path_factory):
    """data and a weight file written the way tests/test_gpu_cli.py writes them (helpers copied: test modules are not imported)"""
    d = tmp_path_factory.mktemp("latprune_cli")
    rng = np.random.RandomState(33)
    f = str(d / "f.ascii"); lbl = str(d / "l.ascii")
    with open(f, "w") as ff, open(lbl, "w") as lf:
        for u, T in enumerate(TS):
            X = rng.random_sample((T, W)).astype(np.float32)
            lab = np.repeat(rng.randint(0, L, T), 2)[:T]
            for t in range(T):
                ff.write("%d %d %s\n" % (u, t, " ".join("%.9g" % v for v in X[t])))
                lf.write("%d %d %d\n" % (u, t, lab[t]))
    model = ["ftr1_file=" + f, "ftr1_format=ascii", "ftr1_extract_seg_ftr=1", "crf_label_size=%d" % L, "crf_featuremap=stdstate",
             "crf_model_type=stdseg_no_dur_no_segtransftr", "label_maximum_duration=%d" % D]
    wf = str(d / "w.out")
    r = subprocess.run([os.path.join(BIN, "CRFTrain")] + model + ["hardtarget_file=" + lbl, "out_weight_file=" + wf, "crf_epochs=6", "crf_lr=1.0",
                        "crf_bunch_size=1", "threads=1"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    # the phone "bigram" LM of tests/test_gpu_cli.py: reads phone-duration labels, writes phone symbols 11 + l
    arcs, finals = [], {}
    cost = rng.rand(L + 1, L) * 2
    for q in range(L + 1):
        for l in range(L):
            for dd in range(D):
                arcs.append((q, l + 1, l + L * dd + 1, 11 + l, float(np.float32(cost[q, l] + (3.0 if q == l + 1 else 0.0) + 0.1 * dd))))
        if q:
            finals[q] = float(np.float32(rng.rand()))
    lmf = str(d / "lm.fst.txt")
    with open(lmf, "w") as fh:
        for a in arcs:
            fh.write("%d %d %d %d %.9g\n" % a)
        for s_, w_ in finals.items():
            fh.write("%d %.9g\n" % (s_, w_))
    olist, osym = str(d / "olist"), str(d / "osym.txt")
    open(olist, "w").write("".join("u%d\n" % i for i in range(len(TS))))
    open(osym, "w").write("<eps> 0\n" + "".join("p%d %d\n" % (l, 11 + l) for l in range(L)))
    return d, model + ["weight_file=" + wf], lmf, olist, osym


def _decode(flags):
    return subprocess.run([os.path.join(BIN, "CRFFstDecode")] + flags, capture_output=True, text=True, timeout=300)


def _read_lat_txt(path):
    rows = [x.split() for x in open(path).read().split("\n") if x]
    arcs = np.zeros(len(rows) - 1, dtype=orc.ARC_DTYPE)
    for i, r in enumerate(rows[:-1]):
        arcs[i] = (int(r[0]), int(r[2]), int(r[3]), np.float32(r[4]), int(r[1]))
    return arcs, int(rows[-1][0])


@pytest.mark.parametrize("bunch", [256, 3])
def test_lattice_dump_with_and_without_the_beam(tiny, bunch):
    d, model, lmf, olist, osym = tiny
    full_dir, cut_dir = d / ("full_%d" % bunch), d / ("cut_%d" % bunch)
    full_dir.mkdir(); cut_dir.mkdir()
    lab0, lab1 = str(d / ("lab0_%d.txt" % bunch)), str(d / ("lab1_%d.txt" % bunch))
    r0 = _decode(model + ["crf_lat_outdir=" + str(full_dir), "crf_output_labelfile=" + lab0])
    assert r0.returncode == 0, r0.stdout + r0.stderr
    r1 = _decode(model + ["crf_lat_outdir=" + str(cut_dir), "crf_output_labelfile=" + lab1, "crf_lat_beam=2", "crf_bunch_size=%d" % bunch])
    assert r1.returncode == 0, r1.stdout + r1.stderr
    assert open(lab0, "rb").read() == open(lab1, "rb").read()
    got = np.loadtxt(lab1).astype(int).reshape(-1, 3)
    kept = total = 0
    for u in range(len(TS)):
        fa, ffin = _read_lat_txt(str(full_dir / ("fst.%d.txt" % u)))
        ca, cfin = _read_lat_txt(str(cut_dir / ("fst.%d.txt" % u)))
        print("sentence %d: %d of %d arcs" % (u, ca.shape[0], fa.shape[0]))
        assert ca.shape[0] < fa.shape[0]
        assert os.path.exists(str(cut_dir / ("fst.%d.final.fst" % u)))
        assert (ca["src"] < ca["dst"]).all() and ca["src"].min() == 0 and cfin == max(ca["dst"].max(), ca["src"].max())
        labs, cost = orc.best_path(ca, cfin + 1, cfin)
        assert list(labs) == list(got[got[:, 0] == u][:, 2])
        kept += ca.shape[0]; total += fa.shape[0]
    m = re.search(r"Lattice beam 2: kept (\d+) of (\d+) arcs", r1.stdout)
    assert m, r1.stdout
    assert (int(m.group(1)), int(m.group(2))) == (kept, total)


def test_mlf_path_consumes_the_pruned_lattice(tiny):
    d, model, lmf, olist, osym = tiny
    mlf = ["crf_olist=" + olist, "crf_osymbols=" + osym]

    def run(tag, extra):
        out = str(d / (tag + ".mlf"))
        r = _decode(model + mlf + ["crf_output_mlffile=" + out, "crf_output_labelfile=" + str(d / (tag + ".lab"))] + extra)
        assert r.returncode == 0, r.stdout + r.stderr
        return open(out, "rb").read(), r.stdout

    # with an LM: a beam that keeps every arc gives the byte-identical MLF
    base, _ = run("lm_full", ["crf_lm_txt=" + lmf])
    wide, so = run("lm_wide", ["crf_lm_txt=" + lmf, "crf_lat_beam=1e30"])
    assert base == wide and base.count(b'"u') == len(TS)
    m = re.search(r"Lattice beam 1e\+30: kept (\d+) of (\d+) arcs", so)
    assert m and m.group(1) == m.group(2), so
    # without an LM the best path survives any beam: beam 2 gives the same MLF as no beam
    plain, _ = run("plain", [])
    cut, so = run("cut", ["crf_lat_beam=2"])
    assert plain == cut
    m = re.search(r"Lattice beam 2: kept (\d+) of (\d+) arcs", so)
    assert m and int(m.group(1)) < int(m.group(2)), so


def test_refusals(tiny):
    d, model, lmf, olist, osym = tiny
    lat = ["crf_lat_outdir=" + str(d)]
    for flags, msg in [(lat + ["crf_lat_beam=0"], "> 0"), (lat + ["crf_lat_beam=-1.5"], "> 0"),
                       (lat + ["crf_lat_beam=2", "crf_decode_mode=align", "hardtarget_file=" + str(d / "l.ascii")], "crf_decode_mode=align"),
                       (["crf_lat_beam=2", "crf_decode_mode=posteriors", "crf_output_posteriorfile=" + str(d / "p.txt")], "crf_decode_mode=posteriors"),
                       (["crf_lat_beam=2", "crf_output_labelfile=" + str(d / "x.lab")], "crf_lat_outdir and/or crf_output_mlffile")]:
        r = _decode(model + flags)
        assert r.returncode == 1 and "crf_lat_beam" in r.stderr and msg in r.stderr, (flags, r.returncode, r.stderr)


def test_a_model_the_engine_refuses_surfaces_its_message(tiny):
    d, model, lmf, olist, osym = tiny
    flags = [x for x in model if not x.startswith(("crf_model_type=", "weight_file=", "crf_label_size="))]
    flags += ["crf_model_type=stdseg", "crf_label_size=%d" % (L * D), "num_actual_labs=%d" % L]
    wf = str(d / "w_stdseg.out")
    open(wf, "w").write("0.25\n-0.5\n" * 40)   # any weights do: the refusal does not depend on them, and lines a model lacks read as 0
    r = _decode(flags + ["weight_file=" + wf, "crf_output_labelfile=" + str(d / "stdseg.lab")])
    assert r.returncode == 0, r.stdout + r.stderr   # the model itself decodes
    r = _decode(flags + ["weight_file=" + wf, "crf_lat_outdir=" + str(d), "crf_lat_beam=2"])
    assert r.returncode != 0 and "lattice beam is not built for the \"stdseg\"" in r.stderr, r.stdout + r.stderr
