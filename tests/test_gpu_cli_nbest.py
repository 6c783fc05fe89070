"""-m gpu: N-best lists through the front-end and crf_amd_nbest, on the tiny segmental model of
tests/test_gpu_cli_align.py: CRFFstDecode crf_nbest=N crf_output_nbestfile=PATH with crf_nbest_unique and crf_nbest_rescore,
against the Python binding on the same frames and weights.  The label file and the confidence file keep their bytes."""
import os
import subprocess

import numpy as np
import pytest

import scrf_amd

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "asr-craft_amd", "bin")
L, D, W = 3, 3, 2
TS = [3, 5, 8, 6, 1]
N = 7


def _decode(flags):
    return subprocess.run([os.path.join(BIN, "CRFFstDecode")] + flags, capture_output=True, text=True, timeout=300)


def _collapse(x):
    return [v for i, v in enumerate(x) if i == 0 or v != x[i - 1]]


@pytest.fixture(scope="module")
def tiny(tmp_path_factory):
    """data and a weight file written the way tests/test_gpu_cli_align.py writes them (copied: test modules are not imported),
    and the binding on the same inputs: the weights as the front-end reads them back, the precision it defaults to"""
    d = tmp_path_factory.mktemp("nbest_cli")
    rng = np.random.RandomState(34)
    f = str(d / "f.ascii"); lbl = str(d / "l.ascii")
    frames = []
    with open(f, "w") as ff, open(lbl, "w") as lf:
        for u, T in enumerate(TS):
            X = rng.random_sample((T, W)).astype(np.float32)
            frames.append(X)
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
    eng = scrf_amd.Engine(scrf_amd.make_config(model_type=scrf_amd.STDSEG_NO_DUR_NO_SEGTRANSFTR, L=L, D=D, F=scrf_amd.window_width(W, D, 0, 0, True),
                                               precision=scrf_amd.PREC_FAST))
    eng.set_lambda(np.loadtxt(wf))
    b = eng.batch_from_frames(frames, None, [scrf_amd.StreamRecipe(W, 0, 0, 1)], None)
    labs, hoff, cost = eng.nbest_batch(b, N)
    hyps = [[([int(x) for x in labs[i]], cost[i]) for i in range(int(hoff[u]), int(hoff[u + 1]))] for u in range(len(TS))]
    seqs = []   # per utterance the distinct collapsed sequences, each with its first (cheapest) path's cost
    for h in hyps:
        s = []
        for p, c in h:
            q = _collapse([l % L for l in p])
            if q not in [x[0] for x in s]:
                s.append((q, c))
        seqs.append(s)
    logp = [[None] * len(s) for s in seqs]
    for r_ in range(max(len(s) for s in seqs)):   # one transcript pass per rank, as crf_amd_nbest runs them
        tr = [np.asarray(s[r_][0] if r_ < len(s) else [], dtype=np.uint32) for s in seqs]
        out = eng.transcript_batch(b, tr, scrf_amd.ALIGN_RUNS, frame=False, end=False)
        for u, s in enumerate(seqs):
            if r_ < len(s):
                logp[u][r_] = float(out["logp"][u])
    b.close(); eng.close()
    return d, model + ["weight_file=" + wf], dict(hyps=hyps, seqs=seqs, logp=logp)


def _rows(path):
    return [ln.split() for ln in open(path).read().splitlines()]


def _label_rows(path):
    out = [[] for _ in TS]
    for u, i, lab in np.loadtxt(path, ndmin=2).astype(int).reshape(-1, 3):
        assert i == len(out[u])
        out[u].append(int(lab))
    return out


def test_the_nbestfile_holds_the_bindings_paths_and_the_other_files_keep_their_bytes(tiny):
    d, flags, ref = tiny
    l0, c0 = str(d / "plain.lab"), str(d / "plain.conf")
    r = _decode(flags + ["crf_output_labelfile=" + l0, "crf_output_conffile=" + c0])
    assert r.returncode == 0, r.stdout + r.stderr
    for bunch in (256, 2):
        nb, lab, conf = (str(d / ("n_%d.%s" % (bunch, x))) for x in ("nbest", "lab", "conf"))
        r = _decode(flags + ["crf_nbest=%d" % N, "crf_output_nbestfile=" + nb, "crf_output_labelfile=" + lab, "crf_output_conffile=" + conf,
                             "crf_bunch_size=%d" % bunch])
        assert r.returncode == 0, r.stdout + r.stderr
        assert open(lab, "rb").read() == open(l0, "rb").read() and os.path.getsize(l0) > 0
        assert open(conf, "rb").read() == open(c0, "rb").read() and os.path.getsize(c0) > 0
        rows = _rows(nb)
        want = [(u, r_, p, c) for u, h in enumerate(ref["hyps"]) for r_, (p, c) in enumerate(h)]
        assert len(rows) == len(want) and len(ref["hyps"][4]) == L and len(ref["hyps"][2]) == N   # T = 1 has L paths only
        for row, (u, r_, p, c) in zip(rows, want):
            assert [int(row[0]), int(row[1]), int(row[3])] == [u, r_, len(p)] and len(row) == 4 + len(p)
            assert [int(x) for x in row[4:]] == p
            assert np.float32(row[2]).tobytes() == np.float32(c).tobytes(), (row, c)   # 9 significant digits hold a float
        best = _label_rows(lab)
        for u in range(len(TS)):   # rank 0 is the label file's path
            assert ref["hyps"][u][0][0] == best[u]
    # without the confidence file as well
    nb, lab = str(d / "n_only.nbest"), str(d / "n_only.lab")
    r = _decode(flags + ["crf_nbest=%d" % N, "crf_output_nbestfile=" + nb, "crf_output_labelfile=" + lab])
    assert r.returncode == 0 and open(lab, "rb").read() == open(l0, "rb").read() and _rows(nb) == rows


def test_unique_phones_lists_distinct_sequences_and_rescoring_appends_the_bindings_logp(tiny):
    d, flags, ref = tiny
    for rescore in (0, 1):
        nb, lab = str(d / ("u_%d.nbest" % rescore)), str(d / ("u_%d.lab" % rescore))
        r = _decode(flags + ["crf_nbest=%d" % N, "crf_output_nbestfile=" + nb, "crf_output_labelfile=" + lab, "crf_nbest_unique=phones",
                             "crf_nbest_rescore=%d" % rescore, "crf_bunch_size=3"])
        assert r.returncode == 0, r.stdout + r.stderr
        rows = _rows(nb)
        # crf_bunch_size=3 cuts the batch differently from the binding's one batch: the per-rank passes differ, the sums do not
        want = [(u, r_, q, c) for u, s in enumerate(ref["seqs"]) for r_, (q, c) in enumerate(s)]
        assert len(rows) == len(want)
        per_utt = {}
        for row, (u, r_, q, c) in zip(rows, want):
            assert [int(row[0]), int(row[1]), int(row[3])] == [u, r_, len(q)] and len(row) == 4 + len(q) + rescore
            assert [int(x) for x in row[4:4 + len(q)]] == q and np.float32(row[2]).tobytes() == np.float32(c).tobytes()
            per_utt.setdefault(u, []).append(tuple(row[4:4 + len(q)]))
            if rescore:
                print("sent %d rank %d: logp %s, binding %.17g" % (u, r_, row[-1], ref["logp"][u][r_]))
                assert float(row[-1]) == ref["logp"][u][r_] and float(row[-1]) < 0.0
        assert all(len(set(v)) == len(v) for v in per_utt.values())   # distinct per utterance
        assert any(len(s) < len(h) for s, h in zip(ref["seqs"], ref["hyps"]))   # the reduction does drop paths here


def test_every_refused_flag_combination_exits_with_its_message(tiny):
    d, flags, _ = tiny
    nb = "crf_output_nbestfile=" + str(d / "never.nbest")
    on = ["crf_nbest=3", nb]
    hard = "hardtarget_file=" + str(d / "l.ascii")
    for fl, msg in [([nb], "crf_output_nbestfile needs crf_nbest=N"),
                    (["crf_nbest_unique=phones"], "crf_nbest_unique needs crf_nbest=N"),
                    (["crf_nbest_rescore=1"], "crf_nbest_rescore needs crf_nbest=N"),
                    (["crf_nbest=3"], "crf_nbest needs crf_output_nbestfile=PATH"),
                    (["crf_nbest=0", nb], "must be 1 .. 65535"),
                    (on + ["crf_nbest_unique=words"], "(path|phones)"),
                    (on + ["crf_nbest_rescore=1"], "crf_nbest_rescore=1 needs crf_nbest_unique=phones"),
                    (on + ["crf_nbest_rescore=1", "crf_nbest_unique=path"], "crf_nbest_rescore=1 needs crf_nbest_unique=phones"),
                    (on + ["crf_decode_mode=align", hard], "not with crf_decode_mode=align"),
                    (on + ["crf_decode_mode=posteriors", "crf_output_posteriorfile=" + str(d / "never.post")], "not with crf_decode_mode=posteriors"),
                    (on + ["crf_lat_outdir=" + str(d)], "not with crf_lat_outdir"),
                    (on + ["crf_output_mlffile=" + str(d / "never.mlf")], "not with crf_output_mlffile"),
                    (on + ["crf_lat_beam=5", "crf_lat_outdir=" + str(d)], "not with crf_lat_")]:
        r = _decode(flags + fl + ["crf_output_labelfile=" + str(d / "never.lab")])
        assert r.returncode != 0 and msg in r.stderr, (fl, r.returncode, r.stderr)
    assert not os.path.exists(str(d / "never.nbest"))
