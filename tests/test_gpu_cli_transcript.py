"""-m gpu: transcript scoring through the front-end and crf_amd_transcript_scores, on the tiny segmental
model of tests/test_gpu_cli_align.py: CRFFstDecode crf_decode_mode=align crf_align_unit=phone with crf_output_scorefile and
crf_conf_given, against the Python binding on the same frames, weights and transcripts."""
import os
import subprocess

import numpy as np
import pytest

import scrf_amd

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "asr-craft_amd", "bin")
L, D, W = 3, 3, 2
NONE = 4294967295   # CRF_LAB_BAD: a frame without a label
# the frame labels of tests/test_gpu_cli_align.py: runs of 1 .. 3 frames; one run of 5 (two pieces); phone-duration labels
# among them; nothing labelled (the transcript that does not fit)
HARD = [[0, 1, 1], [2, 2, 2, 2, 2], [1, 0, 0, 2, 2, 2, 4, 4], [NONE] * 6]
TS = [len(h) for h in HARD]


def _decode(flags):
    return subprocess.run([os.path.join(BIN, "CRFFstDecode")] + flags, capture_output=True, text=True, timeout=300)


def _pieces(frame_labels):
    """phones of the segments the label stream forms: runs of equal labels, a run longer than D in ceil(n / D) pieces"""
    runs = []
    for v in frame_labels:
        if runs and runs[-1][0] == v:
            runs[-1][1] += 1
        else:
            runs.append([v, 1])
    out = []
    for lab, n in runs:
        if lab != NONE:
            out += [lab % L] * (-(-n // D))
    return out


def _collapse(x):
    return [v for i, v in enumerate(x) if i == 0 or v != x[i - 1]]


def _transcripts(repeat):
    ph = [_pieces(h) for h in HARD]
    return [np.array(_collapse(p) if repeat else p, dtype=np.uint32) for p in ph]


@pytest.fixture(scope="module")
def tiny(tmp_path_factory):
    """data and a weight file written the way tests/test_gpu_cli_align.py writes them (copied: test modules are not imported),
    and the binding on the same inputs: the weights as the front-end reads them back, the precision it defaults to"""
    d = tmp_path_factory.mktemp("transcript_cli")
    rng = np.random.RandomState(34)
    f = str(d / "f.ascii"); lbl = str(d / "l.ascii"); hard = str(d / "hard.ascii")
    frames = []
    with open(f, "w") as ff, open(lbl, "w") as lf, open(hard, "w") as hf:
        for u, T in enumerate(TS):
            X = rng.random_sample((T, W)).astype(np.float32)
            frames.append(X)
            lab = np.repeat(rng.randint(0, L, T), 2)[:T]
            for t in range(T):
                ff.write("%d %d %s\n" % (u, t, " ".join("%.9g" % v for v in X[t])))
                lf.write("%d %d %d\n" % (u, t, lab[t]))
                hf.write("%d %d %d\n" % (u, t, HARD[u][t]))
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
    ref = {}
    for repeat, mode in ((1, scrf_amd.ALIGN_RUNS), (0, scrf_amd.ALIGN_ONE)):
        ts = _transcripts(repeat)
        segs, _ = eng.align_batch(b, ts, mode)
        out = eng.transcript_batch(b, ts, mode, frame=False, end=False, segments=segs)
        free = eng.posteriors_batch(b, frame=False, end=False, segments=segs)
        ref[repeat] = dict(ts=ts, labs=[[int(x) for x in s] for s in segs], log_num=out["log_num"].copy(), zx=out["zx"].copy(),
                           given=[np.array(x) for x in out["segments"]], free=[np.array(x) for x in free["segments"]])
    b.close(); eng.close()
    return d, model + ["weight_file=" + wf, "crf_decode_mode=align", "hardtarget_file=" + hard, "crf_align_unit=phone"], ref


def _close(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    same_inf = np.isinf(a) & np.isinf(b) & (np.sign(a) == np.sign(b))
    with np.errstate(invalid="ignore"):
        return bool((same_inf | (np.abs(a - b) <= 1e-12 * np.maximum(1.0, np.abs(b)))).all())


@pytest.mark.parametrize("repeat", [1, 0])
def test_the_scorefile_holds_the_bindings_sums(tiny, repeat):
    d, flags, ref = tiny
    r_ = ref[repeat]
    for bunch in (256, 3):
        sc, lab = str(d / ("s_%d_%d.txt" % (repeat, bunch))), str(d / ("s_%d_%d.lab" % (repeat, bunch)))
        r = _decode(flags + ["crf_align_repeat=%d" % repeat, "crf_output_scorefile=" + sc, "crf_output_labelfile=" + lab, "crf_bunch_size=%d" % bunch])
        assert r.returncode == 0, r.stdout + r.stderr
        rows = np.loadtxt(sc, ndmin=2)
        assert rows.shape == (len(TS), 5)
        assert list(rows[:, 0].astype(int)) == list(range(len(TS)))
        assert list(rows[:, 1].astype(int)) == [len(t) for t in r_["ts"]]
        print("scorefile against the binding (repeat %d, bunch %d): log_num %s\n  binding %s" % (repeat, bunch, rows[:, 2], r_["log_num"]))
        assert _close(rows[:, 2], r_["log_num"]) and _close(rows[:, 3], r_["zx"]) and _close(rows[:, 4], r_["log_num"] - r_["zx"])
        assert np.isfinite(rows[:3, 2]).all() and (rows[:3, 4] < 0).all()
        # nothing labelled: the transcript that does not fit gets the align mode's warning and -inf
        assert rows[3, 2] == -np.inf and rows[3, 4] == -np.inf and np.isfinite(rows[3, 3])
        assert r.stderr.count("WARNING: the labels of sentence 3 do not fit its lattice") == 1
        # the label file is the one the alignment alone writes
        l0 = str(d / ("plain_%d.lab" % repeat))
        r0 = _decode(flags + ["crf_align_repeat=%d" % repeat, "crf_output_labelfile=" + l0])
        assert r0.returncode == 0 and open(l0, "rb").read() == open(lab, "rb").read() and os.path.getsize(l0) > 0


def test_conf_given_selects_the_conffiles_last_column(tiny):
    d, flags, ref = tiny
    r_ = ref[1]
    c0, c1, c2, c3 = (str(d / ("c%d.conf" % i)) for i in range(4))
    lab = str(d / "c.lab")
    runs = [(c0, []), (c1, ["crf_conf_given=none"]), (c2, ["crf_conf_given=transcript"]),
            (c3, ["crf_conf_given=none", "crf_output_scorefile=" + str(d / "c3.score")])]
    for path, extra in runs:
        r = _decode(flags + ["crf_output_labelfile=" + lab, "crf_output_conffile=" + path] + extra)
        assert r.returncode == 0, r.stdout + r.stderr
    # none = today's bytes, with and without the score file beside it
    assert open(c0, "rb").read() == open(c1, "rb").read() == open(c3, "rb").read() and os.path.getsize(c0) > 0
    free, given = np.loadtxt(c0, ndmin=2), np.loadtxt(c2, ndmin=2)
    n_seg = sum(len(l) for l in r_["labs"])
    assert free.shape == given.shape == (n_seg, 6) and np.array_equal(free[:, :5], given[:, :5])
    want_given, want_free = np.concatenate(r_["given"]), np.concatenate(r_["free"])
    print("conffile against the binding: given %.3e, free %.3e" % (np.abs(given[:, 5] - want_given).max(), np.abs(free[:, 5] - want_free).max()))
    assert np.abs(given[:, 5] - want_given).max() <= 1e-12 and np.abs(free[:, 5] - want_free).max() <= 1e-12
    assert ((given[:, 5] > 0.0) & (given[:, 5] <= 1.0 + 1e-12)).all()
    assert np.abs(given[:, 5] - free[:, 5]).max() > 1e-6   # the two columns are different quantities


def test_the_flags_are_refused_outside_phone_alignment(tiny):
    d, flags, _ = tiny
    label_unit = [x for x in flags if x != "crf_align_unit=phone"]
    no_align = [x for x in label_unit if not x.startswith(("crf_decode_mode=", "hardtarget_file="))]
    sc = "crf_output_scorefile=" + str(d / "never.score")
    for fl, msg in [(label_unit + [sc], "crf_output_scorefile needs crf_decode_mode=align crf_align_unit=phone"),
                    (no_align + [sc], "crf_output_scorefile needs crf_decode_mode=align crf_align_unit=phone"),
                    (label_unit + ["crf_conf_given=transcript"], "crf_conf_given needs crf_decode_mode=align crf_align_unit=phone"),
                    (no_align + ["crf_conf_given=none"], "crf_conf_given needs crf_decode_mode=align crf_align_unit=phone"),
                    (flags + ["crf_conf_given=words", "crf_output_conffile=" + str(d / "never.conf")], "(transcript|none)"),
                    (flags + ["crf_conf_given=transcript"], "crf_conf_given=transcript needs crf_output_conffile")]:
        r = _decode(fl + ["crf_output_labelfile=" + str(d / "never.lab")])
        assert r.returncode != 0 and msg in r.stderr, (fl, r.returncode, r.stderr)
    assert not os.path.exists(str(d / "never.score")) and not os.path.exists(str(d / "never.conf"))
