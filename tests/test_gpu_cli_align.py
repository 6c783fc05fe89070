"""-m gpu: CRFFstDecode crf_decode_mode=align crf_align_unit=phone: the batched device alignment through the
front-end and crf_amd_alignments.  On the bundled frame-model fixture it writes the label file of today's align mode byte
for byte; on a tiny segmental model trained by CRFTrain the aligned phones follow the transcript, crf_output_conffile holds
one posterior per aligned segment, crf_align_repeat=0 gives one segment per listed phone, and a transcript that does not
fit gets the warning and an empty entry.  (A hardtarget file holds one label per frame and runs longer than the maximum
duration are split, so a transcript can neither be longer than its utterance nor too short for it in ONE mode; an utterance
without any labelled frame is the transcript that does not fit here.)"""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
BIN = os.path.join(ROOT, "asr-craft_amd", "bin")
L, D, W = 3, 3, 2
NONE = 4294967295   # CRF_LAB_BAD: a frame without a label
# frame labels to align to, per utterance: runs of 1 .. 3 frames; one run of 5 (split in two pieces: the same phone twice in
# ONE mode); phone-duration labels (4 = phone 1, duration 2) among them; nothing labelled
HARD = [[0, 1, 1], [2, 2, 2, 2, 2], [1, 0, 0, 2, 2, 2, 4, 4], [NONE] * 6]
TS = [len(h) for h in HARD]


def _decode(flags):
    return subprocess.run([os.path.join(BIN, "CRFFstDecode")] + flags, capture_output=True, text=True, timeout=300)


def _collapse(x):
    return [v for i, v in enumerate(x) if i == 0 or v != x[i - 1]]


def _pieces(frame_labels):
    """phones of the segments the label stream forms: runs of equal labels, a run longer than D in ceil(n / D) pieces"""
    out = []
    for v in _collapse_runs(frame_labels):
        lab, n = v
        if lab != NONE:
            out += [lab % L] * (-(-n // D))
    return out


def _collapse_runs(x):
    runs = []
    for v in x:
        if runs and runs[-1][0] == v:
            runs[-1][1] += 1
        else:
            runs.append([v, 1])
    return runs


@pytest.fixture(scope="module")
def tiny(tmp_path_factory):
    """data and a weight file written the way tests/test_gpu_cli_latprune.py writes them (copied: test modules are not imported)"""
    d = tmp_path_factory.mktemp("align_cli")
    rng = np.random.RandomState(34)
    f = str(d / "f.ascii"); lbl = str(d / "l.ascii"); hard = str(d / "hard.ascii")
    with open(f, "w") as ff, open(lbl, "w") as lf, open(hard, "w") as hf:
        for u, T in enumerate(TS):
            X = rng.random_sample((T, W)).astype(np.float32)
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
    return d, model + ["weight_file=" + wf, "crf_decode_mode=align", "hardtarget_file=" + hard]


def _labels(path, n_utts):
    rows = np.loadtxt(path, ndmin=2).astype(int).reshape(-1, 3)
    out = [[] for _ in range(n_utts)]
    for u, i, lab in rows:
        assert i == len(out[u])
        out[u].append(int(lab))
    return out


def test_aligned_phones_follow_the_transcript_and_the_conffile_holds_their_posteriors(tiny):
    for bunch in (256, 3):
        _check_runs_mode(tiny, bunch)


def _check_runs_mode(tiny, bunch):
    d, flags = tiny
    lab, conf = str(d / ("runs_%d.lab" % bunch)), str(d / ("runs_%d.conf" % bunch))
    r = _decode(flags + ["crf_align_unit=phone", "crf_output_labelfile=" + lab, "crf_output_conffile=" + conf, "crf_bunch_size=%d" % bunch])
    assert r.returncode == 0, r.stdout + r.stderr
    got = _labels(lab, len(TS))
    n_seg = 0
    for u in range(3):
        assert all(0 <= v < L * D for v in got[u])
        assert sum(v // L + 1 for v in got[u]) == TS[u]                       # the segments tile the utterance
        assert _collapse([v % L for v in got[u]]) == _collapse(_pieces(HARD[u])), u   # collapsed phones = the transcript
        n_seg += len(got[u])
    assert got[3] == []
    assert r.stderr.count("WARNING: the labels of sentence 3 do not fit its lattice") == 1 and r.stderr.count("WARNING") == 1
    c = np.loadtxt(conf, ndmin=2)
    assert c.shape == (n_seg, 6)                                               # one row per aligned segment
    want = [(u, k, sum(x // L + 1 for x in got[u][:k]), sum(x // L + 1 for x in got[u][:k + 1]) - 1, v % L)
            for u in range(3) for k, v in enumerate(got[u])]
    assert np.array_equal(c[:, :5].astype(int), np.array(want))
    assert ((c[:, 5] >= 0.0) & (c[:, 5] <= 1.0)).all(), c[:, 5]
    if bunch != 256:   # the batch size does not show in the files
        assert open(lab, "rb").read() == open(str(d / "runs_256.lab"), "rb").read()
        assert open(conf, "rb").read() == open(str(d / "runs_256.conf"), "rb").read()


def test_without_repeats_every_listed_phone_takes_exactly_one_segment(tiny):
    d, flags = tiny
    lab = str(d / "one.lab")
    r = _decode(flags + ["crf_align_unit=phone", "crf_align_repeat=0", "crf_output_labelfile=" + lab])
    assert r.returncode == 0, r.stdout + r.stderr
    got = _labels(lab, len(TS))
    for u in range(3):
        assert [v % L for v in got[u]] == _pieces(HARD[u]), u    # exactly K segments, segment k carrying phone k
        assert sum(v // L + 1 for v in got[u]) == TS[u]
    assert _pieces(HARD[1]) == [2, 2] and len(got[1]) == 2       # the same phone twice stays two segments
    assert got[3] == [] and "WARNING: the labels of sentence 3 do not fit its lattice" in r.stderr


def test_the_default_unit_is_the_host_path_and_flags_are_refused_where_they_make_no_sense(tiny):
    d, flags = tiny
    l0, l1 = str(d / "host0.lab"), str(d / "host1.lab")
    r0 = _decode(flags + ["crf_output_labelfile=" + l0])
    r1 = _decode(flags + ["crf_align_unit=label", "crf_output_labelfile=" + l1])
    assert r0.returncode == 0 and r1.returncode == 0, r0.stderr + r1.stderr
    assert open(l0, "rb").read() == open(l1, "rb").read() and os.path.getsize(l0) > 0
    no_align = [x for x in flags if not x.startswith(("crf_decode_mode=", "hardtarget_file="))]
    for fl, msg in [(no_align + ["crf_align_unit=phone"], "crf_align_unit=phone needs crf_decode_mode=align"),
                    (no_align + ["crf_align_unit=phone", "crf_decode_mode=posteriors", "crf_output_posteriorfile=" + str(d / "p.txt")],
                     "crf_align_unit=phone needs crf_decode_mode=align"),
                    (flags + ["crf_align_unit=phone", "crf_lat_outdir=" + str(d)], "builds no lattice"),
                    (flags + ["crf_align_unit=phone", "crf_lat_beam=2", "crf_lat_outdir=" + str(d)], "crf_lat_beam makes no sense with crf_decode_mode=align"),
                    (flags + ["crf_align_unit=word"], "(label|phone)"),
                    (flags + ["crf_align_repeat=0"], "crf_align_repeat needs"),
                    (flags + ["crf_align_unit=phone", "crf_align_repeat=2"], "(1|0)"),
                    (flags + ["crf_output_conffile=" + str(d / "never.conf")], "crf_output_conffile goes with the best paths")]:
        r = _decode(fl + ["crf_output_labelfile=" + str(d / "never.lab")])
        assert r.returncode != 0 and msg in r.stderr, (fl, r.returncode, r.stderr)
    assert not os.path.exists(str(d / "never.conf"))


def test_a_model_the_engine_refuses_surfaces_its_message(tiny):
    d, flags = tiny
    fl = [x for x in flags if not x.startswith(("crf_model_type=", "weight_file=", "crf_label_size="))]
    fl += ["crf_model_type=stdseg", "crf_label_size=%d" % (L * D), "num_actual_labs=%d" % L]
    wf = str(d / "w_stdseg.out")
    open(wf, "w").write("0.25\n-0.5\n" * 40)   # any weights do: the refusal does not depend on them
    r = _decode(fl + ["weight_file=" + wf, "crf_align_unit=phone", "crf_output_labelfile=" + str(d / "stdseg.lab")])
    assert r.returncode != 0 and "forced alignment is not built for the \"stdseg\"" in r.stderr, r.stdout + r.stderr


def test_frame_model_fixture_writes_the_default_align_modes_label_file(tmp_path):
    """the bundled frame-model fixture with the reversed-runs label file of test_crffstdecode_align_mode_on_bundled_fixture"""
    common = ["ftr1_file=" + os.path.join(G, "crftrain_test.ascii"), "ftr1_format=ascii",
              "ftr2_file=" + os.path.join(G, "crftrain_test.ftr2.ascii"), "ftr2_format=ascii",
              "crf_label_size=48", "crf_model_type=stdframe", "label_maximum_duration=1", "crf_featuremap=stdstate"]
    out = str(tmp_path / "w.out")
    r = subprocess.run([os.path.join(BIN, "CRFTrain")] + common + ["hardtarget_file=" + os.path.join(G, "crftrain_test.lab.ascii"), "out_weight_file=" + out,
                        "crf_epochs=3", "crf_lr=0.3", "crf_bunch_size=2", "threads=1", "crf_utt_rpt=1", "crf_train_order=seq"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lb = np.loadtxt(os.path.join(G, "crftrain_test.lab.ascii")).astype(int)
    alt = str(tmp_path / "alt.lab")
    with open(alt, "w") as f:
        for u in range(3):
            lab = lb[lb[:, 0] == u][:, 2]
            T = len(lab)
            seq = _collapse([int(v) for v in lab])
            seq = seq[::-1] if len(seq) > 1 else seq
            frames = []
            for i, s_ in enumerate(seq):
                frames += [s_] * (T // len(seq) + (1 if i < T % len(seq) else 0))
            for t in range(T):
                f.write("%d %d %d\n" % (u, t, frames[t]))
    host, dev = str(tmp_path / "host.txt"), str(tmp_path / "dev.txt")
    base = common + ["weight_file=" + out, "crf_decode_mode=align", "hardtarget_file=" + alt]
    r0 = _decode(base + ["crf_output_labelfile=" + host])
    assert r0.returncode == 0, r0.stdout + r0.stderr
    for bunch in (256, 2):
        r1 = _decode(base + ["crf_align_unit=phone", "crf_output_labelfile=" + dev, "crf_bunch_size=%d" % bunch])
        assert r1.returncode == 0, r1.stdout + r1.stderr
        assert open(host, "rb").read() == open(dev, "rb").read() and os.path.getsize(host) > 0, bunch
