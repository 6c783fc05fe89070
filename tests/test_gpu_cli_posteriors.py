"""-m gpu: the posterior output through the front-end and the host class: CRFFstDecode crf_decode_mode=posteriors and
crf_output_conffile on the bundled fixtures with a weight file trained by CRFTrain, against the Python binding on the same
inputs; CRF_NewLocalPosteriorBuilder::buildFtrSeq (tests/host/posterior_conformance.cpp, linked and run) against the
numpy reference."""
import os
import subprocess

import numpy as np
import pytest

import scrf_amd

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
BIN = os.path.join(ROOT, "asr-craft_amd", "bin")
L = 48


def _fixture():
    f1 = np.loadtxt(os.path.join(G, "crftrain_test.ascii"))
    f2 = np.loadtxt(os.path.join(G, "crftrain_test.ftr2.ascii"))
    return [np.concatenate([f1[f1[:, 0] == u, 2:], f2[f1[:, 0] == u, 2:]], axis=1).astype(np.float32) for u in range(3)]


def _common_flags():
    return ["ftr1_file=" + os.path.join(G, "crftrain_test.ascii"), "ftr1_format=ascii",
            "ftr2_file=" + os.path.join(G, "crftrain_test.ftr2.ascii"), "ftr2_format=ascii",
            "crf_label_size=48", "crf_model_type=stdframe", "label_maximum_duration=1", "crf_featuremap=stdstate"]


def _decode(extra):
    return subprocess.run([os.path.join(BIN, "CRFFstDecode")] + _common_flags() + extra, capture_output=True, text=True, timeout=300)


@pytest.fixture(scope="module")
def trained(tmp_path_factory):
    d = tmp_path_factory.mktemp("post_cli")
    out = str(d / "weights.out")
    r = subprocess.run([os.path.join(BIN, "CRFTrain")] + _common_flags() + [
        "hardtarget_file=" + os.path.join(G, "crftrain_test.lab.ascii"), "out_weight_file=" + out, "crf_epochs=3", "crf_lr=0.5",
        "crf_bunch_size=1", "threads=1", "crf_utt_rpt=1", "crf_train_order=seq"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    # the binding on the same inputs: the weights as the front-end reads them back, the precision it defaults to
    utts = _fixture()
    eng = scrf_amd.Engine(scrf_amd.make_config(model_type=scrf_amd.STDFRAME, L=L, D=1, F=6, precision=scrf_amd.PREC_FAST))
    eng.set_lambda(np.loadtxt(out))
    b = eng.batch_from_windows(utts, [x.shape[0] for x in utts])
    labs, _ = eng.viterbi_batch(b)
    post = eng.posteriors_batch(b, segments=labs)
    labs = [np.array(l) for l in labs]
    b.close(); eng.close()
    assert np.abs(np.loadtxt(out)).max() > 0 and max(p.max() for p in post["frame"]) > 2.5 / L   # not the uniform posterior
    return d, out, post, labs


def _rows(path):
    a = np.loadtxt(path, ndmin=2)
    return a[:, 0].astype(int), a[:, 1].astype(int), a[:, 2:]


@pytest.mark.parametrize("bunch", [1, 2, 256])
def test_posteriors_mode_writes_the_bindings_frame_posteriors(trained, bunch):
    d, w, post, _ = trained
    p = str(d / ("post_%d.txt" % bunch))
    r = _decode(["weight_file=" + w, "crf_decode_mode=posteriors", "crf_output_posteriorfile=" + p, "crf_bunch_size=%d" % bunch])
    assert r.returncode == 0, r.stdout + r.stderr
    sent, frame, v = _rows(p)
    want = np.concatenate(post["frame"])
    assert v.shape == want.shape
    assert list(sent) == [u for u, x in enumerate(post["frame"]) for _ in range(len(x))]
    assert list(frame) == [t for x in post["frame"] for t in range(len(x))]
    dev = np.abs(v - want).max()
    print("CLI ascii posteriors against the binding: %.3e" % dev)
    assert dev <= 1e-12
    assert np.abs(v.sum(1) - 1).max() <= 1e-9


def test_posteriors_mode_log_and_unnormalised_forms(trained):
    d, w, post, _ = trained
    want = np.concatenate(post["frame"])
    zx = np.concatenate([np.full(len(x), z) for x, z in zip(post["frame"], post["zx"])])[:, None]
    for tag, flags, ref in (("log", ["crf_posterior_log=1"], np.log(want)),
                            ("lognn", ["crf_posterior_log=1", "crf_posterior_norm=0"], np.log(want) + zx)):
        p = str(d / ("post_%s.txt" % tag))
        r = _decode(["weight_file=" + w, "crf_decode_mode=posteriors", "crf_output_posteriorfile=" + p] + flags)
        assert r.returncode == 0, r.stdout + r.stderr
        np.testing.assert_allclose(_rows(p)[2], ref, rtol=1e-12, atol=1e-12)


def test_posteriors_mode_pfile_round_trips_to_the_float32_of_the_same_values(trained):
    d, w, post, _ = trained
    pa, pf, back = str(d / "post_a.txt"), str(d / "post.pfile"), str(d / "post_back.txt")
    assert _decode(["weight_file=" + w, "crf_decode_mode=posteriors", "crf_output_posteriorfile=" + pa]).returncode == 0
    r = _decode(["weight_file=" + w, "crf_decode_mode=posteriors", "crf_output_posteriorfile=" + pf, "crf_output_posterior_format=pfile"])
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([os.path.join(BIN, "qn_filetool"), "pfile2ascii", pf, back], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    sa, fa, va = _rows(pa)
    sb, fb, vb = _rows(back)
    assert list(sa) == list(sb) and list(fa) == list(fb) and vb.shape == (len(sa), L)
    assert np.array_equal(vb.astype(np.float32), va.astype(np.float32))
    assert np.abs(vb - np.concatenate(post["frame"])).max() <= 1e-7


def test_conffile_leaves_the_label_file_alone_and_matches_the_binding(trained):
    d, w, post, labs = trained
    l0, l1, cf = str(d / "lab0.txt"), str(d / "lab1.txt"), str(d / "conf.txt")
    r = _decode(["weight_file=" + w, "crf_output_labelfile=" + l0])
    assert r.returncode == 0, r.stdout + r.stderr
    r = _decode(["weight_file=" + w, "crf_output_labelfile=" + l1, "crf_output_conffile=" + cf, "crf_bunch_size=2"])
    assert r.returncode == 0, r.stdout + r.stderr
    assert open(l0, "rb").read() == open(l1, "rb").read() and os.path.getsize(l0) > 0
    c = np.loadtxt(cf, ndmin=2)
    want = [(u, k, k, k, int(v) % L, post["segments"][u][k]) for u in range(len(labs)) for k, v in enumerate(labs[u])]   # D = 1: segment k is frame k
    assert c.shape == (len(want), 6)
    assert np.array_equal(c[:, :5].astype(int), np.array([x[:5] for x in want]))
    dev = np.abs(c[:, 5] - np.array([x[5] for x in want])).max()
    print("CLI segment confidences against the binding: %.3e" % dev)
    assert dev <= 1e-12
    assert (c[:, 5] > 0).all() and (c[:, 5] <= 1 + 1e-9).all()


@pytest.mark.parametrize("extra,msg", [
    (["crf_lm_txt=lm.txt"], "crf_lm_txt makes no sense"),
    (["crf_dict_txt=dict.txt"], "crf_dict_txt makes no sense"),
    (["crf_lat_outdir=."], "crf_lat_outdir makes no sense"),
    (["crf_align_mlffile=a.mlf"], "crf_align_mlffile makes no sense"),
    (["crf_output_posterior_format=htk"], "(ascii|pfile)"),
    (["crf_posterior_norm=0"], "crf_posterior_norm=0 needs crf_posterior_log=1"),
])
def test_posteriors_mode_refuses_what_makes_no_sense(trained, extra, msg):
    d, w, _, _ = trained
    r = _decode(["weight_file=" + w, "crf_decode_mode=posteriors", "crf_output_posteriorfile=" + str(d / "never.txt")] + extra)
    assert r.returncode != 0 and msg in r.stdout + r.stderr
    assert not os.path.exists(str(d / "never.txt"))


def test_other_refused_flag_combinations(trained):
    d, w, _, _ = trained
    r = _decode(["weight_file=" + w, "crf_decode_mode=posteriors"])
    assert r.returncode != 0 and "crf_output_posteriorfile required" in r.stdout + r.stderr
    r = _decode(["weight_file=" + w, "crf_output_posteriorfile=" + str(d / "never.txt")])
    assert r.returncode != 0 and "needs crf_decode_mode=posteriors" in r.stdout + r.stderr
    for extra in (["crf_lat_outdir=" + str(d)], ["crf_decode_mode=align", "hardtarget_file=" + os.path.join(G, "crftrain_test.lab.ascii")],
                  ["crf_decode_mode=posteriors", "crf_output_posteriorfile=" + str(d / "never.txt")]):
        r = _decode(["weight_file=" + w, "crf_output_conffile=" + str(d / "never_conf.txt")] + extra)
        assert r.returncode != 0 and "crf_output_conffile goes with the best paths" in r.stdout + r.stderr
    assert not os.path.exists(str(d / "never_conf.txt")) and not os.path.exists(str(d / "never.txt"))


@pytest.mark.parametrize("norm", [1, 0])
def test_local_posterior_builder_on_a_segmental_model(tmp_path, norm):
    """CRF_NewLocalPosteriorBuilder::buildFtrSeq, linked against libcrf_amd_host + libscrf_amd: getAlphaBeta() of every node
    is the log frame posterior (+ Zx when norm is false) of the numpy reference"""
    import orc
    import post_ref
    from cases import Case
    lib = os.path.join(ROOT, "asr-craft_amd", "lib")
    exe = str(tmp_path / "postmain")
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-DPOSTERIOR_CONFORMANCE_MAIN", "-I" + os.path.join(ROOT, "include"),
                        "-I" + os.path.join(ROOT, "asr-craft_amd", "host"), os.path.join(ROOT, "tests", "host", "posterior_conformance.cpp"),
                        "-o", exe, "-L" + lib, "-Wl,-rpath," + lib, "-lcrf_amd_host", "-lscrf_amd"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    c = Case(L=5, D=3, in_w=4, Ts=[7, 2, 11], seed=12)
    c.lam = np.array([float("%.17g" % v) for v in c.lam])
    wf, ff = str(tmp_path / "w.txt"), str(tmp_path / "frames.txt")
    np.savetxt(wf, c.lam, fmt="%.17g")
    with open(ff, "w") as f:
        for x in c.frames:
            f.write("%d\n" % x.shape[0])
            for row in x:
                f.write(" ".join("%.9g" % v for v in row) + "\n")
    r = subprocess.run([exe, wf, ff, str(c.L), str(c.D), str(c.in_w), str(norm)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    got = {u: [] for u in range(len(c.Ts))}
    zx = {}
    for ln in r.stdout.splitlines():
        w = ln.split()
        if w[0] == "zx":
            zx[int(w[1])] = float(w[2])
        else:
            got[int(w[0])].append([float(x) for x in w[2:]])
    for u, T in enumerate(c.Ts):
        g, occ, end, z = post_ref.utterance(c, u)
        assert abs(zx[u] - z) <= 1e-11 * max(1, abs(z))
        v = np.array(got[u])
        assert v.shape == (T, c.L)
        np.testing.assert_allclose(np.exp(v - (0 if norm else zx[u])), occ, rtol=0, atol=1e-9)
