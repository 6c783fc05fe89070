"""-m gpu: every kernel path on signed, per-utterance rescaled, offset and tied input features (cases.family_frames)
instead of U[0, 1): the running extrema of the window kernels on negative values, sign changes and exact ties; the
per-utterance max|x| of the fast-decode screen (its max|x| > 1 branch, the per-utterance fill, the chunk-relative
index); FASTLIN's prefix sums on signed and offset data; every absolute constant under another data scale; and the tie
rule of every decode kernel (the `tied` family has a twin label: every best path through it has a twin of equal cost).

Decode surfaces are compared bit for bit with the oracle, the training side at the project's per-tier bounds of
tests/test_gpu_parity.py.  tests/test_input_families.py establishes on the CPU what these tests lean on (score spreads of
a few nats, ties present, FASTLIN's headroom, screen counts above zero); shapes and seeds live in tests/family_shapes.py.
Every test prints the largest deviation it saw before it asserts."""
import os
import subprocess
import sys

import numpy as np
import pytest

import family_shapes as fs
import latprune_ref as lr
import post_ref
from family_shapes import FAMILY_NAMES, FUSED3, POST_SHAPES, SHAPE_NAMES, SHAPES
from gpu_checks import (EXACT, FAST, FAST32, FASTLIN, NAME, POST_TOL, bits, check_decode_surfaces, check_posteriors,
                        check_training, same_paths)

pytestmark = pytest.mark.gpu

FAST32_FAMILIES = ("signed", "ranged", "tied")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("family", FAMILY_NAMES)
@pytest.mark.parametrize("shape", SHAPE_NAMES)
def test_family_on_every_path(shape, family, monkeypatch):
    """One (shape, family) pair: the decode surfaces bit for bit, then gradient, Zx and numerator under every tier.  The
    mixed shape runs with SCRF_FUSE_MIXED=1 and 0 (fused state part / the general path for everything)."""
    c0, utts, ref = fs.reference(shape, family)
    want_fast = SHAPES[shape][1]
    for mixed in (("1", "0") if shape == "mixed" else (None,)):
        if mixed is not None:
            monkeypatch.setenv("SCRF_FUSE_MIXED", mixed)
        what = "%s %s%s" % (shape, family, "" if mixed is None else " SCRF_FUSE_MIXED=" + mixed)
        c = fs.case(shape, family)
        eng = c.engine(); b = c.batch(eng, with_labels=False)
        check_decode_surfaces(c, utts, eng, b)
        b.close(); eng.close()
        for prec in (EXACT, FAST, FASTLIN, FAST32):
            if prec == FAST32 and family not in FAST32_FAMILIES:
                continue
            mode = check_training(fs.case(shape, family, precision=prec), ref, prec, what)
            if mixed == "0":
                assert mode == 0
            elif prec == FAST and want_fast is not None:
                assert mode == want_fast
            elif prec == FASTLIN and shape in fs.FASTLIN_FORM2:
                assert mode == 2


# ---------------------------------------------------------------------------------------------------------------------
def screen_bracket(c):
    """The screen's count under SCRF_DECODE_BOUND_SCALE=30, predicted from the oracle's scores.  The kernel's score differs
    from the oracle's by at most the bound at factor 1 (that is what the bound says), so an entry the prediction lists at
    factor 29 the kernel lists at 30, and an entry the kernel lists at 30 the prediction lists at 31 (28.9 / 31.1: the
    rounding of the bound itself)."""
    return fs.predicted_screen_count(c, 28.9), fs.predicted_screen_count(c, 31.1)


@pytest.mark.parametrize("family", FAST32_FAMILIES)
@pytest.mark.parametrize("shape", FUSED3)
def test_fast_decode_is_bit_identical_to_exact_decode(shape, family, monkeypatch):
    """tests/test_gpu_parity.py's test of the same name on the families: labels and float costs of the fast decode equal the
    EXACT decode's (and the oracle's shortest path) bit for bit -- plain, with the screen widened
    (SCRF_DECODE_BOUND_SCALE=30) and with the batch cut into chunks, whose utterances under `ranged` have different max|x|.
    No chunk falls back to the EXACT path, and the number of recomputed weights lies in the bracket predicted from the
    oracle's scores with each utterance's own max|x|: a screen that ignored max|x| (all data of the older tests lies in
    [0, 1)) or read another utterance's (a chunk-relative index without the chunk's first frame) falls below it."""
    c0, utts, _ = fs.reference(shape, family)
    res = {}
    for tag, env, scratch in [("exact", {"SCRF_FAST_DECODE": "0"}, 0), ("fast", {}, 0), ("fix", {"SCRF_DECODE_BOUND_SCALE": "30"}, 0),
                              ("chunks", {"SCRF_DECODE_BOUND_SCALE": "30"}, 1 << 16)]:
        for k in ("SCRF_FAST_DECODE", "SCRF_DECODE_BOUND_SCALE"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        c = fs.case(shape, family, scratch_bytes=scratch)
        eng = c.engine(); b = c.batch(eng, with_labels=False)
        assert eng.batch_is_fused(b)
        labs, cost = eng.viterbi_batch(b)
        res[tag] = (labs, cost, eng.decode_stats())
        b.close(); eng.close()
    lo, hi = screen_bracket(c0)
    print("%s %s: recomputed plain %d, widened %d, in chunks %d (predicted %d .. %d); max|x| per utterance %s" % (
        shape, family, res["fast"][2][0], res["fix"][2][0], res["chunks"][2][0], lo, hi, " ".join("%.3g" % np.abs(f).max() for f in c0.frames)))
    el, ec, est = res["exact"]
    assert est == (0, 0)
    assert same_paths(el, ec, [u[6] for u in utts], [u[7] for u in utts])
    for tag in ("fast", "fix", "chunks"):
        gl, gc, st = res[tag]
        assert same_paths(gl, gc, el, ec), tag
        assert st[1] == 0, tag
    assert res["fast"][2][0] <= res["fix"][2][0]
    assert lo <= res["fix"][2][0] <= hi
    assert lo <= res["chunks"][2][0] <= hi


# ---------------------------------------------------------------------------------------------------------------------
def run_everything(c, raw, k, monkeypatch):
    """every output the rescaling test compares, of one case: decode surfaces with fast decode on and off, the training
    scalars, gradient and posteriors per tier, and the widened screen's count"""
    out = {}
    for fd in ("1", "0"):
        monkeypatch.setenv("SCRF_FAST_DECODE", fd)
        eng = c.engine(); b = c.batch(eng, with_labels=False)
        labs, cost = eng.viterbi_batch(b)
        out["viterbi" + fd] = ([list(x) for x in labs], cost.copy())
        out["stats" + fd] = eng.decode_stats()
        if fd == "1":
            out["scores"] = [eng.scores(b, u, T) for u, T in enumerate(c.Ts)]
            out["arcs"] = [eng.lattice_arcs(b, u) for u in range(len(c.Ts))]
        b.close(); eng.close()
    monkeypatch.delenv("SCRF_FAST_DECODE")
    for prec in (EXACT, FAST, FASTLIN):
        cc = fs.case_like(c, precision=prec)
        eng = cc.engine(); b = cc.batch(eng)
        numer, zx = eng.fb_batch(b)
        g = eng.get_grad()
        assert eng.train_stats() == 0
        g[raw] *= 2.0 ** -k       # exact
        post = eng.posteriors_batch(b)
        out[prec] = (numer, zx, g, post["frame_flat"], post["end_flat"])
        b.close(); eng.close()
    monkeypatch.setenv("SCRF_DECODE_BOUND_SCALE", "30")
    eng = c.engine(); b = c.batch(eng, with_labels=False)
    labs, cost = eng.viterbi_batch(b)
    out["viterbi30"] = ([list(x) for x in labs], cost.copy())
    out["n_recomputed"], out["n_fallback"] = eng.decode_stats()
    b.close(); eng.close()
    monkeypatch.delenv("SCRF_DECODE_BOUND_SCALE")
    return out


@pytest.mark.parametrize("shape", FUSED3 + ("mixed",))
def test_power_of_two_rescaling_changes_nothing(shape, monkeypatch):
    """Frames times 2^k, raw-feature weights times 2^-k (biases and one-hot duration weights untouched), k = 4 and -3, on
    the signed case: every product and every float window average scales exactly, so no oracle is needed.  EXACT scores,
    lattice arcs and the best paths (fast decode on and off) keep their bits; Zx and numerator agree to 1e-13, the
    gradient (raw-feature components scaled back) to 1e-12 of its largest component and the posteriors to 1e-13 under
    EXACT, FAST and FASTLIN -- any constant that assumes data in [0, 1) breaks this.  The widened screen: with max|x|
    times 16 and the feature weights over 16 its bound can only grow, so it recomputes at least as many weights as
    before, and some (the mixed shape decodes on the EXACT path: nothing is recomputed there); each count lies in the
    bracket predicted from the oracle's scores."""
    c = fs.case(shape, "signed")
    base = run_everything(c, np.zeros(c.olay.lambda_len, dtype=bool), 0, monkeypatch)
    fused = shape in FUSED3
    n = {0: base["n_recomputed"]}
    for k in (4, -3):
        r, raw = fs.rescaled(c, k)
        got = run_everything(r, raw, k, monkeypatch)
        n[k] = got["n_recomputed"]
        for (S, M), (S0, M0) in zip(got["scores"], base["scores"]):
            assert np.array_equal(bits(S), bits(S0)) and np.array_equal(bits(M[1:]), bits(M0[1:])), k
        for (a, ns, fin), (a0, ns0, fin0) in zip(got["arcs"], base["arcs"]):
            assert (ns, fin) == (ns0, fin0) and a.tobytes() == a0.tobytes(), k
        for tag in ("viterbi1", "viterbi0", "viterbi30"):
            assert got[tag][0] == base[tag][0] and got[tag][1].tobytes() == base[tag][1].tobytes(), (tag, k)
        assert got["stats0"] == (0, 0) and got["stats1"][1] == 0 and got["n_fallback"] == 0
        for prec in (EXACT, FAST, FASTLIN):
            numer, zx, g, pf, pe = got[prec]
            n0, z0, g0, pf0, pe0 = base[prec]
            e_n = np.abs(numer - n0).max() / max(1.0, np.abs(n0).max()); e_z = np.abs(zx - z0).max() / np.abs(z0).max()
            e_g = np.abs(g - g0).max() / np.abs(g0).max()
            e_p = max(np.abs(pf - pf0).max(), np.abs(pe - pe0).max())
            print("%s k=%d %s: numerator %.2e Zx %.2e gradient %.2e posteriors %.2e" % (shape, k, NAME[prec], e_n, e_z, e_g, e_p))
            assert e_n <= 1e-13 and e_z <= 1e-13 and e_g <= 1e-12 and e_p <= 1e-13, (k, NAME[prec])
        if fused:
            lo, hi = screen_bracket(r)
            print("%s k=%d: %d weights recomputed under the widened screen (predicted %d .. %d)" % (shape, k, n[k], lo, hi))
            assert lo <= n[k] <= hi
    print("%s: n_recomputed k=0 %d, k=4 %d, k=-3 %d" % (shape, n[0], n[4], n[-3]))
    if fused:
        lo, hi = screen_bracket(c)
        assert lo <= n[0] <= hi
        assert n[4] >= n[0] > 0
    else:
        assert n[0] == n[4] == n[-3] == 0


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", FAST32_FAMILIES)
@pytest.mark.parametrize("shape", POST_SHAPES)
def test_posteriors_and_pruned_lattices(shape, family):
    """posteriors_batch against tests/post_ref.py at the tier bounds of tests/test_gpu_posteriors.py, and lattice_prune_batch
    against tests/latprune_ref.py byte for byte over its beams.  On `tied` the twin arcs' path costs are equal to the bit,
    so a beam keeps or drops both.  (An arc whose path cost EQUALS a beam's threshold best + beam was looked for on the
    CPU: path costs are sums of float weights, on a grid of about 2^-24, and none of 60 seeds per shape puts one on a
    threshold of 0.5, 2, 8 or 1e-3 above the best cost -- a chance of about 1e-9 per arc -- so that is not asserted.)"""
    c0, utts, _ = fs.reference(shape, family)
    pref = [post_ref.utterance(c0, u) for u in range(len(c0.Ts))]
    for prec in (EXACT, FAST, FASTLIN, FAST32):
        c = fs.case(shape, family, precision=prec)
        eng = c.engine(); b = c.batch(eng, with_labels=False)
        check_posteriors(c, pref, eng, b, POST_TOL[prec], "%s %s %s form %d" % (shape, family, NAME[prec], eng.batch_fused_mode(b)))
        assert eng.train_stats() == 0
        b.close(); eng.close()
    c = fs.case(shape, family)
    eng = c.engine(); b = c.batch(eng, with_labels=False)
    dist = [lr.distances(u[3], u[4], u[5]) for u in utts]
    for beam in lr.BEAMS:
        off, best = eng.lattice_prune_batch(b, beam)
        arcs = eng.pruned_arcs(b)
        assert off[0] == 0 and arcs.shape[0] == off[-1]
        for u, (X, S, M, full, ns, fin, ol, oc) in enumerate(utts):
            fwd, bwd = dist[u]
            want = full[lr.keep_mask(full, fwd, bwd, fin, beam)]
            assert off[u + 1] - off[u] == want.shape[0], (u, beam)
            assert arcs[int(off[u]):int(off[u + 1])].tobytes() == want.tobytes(), (u, beam)
            assert np.float64(best[u]).tobytes() == np.float64(fwd[fin]).tobytes(), (u, beam)
    b.close(); eng.close()


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tool,seed", [("fused_shape_sweep.py", "23"), ("general_shape_sweep.py", "29")])
def test_random_shape_sweeps_on_the_ranged_family(tool, seed):
    """12 random shapes of each sweep tool under SWEEP_FAMILY=ranged (utterance scales 1/4 .. 16 in one batch, weights
    scaled with the data), seeds the existing sweep tests do not use"""
    env = dict(os.environ, SWEEP_FAMILY="ranged")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", tool), "12", seed], capture_output=True, text=True, timeout=300, env=env)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert r.stdout.count("\nok ") + r.stdout.startswith("ok ") == 12
