"""-m gpu: what the engine's second stream carries must not show in any result.  With SCRF_SIDE=1 (default) a FASTLIN / FAST
chunk on the fused linear-domain path forks the second stream right behind the posterior walk k_post_z: the posterior-mass
check, the numerator reduction, the rescaling of the transition factors and -- on the last chunk -- the batch's status
copy run there, ahead of k_ztf and k_atb, while the main stream goes straight to the count kernel; the streams join before
the batch sums and the commit.  With SCRF_SIDE=0 everything runs in one stream, in the order the code states it.

Each case runs under both settings (the knobs are read at scrf_create): status code, failing utterance, redo count,
gradient, numerators and Zx must be EQUAL between the two, and within the tier's bound of the oracle
(tests/test_gpu_input_ranges.py: gradient, Zx, numerator = 1e-6, 1e-8, 1e-6 under FASTLIN and 1e-9, 1e-11, 1e-11 under FAST).
SCRF_EXPF_BLOCKS=3 as in tests/test_gpu_tile_staging.py.  SCRF_EXPF_BIG=0 in both runs: left unset, the count kernel's
tile height follows SCRF_SIDE (100-row tiles when the side stream is off), and another tile list sums the
counts in another order -- the two runs must differ in the streams alone."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import scrf_amd
import spread_ladder as sl
from cases import Case

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAST, FASTLIN = scrf_amd.PREC_FAST, scrf_amd.PREC_FASTLIN
TOL = {FAST: (1e-9, 1e-11, 1e-11), FASTLIN: (1e-6, 1e-8, 1e-6)}


def within_bounds(got, ref, prec, what):
    (g, numer, zx), (og, on, oz) = got, ref
    e = (np.abs(g - og).max() / np.abs(og).max(), np.abs(zx - oz).max() / np.abs(oz).max(),
         np.abs(numer - on).max() / max(1.0, np.abs(on).max()))
    t = TOL[prec]
    print("SIDE %s: gradient %.2e (%.0e)  Zx %.2e (%.0e)  numerator %.2e (%.0e)" % (what, e[0], t[0], e[1], t[1], e[2], t[2]))
    assert e[0] <= t[0] and e[1] <= t[1] and e[2] <= t[2], (what, e)


def equal(a, b, what):
    for x, y, n in zip(a, b, ("gradient", "numerators", "Zx")):
        assert np.asarray(x).tobytes() == np.asarray(y).tobytes(), (what, n, np.abs(np.asarray(x) - np.asarray(y)).max())


# DESIGN.md 4.1, shape `fused` under FASTLIN: the first rung past the last one the linear-domain kernels answer
@pytest.mark.parametrize("family,X", [("lone_max", 735), ("heavy_out", 690), ("heavy_in", 690)])
def test_a_rung_handed_to_the_log_domain_redo(family, X, monkeypatch):
    """the first pass raises NUMERIC in k_dp_lin / k_post_z / k_mass_check; its status travels on the second stream, nothing
    of it is committed, and the caller gets the log-domain pass -- twice, with the same gradient added each time"""
    monkeypatch.setenv("SCRF_EXPF_BLOCKS", "3"); monkeypatch.setenv("SCRF_EXPF_BIG", "0")
    ref = sl.reference("fused", family, X)
    out = {}
    for side in ("1", "0"):
        monkeypatch.setenv("SCRF_SIDE", side)
        c = sl.case("fused", family, X, precision=FASTLIN)
        eng = c.engine(); b = c.batch(eng)
        assert eng.batch_fused_mode(b) == 2
        numer, zx = eng.fb_batch(b)
        g = eng.get_grad()
        assert eng.train_stats() == 1, (side, eng.train_stats())
        within_bounds((g, numer, zx), ref, FASTLIN, "%s %g side=%s" % (family, X, side))
        eng.fb_batch(b, want_scalars=False)
        assert eng.train_stats() == 2
        out[side] = (g, numer.copy(), zx.copy(), eng.get_grad())
        b.close(); eng.close()
    equal(out["1"][:3], out["0"][:3], (family, X))
    assert out["1"][3].tobytes() == out["0"][3].tobytes()


@pytest.mark.parametrize("prec", [FASTLIN, FAST])
def test_one_label_out_of_range_in_a_middle_utterance(prec, monkeypatch):
    """a sound batch, then the same batch with a label >= L * D in utterance 2 of 5: code 5 and the utterance are reported,
    the gradient and the batch sums stay those of the sound batch, and a third call adds the sound batch again"""
    monkeypatch.setenv("SCRF_EXPF_BLOCKS", "3"); monkeypatch.setenv("SCRF_EXPF_BIG", "0")
    kw = dict(L=6, D=4, in_w=5, Ts=[9, 14, 11, 3, 20], seed=1501)
    ref = Case(**kw).oracle_gradient()
    out = {}
    for side in ("1", "0"):
        monkeypatch.setenv("SCRF_SIDE", side)
        c = Case(precision=prec, **kw)
        eng = c.engine(); good = c.batch(eng)
        assert eng.batch_fused_mode(good) == (2 if prec == FASTLIN else 1)
        numer, zx = eng.fb_batch(good)
        g0 = eng.get_grad(); s0 = eng.batch_sums()
        within_bounds((g0, numer, zx), ref, prec, "sound batch prec=%d side=%s" % (prec, side))
        labs = [l.copy() for l in c.labels]
        labs[2][-1] = c.L * c.D + 3
        bad = eng.batch_from_frames(c.frames, labs, c.recipes)
        with pytest.raises(scrf_amd.ScrfError) as ei:
            eng.fb_batch(bad, want_scalars=False)
        assert ei.value.code == 5 and "utterance 2" in str(ei.value), str(ei.value)
        assert np.array_equal(eng.get_grad(), g0) and np.array_equal(eng.batch_sums(), s0)
        assert eng.train_stats() == 0
        eng.fb_batch(good, want_scalars=False)
        out[side] = (g0, numer.copy(), zx.copy(), eng.get_grad(), str(ei.value))
        bad.close(); good.close(); eng.close()
    equal(out["1"][:3], out["0"][:3], prec)
    assert out["1"][3].tobytes() == out["0"][3].tobytes() and out["1"][4] == out["0"][4]


def test_three_chunks_fork_and_join_once_each(tmp_path):
    """a scratch budget below one utterance's need: every utterance is a chunk of its own (the planner never cuts below
    one), so the second stream is forked behind k_post_z and joined before the batch sums three times, and the status
    copy goes out with the third.  Through tools/tile_staging_cases.py in a child per setting."""
    kw = dict(L=48, D=25, in_w=5, Ts=[60, 101, 53], seed=1502, scratch_bytes=1 << 12)
    ref = Case(**kw).oracle_gradient()
    entries = [dict(name="chunks", prec=p, kw=kw) for p in (FAST, FASTLIN)]
    res = {}
    for side in ("1", "0"):
        out = os.path.join(str(tmp_path), "side%s.npz" % side)
        env = dict(os.environ, SCRF_EXPF_BLOCKS="3", SCRF_EXPF_BIG="0", SCRF_SIDE=side)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "tile_staging_cases.py"), out, json.dumps(entries)],
                           capture_output=True, text=True, timeout=600, env=env)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        res[side] = np.load(out)
    for prec in (FAST, FASTLIN):
        key = "chunks_p%d_" % prec
        got = {s: (res[s][key + "grad"], res[s][key + "numer"], res[s][key + "zx"]) for s in res}
        assert int(res["1"][key + "mode"]) == (2 if prec == FASTLIN else 1)
        within_bounds(got["1"], ref, prec, "three chunks prec=%d side=1" % prec)
        equal(got["1"], got["0"], key)
