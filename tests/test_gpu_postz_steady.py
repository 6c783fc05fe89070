"""-m gpu: the posterior walk k_post_z around the seam between its two frame steps.  A one-piece walk (SPLIT = 0) whose D
is the kernel's DMAX and at most 25 (8, 16 or 25) serves frames 0 .. D - 1 with the general loop and every frame from D
on with the steady-state step: no per-duration select, the frame's small inputs (the log-scales, the labels, the true
score) requested ahead of the rows, the scale factors in a register and from the kernel's own exp.  Shapes with another D
(D = 32 and 40 included: their forms keep the one loop), and the split form, take the general loop for every frame.

The launcher splits small launches: at most 512 wavefronts with a longest utterance of at least 4 D frames run the
SPLIT = 1 form, which is the general loop.  Every case with a T >= 4 D therefore runs twice: once with SCRF_POSTZ_SPLIT=0
set before the engine is created (the knobs are read at scrf_create), so that the one-piece walk and the steady-state
step run, and once with the knob unset.  Cases without such a T run once, with the knob at 0.

Shapes (in_w = 5), the smallest at which the step can go wrong: utterance lengths on both sides of every seam of D = 25
(no steady frame up to T = 25; exactly one, which is also the last, at 26; first and last distinct at 27; the Z_avg
ring's first retirement and its wrap at 49, 50, 51), the list reversed, a batch whose LAST utterance has T = 26 (its one
steady frame then reads the end of the chunk's arrays), every utterance as a chunk of its own (u0 != 0, non-zero frame
and row bases), the other instantiations with D == DMAX, two D != DMAX, L = 50 (two output groups, ring width 64) and
L = 6, 7.  scrf_fb_batch refuses a batch without labels, so every batch is labelled.

Bounds, those of tests/test_gpu_scan_forms.py: gradient against the oracle 1e-9 under FAST and 1e-6 under FASTLIN, Zx
1e-11 / 1e-8, numerators 1e-11 / 1e-6 (relative to max(1, |numerator|))."""
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
PRECS = {FAST: (1e-9, 1e-11, 1e-11), FASTLIN: (1e-6, 1e-8, 1e-6)}   # gradient, Zx, numerator
SEAMS = [1, 2, 24, 25, 26, 27, 49, 50, 51, 76, 101]


def lengths(D):
    return [D, D + 1, D + 2, 2 * D + 1, 4 * D + 1]


GROUPS = {
    "seams": {
        "up": dict(L=48, D=25, in_w=5, Ts=SEAMS, seed=1601),
        "down": dict(L=48, D=25, in_w=5, Ts=SEAMS[::-1], seed=1602),
        "last26": dict(L=48, D=25, in_w=5, Ts=[101, 27, 50, 26], seed=1603),
    },
    "chunks": {
        "chunks": dict(L=48, D=25, in_w=5, Ts=[51, 101, 27, 26], seed=1604, scratch_bytes=1 << 12),
        "chunks3": dict(L=48, D=25, in_w=5, Ts=[26, 76, 49], seed=1605, scratch_bytes=1 << 12),
    },
    "dmax": {
        "D8": dict(L=48, D=8, in_w=5, Ts=lengths(8), seed=1611),
        "D16": dict(L=48, D=16, in_w=5, Ts=lengths(16), seed=1612),
        "D32": dict(L=48, D=32, in_w=5, Ts=lengths(32), seed=1613),
        "D40": dict(L=48, D=40, in_w=5, Ts=lengths(40), seed=1614),
    },
    "other_d": {   # D != DMAX: the general loop serves every frame
        "D12": dict(L=48, D=12, in_w=5, Ts=lengths(12), seed=1621),
        "D20": dict(L=48, D=20, in_w=5, Ts=lengths(20), seed=1622),
    },
    "labels": {
        "L50": dict(L=50, D=25, in_w=5, Ts=[26, 51, 101], seed=1631),
        "L6": dict(L=6, D=25, in_w=5, Ts=[26, 51, 101], seed=1632),
        "L7": dict(L=7, D=25, in_w=5, Ts=[26, 51, 101], seed=1633),
    },
}


def split_settings(shapes):
    """SCRF_POSTZ_SPLIT of the runs a group needs: "0" always; unset as well where the launcher would split"""
    return ["0", None] if any(max(kw["Ts"]) >= 4 * kw["D"] for kw in shapes.values()) else ["0"]


RUNS = [(g, s) for g in GROUPS for s in split_settings(GROUPS[g])]


@pytest.fixture(scope="module")
def oracle():
    cache = {}

    def get(group, name):
        if (group, name) not in cache:
            cache[(group, name)] = Case(**GROUPS[group][name]).oracle_gradient()
        return cache[(group, name)]
    return get


def errors(got, ref):
    (g, numer, zx), (og, on, oz) = got, ref
    return (np.abs(g - og).max() / np.abs(og).max(), np.abs(zx - oz).max() / np.abs(oz).max(),
            np.abs(numer - on).max() / max(1.0, np.abs(on).max()))


def within_bounds(got, ref, prec, what):
    e, t = errors(got, ref), PRECS[prec]
    print("POSTZ %s: gradient %.2e (%.0e)  Zx %.2e (%.0e)  numerator %.2e (%.0e)" % (what, e[0], t[0], e[1], t[1], e[2], t[2]))
    assert e[0] <= t[0] and e[1] <= t[1] and e[2] <= t[2], (what, e)


def set_split(monkeypatch, split):
    if split is None:
        monkeypatch.delenv("SCRF_POSTZ_SPLIT", raising=False)
    else:
        monkeypatch.setenv("SCRF_POSTZ_SPLIT", split)


@pytest.mark.parametrize("group,split", RUNS)
def test_walk_against_the_oracle(group, split, tmp_path, oracle):
    """both precisions of every shape of a group in one child (tools/tile_staging_cases.py), the knob set in its environment"""
    shapes = GROUPS[group]
    out = os.path.join(str(tmp_path), "postz.npz")
    entries = [dict(name=n, prec=p, kw=kw) for n, kw in shapes.items() for p in PRECS]
    env = dict(os.environ)
    env.pop("SCRF_POSTZ_SPLIT", None)
    if split is not None:
        env["SCRF_POSTZ_SPLIT"] = split
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "tile_staging_cases.py"), out, json.dumps(entries)],
                       capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    res = np.load(out)
    for name in shapes:
        ref = oracle(group, name)
        for prec in PRECS:
            key = "%s_p%d_" % (name, prec)
            assert int(res[key + "mode"]) == (2 if prec == FASTLIN else 1), key   # the fused kernels ran, FASTLIN its own
            within_bounds((res[key + "grad"], res[key + "numer"], res[key + "zx"]), ref, prec, "split=%s %s" % (split, key))


@pytest.mark.parametrize("prec", [FASTLIN, FAST])
def test_bad_label_in_the_one_steady_frame(prec, monkeypatch):
    """a label >= L * D in the last frame of a middle utterance with T = D + 1 -- its only steady-state frame: code 5
    and the utterance are reported, the gradient stays that of the sound batch"""
    set_split(monkeypatch, "0")
    kw = dict(L=48, D=25, in_w=5, Ts=[27, 26, 51], seed=1641)
    c = Case(precision=prec, **kw)
    eng = c.engine(); good = c.batch(eng)
    assert eng.batch_fused_mode(good) == (2 if prec == FASTLIN else 1)
    numer, zx = eng.fb_batch(good)
    g0 = eng.get_grad(); s0 = eng.batch_sums()
    within_bounds((g0, numer, zx), Case(**kw).oracle_gradient(), prec, "sound batch prec=%d" % prec)
    labs = [l.copy() for l in c.labels]
    labs[1][-1] = c.L * c.D + 3
    bad = eng.batch_from_frames(c.frames, labs, c.recipes)
    with pytest.raises(scrf_amd.ScrfError) as ei:
        eng.fb_batch(bad, want_scalars=False)
    assert ei.value.code == 5 and "utterance 1" in str(ei.value), str(ei.value)
    assert np.array_equal(eng.get_grad(), g0) and np.array_equal(eng.batch_sums(), s0)
    bad.close(); good.close(); eng.close()


def test_a_rung_handed_to_the_log_domain_redo(monkeypatch):
    """config 2's shape (Ts = [60, 33]: steady-state frames in both, none of 4 D frames, so the walk is never split) with
    every transition that carries mass 735 nats below the matrix maximum: the linear-domain pass raises NUMERIC -- the
    steady-state step's error path latches like the general loop's -- and the batch is redone in the log domain, within
    FASTLIN's bounds"""
    split = "0"
    set_split(monkeypatch, split)
    c = sl.case("config2", "lone_max", 735, precision=FASTLIN)
    eng = c.engine(); b = c.batch(eng)
    assert eng.batch_fused_mode(b) == 2
    numer, zx = eng.fb_batch(b)
    g = eng.get_grad()
    assert eng.train_stats() == 1, eng.train_stats()
    within_bounds((g, numer, zx), sl.reference("config2", "lone_max", 735), FASTLIN, "lone_max 735 split=%s" % split)
    b.close(); eng.close()
