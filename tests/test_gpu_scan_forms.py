"""-m gpu: the producers' max | min window scan of the wave-specialised count kernel (k_expf_fused_ws, [max | min] launches
under FASTLIN) at both tile heights.  At 76 rows a steady-state tile is scanned one statistic per wavefront, one
(frame, column) per lane, looping where a tile has more than 128 of them; at 100 rows (SCRF_EXPF_BIG=1) max and min of
a (frame, column) come from one set of loads.  Edge tiles and every tile of a shape whose D is not the kernel's DMAX
(12, 25 or 40) take the generic scan into the same column image.

Every setting runs tools/tile_staging_cases.py in a child, as tests/test_gpu_tile_staging.py does, with
SCRF_EXPF_BLOCKS=3: a workgroup then walks many tiles, and an edge tile lands in an image a full tile used before it.

Bounds: gradient against the oracle at the bounds of tools/fused_shape_sweep.py (1e-9 FAST, 1e-6 FASTLIN) and Zx at a
hundredth of that, as tests/test_gpu_tile_staging.py has them; the numerators at their tier's bound in
tests/test_gpu_input_ranges.py (1e-11 FAST, 1e-6 FASTLIN, relative to max(1, |numerator|))."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from cases import Case

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TS = [2, 25, 53, 60, 7, 101]
GROUPS = {
    "w5": {
        "L48": dict(L=48, D=25, in_w=5, Ts=TS, seed=1401),       # one output block
        "L50": dict(L=50, D=25, in_w=5, Ts=TS, seed=1402),       # two output blocks
        "L6": dict(L=6, D=25, in_w=5, Ts=TS, seed=1403),
        "L7": dict(L=7, D=25, in_w=5, Ts=TS, seed=1404),         # odd: R through registers
        "short": dict(L=48, D=25, in_w=5, Ts=[1, 2, 24], seed=1405),   # no steady-state tile at all
    },
    "narrow": {
        "W1": dict(L=48, D=25, in_w=1, Ts=TS, seed=1411),        # division by W = 1
        "W4": dict(L=48, D=25, in_w=4, Ts=TS, seed=1412),
        "D16": dict(L=48, D=16, in_w=5, Ts=TS, seed=1413),       # D != DMAX: every tile takes the generic scan
        "D20": dict(L=48, D=20, in_w=5, Ts=TS, seed=1414),
        "D40": dict(L=48, D=40, in_w=5, Ts=TS, seed=1415),       # DMAX = 40: one frame per 76-row tile, two per 100-row tile
    },
    "wide": {
        "W39": dict(L=48, D=25, in_w=39, Ts=[30, 60], seed=1421),   # 117 tasks per statistic at 76 rows: one pass; 156 at 100
        "W40": dict(L=48, D=25, in_w=40, Ts=TS, seed=1422),         # 80 columns: the image row is full
        "D8": dict(L=48, D=8, in_w=39, Ts=TS, seed=1423),           # nine frames per tile
        "D12": dict(L=48, D=12, in_w=39, Ts=TS, seed=1424),         # DMAX = 12, 234 tasks per statistic: the split form loops
    },
}
PRECS = {1: (1e-9, 1e-11, 1e-11), 3: (1e-6, 1e-8, 1e-6)}   # FAST, FASTLIN: gradient, Zx, numerator


@pytest.fixture(scope="module")
def oracle():
    cache = {}

    def get(group, name):
        if (group, name) not in cache:
            cache[(group, name)] = Case(**GROUPS[group][name]).oracle_gradient()
        return cache[(group, name)]
    return get


@pytest.mark.parametrize("big", ["0", "1"])
@pytest.mark.parametrize("group", list(GROUPS))
def test_scan_forms_against_the_oracle(group, big, tmp_path, oracle):
    shapes = GROUPS[group]
    out = os.path.join(str(tmp_path), "scan.npz")
    entries = [dict(name=n, prec=p, kw=kw) for n, kw in shapes.items() for p in PRECS]
    env = dict(os.environ, SCRF_EXPF_BLOCKS="3", SCRF_EXPF_BIG=big)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "tile_staging_cases.py"), out, json.dumps(entries)],
                       capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    res = np.load(out)
    for name in shapes:
        og, on, oz = oracle(group, name)
        for prec, (tol, tz, tn) in PRECS.items():
            key = "%s_p%d_" % (name, prec)
            eg = np.abs(res[key + "grad"] - og).max() / np.abs(og).max()
            ez = np.abs(res[key + "zx"] - oz).max() / np.abs(oz).max()
            en = np.abs(res[key + "numer"] - on).max() / max(1.0, np.abs(on).max())
            print("SCAN big=%s %s mode=%d gradient %.2e (%.0e)  Zx %.2e  (%.0e)  numerator %.2e (%.0e)" % (big, key, int(res[key + "mode"]), eg, tol, ez, tz, en, tn))
            assert int(res[key + "mode"]) == (2 if prec == 3 else 1), key   # the fused kernels ran, FASTLIN its own
            assert eg <= tol and ez <= tz and en <= tn, (key, eg, ez, en)
