"""-m gpu: the R tiles of the wave-specialised expected-count kernel staged by LDS-DMA (default, even label counts)
against the register path (SCRF_EXPF_DMA=0), at both tile heights (SCRF_EXPF_BIG) and with the side stream on and off
(SCRF_SIDE).  Every setting runs tools/tile_staging_cases.py in a child: a process per setting is the plainest way to
run a tool script under it (the knobs are read at scrf_create; tests/test_gpu_knobs.py runs two settings
in one process).

SCRF_EXPF_BLOCKS=3 makes each persistent workgroup walk many tiles: an edge tile (rows [nrows, ROWS) must read as zero)
then lands in an LDS image a full tile used before -- launches of fewer tiles than workgroups never get there.

Bounds: the gradient against the oracle at the bounds of tools/fused_shape_sweep.py (1e-9 FAST, 1e-6 FASTLIN); DMA on
against DMA off bit for bit (same tile height: the same values through the same MFMAs in the same order)."""
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
SHAPES = {
    "L48": dict(L=48, D=25, in_w=5, Ts=TS, seed=1201),   # contiguous tile
    "L50": dict(L=50, D=25, in_w=5, Ts=TS, seed=1202),   # two output blocks, the second two outputs wide
    "L6": dict(L=6, D=25, in_w=5, Ts=TS, seed=1203),     # narrow, even
    "L7": dict(L=7, D=25, in_w=5, Ts=TS, seed=1204),     # odd: register path
    "L64": dict(L=64, D=25, in_w=5, Ts=TS, seed=1205),
}
SHORT = {"short": dict(L=48, D=25, in_w=5, Ts=[1, 2, 24], seed=1206)}   # no steady-state tile in either fused kernel
PRECS = {1: 1e-9, 3: 1e-6}   # FAST, FASTLIN: gradient bound against the oracle


@pytest.fixture(scope="module")
def oracle_grads():
    return {name: Case(**kw).oracle_gradient() for name, kw in {**SHAPES, **SHORT}.items()}


def run_child(tmp_path, tag, shapes, env):
    out = os.path.join(str(tmp_path), tag + ".npz")
    entries = [dict(name=n, prec=p, kw=kw) for n, kw in shapes.items() for p in PRECS]
    e = dict(os.environ, SCRF_EXPF_BLOCKS="3", **env)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "tile_staging_cases.py"), out, json.dumps(entries)],
                       capture_output=True, text=True, timeout=600, env=e)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return np.load(out)


def check_oracle(res, shapes, oracle_grads, tag):
    for name in shapes:
        og, on, oz = oracle_grads[name]
        for prec, tol in PRECS.items():
            key = "%s_p%d_" % (name, prec)
            assert int(res[key + "mode"]) == (2 if prec == 3 else 1), (tag, key)   # the fused kernels ran
            err = np.abs(res[key + "grad"] - og).max() / np.abs(og).max()
            print("%s %s grad_vs_oracle=%.2e (bound %.0e)" % (tag, key, err, tol))
            assert err <= tol, (tag, key, err)
            assert np.abs(res[key + "zx"] - oz).max() <= max(1e-11, tol * 1e-2) * np.abs(oz).max(), (tag, key)


@pytest.mark.parametrize("side", ["1", "0"])
@pytest.mark.parametrize("big", ["0", "1"])
def test_dma_staging_equals_register_staging_and_the_oracle(big, side, tmp_path, oracle_grads):
    res = {}
    for dma in ("1", "0"):
        tag = "dma%s_big%s_side%s" % (dma, big, side)
        res[dma] = run_child(tmp_path, tag, SHAPES, dict(SCRF_EXPF_DMA=dma, SCRF_EXPF_BIG=big, SCRF_SIDE=side))
        check_oracle(res[dma], SHAPES, oracle_grads, tag)
    for name in SHAPES:
        for prec in PRECS:
            key = "%s_p%d_grad" % (name, prec)
            a, b = res["1"][key], res["0"][key]
            assert a.tobytes() == b.tobytes(), (key, np.abs(a - b).max())


def test_utterances_shorter_than_the_longest_duration_only(tmp_path, oracle_grads):
    """Ts < D: every tile of the score kernel and of the count kernel is an edge tile (default knobs)."""
    res = run_child(tmp_path, "short", SHORT, {})
    check_oracle(res, SHORT, oracle_grads, "short")


@pytest.mark.parametrize("prec", ["3", "1"])
def test_shape_sweep_with_few_persistent_workgroups(prec):
    """12 random shapes of tools/fused_shape_sweep.py with three count-kernel workgroups per output block (new defaults)."""
    env = dict(os.environ, SWEEP_PREC=prec, SCRF_EXPF_BLOCKS="3")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "fused_shape_sweep.py"), "12", "23"],
                       capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert r.stdout.count("\nok ") + r.stdout.startswith("ok ") == 12
