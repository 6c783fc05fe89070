"""-m gpu: the fused score kernel's staging by LDS-DMA (default: duration table, tile tables, raw frames and -- full
output blocks of an even label count -- the P image) against staging through registers (SCRF_SCORES_DMA=0).  Each
setting runs tools/score_staging_cases.py once, in a child, over every shape below (the knob is read at scrf_create,
DESIGN.md 4.16; tests/test_gpu_knobs.py runs both settings in one process).

Both forms put the same values through the same instructions in the same order, so everything is compared bit for
bit: gradient, numerators, Zx, and the labels and costs of viterbi_batch (the decode form of the kernel).  The DMA form
is also held to the oracle at the project's bounds for these paths: gradient 1e-9 FAST, 1e-6 FASTLIN, 1e-5 FAST32; Zx
max(1e-11, 1e-2 x that) as in tests/test_gpu_tile_staging.py, 1e-6 for FAST32 (tests/test_gpu_input_ranges.py)."""
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
FAST, FAST32, FASTLIN = 1, 2, 3
SHAPES = {
    "L48": dict(L=48, D=25, in_w=5, Ts=TS, seed=1301),      # edge tiles, steady-state tiles and a short last tile in one launch
    # the P image goes by DMA only in full 48-wide output blocks of an even label count: L = 48 here, and the first blocks
    # of L50 / L64.  Partial blocks (the second blocks of L50 / L64, all of L6) and odd counts (L7) cover the REGISTER P
    # path beside front staging by DMA, not the P DMA.
    "L50": dict(L=50, D=25, in_w=5, Ts=TS, seed=1302),      # two output blocks, the second two outputs wide (registers)
    "L64": dict(L=64, D=25, in_w=5, Ts=TS, seed=1303),      # ... 16 outputs wide (registers)
    "L6": dict(L=6, D=25, in_w=5, Ts=TS, seed=1304),        # narrow, even: a partial block, P through registers
    "L7": dict(L=7, D=25, in_w=5, Ts=TS, seed=1305),        # odd: P through registers
    "W39": dict(L=48, D=25, in_w=39, Ts=[300, 64], seed=1306),       # the benchmark's instantiation, 156-byte frame rows
    "W45": dict(L=48, D=25, in_w=45, Ts=[60, 101], seed=1307),       # two chunks per dense group
    "D10": dict(L=48, D=10, in_w=5, Ts=[40, 9, 101], seed=1308),     # the <12, ...> template
    "D30": dict(L=48, D=30, in_w=5, Ts=[95, 31], seed=1309),         # the <40, ...> template
    "short": dict(L=48, D=25, in_w=5, Ts=[1, 2, 24], seed=1310),     # every tile is an edge tile
    # L48 in several chunks: chunk-relative frame_base / fr0 in the DMA sources.  With this budget fb_batch takes one
    # utterance per chunk (6 launches of the score kernel) and viterbi_batch three chunks of several utterances (3 launches
    # of its decode form); 3 << 20 still left the decode call in ONE chunk.  The test asserts both counts.
    "chunked": dict(L=48, D=25, in_w=5, Ts=TS, seed=1301, scratch_bytes=3 << 18),
}
GRAD_TOL = {FAST: 1e-9, FASTLIN: 1e-6, FAST32: 1e-5}
ZX_TOL = {FAST: 1e-11, FASTLIN: 1e-8, FAST32: 1e-6}
ENTRIES = [(n, p) for n in SHAPES for p in (FAST, FASTLIN)] + [("L48", FAST32)]


def run_child(tmp, tag, env):
    out = os.path.join(str(tmp), tag + ".npz")
    entries = [dict(name=n, prec=p, kw=SHAPES[n]) for n, p in ENTRIES]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "score_staging_cases.py"), out, json.dumps(entries)],
                       capture_output=True, text=True, timeout=600, env=dict(os.environ, **env))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return dict(np.load(out))


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("score_staging")
    return {"1": run_child(tmp, "dma1", dict(SCRF_SCORES_DMA="1")), "0": run_child(tmp, "dma0", dict(SCRF_SCORES_DMA="0"))}


@pytest.fixture(scope="module")
def oracle_grads():
    return {name: Case(**kw).oracle_gradient() for name, kw in SHAPES.items() if name != "chunked"}


@pytest.mark.parametrize("name,prec", ENTRIES)
def test_dma_staging_equals_register_staging_bit_for_bit(name, prec, runs):
    key = "%s_p%d_" % (name, prec)
    for what in ("grad", "numer", "zx", "vlabs", "voff", "vcost"):
        a, b = runs["1"][key + what], runs["0"][key + what]
        assert a.shape == b.shape and a.tobytes() == b.tobytes(), (key + what, np.abs(a.astype(np.float64) - b).max())
    for dma in ("1", "0"):
        assert int(runs[dma][key + "mode"]) == (2 if prec == FASTLIN else 1), (key, dma)   # the fused kernels ran
    if name == "chunked":
        # launches of the score kernel = chunks, in the training call and in the decode call, under either knob setting
        for dma in ("1", "0"):
            nc, nv = int(runs[dma][key + "chunks"]), int(runs[dma][key + "vchunks"])
            print("%s dma=%s fb_batch chunks=%d viterbi_batch chunks=%d" % (key, dma, nc, nv))
            assert nc >= 2 and nv >= 2, (key, dma, nc, nv)


@pytest.mark.parametrize("name,prec", ENTRIES)
def test_dma_staging_against_the_oracle(name, prec, runs, oracle_grads):
    og, on, oz = oracle_grads["L48" if name == "chunked" else name]
    key = "%s_p%d_" % (name, prec)
    res = runs["1"]
    err = np.abs(res[key + "grad"] - og).max() / np.abs(og).max()
    ez = np.abs(res[key + "zx"] - oz).max() / np.abs(oz).max()
    print("%s grad_vs_oracle=%.2e (bound %.0e) zx_vs_oracle=%.2e (bound %.0e)" % (key, err, GRAD_TOL[prec], ez, ZX_TOL[prec]))
    assert err <= GRAD_TOL[prec], (key, err)
    assert ez <= ZX_TOL[prec], (key, ez)
