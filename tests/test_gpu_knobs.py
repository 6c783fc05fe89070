"""-m gpu: engines of ONE process under different settings of knobs that used to be read once per process.

Every SCRF_* knob is read at scrf_create into the engine's own struct (csrc/scrf_knobs.h), so two engines
created in turn under SCRF_X=0 and SCRF_X=1 run the two forms.  Before, the first launch of the process fixed
SCRF_EXPF_DMA, SCRF_SCORES_DMA, SCRF_POSTZ_SPLIT and SCRF_DPLIN_MV for every later engine, and a setenv between engines
tested nothing: the child-process tests (test_gpu_tile_staging.py, test_gpu_score_staging.py, test_gpu_parity.py) exist
for that reason and keep their wider shape lists.

Shapes: the smallest that reach the kernels.  FUSED is "D10" of test_gpu_score_staging.py under FASTLIN: one full 48-wide
output block of an even label count (R tiles and the P image go by DMA), three utterances of which the longest has
101 >= 4 D frames (k_post_z splits its walk in a launch this small).  TRANS is the smallest stdtrans shape of
test_gpu_parity.py under FAST: per-frame transition matrices, where so few sweeps take k_dp_lin_mv unless SCRF_DPLIN_MV=0.

Bounds, as for these tiers in test_gpu_parity.py: gradient and numerator 1e-6 (FASTLIN) / 1e-9 (FAST), Zx a hundredth of
that.  The two DMA knobs move the same values through the same instructions in the same order: bit for bit, as the
child-process tests assert."""
import numpy as np
import pytest

import scrf_amd
from cases import Case

pytestmark = pytest.mark.gpu

CASES = {   # Case arguments, precision, bound, Engine.batch_fused_mode
    "FUSED": (dict(L=48, D=10, in_w=5, Ts=[40, 9, 101], seed=1308), scrf_amd.PREC_FASTLIN, 1e-6, 2),
    "TRANS": (dict(L=6, D=4, in_w=5, Ts=[9, 14, 3, 1], trans_ctx=1, seed=830), scrf_amd.PREC_FAST, 1e-9, 1),
}
KNOBS = {   # knob -> (case, bitwise equality between the two settings)
    "SCRF_EXPF_DMA": ("FUSED", True),
    "SCRF_SCORES_DMA": ("FUSED", True),
    "SCRF_POSTZ_SPLIT": ("FUSED", False),
    "SCRF_DPLIN_MV": ("TRANS", False),
}


@pytest.fixture(scope="module")
def oracle():
    return {name: Case(**case[0]).oracle_gradient() for name, case in CASES.items()}


@pytest.mark.parametrize("knob", sorted(KNOBS))
def test_two_engines_of_one_process_under_both_settings(knob, monkeypatch, oracle):
    case, bitwise = KNOBS[knob]
    kw, prec, tol, mode = CASES[case]
    og, on, oz = oracle[case]
    res = {}
    for value in ("0", "1"):
        monkeypatch.setenv(knob, value)
        c = Case(precision=prec, **kw)
        eng = c.engine()
        monkeypatch.delenv(knob)    # read at scrf_create: what the environment says from here on does not matter
        b = c.batch(eng)
        assert eng.batch_fused_mode(b) == mode
        numer, zx = eng.fb_batch(b)
        g = eng.get_grad().copy()
        res[value] = (g, np.asarray(numer).copy(), np.asarray(zx).copy())
        b.close(); eng.close()
        e_g = np.abs(g - og).max() / np.abs(og).max()
        e_n = np.abs(numer - on).max() / max(1, np.abs(on).max())
        e_z = np.abs(zx - oz).max() / np.abs(oz).max()
        print("%s=%s grad=%.2e numer=%.2e (bound %.0e) zx=%.2e (bound %.0e)" % (knob, value, e_g, e_n, tol, e_z, max(1e-11, tol * 1e-2)))
        assert e_g <= tol, (knob, value, e_g)
        assert e_n <= tol, (knob, value, e_n)
        assert e_z <= max(1e-11, tol * 1e-2), (knob, value, e_z)
    if bitwise:
        for a, bb, what in zip(res["0"], res["1"], ("grad", "numer", "zx")):
            assert a.tobytes() == bb.tobytes(), (knob, what, np.abs(a - bb).max())
