"""-m gpu: launch_scores_mfma and launch_expf_mfma (scrf_mfma.hip) against the oracle at every instantiation they pick.

Every row of tests/mfma_forms.py runs one fb_batch over a batch of materialised windows under FAST and under FAST32, under
the row's knobs (read at scrf_create; set before, removed after, as tests/test_gpu_knobs.py), and compares gradient,
numerators and Zx with the CPU oracle's gradient over the same windows.  Which instantiations a row runs is the plan's answer
(tests/test_mfma_forms.py asks the probe; the launchers consume the same function), printed here from the table.

Bounds: the project's own, gpu_checks.TOL.  Under FAST the gradient bound is applied to the state block and to the transition
block separately, each relative to the largest reference component of that block, so that an error confined to the smaller
block cannot hide behind the larger one: a component is an fp64 sum of at most about 6000 products of magnitude at most 1
(rows of a batch, tests/test_mfma_forms.py), which rounds below 1e-12 of the summed magnitudes, three orders under 1e-9.
Under FAST32 the whole-gradient bound of the rest of the suite is asserted and the per-block deviations are printed.

Every case prints, before it asserts: its deviations, the worst component decoded to (label or label pair, feature column),
and the instantiations the row names."""
import numpy as np
import pytest

import gpu_checks as gc
import mfma_forms as mf

pytestmark = pytest.mark.gpu


def block_dev(g, og, mask):
    """largest deviation of a block relative to the block's largest reference component, and where (a block whose
    reference is all zero -- the transitions of a batch of one-frame utterances --: the absolute deviation)"""
    if not mask.any():
        return 0.0, -1
    d = np.where(mask, np.abs(g - og), 0.0)
    i = int(np.argmax(d))
    ref = np.abs(og[mask]).max()
    return float(d[i] / ref) if ref > 0 else float(d[i]), i


@pytest.mark.parametrize("prec", [gc.FAST, gc.FAST32], ids=["FAST", "FAST32"])
@pytest.mark.parametrize("name", mf.ROW_NAMES)
def test_row_against_the_oracle(name, prec, monkeypatch):
    row = mf.ROWS[name]
    og, on, oz = mf.reference(name)
    for k, v in row["knobs"].items():
        monkeypatch.setenv(k, v)
    c = mf.FormCase(name, precision=prec)
    eng = c.engine()
    for k in row["knobs"]:
        monkeypatch.delenv(k)      # read at scrf_create: what the environment says from here on does not matter
    b = c.batch(eng)
    mode = eng.batch_fused_mode(b)
    numer, zx = eng.fb_batch(b)
    g = eng.get_grad().copy()
    stats = eng.train_stats()
    b.close(); eng.close()

    tg, tz, tn = gc.TOL[prec]
    e_s, i_s = block_dev(g, og, c.is_state)
    e_t, i_t = block_dev(g, og, ~c.is_state)
    e_g = float(np.abs(g - og).max() / np.abs(og).max())
    e_z = float(np.abs(zx - oz).max() / np.abs(oz).max())
    e_n = float(np.abs(numer - on).max() / max(1.0, np.abs(on).max()))
    f32 = int(prec == gc.FAST32)
    print("%s %s form %d knobs %s: %s" % (name, gc.NAME[prec], mode, row["knobs"] or "default", row["why"]))
    print("  gradient: state block %.3e, transition block %.3e, whole %.3e (bound %.0e); Zx %.3e (%.0e); numerator %.3e (%.0e)"
          % (e_s, e_t, e_g, tg, e_z, tz, e_n, tn))
    print("  worst of the state block: %s" % c.describe(i_s))
    if i_t >= 0:
        print("  worst of the transition block: %s" % c.describe(i_t))
    print("  calls: %s" % (mf.calls(name, f32),))
    print("  named instantiations: %s" % ", ".join(n for n in mf.REACHES[name] if ("F32=%d" % (1 - f32)) not in n))
    assert mode == 0, "not the general path"
    assert stats == 0, "the log-domain redo ran"
    assert np.isfinite(g).all()
    if prec == gc.FAST:
        assert e_s <= tg, ("state block", e_s, c.describe(i_s))
        assert e_t <= tg, ("transition block", e_t, c.describe(i_t))
    assert e_g <= tg, ("gradient", e_g)
    assert e_z <= tz and e_n <= tn, (e_z, e_n)
