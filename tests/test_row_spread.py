"""CPU: the conditions tests/test_gpu_transcript_spread.py leans on -- no kernel is under test here.  On every case, rung, mode
and transcript of tests/row_spread.py: the oracle's own scores show the designed gap on the spiked rows and the designed
dominance; up to 690 nats the linear form of the scores (transcript_ref.linear_view, with the fp64 and with the float-rounded
row maximum) gives what the log form gives, so that range must be answered in the linear domain; from 735 nats on it gives a
finite A and misses the FAST bound, so a kernel that reads the linear form without a guard must fail the GPU test; and the
free Zx does not notice at any rung.  The rungs from 705 to 728 carry no claim either way."""
import numpy as np
import pytest

import row_spread as rsp
import transcript_ref as tr

FAST_BOUND = 1e-9      # tests/test_gpu_transcript.py, TOL[FAST]


def devs(r, ref, zx):
    """A and logp = A - Zx (the free Zx is the oracle's: it does not notice, below) relative to max(1, |.|), the posteriors
    absolute: tests/test_gpu_transcript.py's all_devs"""
    return [abs(r.A - ref.A) / max(1.0, abs(ref.A)), abs(r.A - ref.A) / max(1.0, abs(ref.A - zx)), np.abs(r.frame_post - ref.frame_post).max(), np.abs(r.end_post - ref.end_post).max(),
            np.abs(r.g - ref.g).max()]


def every(name, X):
    rs = rsp.RowSpread(name, X)
    for tname, mode, ts in rs.transcripts():
        for u, (w, g, zx) in enumerate(rsp.reference(name, X)):
            yield rs, tname, mode, ts[u], u, w, zx


@pytest.mark.parametrize("name", rsp.NAMES)
def test_the_design_holds_on_the_oracles_scores(name):
    for X in rsp.RUNGS:
        rs = rsp.RowSpread(name, X)
        for u, (w, g, zx) in enumerate(rsp.reference(name, X)):
            rows = rs.spiked_rows(u)
            assert 0 < len(rows) < w.S.shape[0], (X, u)
            S = w.S[rows]
            rest = np.delete(np.arange(w.L), [rsp.TOP, rsp.LOW])
            assert (S.argmax(axis=1) == rsp.TOP).all() and np.abs(S[:, rsp.TOP] - S[:, rsp.LOW] - X).max() <= 1e-3, (X, u)
            if rest.size:   # a third label within 700 nats of the top, at every rung
                assert (S[:, rsp.TOP, None] - S[:, rest]).max() < 700.0 and (S[:, rsp.TOP, None] - S[:, rest]).min() > 100.0, (X, u)
            other = np.delete(w.S, rows, axis=0)
            assert (other.max(axis=1) - other.min(axis=1)).max() < rsp.P_FRAME + 20.0, (X, u)   # the other rows are ordinary
    for X in rsp.RUNGS:
        for rs, tname, mode, ph, u, w, zx in every(name, X):
            assert tr.feasible(w.T, len(ph), w.D, mode), (tname, u)
            A = rsp.ref_dp(name, X, u, mode, ph).A
            S = w.S.copy()
            S[rs.spiked_rows(u), rsp.LOW] = -np.inf       # the alignments that keep `low` off the spiked rows
            rest = tr.dp(tr.Scores(S, w.M, w.T, w.L, w.D, w.frame_model), ph, mode).A
            assert np.isfinite(A) and np.isfinite(rest), (X, tname, u)                 # at least one of them exists
            assert A - rest >= rsp.MARGIN, (X, tname, u, A, rest)                      # the others carry all but e^-MARGIN


@pytest.mark.parametrize("float_smax", [False, True])
@pytest.mark.parametrize("name", rsp.NAMES)
def test_the_linear_form_is_right_up_to_690_and_wrong_but_finite_from_735(name, float_smax):
    for X in rsp.RUNGS:
        worst = 0.0
        for rs, tname, mode, ph, u, w, zx in every(name, X):
            ref = rsp.ref_dp(name, X, u, mode, ph)
            r = tr.dp(tr.linear_view(w, float_smax), ph, mode)
            d = max(devs(r, ref, zx))
            if X <= rsp.EXACT_UP_TO:
                assert d <= 1e-12, (X, tname, u, devs(r, ref, zx))
            if X >= rsp.WRONG_FROM:
                assert np.isfinite(r.A), (X, tname, u)      # no redo comes for free
            worst = max(worst, d)
        print("%s X = %g: the linear form deviates by %.3e" % (name, X, worst))
        if X >= rsp.WRONG_FROM:
            assert worst > 10 * FAST_BOUND, (X, worst)


@pytest.mark.parametrize("name", rsp.NAMES)
def test_the_free_zx_does_not_notice(name):
    for X in rsp.RUNGS:
        for u, (w, g, zx) in enumerate(rsp.reference(name, X)):
            assert abs(rsp.free_zx(w) - zx) <= 1e-13 * abs(zx), (X, u)     # the numpy recursion is the oracle's
            for float_smax in (False, True):
                zl = rsp.free_zx(tr.linear_view(w, float_smax))
                assert abs(zl - zx) <= 1e-12 * abs(zx), (X, u, zl, zx)


def test_the_rungs_visit_all_three_regimes_of_exp():
    tiny = np.finfo(np.float64).tiny
    with np.errstate(under="ignore"):
        e = {X: np.exp(-np.float64(X)) for X in rsp.RUNGS}
    assert all(e[X] >= tiny for X in rsp.RUNGS if X <= 705)
    assert all(0.0 < e[X] < tiny for X in rsp.RUNGS if 712 <= X <= 744.5)
    assert all(e[X] == 0.0 for X in rsp.RUNGS if X >= rsp.GONE_FROM)
    assert set(rsp.REDUCED) <= set(rsp.RUNGS)
