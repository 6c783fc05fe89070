"""-m gpu: transcript scoring (scrf_transcript_batch) on the row-spread design of tests/row_spread.py: a label
of the transcript lies X nats under the row maximum of a few lattice rows, the alignments through those rows carry all but
e^-50 of the mass, and the alignments that avoid them keep A finite.  Every output of every case, rung, mode and transcript
is compared with form 1 of tests/transcript_ref.py on the oracle's log scores, at the bounds of tests/test_gpu_transcript.py;
tests/test_row_spread.py shows on the CPU that the linear form of the scores, read without a guard, misses the FAST bound
at every rung from 735 on.  The route is read from transcript_stats: EXACT is never redone, the linear tiers answer the
rungs up to 690 in the linear domain and redo those from 746 on; in between either route is allowed and printed.
Controls on the same batches: posteriors_batch and fb_batch, whose sums hold the label of the row maximum."""
import numpy as np
import pytest

import gpu_checks as gc
import post_ref
import row_spread as rsp
from gpu_checks import EXACT, FAST, FAST32, FASTLIN, NAME, all_devs, bits

pytestmark = pytest.mark.gpu

TOL = {EXACT: 1e-9, FAST: 1e-9, FAST32: 1e-5, FASTLIN: 1e-6}      # tests/test_gpu_transcript.py
KEYS = ("log_num", "zx", "logp", "frame_flat", "end_flat")


def check_rung(name, X, prec, eng, b):
    """every transcript set of one case at one rung, with and without segment queries; returns (failures, the largest
    deviation, calls redone, calls)"""
    ref = rsp.reference(name, X)
    rs = rsp.RowSpread(name, X)
    fails, dev, redone, calls = [], 0.0, 0, 0
    for tname, mode, ts in rs.transcripts():
        r0 = eng.transcript_stats()[2]
        segs, _ = eng.align_batch(b, ts, mode)
        out = eng.transcript_batch(b, ts, mode, segments=segs)
        r1 = eng.transcript_stats()[2]
        bare = eng.transcript_batch(b, ts, mode)
        r2 = eng.transcript_stats()[2]
        redone += r2 - r0; calls += 2
        if r1 - r0 != r2 - r1:
            fails.append((X, tname, "redone with queries %d, without %d" % (r1 - r0, r2 - r1)))
        for k in KEYS:   # the queries change nothing else
            if not np.array_equal(bits(out[k]), bits(bare[k])):
                fails.append((X, tname, "%s differs without queries" % k))
        for u, (w, g, zx) in enumerate(ref):
            devs = all_devs(out, u, rsp.ref_dp(name, X, u, mode, ts[u]), zx, [int(x) for x in segs[u]])
            d = max(devs) if np.isfinite(devs).all() else np.inf
            dev = max(dev, d)
            if not d <= TOL[prec]:
                fails.append((X, tname, "utterance %d" % u, ["%.2e" % v for v in devs]))
    return fails, dev, redone, calls


def run_ladder(name, prec, rungs):
    rs = rsp.RowSpread(name, 0, precision=prec)
    eng = rs.engine(); b = rs.batch(eng)
    fails, last_linear, first_redone = [], None, None
    for X in rungs:
        eng.set_lambda(rsp.RowSpread(name, X).lam)
        f, dev, redone, calls = check_rung(name, X, prec, eng, b)
        print("%s %s X = %g: max deviation %.3e (bound %.0e), %d of %d calls redone" % (name, NAME[prec], X, dev, TOL[prec], redone, calls))
        fails += f
        if redone not in (0, calls):
            fails.append((X, "%d of %d calls redone" % (redone, calls)))
        if prec == EXACT and redone:
            fails.append((X, "EXACT was redone"))
        if prec != EXACT and X <= rsp.EXACT_UP_TO and redone:
            fails.append((X, "an ordinary input was sent to the log domain"))
        if prec != EXACT and X >= rsp.GONE_FROM and redone != calls:
            fails.append((X, "not redone"))
        if redone == 0:
            last_linear = X
        elif first_redone is None:
            first_redone = X
    if prec == EXACT:
        print("%s EXACT: the log domain throughout, never redone" % name)
    else:
        print("%s %s: last rung answered in the linear domain %s, first rung redone %s" % (name, NAME[prec], last_linear, first_redone))
    b.close(); eng.close()
    assert not fails, fails


@pytest.mark.parametrize("name", rsp.NAMES)
def test_every_rung_equals_the_log_domain_reference_under_FAST(name):
    run_ladder(name, FAST, rsp.RUNGS)


@pytest.mark.parametrize("prec", [EXACT, FASTLIN, FAST32])
@pytest.mark.parametrize("name", rsp.ALL_TIERS)
def test_the_other_tiers_on_the_reduced_rungs(name, prec):
    run_ladder(name, prec, rsp.REDUCED)


@pytest.mark.parametrize("name", rsp.NAMES)
def test_the_free_posteriors_and_the_training_pass_hold_at_every_rung(name):
    """the controls: the free sums hold the label of the row maximum, so what they lose beside it is below their resolution"""
    rs = rsp.RowSpread(name, 0, precision=FAST)
    eng = rs.engine(); b = rs.batch(eng); bl = rs.batch(eng, with_labels=True)
    tg, tz, tn = gc.TOL[FAST]
    fails = []
    for X in rsp.RUNGS:
        rx = rsp.RowSpread(name, X)
        eng.set_lambda(rx.lam)
        ref = [(g,) + post_ref.occupancy(g, w.T, w.D, w.L) + (zx,) for w, g, zx in rsp.reference(name, X)]
        n0 = eng.train_stats()
        try:
            gc.check_posteriors(rs, ref, eng, b, gc.POST_TOL[FAST], "%s X = %g" % (name, X))
        except AssertionError as e:
            fails.append((X, "posteriors_batch", str(e)[:200]))
        n1 = eng.train_stats()
        numer, zx = eng.fb_batch(bl)
        n2 = eng.train_stats()
        on, oz = rx.oracle_numer_zx()
        e_z = np.abs(zx - oz).max() / np.abs(oz).max()
        e_n = np.abs(numer - on).max() / max(1.0, np.abs(on).max())
        print("%s X = %g: fb_batch Zx %.3e (%.0e) numerator %.3e (%.0e); redone: posteriors_batch %d, fb_batch %d" % (name, X, e_z, tz, e_n, tn, n1 - n0, n2 - n1))
        if not (e_z <= tz and e_n <= tn):
            fails.append((X, "fb_batch", e_z, e_n))
    b.close(); bl.close(); eng.close()
    assert not fails, fails


def test_a_spiked_utterance_among_ordinary_ones():
    """weights of rung 2400, spikes in utterance 1 only: the call is redone for its sake, and the ordinary utterances come back
    from the log domain as their no-spike, linear-domain, one-chunk run gave them, within the bound; under a budget that splits
    the batch the redone call gives the same bytes"""
    name, X, tol = "mixed66", 2400, TOL[FAST]
    mixed = rsp.RowSpread(name, X, precision=FAST)
    plain = rsp.RowSpread(name, X, precision=FAST, spiked=False)
    small = rsp.RowSpread(name, X, precision=FAST, scratch_bytes=1 << 18)
    em = mixed.engine(); bm = mixed.batch(em)
    ep = plain.engine(); bp = plain.batch(ep)
    es = small.engine(); bs = small.batch(es)
    ref = rsp.reference(name, X)
    dev = 0.0
    for tname, mode, ts in mixed.transcripts():
        segs, _ = em.align_batch(bm, ts, mode)
        om = em.transcript_batch(bm, ts, mode, segments=segs)
        psegs = [segs[u] if u != 1 else ep.align_batch(bp, ts, mode)[0][1] for u in range(len(ts))]   # queries that fit both batches
        op = ep.transcript_batch(bp, ts, mode, segments=psegs)
        for u, (w, g, zx) in enumerate(ref):
            devs = all_devs(om, u, rsp.ref_dp(name, X, u, mode, ts[u]), zx, [int(x) for x in segs[u]])
            assert max(devs) <= tol, (tname, u, devs)
            dev = max(dev, max(devs))
            if u != 1:
                d = [abs(om[k][u] - op[k][u]) / max(1.0, abs(op[k][u])) for k in ("log_num", "zx", "logp")] + \
                    [np.abs(om[k][u] - op[k][u]).max() for k in ("frame", "end", "segments")]
                assert max(d) <= tol, (tname, u, d)
        c0, k0, r0 = es.transcript_stats()
        osm = es.transcript_batch(bs, ts, mode, segments=segs)
        c1, k1, r1 = es.transcript_stats()
        assert c1 == c0 + 1 and r1 == r0 + 1 and k1 - k0 >= 4, (c1 - c0, k1 - k0, r1 - r0)   # two passes of several chunks each
        for k in KEYS + ("segments_flat",):
            assert np.array_equal(bits(osm[k]), bits(om[k])), (tname, k)
    n = len(mixed.transcripts())
    assert em.transcript_stats() == (n, 2 * n, n) and ep.transcript_stats() == (n, n, 0)
    print("mixed batch: max deviation %.3e" % dev)
    for x in (bm, bp, bs):
        x.close()
    for x in (em, ep, es):
        x.close()
