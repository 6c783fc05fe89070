"""Checks shared by tests/test_gpu_input_ranges.py and tests/test_gpu_fmap_settings.py: the decode surfaces of a batch against
the oracle bit for bit, one training call per tier at the project's per-tier bounds of tests/test_gpu_parity.py, and the
posterior output against tests/post_ref.py; and all_devs, the deviations of one transcript-scoring result (tests/test_gpu_transcript.py,
tests/test_gpu_transcript_spread.py).  Each check prints the largest deviation it saw before it asserts."""
import numpy as np

import orc
import post_ref
import scrf_amd

EXACT, FAST, FAST32, FASTLIN = scrf_amd.PREC_EXACT, scrf_amd.PREC_FAST, scrf_amd.PREC_FAST32, scrf_amd.PREC_FASTLIN
NAME = {EXACT: "EXACT", FAST: "FAST", FAST32: "FAST32", FASTLIN: "FASTLIN"}
# gradient (relative to its largest component), Zx (relative), numerator (relative to max(1, |numerator|))
TOL = {EXACT: (1e-9, 1e-11, 1e-11), FAST: (1e-9, 1e-11, 1e-11), FASTLIN: (1e-6, 1e-8, 1e-6), FAST32: (1e-5, 1e-6, 1e-5)}
POST_TOL = {EXACT: 1e-9, FAST: 1e-9, FAST32: 1e-5, FASTLIN: 1e-6}     # tests/test_gpu_posteriors.py


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def same_paths(labs, cost, want_labs, want_cost):
    return all(list(a) == list(b) for a, b in zip(labs, want_labs)) and \
        np.asarray(cost, dtype=np.float32).tobytes() == np.asarray(want_cost, dtype=np.float32).tobytes()


def check_decode_surfaces(c, utts, eng, b):
    """windows, EXACT scores, lattice arcs and the batched best path against the oracle, bit for bit"""
    mt = c.ocfg.model_type
    L = c.ocfg.num_labs
    ok = (c.olay.trans_idx != 0xffffffff) if c.ocfg.num_states > 1 else None     # the n-state topology's transitions
    labs, cost = eng.viterbi_batch(b)
    for u, T in enumerate(c.Ts):
        X, So, Mo, oa, ons, ofin, ol, oc = utts[u]
        assert np.array_equal(bits(eng.windows(b, u, T)), bits(X)), ("windows", u)
        S, M = eng.scores(b, u, T)
        assert np.array_equal(bits(S), bits(So)), ("S", u)
        if mt in (orc.STDSEG, orc.STDSEG_NO_DUR):
            assert np.array_equal(bits(M), bits(Mo)), ("M", u)
        elif ok is not None:
            assert np.array_equal(bits(M[1:, ok]), bits(Mo[1:, ok])), ("M", u)
        else:      # the transition into frame t; the first frame has none
            assert np.array_equal(bits(M[1:]), bits(Mo[1:])), ("M", u)
        ga, gns, gfin = eng.lattice_arcs(b, u)
        assert (gns, gfin) == (ons, ofin) and ga.tobytes() == oa.tobytes(), ("arcs", u)
        assert list(labs[u]) == list(ol), ("best path", u, list(labs[u]), list(ol))
        assert np.float32(cost[u]).tobytes() == np.float32(oc).tobytes(), ("cost", u)


def check_training(c, ref, prec, what):
    """one fb_batch under a tier against the oracle gradient; returns the engine's form of the batch"""
    og, on, oz = ref
    eng = c.engine(); b = c.batch(eng)
    mode = eng.batch_fused_mode(b)
    numer, zx = eng.fb_batch(b)
    g = eng.get_grad()
    stats = eng.train_stats()
    b.close(); eng.close()
    e_g = np.abs(g - og).max() / np.abs(og).max()
    e_z = np.abs(zx - oz).max() / np.abs(oz).max()
    e_n = np.abs(numer - on).max() / max(1.0, np.abs(on).max())
    tg, tz, tn = TOL[prec]
    print("%s %s form %d: gradient %.3e (%.0e)  Zx %.3e (%.0e)  numerator %.3e (%.0e)" % (what, NAME[prec], mode, e_g, tg, e_z, tz, e_n, tn))
    assert stats == 0, "the log-domain redo ran"
    assert e_g <= tg and e_z <= tz and e_n <= tn, (NAME[prec], e_g, e_z, e_n)
    return mode


def check_posteriors(c, ref, eng, b, tol, what):
    """every output of one posteriors_batch call against tests/post_ref.py (as tests/test_gpu_posteriors.py's compare)"""
    labs, _ = eng.viterbi_batch(b)
    out = eng.posteriors_batch(b, segments=labs)
    dev = 0.0
    for u, T in enumerate(c.Ts):
        g, occ, end, zx = ref[u]
        sp = post_ref.seg_post(g, labs[u], c.L, c.D)
        assert out["frame"][u].shape == (T, c.L) and out["end"][u].shape == (T,) and out["segments"][u].shape == sp.shape
        dev = max(dev, np.abs(out["frame"][u] - occ).max(), np.abs(out["end"][u] - end).max(), np.abs(out["segments"][u] - sp).max(),
                  np.abs(out["frame"][u].sum(1) - 1).max(), abs(out["end"][u][-1] - 1))
        assert abs(out["zx"][u] - zx) <= max(1e-11, tol * 1e-2) * max(1, abs(zx))
    print("posteriors %s: max deviation %.3e (bound %.0e)" % (what, dev, tol))
    assert dev <= tol, dev


def all_devs(out, u, r, zx, labs):
    """every output of utterance u (a transcript that fits) against a reference Result and the free log-partition"""
    T = r.frame_post.shape[0]
    return [abs(out["zx"][u] - zx) / max(1.0, abs(zx)), abs(out["log_num"][u] - r.A) / max(1.0, abs(r.A)),
            abs(out["logp"][u] - (r.A - zx)) / max(1.0, abs(r.A - zx)),
            np.abs(out["frame"][u] - r.frame_post).max(), np.abs(out["end"][u] - r.end_post).max(),
            np.abs(out["frame"][u].sum(axis=1) - 1.0).max(), abs(out["end"][u][T - 1] - 1.0),
            np.abs(out["segments"][u] - r.queries(labs)).max()]
