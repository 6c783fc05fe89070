"""-m gpu: the result buffers an engine keeps across calls, as they grow and are used again.

The decode results, the posterior buffer, the transcripts and the pruned lattice of the handle are arrays that are dropped and
re-allocated when a larger batch comes (DevArray::reserve), and the lattice's arc array grows in the middle of a call with the
arcs of the chunks done moving along (reserve_keep).  One engine runs a small batch, a larger one and the small one again;
every array each call returns must equal what a fresh engine returns for that batch alone: nothing of an earlier call shows
through a re-used buffer, and nothing is lost when one moves.

FAST precision on a tiny model (L = 12, D = 4, one 4-wide segment-recipe stream).  The engine's scratch budget is 128 KB, set
through the configuration as tests/test_gpu_chunk_plan.py does: a 40-frame utterance takes about 53 KB of a lattice chunk
(22 KB of window vectors, 15 KB of scores, four 3.8 KB distance arrays), so the larger batch runs in chunks of two or three
utterances.  Its full lattice has 80,496 arcs (60,480 boundary arcs, 19,872 segment arcs, 144 final arcs): past the arc
array's first capacity of 65,536."""
import numpy as np
import pytest

import scrf_amd
from cases import Case

pytestmark = pytest.mark.gpu

SHAPE = dict(L=12, D=4, in_w=4, precision=scrf_amd.PREC_FAST)
SMALL_TS = [4, 7]
LARGE_TS = [40, 33, 38, 29, 40, 36, 31, 39, 35, 40, 37, 34]
BUDGET = 1 << 17
WIDE_BEAM = 1e6     # costs are a few nats per frame: every arc lies inside it
FIRST_ARC_CAP = 65536


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype.names:   # arcs: field by field
        return a.dtype == b.dtype and all(np.array_equal(a[f], b[f]) for f in a.dtype.names)
    return np.array_equal(a, b)


def run_all(eng, frames, recipes, L, beam):
    """every result array of the five batch entry points on one batch, by name; the transcripts are the Viterbi phones and the
    segment queries the Viterbi path"""
    b = eng.batch_from_frames(frames, None, recipes, None)
    out = {}
    labs, cost = eng.viterbi_batch(b)
    U = len(frames)
    out["vit_labels"], out["vit_off"], out["vit_cost"] = labs.flat[:int(labs.off[U])].copy(), labs.off.copy(), cost
    phones = [(np.asarray(labs[u], dtype=np.int64) % L).astype(np.uint32) for u in range(U)]
    al, al_cost = eng.align_batch(b, phones, scrf_amd.ALIGN_ONE)
    out["al_labels"], out["al_off"], out["al_cost"] = al.flat[:int(al.off[U])].copy(), al.off.copy(), al_cost
    po = eng.posteriors_batch(b, segments=labs)
    for k in ("zx", "frame_flat", "end_flat", "segments_flat"):
        out["post_" + k] = po[k]
    tr = eng.transcript_batch(b, phones, scrf_amd.ALIGN_ONE, segments=labs)
    for k in ("log_num", "zx", "frame_flat", "end_flat", "segments_flat"):
        out["tr_" + k] = tr[k]
    off, best = eng.lattice_prune_batch(b, beam)
    out["lat_off"], out["lat_best"], out["lat_arcs"] = off, best, eng.pruned_arcs(b)
    b.close()
    return out


def test_results_survive_growing_and_reused_buffers():
    large = Case(Ts=LARGE_TS, seed=901, scratch_bytes=BUDGET, **SHAPE)
    small = Case(Ts=SMALL_TS, seed=902, scratch_bytes=BUDGET, **SHAPE)
    lam, L = large.lam, SHAPE["L"]
    assert small.lam.shape == lam.shape

    def engine(cfg):
        e = scrf_amd.Engine(cfg)
        e.set_lambda(lam)
        return e

    def fresh(case, cfg=None):
        e = engine(cfg or case.gcfg)
        out = run_all(e, case.frames, case.recipes, L, WIDE_BEAM)
        stats = e.lattice_prune_stats()
        e.close()
        return out, stats

    ref_small, _ = fresh(small)
    ref_large, _ = fresh(large)
    whole, whole_stats = fresh(large, Case(Ts=LARGE_TS, seed=901, **SHAPE).gcfg)   # the default budget: one chunk
    assert whole_stats == (1, 1)

    eng = engine(large.gcfg)
    for what, case, ref in (("small", small, ref_small), ("large", large, ref_large), ("small again", small, ref_small)):
        chunks0 = eng.lattice_prune_stats()[1]
        got = run_all(eng, case.frames, case.recipes, L, WIDE_BEAM)
        assert sorted(got) == sorted(ref)
        for k in sorted(ref):
            assert same(got[k], ref[k]), (what, k)
        if case is large:
            # the arc array grew in mid-call, past its first capacity, with arcs of earlier chunks in it
            n_chunks = eng.lattice_prune_stats()[1] - chunks0
            print("large batch: %d lattice chunks, %d arcs kept" % (n_chunks, int(got["lat_off"][-1])))
            assert n_chunks >= 3
            assert int(got["lat_off"][-1]) > FIRST_ARC_CAP
            for k in ("lat_off", "lat_best", "lat_arcs"):
                assert same(got[k], whole[k]), ("one chunk", k)
    eng.close()
