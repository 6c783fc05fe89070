"""-m gpu: beam-pruned lattices (scrf_lattice_prune_batch / scrf_lattice_pruned_arcs) against the numpy
reference tests/latprune_ref.py over the CPU oracle's full lattices.  The rule fixes every bit (fp64 min-plus, one
rounding per +), so everything here is compared as raw bytes: no tolerance, no excluded case."""
import ctypes as C
import functools

import numpy as np
import pytest

import latprune_ref as lr
import orc
import scrf_amd
import sparse_ref as sr
from cases import Case

pytestmark = pytest.mark.gpu

BEAMS = lr.BEAMS
SHAPES = lr.GPU_SHAPES
CHUNKED = 5   # the shape that also runs under scratch_bytes = 1 << 18


@functools.lru_cache(maxsize=None)
def reference(si):
    """per utterance (full arcs, n_states, final, fwd, bwd) on the CPU oracle; computed once per shape and not modified"""
    c = Case(seed=600 + si, **SHAPES[si])
    out = []
    for u in range(len(c.Ts)):
        arcs, ns, fin = lr.oracle_lattice(c, u)
        fwd, bwd = lr.distances(arcs, ns, fin)
        arcs.flags.writeable = False
        out.append((arcs, ns, fin, fwd, bwd))
    return out


def case(si, **kw):
    return Case(seed=600 + si, **dict(SHAPES[si], **kw))


def check_against_reference(si, eng, b, beam):
    """one prune call: offsets, costs and every utterance's arcs, byte for byte; returns (kept fractions, all arcs)"""
    ref = reference(si)
    off, best = eng.lattice_prune_batch(b, beam)
    arcs = eng.pruned_arcs(b)
    assert off[0] == 0 and arcs.shape[0] == off[-1]
    frac = []
    for u, (full, ns, fin, fwd, bwd) in enumerate(ref):
        keep = lr.keep_mask(full, fwd, bwd, fin, beam)
        want = full[keep]
        assert off[u + 1] - off[u] == want.shape[0], (u, beam)
        assert arcs[int(off[u]):int(off[u + 1])].tobytes() == want.tobytes(), (u, beam)
        assert np.float64(best[u]).tobytes() == np.float64(fwd[fin]).tobytes(), (u, beam)
        frac.append(want.shape[0] / full.shape[0])
    return frac, arcs


@pytest.mark.parametrize("si", range(len(SHAPES)))
def test_pruned_arcs_equal_the_reference_byte_for_byte(si):
    c = case(si)
    eng = c.engine(); b = c.batch(eng, with_labels=False)
    fracs = {}
    for beam in BEAMS:
        fracs[beam], _ = check_against_reference(si, eng, b, beam)
    for u, T in enumerate(c.Ts):
        print("shape %d utterance %d (T=%d): kept %s" % (si, u, T, " ".join("%g:%.4f" % (bm, fracs[bm][u]) for bm in BEAMS)))
        if T > 1:
            assert any(0.0 < fracs[bm][u] < 1.0 for bm in BEAMS), (u, T)
    calls, chunks = eng.lattice_prune_stats()
    assert calls == len(BEAMS) and chunks == len(BEAMS)   # the default budget: one chunk per call
    b.close(); eng.close()


@pytest.mark.parametrize("si", range(len(SHAPES)))
def test_the_full_lattice_equals_the_reference_byte_for_byte(si):
    """scrf_lattice_arcs at every shape of the beam's table: the lattice the beam prunes, from the same enumeration of a
    node's arcs (the frame model with one transition matrix has no other byte-exact lattice test)"""
    c = case(si)
    eng = c.engine(); b = c.batch(eng, with_labels=False)
    for u, (full, ns, fin, _, _) in enumerate(reference(si)):
        arcs, gns, gfin = eng.lattice_arcs(b, u)
        assert (gns, gfin) == (ns, fin), u
        assert arcs.tobytes() == full.tobytes(), u
    b.close(); eng.close()


def test_chunked_runs_equal_the_one_chunk_run_and_repeat_bit_for_bit():
    si = CHUNKED
    c1 = case(si); cn = case(si, scratch_bytes=1 << 18)
    e1 = c1.engine(); b1 = c1.batch(e1, with_labels=False)
    en = cn.engine(); bn = cn.batch(en, with_labels=False)
    for beam in BEAMS:
        _, a1 = check_against_reference(si, e1, b1, beam)
        calls0, chunks0 = en.lattice_prune_stats()
        _, an = check_against_reference(si, en, bn, beam)
        calls, chunks = en.lattice_prune_stats()
        assert calls == calls0 + 1 and chunks - chunks0 > 1   # the small budget really splits the batch
        assert an.tobytes() == a1.tobytes()
        off2, best2 = en.lattice_prune_batch(bn, beam)
        assert en.pruned_arcs(bn).tobytes() == an.tobytes()   # a second call on one engine
    assert e1.lattice_prune_stats() == (len(BEAMS), len(BEAMS))
    b1.close(); e1.close(); bn.close(); en.close()


def _sparse_case():
    """the stdsparsetrans segmental case of tests/test_gpu_sparse.py (copied: test modules are not imported)"""
    L, N, P, D, Ts = 5, 40, 6, 4, [9, 14, 6]
    rng = np.random.RandomState(3)
    lay = sr.SparseLayout(L, sfe=N - 1, tfe=N - 1, use_tf=True)
    X = [sr.random_windows(rng, orc.num_segs(T, D), P, N, messy=True, values=None) for T in Ts]
    lam = rng.uniform(-0.5, 0.5, lay.lambda_len)
    cfg = scrf_amd.make_config(model_type=scrf_amd.STDSEG_NO_DUR_NO_SEGTRANSFTR, L=L, D=D, F=2 * P, sfe=N - 1, tfe=N - 1,
                               use_trans_ftrs=True, sparse=True, state_bias_val=2.5, trans_bias_val=0.5)
    eng = scrf_amd.Engine(cfg)
    eng.set_lambda(lam)
    return eng, eng.batch_from_windows(X, Ts), Ts


def _check_against_engine_lattices(eng, b, Ts):
    for beam in BEAMS:
        off, best = eng.lattice_prune_batch(b, beam)
        arcs = eng.pruned_arcs(b)
        for u in range(len(Ts)):
            full, ns, fin = eng.lattice_arcs(b, u)
            fwd, bwd = lr.distances(full, ns, fin)
            want = full[lr.keep_mask(full, fwd, bwd, fin, beam)]
            assert arcs[int(off[u]):int(off[u + 1])].tobytes() == want.tobytes(), (u, beam)
            assert np.float64(best[u]).tobytes() == np.float64(fwd[fin]).tobytes()
            assert 0 < want.shape[0] <= full.shape[0]


def test_sparse_map_and_a_batch_of_materialised_windows():
    eng, b, Ts = _sparse_case()
    _check_against_engine_lattices(eng, b, Ts)
    b.close(); eng.close()
    c = case(1)   # dense, per-frame M: the same utterances given as window vectors
    eng = c.engine()
    b = eng.batch_from_windows([c.windows(u) for u in range(len(c.Ts))], c.Ts)
    for beam in BEAMS:
        check_against_reference(1, eng, b, beam)
    b.close(); eng.close()


@pytest.mark.parametrize("si", range(len(SHAPES)))
def test_the_best_path_of_the_pruned_lattice_is_viterbi_batch(si):
    c = case(si)
    eng = c.engine(); b = c.batch(eng, with_labels=False)
    labs, cost = eng.viterbi_batch(b)
    ref = reference(si)
    for beam in (1e-3, 2.0):
        off, _ = eng.lattice_prune_batch(b, beam)
        arcs = eng.pruned_arcs(b)
        for u in range(len(c.Ts)):
            pl, pc = orc.best_path(arcs[int(off[u]):int(off[u + 1])], ref[u][1], ref[u][2])
            assert list(pl) == list(labs[u]) and np.float32(pc).tobytes() == np.float32(cost[u]).tobytes(), (u, beam)
    b.close(); eng.close()


def _code(fn):
    with pytest.raises(scrf_amd.ScrfError) as e:
        fn()
    return e.value.code, str(e.value)


def test_lifetime_and_refusals():
    c = case(3)
    eng = c.engine(); b = c.batch(eng, with_labels=False)
    INVALID = 1
    assert _code(lambda: eng.pruned_arcs(b))[0] == INVALID   # nothing pruned yet
    for beam in (0.0, -1.0, float("inf"), float("nan")):
        code, msg = _code(lambda: eng.lattice_prune_batch(b, beam))
        assert code == INVALID and "beam" in msg
    off, _ = eng.lattice_prune_batch(b, 2.0)
    full = eng.pruned_arcs(b)
    assert eng.pruned_arcs(b, 1, 2).tobytes() == full[int(off[1]):int(off[3])].tobytes()
    assert eng.pruned_arcs(b, 3, 1).tobytes() == full[int(off[3]):].tobytes()
    assert eng.pruned_arcs(b, 2, 0).shape[0] == 0
    # a capacity one short of the kept count: refused, and the message holds the count
    n = int(off[-1])
    buf = np.zeros(n, dtype=scrf_amd.ARC_DTYPE)
    rc = eng.lib.scrf_lattice_pruned_arcs(eng.h, b.handle, C.c_uint32(0), C.c_uint32(b.n), buf.ctypes.data_as(C.c_void_p), C.c_uint64(n - 1))
    assert rc == INVALID and str(n) in eng.lib.scrf_last_error(eng.h).decode()
    rc = eng.lib.scrf_lattice_pruned_arcs(eng.h, b.handle, C.c_uint32(2), C.c_uint32(b.n - 1), buf.ctypes.data_as(C.c_void_p), C.c_uint64(n))
    assert rc == INVALID   # u0 + n past the batch
    # a second batch's call replaces the result; new weights drop it
    b2 = c.batch(eng, with_labels=False)
    eng.lattice_prune_batch(b2, 2.0)
    assert _code(lambda: eng.pruned_arcs(b))[0] == INVALID
    assert eng.pruned_arcs(b2).tobytes() == full.tobytes()
    eng.set_lambda(c.lam)
    assert _code(lambda: eng.pruned_arcs(b2))[0] == INVALID
    eng.lattice_prune_batch(b, 2.0)
    eng.sgd_step(0.0)
    assert _code(lambda: eng.pruned_arcs(b))[0] == INVALID
    b2.close(); b.close(); eng.close()


@pytest.mark.parametrize("kw,name", [(dict(model_type=orc.STDSEG), "stdseg"), (dict(model_type=orc.STDSEG_NO_DUR, trans_share=(0, 9)), "stdseg_no_dur"),
                                     (dict(num_states=3), "stdseg_no_dur_no_segtransftr")])
def test_models_the_beam_is_not_built_for_are_refused_by_name(kw, name):
    c = Case(L=6, D=3, in_w=3, Ts=[6, 5], seed=2, **kw)
    eng = c.engine(); b = c.batch(eng, with_labels=False)
    code, msg = _code(lambda: eng.lattice_prune_batch(b, 2.0))
    assert code == 1 and '"%s"' % name in msg, msg
    assert eng.lib.scrf_last_error(eng.h).decode() in msg
    if "num_states" in kw:
        assert "crf_states = 3" in msg
    assert _code(lambda: eng.pruned_arcs(b))[0] == 1
    b.close(); eng.close()
