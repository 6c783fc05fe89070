"""not-gpu: the lattice beam's numpy reference (tests/latprune_ref.py) against brute force, the trimness of what it keeps on
every shape of the GPU tests, the ABI surface of the feature and crf_amd::compactLattice (tests/host/compact_lattice.cpp)."""
import os
import re
import subprocess

import numpy as np
import pytest

import latprune_ref as lr
import orc
import scrf_amd
from cases import Case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BEAMS = [1e-3, 0.5, 2.0, 8.0]

BRUTE_CASES = [dict(L=3, D=3, in_w=2, Ts=[1, 2, 3, 4]), dict(L=2, D=4, in_w=3, Ts=[3, 4], trans_ctx=1)]


@pytest.mark.parametrize("ci", range(len(BRUTE_CASES)))
def test_the_reference_equals_brute_force(ci):
    c = Case(seed=500 + ci, **BRUTE_CASES[ci])
    nearest = np.inf
    for u in range(len(c.Ts)):
        arcs, ns, fin = lr.oracle_lattice(c, u)
        fwd, bwd = lr.distances(arcs, ns, fin)
        tb = lr.through_brute(arcs, ns, fin)
        assert np.isfinite(tb).all()   # every arc of the full lattice lies on a complete path
        slack = tb - tb.min()
        assert abs(tb.min() - fwd[fin]) <= 1e-9
        for beam in BEAMS:
            # brute force sums in another order: no arc may sit within 1e-9 of the limit (it excludes no case here)
            nearest = min(nearest, np.abs(slack - beam).min())
            assert np.abs(slack - beam).min() > 1e-9
            assert np.array_equal(lr.keep_mask(arcs, fwd, bwd, fin, beam), slack <= beam), (u, beam)
    print("brute force case %d: nearest arc %.4g from a limit" % (ci, nearest))


@pytest.mark.parametrize("si", range(len(lr.GPU_SHAPES)))
def test_the_kept_arcs_are_trim_and_hold_the_best_path(si):
    c = Case(seed=600 + si, **lr.GPU_SHAPES[si])
    for u in range(len(c.Ts)):
        arcs, ns, fin = lr.oracle_lattice(c, u)
        fwd, bwd = lr.distances(arcs, ns, fin)
        labs, cost = orc.best_path(arcs, ns, fin)
        assert lr.through(arcs, fwd, bwd).min() == fwd[fin]   # the best path has slack exactly 0
        for beam in BEAMS:
            kept = arcs[lr.keep_mask(arcs, fwd, bwd, fin, beam)]
            assert lr.is_trim(kept, ns, fin), (u, beam)
            kl, kc = orc.best_path(kept, ns, fin)
            assert list(kl) == list(labs) and np.float32(kc) == np.float32(cost), (u, beam)


def _decl(src, name, args):
    """`int name(type ident, ...);` with the given types ("uint64_t*" = pointer), any spacing and parameter names"""
    pats = [re.escape(a.rstrip("*")) + (r"\s*\*\s*" if a.endswith("*") else r"\s+") + r"\w+" for a in args]
    return re.search(r"\bint\s+" + name + r"\s*\(\s*" + r"\s*,\s*".join(pats) + r"\s*\)\s*;", src)


def test_the_lattice_beam_is_part_of_the_abi_the_library_and_the_engine():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "scrf_abi.h")).read(), flags=re.S)
    assert _decl(src, "scrf_lattice_prune_batch", ["scrf_handle", "scrf_batch", "double", "uint64_t*", "double*"])
    assert _decl(src, "scrf_lattice_pruned_arcs", ["scrf_handle", "scrf_batch", "uint32_t", "uint32_t", "scrf_arc*", "uint64_t"])
    assert _decl(src, "scrf_lattice_prune_stats", ["scrf_handle", "uint64_t*", "uint64_t*"])
    if not os.path.exists(scrf_amd.lib_path()):
        import __graft_entry__ as g
        g.build()
    lib = scrf_amd.load_library()
    for name in ("scrf_lattice_prune_batch", "scrf_lattice_pruned_arcs", "scrf_lattice_prune_stats"):
        assert hasattr(lib, name), name
    for name in ("lattice_prune_batch", "pruned_arcs", "lattice_prune_stats"):
        assert hasattr(scrf_amd.Engine, name), name
    host = os.path.join(ROOT, "asr-craft_amd", "host")
    # tests/test_host_multirank.py links crf_amd.cpp and CRFTrain_main.cpp against a stub ABI without the new symbols
    for f in ("crf_amd.cpp", "CRFTrain_main.cpp"):
        assert not re.search(r"scrf_lattice_prune|scrf_lattice_pruned", open(os.path.join(host, f)).read()), f
    assert "scrf_lattice_prune_batch" in open(os.path.join(host, "crf_lattice_prune.cpp")).read()
    assert "crf_lattice_prune.cpp" in open(os.path.join(host, "Makefile")).read()
    assert "scrf_latprune.hip" in open(os.path.join(ROOT, "asr-craft_amd", "csrc", "Makefile")).read()


def test_compact_lattice_on_the_host(tmp_path):
    lib = os.path.join(ROOT, "asr-craft_amd", "lib")
    if not os.path.exists(os.path.join(lib, "libcrf_amd_host.so")):
        pytest.fail("libcrf_amd_host.so not built: run __graft_entry__.build()")
    exe = str(tmp_path / "compact_lattice")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                        "-I" + os.path.join(ROOT, "asr-craft_amd", "host"), os.path.join(ROOT, "tests", "host", "compact_lattice.cpp"),
                        "-o", exe, "-L" + lib, "-Wl,-rpath," + lib, "-lcrf_amd_host", "-lscrf_amd"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "compact_lattice OK" in r.stdout
