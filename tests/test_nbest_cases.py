"""not-gpu: the conditions tests/test_gpu_nbest_edges.py leans on, from the numpy reference alone (tests/nbest_cases.py, DESIGN.md
4.18).  Ties are present where a row is there for ties; the edge named in a row's "reaches" occurs -- above all a merge in which
two equal least heads lie in lists j and j + 64, that is in one lane of the kernel's merge, searched for in the reference's
candidate arrays --; the two forms of the reference agree on every row or on a small copy at the same generator; every row
fits the LDS limit and lds_max at N + 1 does not; and the scan and split batches are what their tests take them for."""
import numpy as np
import pytest

import nbest_cases as nc
import nbest_ref as nr
from nbest_cases import ROW_NAMES, ROWS


def bits(x):
    return np.float32(x).tobytes()


def distinct_costs(hyps):
    return len(set(bits(c) for _, c in hyps))


def test_grid_weights_leave_only_the_biases_and_every_score_is_a_multiple_of_the_step():
    c = nc.make_case("grid_final")
    lay = c.olay
    L = c.L
    idx = sorted(set([int(lay.state_idx[l]) + lay.num_state_funcs - 1 for l in range(L)]
                     + [int(lay.trans_idx[i]) + lay.num_trans_funcs - 1 for i in range(L * L)]))
    mask = np.zeros(c.lam.shape[0], dtype=bool)
    mask[idx] = True
    assert not c.lam[~mask].any()
    v = c.lam[mask] / 0.5
    assert np.array_equal(v, np.round(v)) and np.abs(v).max() == 4 and len(set(v)) == 9
    assert c.ocfg.state_bias_val == 1.0 and c.ocfg.trans_bias_val == 1.0
    w = nc.weights("grid_final")[1]
    for a in (w.S, w.M):     # exact multiples of the step, the same at every frame and for every duration
        assert np.array_equal(a * 2, np.round(a * 2)) and (a == a[:1]).all()
    assert np.array_equal(nc.make_case("grid_final").lam, c.lam)
    assert not nc.make_case("grid_both_zero").lam.any()


@pytest.mark.parametrize("name", nc.TIES_PRESENT)
def test_ties_are_present(name):
    """at most N / 4 distinct costs among the N hypotheses of every utterance that has N of them"""
    N = max(ROWS[name]["ns"])
    full = [h for h in nc.reference(name, N) if len(h) == N]
    d = [distinct_costs(h) for h in full]
    print("%s: N = %d, distinct costs per utterance %s" % (name, N, d))
    assert full and all(4 * x <= N for x in d), d


@pytest.mark.parametrize("name", nc.TIED_ROWS)
def test_the_twin_labels_tie_hypotheses_on_every_tied_row(name):
    N = max(ROWS[name]["ns"])
    ref = nc.reference(name, N)
    assert any(distinct_costs(h) < len(h) for h in ref)


# row -> the merges in which two equal least heads must lie in lists j and j + 64
LANE_TIES = {"grid_labels": ("boundary",), "grid_durs": ("end",), "grid_both": ("boundary",), "grid_both_zero": ("boundary", "end"),
             "grid_frame": ("boundary",), "grid_final": ("final",)}


@pytest.mark.parametrize("name", sorted(LANE_TIES))
def test_equal_least_heads_lie_in_lists_j_and_j_plus_64(name):
    N = max(ROWS[name]["ns"])
    total = {"boundary": 0, "end": 0, "final": 0}
    for w in nc.weights(name):
        count, agree = nc.lane_tie_steps(w, N)
        assert agree        # the merge redone head by head gives the stable sort's values
        for k in total:
            total[k] += count[k]
    print("%s: output steps with equal least heads in one lane %s" % (name, total))
    for kind in LANE_TIES[name]:
        assert total[kind] > 0, (kind, total)


def test_merge_by_heads_flags_exactly_the_ties_within_a_lane():
    inf = np.float32(np.inf)
    cand = np.full((66, 2, 1), inf, np.float32)
    cand[0, :, 0] = (1.0, 3.0); cand[1, :, 0] = (1.0, 2.0); cand[64, :, 0] = (2.0, 3.0); cand[65, :, 0] = (2.0, 5.0)
    val, src, same = nr.merge_by_heads(cand, 2)
    assert val[:, 0].tolist() == [1.0, 1.0] and src[:, 0].tolist() == [0, 1] and not same.any()     # lists 0 and 1: two lanes
    cand = np.concatenate([cand, np.full((66, 2, 1), inf, np.float32)], axis=1)
    val, src, same = nr.merge_by_heads(cand, 4)
    # step 2: the heads 2.0 of lists 1 and 65 (one lane) and of list 64; step 3: lists 64 and 65 are left, two lanes
    assert val[:, 0].tolist() == [1.0, 1.0, 2.0, 2.0] and src[:, 0].tolist() == [0, 1, 1, 64] and same[:, 0].tolist() == [False, False, True, False]


@pytest.mark.parametrize("name", ROW_NAMES)
def test_the_edge_a_row_is_there_for_occurs(name):
    row, kw = ROWS[name], nc.shape_of(name)
    L, D, Ts = kw["L"], kw["D"], kw["Ts"]
    N = max(row["ns"])
    ref = nc.reference(name, N)
    if name == "grid_labels":
        assert L > nc.LANES and N > nc.LANES and (D + 2) * L * N * 4 == 140000 and 1 in row["ns"]
    elif name == "grid_durs":
        assert 1 + D == 67 and Ts[0] > D and N > nc.LANES       # more lists than lanes; slot t % D is written a second time
    elif name in ("grid_both", "grid_both_zero"):
        assert L > nc.LANES and 1 + D > nc.LANES and Ts[0] > D and nc.lds_bytes(L, D, N) > 0.85 * nc.LDS_LIMIT
    elif name == "grid_long":
        assert N > 256 and len(ref[0]) == N                      # head ranks up to N - 1 in the final merge
    elif name == "grid_frame":
        assert kw["frame_model"] and L > nc.LANES and N > nc.LANES
    elif name == "grid_final":
        assert L > nc.LANES and Ts == [1, 2] and len(ref[0]) == nr.num_paths(1, L, D) == L < N and len(ref[1]) == N
    elif name == "large":
        m = [abs(float(c)) for h in ref for _, c in h]
        assert 1e4 <= max(m) < 1e6 and all(distinct_costs(h) == len(h) for h in ref)
        # the order of additions decides bits: some hypothesis summed last arc first gives another float
        w = nc.weights(name)
        assert any(bits(nr.path_cost(w[u], p)) != bits(reversed_sum(w[u], p)) for u, h in enumerate(ref) for p, _ in h)
    elif name == "lds_max":
        assert len(ref[0]) == N and nc.count_paths(Ts[0], L, D) > N + 1
    else:
        assert name in nc.TIED_ROWS and N == 16
        assert all(len(h) == min(N, nr.num_paths(T, L, D)) if T <= 2 else len(h) == N for h, T in zip(ref, Ts))


def reversed_sum(w, labels):
    """the arc weights of a segmental path added last to first"""
    L = w.L
    arcs, t, prev = [], -1, None
    for lab in labels:
        ph, d = int(lab) % L, int(lab) // L + 1
        t += d
        if prev is not None:
            arcs.append(w.boundary(t - d + 1, prev, ph))
        arcs.append(w.seg(t, d, ph))
        prev = ph
    c = np.float32(0.0)
    for a in arcs[::-1]:
        c = np.float32(c + a)
    return c


def _forms_agree(w, Ns):
    allp = [(tuple(p), c) for p, c in nr.enumerate_all(w)]
    assert len(allp) == nr.num_paths(w.T, w.L, w.D) == len(set(p for p, _ in allp))
    want = sorted(allp, key=lambda pc: pc[1])
    by_path = dict(allp)
    for N in Ns:
        got = nr.nbest(w, N)
        assert len(got) == min(N, len(allp)), (N, len(got))
        assert [bits(c) for _, c in got] == [bits(c) for _, c in want[:len(got)]], N
        assert len(set(tuple(p) for p, _ in got)) == len(got)
        for p, c in got:
            assert bits(c) == bits(nr.path_cost(w, p)) == bits(by_path[tuple(p)])
            assert sum(l // w.L + 1 for l in p) == w.T


@pytest.mark.parametrize("name", ROW_NAMES)
def test_the_reference_agrees_with_itself(name):
    """nbest (form 1) against enumerate_all (form 2): on the row's own utterances where they have few enough paths, and on a
    small copy at the same generator (L <= 3, D <= 3, T <= 6) for every row"""
    import align_ref as ar
    row, kw = ROWS[name], nc.shape_of(name)
    Ns = tuple(sorted(set(min(N, 400) for N in row["ns"]) | {3}))
    n_own = 0
    for u, T in enumerate(kw["Ts"]):
        if nc.count_paths(T, kw["L"], kw["D"]) <= nc.ENUMERABLE:
            _forms_agree(nc.weights(name)[u], Ns)
            n_own += 1
    c = nc.small_copy(name)
    assert c.L <= 3 and c.D <= 3 and max(c.Ts) <= 6
    for u in range(len(c.Ts)):
        _forms_agree(ar.case_weights(c, u), Ns)
    print("%s: %d of its own utterances enumerated, and a small copy with T = %s" % (name, n_own, c.Ts))
    if name in ("grid_final", "tied_mw", "tied_mixed"):
        assert n_own >= 1


def test_every_row_fits_the_lds_limit_and_one_more_hypothesis_at_the_limit_does_not():
    for name in ROW_NAMES:
        kw = nc.shape_of(name)
        for N in ROWS[name]["ns"]:
            b = nc.lds_bytes(kw["L"], kw["D"], N)
            print("%s: N = %d, %d bytes of LDS" % (name, N, b))
            assert b <= nc.LDS_LIMIT == 163840, (name, N, b)
    kw = nc.shape_of("lds_max")
    N = ROWS["lds_max"]["ns"][0]
    assert N == nc.largest_n(kw["L"], kw["D"]) and nc.lds_bytes(kw["L"], kw["D"], N) <= nc.LDS_LIMIT < nc.lds_bytes(kw["L"], kw["D"], N + 1)
    assert (nc.LDS_LIMIT - 128) // 32 == N     # (2 + 2) * 2 * 4 = 32 bytes per hypothesis, 16 wavefronts * 4 head ranks * 2 bytes
    assert N <= 0xffff


def test_the_scan_batches_give_every_thread_several_entries_and_hold_empty_entries_in_the_middle():
    for name, per in (("scan_even", 2), ("scan_odd", 3)):
        kw, N = nc.BATCHES[name]
        U = len(kw["Ts"])
        assert U * N > nc.SCAN_THREADS and nc.scan_per(U, N) == per
        counts = np.array([len(h) for h in nc.reference(name, N)])
        assert [int(x) for x in counts[:6]] == [min(N, nr.num_paths(T, 2, 2)) for T in range(1, 7)]
        filled = (np.arange(N)[None, :] < counts[:, None]).ravel()         # entry (utterance, rank) holds a hypothesis
        first, last = int(np.argmax(filled)), len(filled) - 1 - int(np.argmax(filled[::-1]))
        assert (~filled[first:last]).sum() > U                               # empty entries between full ones
        # threads whose range is all empty, all full, and mixed; with a boundary between threads inside an utterance's ranks
        pad = np.concatenate([filled, np.zeros(per * nc.SCAN_THREADS - len(filled), dtype=bool)]).reshape(nc.SCAN_THREADS, per)
        s = pad.sum(1)
        assert (s == 0).any() and (s == per).any()
        if per > 2 or N % per:
            assert ((s > 0) & (s < per)).any()
        assert N % per != 0 or name == "scan_even"
    kw, N = nc.BATCHES["scan_odd"]
    n = len(kw["Ts"]) * N
    assert n % 3 == 1 and n // 3 < nc.SCAN_THREADS - 1     # the last thread with entries holds one of three; threads after it none


def test_count_paths_is_the_references_count():
    for T, L, D in ((1, 3, 3), (2, 2, 2), (5, 2, 3), (6, 3, 2), (4, 2, 6)):
        assert nc.count_paths(T, L, D) == nr.num_paths(T, L, D)


def test_every_utterance_of_the_split_batch_has_fewer_than_n_paths():
    kw, N = nc.BATCHES["split"]
    assert len(kw["Ts"]) >= 300 and set(kw["Ts"]) == {1, 2, 3}
    assert all(nr.num_paths(T, kw["L"], kw["D"]) < N for T in (1, 2, 3))
    ref = nc.reference("split", N)
    assert [len(h) for h in ref] == [nr.num_paths(T, kw["L"], kw["D"]) for T in kw["Ts"]]
