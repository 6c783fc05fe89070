"""numpy float32 reference of N-best decoding (scrf_nbest_batch), in two independent forms, on align_ref.Weights.

The hypotheses are the complete paths of the full lattice (scrf_lattice_arcs, norm = 0); the cost of a path is its left-to-right
float32 sum, 0.0f + w_seg(start), then alternately + w_boundary and + w_seg, then + (-0.0f) and + 0.0f (frame model: + w_frame
per frame, final weight 0.0f).  Float addition is monotone, so the multiset of the N least costs is defined bit for bit.

  nbest(w, N)        form 1: k_viterbi's recursion with a sorted list of up to N costs per state; every merge is a stable sort of
                     the candidates laid out in the order of the tie rule (boundary: p, r; end: the start arc, then t' ascending,
                     r; final: l, r).  Returns [(labels, cost)] ascending, min(N, number of paths) of them
  enumerate_all(w)   form 2: every (segmentation, labelling), each path summed left to right; [(labels, cost)] in enumeration order
  path_cost(w, labs) the left-to-right float32 sum of one path
  merge_by_heads(c, N)   a merge of form 1 redone head by head, the way a wavefront of 64 lanes does it: which output steps had
                         two equal least heads in lists j and j + 64 (nbest(w, N, on_merge=...) hands over the candidates)
"""
import itertools

import numpy as np

import align_ref as ar

F32 = np.float32
INF = F32(np.inf)


def variant(w, kind):
    """the Weights with its scores quantised to 0.5 ("ties": equal costs abound) or scaled by 1e4 ("absorb": small weights
    vanish in the float sums); None: unchanged"""
    if kind is None:
        return w
    f = (lambda x: np.round(np.asarray(x) * 2.0) / 2.0) if kind == "ties" else (lambda x: np.asarray(x) * 1e4)
    return ar.Weights(f(w.S), f(w.M), w.T, w.L, w.D, w.frame_model)


def _merge(flat, N):
    """the first N rows of the stable sort of the candidate rows, per column: (values [N, cols], source rows [N, cols])"""
    if flat.shape[0] < N:
        flat = np.concatenate([flat, np.full((N - flat.shape[0], flat.shape[1]), INF, F32)])
    order = np.argsort(flat, axis=0, kind="stable")[:N]
    return np.take_along_axis(flat, order, 0), order


def merge_by_heads(cand, N, lanes=64):
    """cand [n_lists, N, cols]: per column n_lists sorted candidate lists in the order of the tie rule, +inf padded.  The first N
    outputs of their merge, one head at a time; of all equal least heads the list of least j gives its head.  Returns (values
    [N, cols], list taken [N, cols], and per (step, column) whether two of the equal least finite heads lay in lists j and j'
    with j = j' mod lanes, that is in one lane of the kernel's nb_merge, [N, cols] bool)"""
    n_lists, n, cols = cand.shape
    assert n == N
    padded = np.concatenate([cand, np.full((n_lists, 1, cols), INF, F32)], axis=1)
    head = np.zeros((n_lists, cols), dtype=np.int64)
    col = np.arange(cols)
    lane = np.arange(n_lists) % lanes
    val = np.full((N, cols), INF, F32)
    src = np.zeros((N, cols), dtype=np.int64)
    same_lane = np.zeros((N, cols), dtype=bool)
    for s in range(N):
        h = np.take_along_axis(padded, head[:, None, :], 1)[:, 0, :]   # [n_lists, cols]
        m = h.min(0)
        tie = (h == m[None, :]) & (m < INF)[None, :]
        for k in range(min(lanes, n_lists - lanes) if n_lists > lanes else 0):
            same_lane[s] |= tie[lane == k].sum(0) >= 2
        j = np.argmax(h == m[None, :], axis=0)                          # the first list of least head
        val[s], src[s] = m, j
        head[j, col] += (m < INF)
    return val, src, same_lane


def nbest(w, N, on_merge=None):
    """on_merge(kind, t, cand [n_lists, N, cols], values [N, cols]): called with the candidates of every merge ("boundary", "end",
    "final") and its result"""
    T, L, D = w.T, w.L, w.D
    if T == 0:
        return []
    labs = np.arange(L)
    end = np.full((T, L, N), INF, F32)
    bnd = np.full((T, L, N), INF, F32)
    bp_b = np.zeros((T, L, N, 2), dtype=np.int64)   # (previous label, its rank)
    bp_e = np.zeros((T, L, N, 2), dtype=np.int64)   # (duration, rank in the boundary list)
    for t in range(T):
        if t >= 1:
            arc = w.frame if w.frame_model else w.boundary
            wt = np.stack([arc(t, p, labs) for p in range(L)]).astype(F32)    # [p, l]
            cand = (end[t - 1][:, :, None] + wt[:, None, :]).astype(F32)     # [p, r, l]: rows in (p, r) order
            val, order = _merge(cand.reshape(L * N, L), N)
            if on_merge:
                on_merge("boundary", t, cand, val)
            (end if w.frame_model else bnd)[t] = val.T
            bp_b[t, :, :, 0], bp_b[t, :, :, 1] = (order // N).T, (order % N).T
        if w.frame_model:
            if t == 0:
                end[0, :, 0] = F32(0.0) + w.seg(0, 1, labs)
            continue
        rows = [np.full((1, L), INF, F32)]   # the start arc first
        dur, rank = [t + 1], [0]
        if t < D:
            rows[0][0] = F32(0.0) + w.seg(t, t + 1, labs)
        for tp in range(max(t - D + 1, 1), t + 1):   # t' ascending = d descending
            d = t - tp + 1
            rows.append((bnd[tp] + w.seg(t, d, labs)[:, None]).astype(F32).T)   # [r, l]
            dur += [d] * N
            rank += list(range(N))
        val, order = _merge(np.concatenate(rows), N)
        if on_merge:
            start = np.full((1, N, L), INF, F32)
            start[0, 0] = rows[0][0]
            on_merge("end", t, np.concatenate([start] + [r[None] for r in rows[1:]]), val)
        order = np.minimum(order, len(dur) - 1)   # padding rows: +inf, never followed
        end[t] = val.T
        bp_e[t, :, :, 0], bp_e[t, :, :, 1] = np.asarray(dur)[order].T, np.asarray(rank)[order].T
    wf = F32(0.0) if w.frame_model else F32(-0.0)
    val, order = _merge((end[T - 1] + wf).astype(F32).reshape(L * N, 1), N)
    if on_merge:
        on_merge("final", T - 1, (end[T - 1] + wf).astype(F32)[:, :, None], val)
    out = []
    for i in range(N):
        c = val[i, 0]
        if not c < INF:
            break
        l, r = int(order[i, 0]) // N, int(order[i, 0]) % N
        t, path = T - 1, []
        while True:
            if w.frame_model:
                path.append(l)
                if t == 0:
                    break
                l, r = (int(x) for x in bp_b[t, l, r])
                t -= 1
            else:
                d, r = (int(x) for x in bp_e[t, l, r])
                path.append(l + L * (d - 1))
                ts = t - d + 1
                if ts == 0:
                    break
                l, r = (int(x) for x in bp_b[ts, l, r])
                t = ts - 1
        out.append((path[::-1], F32(c + F32(0.0))))
    return out


def path_cost(w, labels):
    L = w.L
    c = F32(0.0)
    t, prev = -1, None
    for lab in labels:
        ph, d = int(lab) % L, int(lab) // L + 1
        t += d
        if w.frame_model:
            c = c + (w.seg(0, 1, ph) if prev is None else w.frame(t, prev, ph))
        else:
            if prev is not None:
                c = c + w.boundary(t - d + 1, prev, ph)
            c = c + w.seg(t, d, ph)
        prev = ph
    assert t == w.T - 1
    c = c + (F32(0.0) if w.frame_model else F32(-0.0))
    return F32(c + F32(0.0))


def enumerate_all(w):
    T, L, D = w.T, w.L, w.D
    out = []
    for n in range(1, T + 1):
        for durs in ar._compositions(T, n, D):
            for phs in itertools.product(range(L), repeat=n):
                labels = [p + L * (d - 1) for p, d in zip(phs, durs)]
                out.append((labels, path_cost(w, labels)))
    return out


def num_paths(T, L, D):
    return sum(L ** n * sum(1 for _ in ar._compositions(T, n, D)) for n in range(1, T + 1))


def collapsed(labels, L):
    """the collapsed phone sequence of a hypothesis"""
    return tuple(int(p) for p in ar.collapse(np.asarray(labels, dtype=np.int64) % L))
