"""Time batched forced alignment (scrf_align_batch) against free decoding on the same batch and against what
the per-utterance host path has to move.  One process; per shape one engine and one batch:

  config2  4096 utterances x 300 frames, 48 labels, D = 25, 39-dim segment stream, stdstate (the fast-decode score path)
  config3  256 utterances x 304 frames, 48 labels, D = 10, 144-dim segment stream + a +-6-frame context stream, stdtrans

The transcripts are derived from the batch's own best paths (viterbi_batch): their collapsed phones for SCRF_ALIGN_RUNS,
their per-segment phones for SCRF_ALIGN_ONE; `align_runs_short` aligns random transcripts of T / 8 phones.  Per shape: `align_runs`, `align_one` and `viterbi` with `wall_ms` (a host
clock around the call and a device synchronise), `kernel_ms` and `search_ms`, taken in repetitions of their own (the
per-kernel events serialise host and device).  `search_ms` is the search phase of scrf_last_timing (k_viterbi* or k_align_*,
with the fix-up kernel of the fast-decode path in both); `kernel_ms` adds the HIP-event times of the score stage's kernels
from scrf_kernel_timing (which does not list the free search's kernel, so the search comes from the phase in both calls).
`lattice_loop_16`
is the wall time of scrf_lattice_arcs over 16 utterances, a lower bound of what the host path (full lattice to the host,
label acceptor, composition on one CPU thread) moves for them.  Medians over the repetitions after a warm-up; min and max
beside them.  Writes profiles/align_time.json (--out) and prints it as one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "asr-craft_amd", "python"))
import scrf_amd  # noqa: E402

SHAPES = {
    "config2": dict(L=48, D=25, W=39, T=300, U=4096, ctx=None, seed=2, lam_scale=0.05, l1=False),
    "config3": dict(L=48, D=10, W=144, T=304, U=256, ctx=6, seed=4, lam_scale=0.05, l1=True),
}


def make_batch(s, scratch_gib):
    rng = np.random.RandomState(s["seed"])
    L, D, W, T, U, ctx = s["L"], s["D"], s["W"], s["T"], s["U"], s["ctx"]
    frames = [rng.random_sample((T, W)).astype(np.float32) for _ in range(U)]
    if s["l1"]:   # rows L1-normalised like the MLP posteriors of the TIMIT demo
        frames = [(f / f.sum(1, keepdims=True)).astype(np.float32) for f in frames]
    Fs = 8 * W + D
    recipes = [scrf_amd.StreamRecipe(W, 0, 0, 1)]
    streams2 = None
    kw = dict(L=L, D=D, F=Fs)
    if ctx:
        Ft = (2 * ctx + 1) * W
        kw = dict(L=L, D=D, F=Fs + Ft, sfe=Fs - 1, use_trans_ftrs=True, tfs=Fs)
        recipes.append(scrf_amd.StreamRecipe(W, ctx, ctx, 0))
        streams2 = [[np.concatenate([np.repeat(f[:1], ctx, 0), f, np.repeat(f[-1:], ctx, 0)]) for f in frames]]
    eng = scrf_amd.Engine(scrf_amd.make_config(scratch_bytes=scratch_gib << 30, **kw))
    eng.set_lambda(rng.normal(0, s["lam_scale"], eng.lambda_len))
    return eng, eng.batch_from_frames(frames, None, recipes, streams2)


def stats(v):
    return {"median": round(float(np.median(v)), 4), "min": round(float(np.min(v)), 4), "max": round(float(np.max(v)), 4)}


def timed(eng, f, reps):
    out = []
    for _ in range(reps):
        eng.synchronize()
        t0 = time.perf_counter()
        f()
        eng.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def kernel_timed(eng, f, reps):
    kern, search, per_kernel = [], [], {}
    eng.enable_timing(True)
    for _ in range(reps):
        f()
        kt = eng.kernel_timing()
        search.append(eng.last_timing()["viterbi"][0])
        kern.append(sum(ms for nm, ms, _ in kt if not nm.startswith("k_align")) + search[-1])
        for nm, ms, _ in kt:
            per_kernel.setdefault(nm, []).append(ms)
    eng.enable_timing(False)
    return stats(kern), stats(search), {nm: round(float(np.median(v)), 4) for nm, v in sorted(per_kernel.items(), key=lambda kv: -np.median(kv[1]))}


def ragged(arrays):
    off = np.zeros(len(arrays) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(a) for a in arrays])
    flat = np.concatenate(arrays).astype(np.uint32) if arrays else np.zeros(0, dtype=np.uint32)
    return scrf_amd.RaggedLabels(flat, off)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="config2,config3")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--utts", type=int, default=0, help="override the utterance count (quick runs)")
    ap.add_argument("--scratch-gib", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "align_time.json"))
    a = ap.parse_args()
    res = {"tool": "tools/time_align.py", "repetitions": a.reps, "warmup": a.warmup, "shapes": []}
    for name in a.shapes.split(","):
        s = dict(SHAPES[name])
        if a.utts:
            s["U"] = a.utts
        eng, b = make_batch(s, a.scratch_gib)
        L = s["L"]
        labs, _ = eng.viterbi_batch(b)
        per_seg = [np.asarray(l) % L for l in labs]
        collapsed = [p[np.concatenate([[True], p[1:] != p[:-1]])] if len(p) else p for p in per_seg]
        tr = {"align_runs": (ragged(collapsed), scrf_amd.ALIGN_RUNS), "align_one": (ragged(per_seg), scrf_amd.ALIGN_ONE)}
        # beside the issue's transcripts (on these synthetic frames the best paths hold nearly one segment per frame): random
        # phones, one per 8 frames as in read speech, which the wavefront kernel takes
        rng = np.random.RandomState(s["seed"] + 100)
        tr["align_runs_short"] = (ragged([rng.randint(0, L, max(1, s["T"] // 8)) for _ in range(b.n)]), scrf_amd.ALIGN_RUNS)
        calls = {k: (lambda t=t, m=m: eng.align_batch(b, t, m)) for k, (t, m) in tr.items()}
        calls["viterbi"] = lambda: eng.viterbi_batch(b)
        n_loop = min(16, b.n)

        def loop():
            for u in range(n_loop):
                eng.lattice_arcs(b, u)

        for _ in range(a.warmup):
            for f in calls.values():
                f()
            loop()
        entry = {"shape": name, "utts": s["U"], "T": s["T"], "L": L, "D": s["D"], "in_width": s["W"], "lambda_scale": s["lam_scale"],
                 "fused_batch": bool(eng.batch_is_fused(b)),
                 "phones_per_utt": {k: round(float(np.mean(np.diff(t.off.astype(np.int64)))), 2) for k, (t, _) in tr.items()},
                 "max_phones": {k: int(np.max(np.diff(t.off.astype(np.int64)))) for k, (t, _) in tr.items()}}
        for k, f in calls.items():
            wall = timed(eng, f, a.reps)
            kern, search, per_kernel = kernel_timed(eng, f, a.reps)
            entry[k] = {"wall_ms": stats(wall), "kernel_ms": kern, "search_ms": search, "kernels_ms": per_kernel,
                        "utts_per_s": round(s["U"] / (float(np.median(wall)) * 1e-3), 1)}
        entry["lattice_loop_16"] = {"utts": n_loop, "wall_ms": stats(timed(eng, loop, a.reps)),
                                    "lattice_mb": round(b.n_arcs / b.n * n_loop * 20 / 1e6, 1)}
        for k in tr:
            entry[k]["kernel_ratio_over_viterbi"] = round(entry[k]["kernel_ms"]["median"] / entry["viterbi"]["kernel_ms"]["median"], 4)
            entry[k]["search_ratio_over_viterbi"] = round(entry[k]["search_ms"]["median"] / entry["viterbi"]["search_ms"]["median"], 4)
        st = eng.align_stats()
        entry["align_stats"] = {"calls": st[0], "chunks": st[1], "wave_chunks": st[2], "group_chunks": st[3]}
        res["shapes"].append(entry)
        b.close(); eng.close()
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
