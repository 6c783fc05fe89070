"""Time batched N-best decoding (scrf_nbest_batch + the fetch) against free decoding on the same batch, by
tools/time_align.py's protocol.  One process; per shape one engine and one batch:

  config2  4096 utterances x 300 frames, 48 labels, D = 25, 39-dim segment stream, stdstate (the fast-decode score path)
  config3  256 utterances x 304 frames, 48 labels, D = 10, 144-dim segment stream + a +-6-frame context stream, stdtrans

Per shape: `nbest_N` for N in 1, 4, 16 and, where (D + 2) L N 4 bytes of lists fit a workgroup's LDS, 64, and `viterbi`, each
with `wall_ms` (a host clock around the call and a device synchronise; Engine.nbest_batch includes the fetch of every
hypothesis), `kernel_ms` and `search_ms`, taken in repetitions of their own (the per-kernel events serialise host and device).
`search_ms` is the search phase of scrf_last_timing (k_viterbi*, or k_nbest with its count, scan and trace kernels, with the
fix-up kernel of the fast-decode path in both); `kernel_ms` adds the HIP-event times of the score stage's kernels from
scrf_kernel_timing.  Medians over the repetitions after a warm-up; min and max beside them.  The N = 1 ratio over `viterbi`
is the number to look at first: the same search with lists of one.  Writes profiles/nbest_time.json (--out) and prints it as
one JSON line."""
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
NS = (1, 4, 16, 64)
LDS_BYTES = 160 * 1024


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
        kern.append(sum(ms for nm, ms, _ in kt if not nm.startswith("k_nbest")) + search[-1])
        for nm, ms, _ in kt:
            per_kernel.setdefault(nm, []).append(ms)
    eng.enable_timing(False)
    return stats(kern), stats(search), {nm: round(float(np.median(v)), 4) for nm, v in sorted(per_kernel.items(), key=lambda kv: -np.median(kv[1]))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="config2,config3")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--utts", type=int, default=0, help="override the utterance count (quick runs)")
    ap.add_argument("--scratch-gib", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nbest_time.json"))
    a = ap.parse_args()
    res = {"tool": "tools/time_nbest.py", "repetitions": a.reps, "warmup": a.warmup, "shapes": []}
    for name in a.shapes.split(","):
        s = dict(SHAPES[name])
        if a.utts:
            s["U"] = a.utts
        eng, b = make_batch(s, a.scratch_gib)
        ns = [n for n in NS if (s["D"] + 2) * s["L"] * n * 4 + 16 * 2 * max(s["L"], s["D"] + 1) <= LDS_BYTES]
        calls = {"nbest_%d" % n: (lambda n=n: eng.nbest_batch(b, n)) for n in ns}
        calls["viterbi"] = lambda: eng.viterbi_batch(b)
        for _ in range(a.warmup):
            for f in calls.values():
                f()
        entry = {"shape": name, "utts": s["U"], "T": s["T"], "L": s["L"], "D": s["D"], "in_width": s["W"], "lambda_scale": s["lam_scale"],
                 "fused_batch": bool(eng.batch_is_fused(b)), "n_best": ns,
                 "lds_bytes": {str(n): (s["D"] + 2) * s["L"] * n * 4 + 16 * 2 * ((max(s["L"], s["D"] + 1) + 1) & ~1) for n in NS}}
        for k, f in calls.items():
            c0 = eng.nbest_stats()
            wall = timed(eng, f, a.reps)
            c1 = eng.nbest_stats()
            kern, search, per_kernel = kernel_timed(eng, f, a.reps)
            entry[k] = {"wall_ms": stats(wall), "kernel_ms": kern, "search_ms": search, "kernels_ms": per_kernel,
                        "utts_per_s": round(s["U"] / (float(np.median(wall)) * 1e-3), 1)}
            if k != "viterbi":
                entry[k]["chunks_per_call"] = (c1[1] - c0[1]) / a.reps
                entry[k]["fast_chunks_per_call"] = (c1[2] - c0[2]) / a.reps
        for k in calls:
            if k != "viterbi":
                entry[k]["wall_ratio_over_viterbi"] = round(entry[k]["wall_ms"]["median"] / entry["viterbi"]["wall_ms"]["median"], 4)
                entry[k]["kernel_ratio_over_viterbi"] = round(entry[k]["kernel_ms"]["median"] / entry["viterbi"]["kernel_ms"]["median"], 4)
                entry[k]["search_ratio_over_viterbi"] = round(entry[k]["search_ms"]["median"] / entry["viterbi"]["search_ms"]["median"], 4)
        res["shapes"].append(entry)
        b.close(); eng.close()
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
