"""Time the batched beam-pruned lattice output (scrf_lattice_prune_batch + scrf_lattice_pruned_arcs) against
the way to the same utterances' lattices without it: a loop of scrf_lattice_arcs, one utterance and one full lattice per
call.  One process, one engine, one batch, at BASELINE config 3's shape:

  config3  64 utterances x 304 frames, 48 labels, D = 10, 144-dim segment stream + a +-6-frame context stream, stdtrans

Per beam (2, 5, 10): the kept fraction of the arcs, `wall_ms` of prune + fetch (a host clock around both calls and a device
synchronise) and `kernel_ms` (the sum of the HIP-event times of the prune call's kernels, scrf_kernel_timing, taken in
repetitions of their own: the per-kernel events serialise host and device).  `loop` is the wall time of fetching every
utterance's full lattice with scrf_lattice_arcs.  Medians over the repetitions after a warm-up; min and max beside them.
Writes profiles/lattice_prune_time.json (--out) and prints it as one JSON line."""
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

SHAPE = dict(L=48, D=10, W=144, T=304, U=64, ctx=6, seed=4, lam_scale=0.05)


def make_batch(s, scratch_gib):
    rng = np.random.RandomState(s["seed"])
    L, D, W, T, U, ctx = s["L"], s["D"], s["W"], s["T"], s["U"], s["ctx"]
    # rows L1-normalised like the MLP posteriors of the TIMIT demo
    frames = [rng.random_sample((T, W)).astype(np.float32) for _ in range(U)]
    frames = [(f / f.sum(1, keepdims=True)).astype(np.float32) for f in frames]
    Fs, Ft = 8 * W + D, (2 * ctx + 1) * W
    recipes = [scrf_amd.StreamRecipe(W, 0, 0, 1), scrf_amd.StreamRecipe(W, ctx, ctx, 0)]
    streams2 = [[np.concatenate([np.repeat(f[:1], ctx, 0), f, np.repeat(f[-1:], ctx, 0)]) for f in frames]]
    eng = scrf_amd.Engine(scrf_amd.make_config(L=L, D=D, F=Fs + Ft, sfe=Fs - 1, use_trans_ftrs=True, tfs=Fs, scratch_bytes=scratch_gib << 30))
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--beams", default="2,5,10")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--utts", type=int, default=0, help="override the utterance count (quick runs)")
    ap.add_argument("--scratch-gib", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lattice_prune_time.json"))
    a = ap.parse_args()
    s = dict(SHAPE)
    if a.utts:
        s["U"] = a.utts
    eng, b = make_batch(s, a.scratch_gib)
    beams = [float(x) for x in a.beams.split(",")]
    res = {"tool": "tools/time_lattice_prune.py", "shape": "config3", "utts": s["U"], "T": s["T"], "L": s["L"], "D": s["D"],
           "in_width": s["W"], "lambda_scale": s["lam_scale"], "repetitions": a.reps, "warmup": a.warmup,
           "full_arcs": int(b.n_arcs), "full_lattice_mb": round(b.n_arcs * 20 / 1e6, 1), "beams": []}

    def loop():
        for u in range(b.n):
            eng.lattice_arcs(b, u)

    def prune_fetch(beam):
        eng.lattice_prune_batch(b, beam)
        return eng.pruned_arcs(b)

    for _ in range(a.warmup):
        loop()
        for beam in beams:
            prune_fetch(beam)
    res["loop"] = {"wall_ms": stats(timed(eng, loop, a.reps))}
    for beam in beams:
        kept = int(prune_fetch(beam).shape[0])
        wall = timed(eng, lambda: prune_fetch(beam), a.reps)
        kern, per_kernel = [], {}
        eng.enable_timing(True)
        for _ in range(a.reps):
            eng.lattice_prune_batch(b, beam)
            kt = eng.kernel_timing()
            kern.append(sum(ms for _, ms, _ in kt))
            for nm, ms, _ in kt:
                per_kernel.setdefault(nm, []).append(ms)
        eng.enable_timing(False)
        calls, chunks = eng.lattice_prune_stats()
        res["beams"].append({
            "beam": beam, "kept_arcs": kept, "kept_fraction": round(kept / b.n_arcs, 5), "kept_mb": round(kept * 20 / 1e6, 2),
            "wall_ms": stats(wall), "kernel_ms": stats(kern),
            "kernels_ms": {nm: round(float(np.median(v)), 4) for nm, v in sorted(per_kernel.items(), key=lambda kv: -np.median(kv[1]))},
            "wall_ratio_over_loop": round(float(np.median(wall)) / res["loop"]["wall_ms"]["median"], 4),
        })
    res["chunks_per_call"] = round(chunks / calls, 2)
    b.close(); eng.close()
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
