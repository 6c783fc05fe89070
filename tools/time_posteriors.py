"""Time the posterior output (scrf_posteriors_batch) against the training step (scrf_fb_batch) on the same batch in the
same build, under SCRF_PREC_FASTLIN, at two BASELINE shapes:

  config2  4096 utterances x 300 frames, 48 labels, D = 25, 39-dim segment stream, stdstate
  config3  256 utterances x 304 frames, 48 labels, D = 10, 144-dim segment stream + a +-6-frame context stream, stdtrans

Three calls, alternated inside every repetition after a warm-up of each:
  post_all    scrf_posteriors_batch with every output (zx, frame_post, end_post, seg_post of the best paths)
  post_small  the same with frame_post = NULL (no [sum T][L] device-to-host copy, no frame sums)
  step        scrf_zero_grad + scrf_fb_batch
`wall_ms` is a host clock around the call and a device synchronise, `kernel_ms` the sum of the HIP-event times of the
call's kernels (scrf_kernel_timing, taken in repetitions of their own: the per-kernel events serialise host and device).
Every figure is the median over the repetitions; min and max are kept beside it.  A posterior call without the frame
copy does a strict subset of the step's device work, so `kernel_ratio_post_small_over_step` must come out below 1.
Writes profiles/posteriors_time.json (--out) and prints one JSON line per shape."""
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
from scrf_amd import synth  # noqa: E402

SHAPES = {
    "config2": dict(L=48, D=25, W=39, T=300, U=4096, ctx=None, seed=2),
    "config3": dict(L=48, D=10, W=144, T=304, U=256, ctx=6, seed=4),
}


def make_batch(s, scratch_gib):
    rng = np.random.RandomState(s["seed"])
    L, D, W, T, U, ctx = s["L"], s["D"], s["W"], s["T"], s["U"], s["ctx"]
    frames = [rng.random_sample((T, W)).astype(np.float32) for _ in range(U)]
    if ctx:   # rows L1-normalised like the MLP posteriors of the TIMIT demo
        frames = [(f / f.sum(1, keepdims=True)).astype(np.float32) for f in frames]
    labels = [synth.group_labels(synth.frame_labels(rng, T, L, D), D, L) for _ in range(U)]
    Fs = 8 * W + D
    recipes = [scrf_amd.StreamRecipe(W, 0, 0, 1)]
    streams2 = None
    kw = dict(L=L, D=D, F=Fs)
    if ctx:
        Ft = (2 * ctx + 1) * W
        kw = dict(L=L, D=D, F=Fs + Ft, sfe=Fs - 1, use_trans_ftrs=True, tfs=Fs)
        recipes.append(scrf_amd.StreamRecipe(W, ctx, ctx, 0))
        streams2 = [[np.concatenate([np.repeat(f[:1], ctx, 0), f, np.repeat(f[-1:], ctx, 0)]) for f in frames]]
    eng = scrf_amd.Engine(scrf_amd.make_config(scratch_bytes=scratch_gib << 30, precision=scrf_amd.PREC_FASTLIN, **kw))
    eng.set_lambda(rng.normal(0, 0.01, eng.lambda_len))
    return eng, eng.batch_from_frames(frames, labels, recipes, streams2)


def stats(v):
    return {"median": round(float(np.median(v)), 4), "min": round(float(np.min(v)), 4), "max": round(float(np.max(v)), 4)}


def run(name, s, reps, warmup, scratch_gib):
    eng, b = make_batch(s, scratch_gib)
    labs, _ = eng.viterbi_batch(b)
    calls = {
        "post_all": lambda: eng.posteriors_batch(b, frame=True, end=True, segments=labs),
        "post_small": lambda: eng.posteriors_batch(b, frame=False, end=True, segments=labs),
        "step": lambda: (eng.zero_grad(), eng.fb_batch(b, want_scalars=False)),
    }
    for _ in range(warmup):
        for f in calls.values():
            f()
    eng.synchronize()
    wall = {k: [] for k in calls}
    for _ in range(reps):
        for k, f in calls.items():
            eng.synchronize()
            t0 = time.perf_counter()
            f()
            eng.synchronize()
            wall[k].append((time.perf_counter() - t0) * 1e3)
    kern = {k: [] for k in calls}
    per_kernel = {k: {} for k in calls}
    eng.enable_timing(True)
    for _ in range(reps):
        for k, f in calls.items():
            f()
            eng.synchronize()
            kt = eng.kernel_timing()
            kern[k].append(sum(ms for _, ms, _ in kt))
            for nm, ms, _ in kt:
                per_kernel[k].setdefault(nm, []).append(ms)
    eng.enable_timing(False)
    out = {"shape": name, "utts": s["U"], "T": s["T"], "L": s["L"], "D": s["D"], "in_width": s["W"], "precision": "fastlin",
           "batch_form": eng.batch_fused_mode(b), "repetitions": reps, "warmup": warmup,
           "frame_post_copy_mb": round(s["U"] * s["T"] * s["L"] * 8 / 1e6, 1)}
    for k in calls:
        out[k] = {"wall_ms": stats(wall[k]), "kernel_ms": stats(kern[k]),
                  "kernels_ms": {nm: round(float(np.median(v)), 4) for nm, v in sorted(per_kernel[k].items(), key=lambda kv: -np.median(kv[1]))}}
    step = out["step"]["kernel_ms"]["median"]
    out["kernel_ratio_post_small_over_step"] = round(out["post_small"]["kernel_ms"]["median"] / step, 4)
    out["kernel_ratio_post_all_over_step"] = round(out["post_all"]["kernel_ms"]["median"] / step, 4)
    out["wall_ratio_post_small_over_step"] = round(out["post_small"]["wall_ms"]["median"] / out["step"]["wall_ms"]["median"], 4)
    b.close(); eng.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="config2,config3")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--utts", type=int, default=0, help="override the utterance count of every shape (quick runs)")
    ap.add_argument("--scratch-gib", type=int, default=160)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "posteriors_time.json"))
    a = ap.parse_args()
    res = []
    for name in a.shapes.split(","):
        s = dict(SHAPES[name])
        if a.utts:
            s["U"] = a.utts
        res.append(run(name, s, a.reps, a.warmup, a.scratch_gib))
        print(json.dumps(res[-1]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump({"tool": "tools/time_posteriors.py", "shapes": res}, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
