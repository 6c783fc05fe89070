"""Time training from transcripts (scrf_fb_transcript_batch) against the labelled training pass (scrf_fb_batch)
on the same frames, in tools/time_transcript.py's protocol: one process; per shape (its config2 and config3) one engine under
SCRF_PREC_FAST, one labelled batch for fb_batch and the same batch for the soft pass (which ignores the labels); a warm-up,
then medians of the repetitions.

Transcripts, both in SCRF_ALIGN_RUNS mode: `best_path` = the collapsed phones of the batch's own best paths, `short` = random
phones without equal neighbours, one per 8 frames.  Per transcript set `soft` and once per shape `fb`, each with `wall_ms` (a
host clock around the call and a device synchronise) and `kernel_ms` / `kernels_ms` (HIP-event times per kernel, taken in
repetitions of their own).  --fb-only times fb_batch alone: run it with SCRF_AMD_LIB pointing at another build of the library
(the parent commit's) and hand its output to the full run with --parent, which records it beside its own fb figure.
Writes profiles/softgrad_time.json (--out) and prints it as one JSON line.  Nothing gates on these figures."""
import argparse
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "asr-craft_amd", "python"))
import scrf_amd  # noqa: E402
from scrf_amd import synth  # noqa: E402
from time_align import SHAPES, ragged, stats, timed  # noqa: E402
from time_transcript import no_repeat  # noqa: E402


def make_batch(s, scratch_gib):
    """time_transcript.make_batch with training labels (a random segmentation per utterance)"""
    rng = np.random.RandomState(s["seed"])
    L, D, W, T, U, ctx = s["L"], s["D"], s["W"], s["T"], s["U"], s["ctx"]
    frames = [rng.random_sample((T, W)).astype(np.float32) for _ in range(U)]
    if s["l1"]:
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
    eng = scrf_amd.Engine(scrf_amd.make_config(scratch_bytes=scratch_gib << 30, precision=scrf_amd.PREC_FAST, **kw))
    eng.set_lambda(rng.normal(0, s["lam_scale"], eng.lambda_len))
    lrng = np.random.RandomState(s["seed"] + 7)
    labels = [synth.group_labels(synth.frame_labels(lrng, T, L, D), D, L) for _ in range(U)]
    return eng, eng.batch_from_frames(frames, labels, recipes, streams2)


def kernel_timed(eng, f, reps):
    kern, per_kernel = [], {}
    eng.enable_timing(True)
    for _ in range(reps):
        f()
        kt = eng.kernel_timing()
        kern.append(sum(ms for _, ms, _ in kt))
        for nm, ms, _ in kt:
            per_kernel.setdefault(nm, []).append(ms)
    eng.enable_timing(False)
    return stats(kern), {nm: round(float(np.median(v)), 4) for nm, v in sorted(per_kernel.items(), key=lambda kv: -np.median(kv[1]))}


def measure(eng, f, a, U):
    for _ in range(a.warmup):
        f()
    wall = timed(eng, f, a.reps)
    kern, per_kernel = kernel_timed(eng, f, a.reps)
    return {"wall_ms": stats(wall), "kernel_ms": kern, "kernels_ms": per_kernel, "utts_per_s": round(U / (float(np.median(wall)) * 1e-3), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="config2,config3")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--utts", type=int, default=0, help="override the utterance count (quick runs)")
    ap.add_argument("--scratch-gib", type=int, default=16)
    ap.add_argument("--fb-only", action="store_true", help="time fb_batch alone (another build of the library through SCRF_AMD_LIB)")
    ap.add_argument("--parent", default=None, help="the --fb-only output of the parent commit's library, recorded beside this build's")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "softgrad_time.json"))
    a = ap.parse_args()
    parent = {e["shape"]: e["fb"] for e in json.load(open(a.parent))["shapes"]} if a.parent else {}
    res = {"tool": "tools/time_softgrad.py", "precision": "FAST", "mode": "SCRF_ALIGN_RUNS", "repetitions": a.reps, "warmup": a.warmup,
           "library": os.environ.get("SCRF_AMD_LIB") or "in-tree", "shapes": []}
    for name in a.shapes.split(","):
        s = dict(SHAPES[name])
        if a.utts:
            s["U"] = a.utts
        eng, b = make_batch(s, a.scratch_gib)
        L, U = s["L"], s["U"]
        entry = {"shape": name, "utts": U, "T": s["T"], "L": L, "D": s["D"], "in_width": s["W"], "lambda_scale": s["lam_scale"]}

        def fb():
            eng.zero_grad()
            eng.fb_batch(b, want_scalars=False)
        entry["fb"] = measure(eng, fb, a, U)
        if name in parent:
            entry["fb_parent_library"] = parent[name]
        if not a.fb_only:
            labs, _ = eng.viterbi_batch(b)
            per_seg = [np.asarray(l) % L for l in labs]
            collapsed = [p[np.concatenate([[True], p[1:] != p[:-1]])] if len(p) else p for p in per_seg]
            rng = np.random.RandomState(s["seed"] + 100)
            tr = {"best_path": ragged(collapsed), "short": ragged([no_repeat(rng, max(1, s["T"] // 8), L) for _ in range(b.n)])}
            entry["phones_per_utt"] = {k: round(float(np.mean(np.diff(t.off.astype(np.int64)))), 2) for k, t in tr.items()}
            for k, t in tr.items():
                def soft(t=t):
                    eng.zero_grad()
                    eng.fb_transcript_batch(b, t, scrf_amd.ALIGN_RUNS, want_scalars=False)
                e = measure(eng, soft, a, U)
                e["wall_ratio_over_fb"] = round(e["wall_ms"]["median"] / entry["fb"]["wall_ms"]["median"], 4)
                entry["soft_" + k] = e
            st = eng.soft_stats()
            entry["soft_stats"] = {"calls": st[0], "chunks": st[1], "redone": st[2]}
        res["shapes"].append(entry)
        b.close(); eng.close()
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
