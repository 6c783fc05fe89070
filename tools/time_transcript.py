"""Time transcript scoring (scrf_transcript_batch) against forced alignment (scrf_align_batch) on the same
batch and the same transcripts, in tools/time_align.py's protocol: one process; per shape (its config2 and config3) one
engine under SCRF_PREC_FAST and one batch; a warm-up, then medians of the repetitions.

Transcripts, both in SCRF_ALIGN_RUNS mode: `best_path` = the collapsed phones of the batch's own best paths (viterbi_batch),
`short` = random phones without equal neighbours, one per 8 frames as in read speech.  Per transcript set: `transcript` (log_num,
zx, frame and boundary posteriors; no segment queries) and `align`, each with `wall_ms` (a host clock around the call and a
device synchronise) and `kernel_ms` (HIP-event times, taken in repetitions of their own: the per-kernel events serialise host
and device).  For `transcript` kernel_ms is the sum of scrf_kernel_timing and `sweep_ms` its k_transcript line; for `align` it
is tools/time_align.py's sum (score kernels + the search phase of scrf_last_timing) and `sweep_ms` that search phase.  The
ratios compare the two calls and the two sweeps.  Writes profiles/transcript_time.json (--out) and prints it as one JSON line."""
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
from time_align import SHAPES, kernel_timed, ragged, stats, timed  # noqa: E402


def make_batch(s, scratch_gib):
    """time_align.make_batch with the engine under SCRF_PREC_FAST (the alignment does not look at the precision)"""
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
    return eng, eng.batch_from_frames(frames, None, recipes, streams2)


def no_repeat(rng, K, L):
    ph = np.empty(K, dtype=np.int64)
    ph[0] = rng.randint(0, L)
    step = rng.randint(1, L, K)
    for i in range(1, K):
        ph[i] = (ph[i - 1] + step[i]) % L
    return ph


def transcript_kernel_timed(eng, f, reps):
    kern, sweep, per_kernel = [], [], {}
    eng.enable_timing(True)
    for _ in range(reps):
        f()
        kt = eng.kernel_timing()
        kern.append(sum(ms for _, ms, _ in kt))
        sweep.append(sum(ms for nm, ms, _ in kt if nm == "k_transcript"))
        for nm, ms, _ in kt:
            per_kernel.setdefault(nm, []).append(ms)
    eng.enable_timing(False)
    return stats(kern), stats(sweep), {nm: round(float(np.median(v)), 4) for nm, v in sorted(per_kernel.items(), key=lambda kv: -np.median(kv[1]))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="config2,config3")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--utts", type=int, default=0, help="override the utterance count (quick runs)")
    ap.add_argument("--scratch-gib", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "transcript_time.json"))
    a = ap.parse_args()
    res = {"tool": "tools/time_transcript.py", "precision": "FAST", "mode": "SCRF_ALIGN_RUNS", "repetitions": a.reps, "warmup": a.warmup, "shapes": []}
    for name in a.shapes.split(","):
        s = dict(SHAPES[name])
        if a.utts:
            s["U"] = a.utts
        eng, b = make_batch(s, a.scratch_gib)
        L = s["L"]
        labs, _ = eng.viterbi_batch(b)
        per_seg = [np.asarray(l) % L for l in labs]
        collapsed = [p[np.concatenate([[True], p[1:] != p[:-1]])] if len(p) else p for p in per_seg]
        rng = np.random.RandomState(s["seed"] + 100)
        tr = {"best_path": ragged(collapsed), "short": ragged([no_repeat(rng, max(1, s["T"] // 8), L) for _ in range(b.n)])}
        entry = {"shape": name, "utts": s["U"], "T": s["T"], "L": L, "D": s["D"], "in_width": s["W"], "lambda_scale": s["lam_scale"],
                 "phones_per_utt": {k: round(float(np.mean(np.diff(t.off.astype(np.int64)))), 2) for k, t in tr.items()},
                 "max_phones": {k: int(np.max(np.diff(t.off.astype(np.int64)))) for k, t in tr.items()}}
        for k, t in tr.items():
            calls = {"transcript": lambda t=t: eng.transcript_batch(b, t, scrf_amd.ALIGN_RUNS),
                     "align": lambda t=t: eng.align_batch(b, t, scrf_amd.ALIGN_RUNS)}
            for _ in range(a.warmup):
                for f in calls.values():
                    f()
            e = {}
            for c, f in calls.items():
                wall = timed(eng, f, a.reps)
                kern, sweep, per_kernel = (transcript_kernel_timed if c == "transcript" else kernel_timed)(eng, f, a.reps)
                e[c] = {"wall_ms": stats(wall), "kernel_ms": kern, "sweep_ms": sweep, "kernels_ms": per_kernel,
                        "utts_per_s": round(s["U"] / (float(np.median(wall)) * 1e-3), 1)}
            e["wall_ratio_over_align"] = round(e["transcript"]["wall_ms"]["median"] / e["align"]["wall_ms"]["median"], 4)
            e["kernel_ratio_over_align"] = round(e["transcript"]["kernel_ms"]["median"] / e["align"]["kernel_ms"]["median"], 4)
            e["sweep_ratio_over_align"] = round(e["transcript"]["sweep_ms"]["median"] / e["align"]["sweep_ms"]["median"], 4)
            e["sweep_share_of_transcript_kernels"] = round(e["transcript"]["sweep_ms"]["median"] / e["transcript"]["kernel_ms"]["median"], 4)
            entry[k] = e
        st = eng.transcript_stats()
        entry["transcript_stats"] = {"calls": st[0], "chunks": st[1], "redone": st[2]}
        res["shapes"].append(entry)
        b.close(); eng.close()
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
