"""Time the sparse feature maps (stdsparse / stdsparsetrans) against the dense map on the host-densified frames of the
same data: ms per training step (scrf_fb_batch, FAST tier, device-synchronised) and utterances/s.

  A  stdframe + stdsparse,                       L=48, T=300, 4096 utterances, index space 4000, 24 pairs per frame
  B  as A with stdsparsetrans,                   index space 1000
  C  stdseg_no_dur_no_segtransftr D=25 + stdsparse, first-frame windows, 40 pairs, index space 2000, 1024 utterances

The densified frames of A hold 4096 * 300 * 4000 floats (20 GB); --dense-utts caps the utterances of the dense run
(default 1024) and its ms per step is scaled to the full batch (the step is linear in the utterances).  Prints one
JSON line per shape."""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "asr-craft_amd", "python"))
import scrf_amd  # noqa: E402

SHAPES = {
    "A": dict(model=scrf_amd.STDFRAME, D=1, use_tf=False, L=48, T=300, U=4096, N=4000, P=24),
    "B": dict(model=scrf_amd.STDFRAME, D=1, use_tf=True, L=48, T=300, U=4096, N=1000, P=24),
    "C": dict(model=scrf_amd.STDSEG_NO_DUR_NO_SEGTRANSFTR, D=25, use_tf=False, L=48, T=300, U=1024, N=2000, P=40),
}


def make_data(s, seed):
    rng = np.random.RandomState(seed)
    frames, labels = [], []
    for _ in range(s["U"]):
        f = np.empty((s["T"], 2 * s["P"]), dtype=np.float32)
        f[:, 0::2] = rng.randint(0, s["N"], (s["T"], s["P"])).astype(np.float32)   # unsorted, duplicates possible
        f[:, 1::2] = rng.uniform(0, 1, (s["T"], s["P"])).astype(np.float32)
        frames.append(f)
        if s["model"] == scrf_amd.STDFRAME:
            labels.append(rng.randint(0, s["L"], s["T"]).astype(np.uint32))
        else:
            lab = np.full(s["T"], scrf_amd.LAB_BAD, dtype=np.uint32)
            t = -1
            while t + 1 < s["T"]:
                d = int(rng.randint(1, min(s["D"], s["T"] - 1 - t) + 1))
                t += d
                lab[t] = rng.randint(0, s["L"]) + s["L"] * (d - 1)
            labels.append(lab)
    return frames, labels


def densify(f, N):
    out = np.zeros((f.shape[0], N), dtype=np.float32)
    rows = np.repeat(np.arange(f.shape[0]), f.shape[1] // 2)
    np.add.at(out, (rows, f[:, 0::2].astype(np.int64).ravel()), f[:, 1::2].ravel())
    return out


def time_steps(eng, b, steps, warmup):
    for _ in range(warmup):
        eng.fb_batch(b, want_scalars=False)
    eng.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        eng.fb_batch(b, want_scalars=False)
    eng.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def run(name, s, steps, warmup, dense_utts, seed, sparse_only=False):
    frames, labels = make_data(s, seed)
    F = 2 * s["P"]
    rng = np.random.RandomState(seed + 1)
    out = {"shape": name, "utts": s["U"], "T": s["T"], "L": s["L"], "D": s["D"], "index_space": s["N"], "pairs": s["P"],
           "map": "stdsparsetrans" if s["use_tf"] else "stdsparse"}
    cfg = scrf_amd.make_config(model_type=s["model"], L=s["L"], D=s["D"], F=F, sfe=s["N"] - 1, tfe=s["N"] - 1,
                               use_trans_ftrs=s["use_tf"], sparse=True, precision=scrf_amd.PREC_FAST)
    eng = scrf_amd.Engine(cfg)
    lam = rng.uniform(-0.05, 0.05, eng.lambda_len)
    eng.set_lambda(lam)
    b = eng.batch_from_frames(frames, labels, recipes=[scrf_amd.StreamRecipe(F, 0, 0, 0)])
    ms = time_steps(eng, b, steps, warmup)
    out["sparse_ms_per_step"] = round(ms, 3)
    out["sparse_utts_per_s"] = round(s["U"] / ms * 1e3, 1)
    b.close(); eng.close()
    if sparse_only:
        return out
    nd = min(dense_utts, s["U"])
    dframes = [densify(f, s["N"]) for f in frames[:nd]]
    del frames
    dcfg = scrf_amd.make_config(model_type=s["model"], L=s["L"], D=s["D"], F=s["N"], use_trans_ftrs=s["use_tf"],
                                precision=scrf_amd.PREC_FAST)
    deng = scrf_amd.Engine(dcfg)
    deng.set_lambda(lam)
    db = deng.batch_from_frames(dframes, labels[:nd], recipes=[scrf_amd.StreamRecipe(s["N"], 0, 0, 0)])
    dms = time_steps(deng, db, steps, warmup)
    out["dense_utts"] = nd
    out["dense_ms_per_step"] = round(dms * s["U"] / nd, 3)
    out["dense_utts_per_s"] = round(nd / dms * 1e3, 1)
    out["speedup"] = round(out["dense_ms_per_step"] / out["sparse_ms_per_step"], 2)
    db.close(); deng.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="A,B,C")
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--dense-utts", type=int, default=1024)
    ap.add_argument("--utts", type=int, default=0, help="override the utterance count of every shape (quick runs)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--sparse-only", action="store_true", help="skip the dense run (profiling the sparse kernels)")
    a = ap.parse_args()
    for name in a.shapes.split(","):
        s = dict(SHAPES[name])
        if a.utts:
            s["U"] = a.utts
        print(json.dumps(run(name, s, a.steps, a.warmup, a.dense_utts, a.seed, a.sparse_only)), flush=True)


if __name__ == "__main__":
    main()
