"""tile_staging_cases.py plus the decode side: gradients AND best paths of a list of cases under the knobs of the calling
environment (GPU box), for comparisons between knob settings (SCRF_SCORES_DMA ...: read at scrf_create).
usage: python tools/score_staging_cases.py OUT.npz '<json list of {"name": .., "prec": .., "kw": {Case arguments}}>'
OUT.npz holds <name>_p<prec>_{grad,numer,zx,mode,chunks,vchunks,vlabs,voff,vcost} for every entry (mode:
Engine.batch_fused_mode; chunks / vchunks: chunks of the timed fb_batch / viterbi_batch, counted as launches of the score
kernel -- last_timing()["k_scores"], one per chunk; vlabs/voff/vcost: viterbi_batch's flat labels, offsets, costs)."""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "asr-craft_amd", "python")); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
from cases import Case

out = {}
for e in json.loads(sys.argv[2]):
    c = Case(precision=e["prec"], **e["kw"])
    eng = c.engine(); b = c.batch(eng)
    eng.enable_timing(True)
    numer, zx = eng.fb_batch(b)
    key = "%s_p%d_" % (e["name"], e["prec"])
    out[key + "grad"] = eng.get_grad().copy()
    out[key + "numer"] = np.asarray(numer).copy()
    out[key + "zx"] = np.asarray(zx).copy()
    out[key + "mode"] = np.array(eng.batch_fused_mode(b))
    out[key + "chunks"] = np.array(eng.last_timing()["k_scores"][1])
    labs, cost = eng.viterbi_batch(b)
    out[key + "vchunks"] = np.array(eng.last_timing()["k_scores"][1])
    off = np.asarray(labs.off).copy()
    out[key + "vlabs"] = np.asarray(labs.flat[:int(off[-1])]).copy()
    out[key + "voff"] = off
    out[key + "vcost"] = np.asarray(cost).copy()
    b.close(); eng.close()
    print("ran %s prec=%d mode=%d chunks=%d vchunks=%d" % (e["name"], e["prec"], int(out[key + "mode"]), int(out[key + "chunks"]), int(out[key + "vchunks"])), flush=True)
np.savez(sys.argv[1], **out)
