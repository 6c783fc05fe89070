"""Gradients of a list of cases under the knobs of the calling environment (GPU box), for comparisons between knob
settings (SCRF_EXPF_DMA, SCRF_EXPF_BIG, SCRF_SIDE, SCRF_EXPF_BLOCKS ...: read at scrf_create).
usage: python tools/tile_staging_cases.py OUT.npz '<json list of {"name": .., "prec": .., "kw": {Case arguments}}>'
OUT.npz holds <name>_p<prec>_{grad,numer,zx,mode} for every entry (mode: Engine.batch_fused_mode)."""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "asr-craft_amd", "python")); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
from cases import Case

out = {}
for e in json.loads(sys.argv[2]):
    c = Case(precision=e["prec"], **e["kw"])
    eng = c.engine(); b = c.batch(eng)
    numer, zx = eng.fb_batch(b)
    key = "%s_p%d_" % (e["name"], e["prec"])
    out[key + "grad"] = eng.get_grad().copy()
    out[key + "numer"] = np.asarray(numer).copy()
    out[key + "zx"] = np.asarray(zx).copy()
    out[key + "mode"] = np.array(eng.batch_fused_mode(b))
    b.close(); eng.close()
    print("ran %s prec=%d mode=%d" % (e["name"], e["prec"], int(out[key + "mode"])), flush=True)
np.savez(sys.argv[1], **out)
