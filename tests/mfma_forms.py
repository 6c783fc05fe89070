"""Cases shared by tests/test_mfma_forms.py (CPU: which kernels a row runs) and tests/test_gpu_mfma_forms.py (GPU: the two MFMA
contractions of scrf_mfma.hip against the oracle, at every instantiation their launchers pick).

A row is a small batch of materialised windows (Engine.batch_from_windows: the engine's general path, form 0), so the
window width F and both feature ranges are free.  Three call sites reach the launchers with free shapes:

  S  state                    STDSTATE map: scores (n_out = L, nfe = nsfe) and counts (n_out = L, nfun = nsfe + bias), no row
                              map, rows = windows.  The transitions are bias-only and touch neither launcher.
  F  per-frame transitions    STDTRANS map with tfs..tfe inside the window vector: the S calls, and scores / counts with
                              n_out = L * L over ntfe features through a row map (xrow), rows = frames.
  W  per-window transitions   STDSEG_NO_DUR: the S calls, and scores / counts with n_out = L * L, no row map, rows = windows.

STDSEG's per-duration calls (a row map with n_out = La) are not needed: every instantiation with a row map is reached by an
F row, since L * L mod 48 and mod 64 take every remainder class the launchers distinguish (L = 4 .. 7, 9, 10, 11, 14), and
every one without by an S or W row.  UNREACHED, the instantiations no row runs, is therefore empty.

Windows: float32, U[-1, 1) inside the feature ranges and 100 times that outside (columns before, between and after the
ranges), so a range shifted by one column shows at order 1.  sfs = 3: the first feature is not 16-byte aligned.  D = 2, so an
utterance of T >= 2 frames has 2 T - 1 windows.  The bias values 0.1 and 0.3 are not floats: the count kernels' bfix rescale
of the bias column is exercised.  Weights N(0, s^2) per block with s = min(0.3, 3 / sqrt(features)): scores of a few nats.

Row counts are chosen against the kernels' staging: the score kernels tile rows by 256; the count kernels stage KC rows at a
time (KC = 16 split, 32 one- and eight-wave, 64 two- to four-wave) and the double-buffered and role-split forms fetch two
chunks ahead, so KC - 1, KC, KC + 1, 2 KC + 1 and 3 KC + 1 rows are different code."""
import functools

import numpy as np

import orc
import scrf_amd
from scrf_amd import synth

D = 2
SFS = 3                      # first state feature: quads of the row are not 16-byte aligned
GAP = 2                      # junk columns between the state and the transition range
STATE_BIAS, TRANS_BIAS = 0.1, 0.3
JUNK = 100.0
KNOBS = ("SCRF_SCORES_MFMA_WS", "SCRF_EXPF_MFMA_WS", "SCRF_EXPF_DB", "SCRF_TRANS_CHUNKS")
WS0 = {"SCRF_EXPF_MFMA_WS": "0"}
WS0_DB0 = {"SCRF_EXPF_MFMA_WS": "0", "SCRF_EXPF_DB": "0"}


def _row(site, L, Ts, nsfe, ntfe=0, knobs=None, bias=True, seed=0, why=""):
    assert site in "SFW" and (ntfe > 0) == (site != "S")
    return dict(site=site, L=L, Ts=tuple(Ts), nsfe=nsfe, ntfe=ntfe, knobs=dict(knobs or {}), bias=bias, seed=seed, why=why)


# name -> row.  nsfe / ntfe: state / transition features (the bias column comes on top: nfun = features + 1).
# rows of the calls: S calls sum(2 T - 1) windows; F transition calls sum(T) frames; W transition calls the windows.
ROWS = {
    # ---- state calls: the feature tail (nfe not a multiple of the 4-float quads / 32-feature chunks), the score kernel's
    # N-tiles (L = 8, 24, 40, 56: NT = 1, 2, 3, full + 1) and its 256-row tiles (1, 255, 256, 257, 513 windows)
    "s_tail1": _row("S", 8, [1], 1, why="one feature, one window"),
    "s_tail3": _row("S", 24, [128], 3, why="255 windows"),
    "s_tail4": _row("S", 40, [100, 29], 4, why="256 windows"),
    "s_tail5": _row("S", 56, [129], 5, why="257 windows; a full 48 and 8 more outputs"),
    "s_tail31": _row("S", 8, [257], 31, why="513 windows; one feature short of a chunk"),
    "s_tail32": _row("S", 24, [16], 32, why="a whole chunk, the bias alone in the next; 31 rows"),
    "s_tail33": _row("S", 40, [9, 8], 33, why="a chunk and one feature; 32 rows"),
    # ---- state calls: wavefronts per workgroup by nfun = nsfe + 1, at both sides of every step
    "s_nf48": _row("S", 5, [17], 47, why="nfun 48: one wave tile, full; 33 rows = KC + 1"),
    "s_nf49": _row("S", 20, [32], 48, why="nfun 49: the bias column alone in a second wave tile; 63 rows = KC - 1"),
    "s_nf96": _row("S", 40, [17, 16], 95, why="nfun 96; 64 rows = KC"),
    "s_nf97": _row("S", 5, [33], 96, why="nfun 97: three waves; 65 rows = KC + 1"),
    "s_nf144": _row("S", 20, [65], 143, why="nfun 144; 129 rows = 2 KC + 1"),
    "s_nf145": _row("S", 40, [97], 144, why="nfun 145: four waves; 193 rows = 3 KC + 1"),
    "s_nf192": _row("S", 5, [33, 32], 191, why="nfun 192: the last narrow form; 128 rows"),
    "s_nf193": _row("S", 50, [16], 192, why="nfun 193: eight waves; 50 outputs: MT = 4 of a 64-wide tile (f64), 48 + 2 (f32); 31 rows"),
    "s_nf384": _row("S", 20, [9, 8], 383, why="nfun 384: the feature tile full; 32 rows"),
    "s_nf385": _row("S", 40, [17], 384, why="nfun 385: a second feature tile that holds the bias column alone; 33 rows"),
    "s_nw1_mt2": _row("S", 20, [49], 20, why="one wave, MT = 2; 97 rows = 3 KC + 1"),
    "s_nw2_mt1": _row("S", 5, [3], 59, why="two waves, MT = 1; 5 rows"),
    "s_nw3_mt3": _row("S", 40, [2], 119, why="three waves, MT = 3; 3 rows"),
    "s_nw4_mt2": _row("S", 20, [20, 13], 169, why="four waves, MT = 2; 64 rows"),
    "s_wide_mt1": _row("S", 70, [33], 200, why="eight waves: a full tile and 6 (f64) / 22 (f32) outputs; 65 rows = 2 KC + 1"),
    "s_chunks": _row("S", 3, [2065], 40, why="4129 windows: over the 4096-row floor of a row chunk, the second chunk has 33 rows"),
    "s_nobias": _row("S", 20, [30, 3], 48, bias=False, why="no bias column: nfun = nfe = 48 stays one wave tile; no bfix"),
    # ---- per-frame transitions, narrow forms: L * L = 16, 25, 36, 49 outputs (MT = 1, 2, 3, full + 1) per wave count
    "f_nw1_mt1": _row("F", 4, [20, 11], 6, 19, why="31 frames = KC - 1"),
    "f_nw1_mt2": _row("F", 5, [25, 7], 6, 31, why="32 frames = KC"),
    "f_nw1_mt3": _row("F", 6, [33], 6, 47, why="33 frames = KC + 1; nfun 48"),
    "f_nw1_full": _row("F", 7, [60, 5], 6, 5, why="65 frames = 2 KC + 1; 48 + 1 outputs"),
    "f_nw2_mt1": _row("F", 4, [63], 6, 48, why="63 frames = KC - 1; nfun 49"),
    "f_nw2_mt2": _row("F", 5, [40, 24], 6, 60, why="64 frames = KC"),
    "f_nw2_mt3": _row("F", 6, [64, 1], 6, 95, why="65 frames = KC + 1, an utterance of one frame"),
    "f_nw3_mt1": _row("F", 4, [100, 29], 6, 96, why="129 frames = 2 KC + 1"),
    "f_nw3_mt2": _row("F", 5, [193], 6, 110, why="193 frames = 3 KC + 1"),
    "f_nw3_mt3": _row("F", 6, [50, 13], 6, 143, why="63 frames"),
    "f_nw4_mt1": _row("F", 4, [64], 6, 144, why="64 frames"),
    "f_nw4_mt2": _row("F", 5, [33, 32], 6, 170, why="65 frames"),
    "f_nw4_mt3": _row("F", 6, [129], 6, 191, why="129 frames; nfe 191: the last below the score kernels' role split"),
    # ---- per-frame transitions, the 8-wave form (at least 193 transition functions): 81, 100, 121, 196 outputs are MT = 2, 3,
    # 4 and 1 remainders of 64-wide tiles in f64 and MT = 3, 1, 2, 1 of 48-wide ones in f32; 31 .. 97 frames are 1 to 4 staged
    # chunks.  The score calls: 100 outputs <2,7> alone, 121 <4,3> and a 25-output single-role launch at o_base 96, 196 both.
    "f_ws_81": _row("F", 9, [31], 6, 192, why="31 frames: one chunk, short"),
    "f_ws_100": _row("F", 10, [20, 12], 6, 200, why="32 frames: one whole chunk"),
    "f_ws_121": _row("F", 11, [33], 6, 230, why="33 frames: two chunks; the MT = 4 remainder at o_base 64"),
    "f_ws_196": _row("F", 14, [65], 6, 384, why="65 frames: three chunks; nfun 385: a second feature tile, mostly masked"),
    "f_db_81": _row("F", 9, [97], 6, 200, knobs=WS0, why="97 frames: four chunks"),
    "f_db_100": _row("F", 10, [31], 6, 384, knobs=WS0, why="31 frames; a second feature tile"),
    "f_db_121": _row("F", 11, [32], 6, 192, knobs=WS0, why="32 frames"),
    "f_db_196": _row("F", 14, [30, 3], 6, 200, knobs=WS0, why="33 frames"),
    "f_one_81": _row("F", 9, [65], 6, 192, knobs=WS0_DB0, why="65 frames"),
    "f_one_100": _row("F", 10, [97], 6, 200, knobs=WS0_DB0, why="97 frames"),
    "f_one_121": _row("F", 11, [31], 6, 384, knobs=WS0_DB0, why="31 frames; a second feature tile"),
    "f_one_196": _row("F", 14, [32], 6, 230, knobs=WS0_DB0, why="32 frames"),
    "f_ws_144": _row("F", 12, [40], 6, 192, why="144 outputs: <4,3> and one full single-role 48; nfe 192: the first with the role split"),
    "f_ws_100_191": _row("F", 10, [40], 6, 191, why="100 outputs at nfe 191: single-role score kernels, two full tiles and 4"),
    "f_noscws_121": _row("F", 11, [40], 6, 200, knobs={"SCRF_SCORES_MFMA_WS": "0"}, why="the single-role score kernel from 192 features on"),
    "f_chunks": _row("F", 9, [120, 80], 6, 200, knobs={"SCRF_TRANS_CHUNKS": "3"}, why="200 frames in 3 row chunks of 67: chunks start off the KC grid"),
    # ---- the split count form (at most 48 transition functions, at least 192 outputs; KC = 16)
    "f_split_15": _row("F", 14, [9, 6], 6, 47, why="196 outputs: the second workgroup holds 4; 15 frames = KC - 1; nfun 48"),
    "f_split_17": _row("F", 14, [17], 6, 20, why="17 frames = KC + 1"),
    "f_nosplit_169": _row("F", 13, [20], 6, 20, why="169 < 192 outputs stay with the one-wave form: three full tiles and 25"),
    # ---- per-window transitions (no row map, n_out = L * L): the 8-wave forms without a row map, the split form
    "w_ws_196": _row("W", 14, [16], 6, 200, why="31 windows; three full tiles and MT = 1"),
    "w_ws_121": _row("W", 11, [17], 6, 192, why="33 windows; MT = 4 remainder"),
    "w_ws_100": _row("W", 10, [9, 8], 6, 230, why="32 windows; MT = 3"),
    "w_ws_81": _row("W", 9, [33], 6, 384, why="65 windows; MT = 2; a second feature tile"),
    "w_db_81": _row("W", 9, [16], 6, 200, knobs=WS0, why="31 windows"),
    "w_db_100": _row("W", 10, [17], 6, 192, knobs=WS0, why="33 windows"),
    "w_db_121": _row("W", 11, [49], 6, 384, knobs=WS0, why="97 windows; a second feature tile"),
    "w_db_196": _row("W", 14, [9, 8], 6, 230, knobs=WS0, why="32 windows"),
    "w_one_81": _row("W", 9, [17], 6, 230, knobs=WS0_DB0, why="33 windows"),
    "w_one_100": _row("W", 10, [16], 6, 384, knobs=WS0_DB0, why="31 windows; a second feature tile"),
    "w_one_121": _row("W", 11, [9, 8], 6, 200, knobs=WS0_DB0, why="32 windows"),
    "w_one_196": _row("W", 14, [33], 6, 192, knobs=WS0_DB0, why="65 windows"),
    "w_split_16": _row("W", 14, [5, 4], 6, 40, why="16 windows = KC"),
    "w_split_33": _row("W", 14, [17], 6, 47, why="33 windows = 2 KC + 1; nfun 48"),
    "w_split_49": _row("W", 14, [25], 6, 5, why="49 windows = 3 KC + 1"),
}
for _i, _n in enumerate(ROWS):
    ROWS[_n]["seed"] = 4100 + _i
ROW_NAMES = tuple(ROWS)


# ---- instantiation names, as tests/test_mfma_plan.py's inst() writes them
def SC(f32, nt):
    return "k_scores_mfma<F32=%d,NT=%d>" % (f32, nt)


def SW(mw, ntw):
    return "k_scores_mfma_ws<MW=%d,NTW=%d>" % (mw, ntw)


def E(x, nw, f32, mt, db=None):
    """k_expf_mfma unsplit: db defaults to what the default knobs give (the second image pair in the 8-wave form)"""
    db = int(nw == 8) if db is None else db
    return "k_expf_mfma<XROW=%d,NW=%d,KC=%d,F32=%d,MT=%d,DB=%d,MTW=%d>" % (x, nw, 32 if nw in (1, 8) else 64, f32, mt, db, 4 if nw == 8 and not f32 else 3)


def EW(x, mt):
    return "k_expf_mfma_ws<XROW=%d,MT=%d>" % (x, mt)


def SP(x, f32):
    return "k_expf_mfma<XROW=%d,NW=4,KC=16,F32=%d,SPLIT>" % (x, f32)


# name -> the instantiations the row is there for: those of its state calls (S rows) or of its transition calls (F and W rows;
# their state calls run a small one-wave form besides), under FAST and then FAST32.  tests/test_mfma_forms.py asks the probe.
REACHES = {
    "s_tail1": (SC(0, 1), E(0, 1, 0, 1), SC(1, 1), E(0, 1, 1, 1)),
    "s_tail3": (SC(0, 2), E(0, 1, 0, 2), SC(1, 2), E(0, 1, 1, 2)),
    "s_tail4": (SC(0, 3), E(0, 1, 0, 3), SC(1, 3), E(0, 1, 1, 3)),
    "s_tail5": (SC(0, 3), SC(0, 1), E(0, 1, 0, 3), E(0, 1, 0, 1), SC(1, 3), SC(1, 1), E(0, 1, 1, 3), E(0, 1, 1, 1)),
    "s_tail31": (SC(0, 1), E(0, 1, 0, 1), SC(1, 1), E(0, 1, 1, 1)),
    "s_tail32": (SC(0, 2), E(0, 1, 0, 2), SC(1, 2), E(0, 1, 1, 2)),
    "s_tail33": (SC(0, 3), E(0, 1, 0, 3), SC(1, 3), E(0, 1, 1, 3)),
    "s_nf48": (SC(0, 1), E(0, 1, 0, 1), SC(1, 1), E(0, 1, 1, 1)),
    "s_nf49": (SC(0, 2), E(0, 2, 0, 2), SC(1, 2), E(0, 2, 1, 2)),
    "s_nf96": (SC(0, 3), E(0, 2, 0, 3), SC(1, 3), E(0, 2, 1, 3)),
    "s_nf97": (SC(0, 1), E(0, 3, 0, 1), SC(1, 1), E(0, 3, 1, 1)),
    "s_nf144": (SC(0, 2), E(0, 3, 0, 2), SC(1, 2), E(0, 3, 1, 2)),
    "s_nf145": (SC(0, 3), E(0, 4, 0, 3), SC(1, 3), E(0, 4, 1, 3)),
    "s_nf192": (SC(0, 1), E(0, 4, 0, 1), SC(1, 1), E(0, 4, 1, 1)),
    "s_nf193": (SC(0, 3), SC(0, 1), EW(0, 4), SC(1, 3), SC(1, 1), E(0, 8, 1, 3), E(0, 8, 1, 1)),
    "s_nf384": (SC(0, 2), EW(0, 2), SC(1, 2), E(0, 8, 1, 2)),
    "s_nf385": (SC(0, 3), EW(0, 3), SC(1, 3), E(0, 8, 1, 3)),
    "s_nw1_mt2": (SC(0, 2), E(0, 1, 0, 2), SC(1, 2), E(0, 1, 1, 2)),
    "s_nw2_mt1": (SC(0, 1), E(0, 2, 0, 1), SC(1, 1), E(0, 2, 1, 1)),
    "s_nw3_mt3": (SC(0, 3), E(0, 3, 0, 3), SC(1, 3), E(0, 3, 1, 3)),
    "s_nw4_mt2": (SC(0, 2), E(0, 4, 0, 2), SC(1, 2), E(0, 4, 1, 2)),
    "s_wide_mt1": (SC(0, 3), SC(0, 2), EW(0, 4), EW(0, 1), SC(1, 3), SC(1, 2), E(0, 8, 1, 3), E(0, 8, 1, 2)),
    "s_chunks": (SC(0, 1), E(0, 1, 0, 1), SC(1, 1), E(0, 1, 1, 1)),
    "s_nobias": (SC(0, 2), E(0, 1, 0, 2), SC(1, 2), E(0, 1, 1, 2)),
    "f_nw1_mt1": (SC(0, 1), E(1, 1, 0, 1), SC(1, 1), E(1, 1, 1, 1)),
    "f_nw1_mt2": (SC(0, 2), E(1, 1, 0, 2), SC(1, 2), E(1, 1, 1, 2)),
    "f_nw1_mt3": (SC(0, 3), E(1, 1, 0, 3), SC(1, 3), E(1, 1, 1, 3)),
    "f_nw1_full": (SC(0, 3), SC(0, 1), E(1, 1, 0, 3), E(1, 1, 0, 1), SC(1, 3), SC(1, 1), E(1, 1, 1, 3), E(1, 1, 1, 1)),
    "f_nw2_mt1": (SC(0, 1), E(1, 2, 0, 1), SC(1, 1), E(1, 2, 1, 1)),
    "f_nw2_mt2": (SC(0, 2), E(1, 2, 0, 2), SC(1, 2), E(1, 2, 1, 2)),
    "f_nw2_mt3": (SC(0, 3), E(1, 2, 0, 3), SC(1, 3), E(1, 2, 1, 3)),
    "f_nw3_mt1": (SC(0, 1), E(1, 3, 0, 1), SC(1, 1), E(1, 3, 1, 1)),
    "f_nw3_mt2": (SC(0, 2), E(1, 3, 0, 2), SC(1, 2), E(1, 3, 1, 2)),
    "f_nw3_mt3": (SC(0, 3), E(1, 3, 0, 3), SC(1, 3), E(1, 3, 1, 3)),
    "f_nw4_mt1": (SC(0, 1), E(1, 4, 0, 1), SC(1, 1), E(1, 4, 1, 1)),
    "f_nw4_mt2": (SC(0, 2), E(1, 4, 0, 2), SC(1, 2), E(1, 4, 1, 2)),
    "f_nw4_mt3": (SC(0, 3), E(1, 4, 0, 3), SC(1, 3), E(1, 4, 1, 3)),
    "f_ws_81": (SC(0, 3), EW(1, 4), EW(1, 2), SC(1, 3), E(1, 8, 1, 3)),
    "f_ws_100": (SW(2, 7), EW(1, 4), EW(1, 3), SC(1, 3), SC(1, 1), E(1, 8, 1, 3), E(1, 8, 1, 1)),
    "f_ws_121": (SW(4, 3), SC(0, 2), EW(1, 4), SC(1, 3), SC(1, 2), E(1, 8, 1, 3), E(1, 8, 1, 2)),
    "f_ws_196": (SW(4, 3), SW(2, 7), EW(1, 4), EW(1, 1), SC(1, 3), SC(1, 1), E(1, 8, 1, 3), E(1, 8, 1, 1)),
    "f_db_81": (SC(0, 3), E(1, 8, 0, 4), E(1, 8, 0, 2), SC(1, 3), E(1, 8, 1, 3)),
    "f_db_100": (SW(2, 7), E(1, 8, 0, 4), E(1, 8, 0, 3), SC(1, 3), SC(1, 1), E(1, 8, 1, 3), E(1, 8, 1, 1)),
    "f_db_121": (SW(4, 3), SC(0, 2), E(1, 8, 0, 4), SC(1, 3), SC(1, 2), E(1, 8, 1, 3), E(1, 8, 1, 2)),
    "f_db_196": (SW(4, 3), SW(2, 7), E(1, 8, 0, 4), E(1, 8, 0, 1), SC(1, 3), SC(1, 1), E(1, 8, 1, 3), E(1, 8, 1, 1)),
    "f_one_81": (SC(0, 3), E(1, 8, 0, 4, db=0), E(1, 8, 0, 2, db=0), SC(1, 3), E(1, 8, 1, 3, db=0)),
    "f_one_100": (SW(2, 7), E(1, 8, 0, 4, db=0), E(1, 8, 0, 3, db=0), SC(1, 3), SC(1, 1), E(1, 8, 1, 3, db=0), E(1, 8, 1, 1, db=0)),
    "f_one_121": (SW(4, 3), SC(0, 2), E(1, 8, 0, 4, db=0), SC(1, 3), SC(1, 2), E(1, 8, 1, 3, db=0), E(1, 8, 1, 2, db=0)),
    "f_one_196": (SW(4, 3), SW(2, 7), E(1, 8, 0, 4, db=0), E(1, 8, 0, 1, db=0), SC(1, 3), SC(1, 1), E(1, 8, 1, 3, db=0), E(1, 8, 1, 1, db=0)),
    "f_ws_144": (SW(4, 3), SC(0, 3), EW(1, 4), EW(1, 1), SC(1, 3), E(1, 8, 1, 3)),
    "f_ws_100_191": (SC(0, 3), SC(0, 1), E(1, 4, 0, 3), E(1, 4, 0, 1), SC(1, 3), SC(1, 1), E(1, 4, 1, 3), E(1, 4, 1, 1)),
    "f_noscws_121": (SC(0, 3), SC(0, 2), EW(1, 4), SC(1, 3), SC(1, 2), E(1, 8, 1, 3), E(1, 8, 1, 2)),
    "f_chunks": (SC(0, 3), EW(1, 4), EW(1, 2), SC(1, 3), E(1, 8, 1, 3)),
    "f_split_15": (SC(0, 3), SC(0, 1), SP(1, 0), SC(1, 3), SC(1, 1), SP(1, 1)),
    "f_split_17": (SC(0, 3), SC(0, 1), SP(1, 0), SC(1, 3), SC(1, 1), SP(1, 1)),
    "f_nosplit_169": (SC(0, 3), SC(0, 2), E(1, 1, 0, 3), E(1, 1, 0, 2), SC(1, 3), SC(1, 2), E(1, 1, 1, 3), E(1, 1, 1, 2)),
    "w_ws_196": (SW(4, 3), SW(2, 7), EW(0, 4), EW(0, 1), SC(1, 3), SC(1, 1), E(0, 8, 1, 3), E(0, 8, 1, 1)),
    "w_ws_121": (SW(4, 3), SC(0, 2), EW(0, 4), SC(1, 3), SC(1, 2), E(0, 8, 1, 3), E(0, 8, 1, 2)),
    "w_ws_100": (SW(2, 7), EW(0, 4), EW(0, 3), SC(1, 3), SC(1, 1), E(0, 8, 1, 3), E(0, 8, 1, 1)),
    "w_ws_81": (SC(0, 3), EW(0, 4), EW(0, 2), SC(1, 3), E(0, 8, 1, 3)),
    "w_db_81": (SC(0, 3), E(0, 8, 0, 4), E(0, 8, 0, 2), SC(1, 3), E(0, 8, 1, 3)),
    "w_db_100": (SW(2, 7), E(0, 8, 0, 4), E(0, 8, 0, 3), SC(1, 3), SC(1, 1), E(0, 8, 1, 3), E(0, 8, 1, 1)),
    "w_db_121": (SW(4, 3), SC(0, 2), E(0, 8, 0, 4), SC(1, 3), SC(1, 2), E(0, 8, 1, 3), E(0, 8, 1, 2)),
    "w_db_196": (SW(4, 3), SW(2, 7), E(0, 8, 0, 4), E(0, 8, 0, 1), SC(1, 3), SC(1, 1), E(0, 8, 1, 3), E(0, 8, 1, 1)),
    "w_one_81": (SC(0, 3), E(0, 8, 0, 4, db=0), E(0, 8, 0, 2, db=0), SC(1, 3), E(0, 8, 1, 3, db=0)),
    "w_one_100": (SW(2, 7), E(0, 8, 0, 4, db=0), E(0, 8, 0, 3, db=0), SC(1, 3), SC(1, 1), E(0, 8, 1, 3, db=0), E(0, 8, 1, 1, db=0)),
    "w_one_121": (SW(4, 3), SC(0, 2), E(0, 8, 0, 4, db=0), SC(1, 3), SC(1, 2), E(0, 8, 1, 3, db=0), E(0, 8, 1, 2, db=0)),
    "w_one_196": (SW(4, 3), SW(2, 7), E(0, 8, 0, 4, db=0), E(0, 8, 0, 1, db=0), SC(1, 3), SC(1, 1), E(0, 8, 1, 3, db=0), E(0, 8, 1, 1, db=0)),
    "w_split_16": (SC(0, 3), SC(0, 1), SP(0, 0), SC(1, 3), SC(1, 1), SP(0, 1)),
    "w_split_33": (SC(0, 3), SC(0, 1), SP(0, 0), SC(1, 3), SC(1, 1), SP(0, 1)),
    "w_split_49": (SC(0, 3), SC(0, 1), SP(0, 0), SC(1, 3), SC(1, 1), SP(0, 1)),
}

# the instantiations no row runs (tests/test_mfma_forms.py prints and checks this list): none -- see the module text
UNREACHED = ()


def calls(name, f32):
    """the launcher calls of a row under a precision, as probe arguments: ("scores", n_out, nfe, f32) and
    ("counts", n_out, nfun, f32, has_xrow)"""
    r = ROWS[name]
    L, b = r["L"], int(r["bias"])
    out = [("scores", L, r["nsfe"], f32), ("counts", L, r["nsfe"] + b, f32, 0)]
    if r["site"] != "S":
        out += [("scores", L * L, r["ntfe"], f32), ("counts", L * L, r["ntfe"] + b, f32, int(r["site"] == "F"))]
    return out


def n_windows(Ts):
    return sum(orc_num_segs(T) for T in Ts)


def orc_num_segs(T):
    return T * (T + 1) // 2 if T < D else D * (D + 1) // 2 + (T - D) * D


class FormCase:
    """the windows, labels, weights and configurations of a row; the same for the oracle and the engine"""

    def __init__(self, name, precision=0):
        r = ROWS[name]
        self.name, self.row = name, r
        L, nsfe, ntfe = r["L"], r["nsfe"], r["ntfe"]
        self.L, self.Ts = L, list(r["Ts"])
        sfs, sfe = SFS, SFS + nsfe - 1
        tfs = sfe + 1 + GAP
        tfe = tfs + ntfe - 1
        self.F = (tfe if ntfe else sfe) + 1 + 3
        rng = np.random.RandomState(r["seed"])
        inside = np.zeros(self.F, dtype=bool)
        inside[sfs:sfe + 1] = True
        if ntfe:
            inside[tfs:tfe + 1] = True
        self.inside = inside
        scale = np.where(inside, 1.0, JUNK)
        self.windows = [((rng.random_sample((orc_num_segs(T), self.F)) * 2.0 - 1.0) * scale).astype(np.float32) for T in self.Ts]
        self.labels = [synth.group_labels(synth.frame_labels(rng, T, L, D), D, L) for T in self.Ts]
        mt = orc.STDSEG_NO_DUR if r["site"] == "W" else orc.STDSEG_NO_DUR_NO_SEGTRANSFTR
        kw = dict(model_type=mt, L=L, D=D, F=self.F, sfs=sfs, sfe=sfe, use_state_bias=r["bias"], use_trans_bias=r["bias"],
                  state_bias_val=STATE_BIAS, trans_bias_val=TRANS_BIAS)
        if ntfe:
            kw.update(use_trans_ftrs=True, tfs=tfs, tfe=tfe)
        self.ocfg = orc.config(**kw)
        self.olay = orc.Layout(self.ocfg)
        self.gcfg = scrf_amd.make_config(precision=precision, **kw)
        lay = self.olay
        self.nsf, self.ntf = lay.num_state_funcs, lay.num_trans_funcs
        assert self.nsf == nsfe + int(r["bias"]) and self.ntf == ntfe + int(r["bias"]), (self.nsf, self.ntf)
        # owner of every weight: the state block (label, column) and the transition block (label pair, column)
        n = lay.lambda_len
        self.is_state = np.zeros(n, dtype=bool)
        self.owner = np.full((n, 2), -1, dtype=np.int64)
        for l in range(L):
            i = int(lay.state_idx[l])
            self.is_state[i:i + self.nsf] = True
            self.owner[i:i + self.nsf, 0] = l
            self.owner[i:i + self.nsf, 1] = np.arange(self.nsf)
        for pc in range(L * L):
            i = int(lay.trans_idx[pc])
            if self.ntf and i != 0xffffffff:
                self.owner[i:i + self.ntf, 0] = pc
                self.owner[i:i + self.ntf, 1] = np.arange(self.ntf)
        assert (self.owner[:, 0] >= 0).all()
        s = np.where(self.is_state, min(0.3, 3.0 / np.sqrt(max(1, nsfe))), min(0.3, 3.0 / np.sqrt(max(1, ntfe))))
        self.lam = rng.normal(0.0, 1.0, n) * s

    def describe(self, i):
        """weight index -> text: the block, the label or label pair, the feature column (the last column is the bias)"""
        o, col = int(self.owner[i, 0]), int(self.owner[i, 1])
        if self.is_state[i]:
            return "state label %d column %d of %d" % (o, col, self.nsf)
        return "transition %d -> %d (output %d) column %d of %d" % (o // self.L, o % self.L, o, col, self.ntf)

    def engine(self):
        e = scrf_amd.Engine(self.gcfg)
        e.set_lambda(self.lam)
        return e

    def batch(self, eng):
        return eng.batch_from_windows(self.windows, self.Ts, self.labels)

    def oracle_gradient(self):
        g = np.zeros(self.olay.lambda_len)
        numer, zx = [], []
        fn = orc.segtrans_build_gradient if self.row["site"] == "W" else orc.seg_build_gradient
        for u, T in enumerate(self.Ts):
            rc, g, n, z = fn(self.ocfg, self.olay, self.lam, self.windows[u], self.labels[u], T, grad=g)
            assert rc == 0, rc
            numer.append(n); zx.append(z)
        return g, np.array(numer), np.array(zx)


@functools.lru_cache(maxsize=None)
def reference(name):
    """the oracle's gradient, numerators and Zx of a row; computed once and not modified"""
    g, n, z = FormCase(name).oracle_gradient()
    for a in (g, n, z):
        a.setflags(write=False)
    return g, n, z
