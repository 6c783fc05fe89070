// scrf_mfma_plan.h -- which template instantiations the two MFMA contractions of scrf_mfma.hip launch, and over which
// outputs.  Host-only (no HIP), like scrf_knobs.h: launch_scores_mfma and launch_expf_mfma call the two functions below
// and switch on the result, and tests/host/mfma_plan_probe.cpp prints the same result without a GPU, so what the probe
// says about a shape is what the launcher does.  Every threshold of the choice lives here and only here; the tile
// geometry the kernels and the choice share (outputs per workgroup, LDS image sizes) is defined here for both.
#ifndef SCRF_MFMA_PLAN_H_
#define SCRF_MFMA_PLAN_H_

#include <stddef.h>
#include <stdint.h>

#include "scrf_knobs.h"

// ---- k_scores_mfma (single-role) and k_scores_mfma_ws (wave-specialised)
#define SM_ROWS 256  // rows per workgroup (4 waves x 4 M-tiles)
#define SM_KC 32     // features per staged chunk (8 MFMA k-steps)
#define SM_XS 34     // float row stride of the X image (== 2 mod 32: conflict-free A fragments)
#define SM_NO 48     // outputs per workgroup (3 N-tiles)
#define SM_WS 49     // double row stride of the lambda image [k][SM_WS]: transposed stores stay <= 2-way
#define SW_ROWS 256
#define SW_NO 96     // outputs per workgroup of k_scores_mfma_ws<4, 3>
#define SW_NO7 112   // ... and of <2, 7>
#define SW_WS 113
#define SW_IMG (sizeof(float) * SW_ROWS * SM_XS + sizeof(double) * SM_KC * SW_WS)
#define SW_MIN_NFE 192   // features from which the role split pays (below: with only a few 32-feature chunks it is all prologue)

// ---- k_expf_mfma (plain, double-buffered, split) and k_expf_mfma_ws
// M-tiles (16 outputs each) of a workgroup tile of the unsplit form.  f64: 4 -- a wavefront carries 64 outputs x 48 feature
// columns, 12 MFMAs per 7 operand loads and 96 per barrier (3: 9 per 6, 72 per barrier; measured at the TIMIT transition
// counts 14.8 -> 13.5 ms, config 5's state counts 96.6 -> 91.1 ms; 231 VGPRs, no spills).  The f32 form spills at 4 and stays at 3.
#ifndef EM_MTF
#define EM_MTF 4
#endif
// (the narrow forms keep 3: with 1-4 wavefronts per workgroup a 64-wide posterior image means a third more staging
// registers per thread -- the frame model's 40-column count contraction went from 0.58 to 1.54 ms with it)
#define EM_MTW(F32, NW) (((F32) || (NW) < 8) ? 3 : EM_MTF)
#define EM_SPLIT_NO 48        // outputs per wavefront of the split form (3 M-tiles)
#define EM_SPLIT_NW 4         // wavefronts of the split form
#define EM_SPLIT_KC 16        // rows per staged chunk of the split form
#define EM_NF 48              // feature columns per wavefront (3 N-tiles)
// row stride (doubles) of the posterior image [k][outputs]: == 16 (mod 32), so that the two k rows a 32-lane half of a
// ds_read_b64 fragment read covers fall on disjoint bank halves (a stride of 64 or 192 doubles puts them on the same banks)
// (only the 64-wide image of the wide form is padded: the split form's 192-wide image measured FASTER unpadded, 4.8 against
// 6.6 ms at the per-window transition counts of STDSEG_NO_DUR)
constexpr int em_rss(int no) { return no == 64 ? 80 : no; }
#define EW_KC 32
#define EW_NO 64
#define EW_NF 384
#define EW_XS (EW_NF + 16)
#define EW_RS 80   // em_rss(EW_NO)
#define EW_IMG (sizeof(double) * EW_KC * EW_RS + sizeof(float) * EW_KC * EW_XS)

enum ScrfMfmaKernel {
  SCRF_MK_SINGLE,   // k_scores_mfma<F32, NT>
  SCRF_MK_WS,       // k_scores_mfma_ws<MW, NTW> / k_expf_mfma_ws<HAS_XROW, MT>
  SCRF_MK_PLAIN,    // k_expf_mfma<HAS_XROW, NW, KC, F32, 0, MT, 0, MTW>: one LDS image pair
  SCRF_MK_DB,       // k_expf_mfma<HAS_XROW, NW, KC, F32, 0, MT, 1, MTW>: two LDS image pairs
  SCRF_MK_SPLIT,    // k_expf_mfma<HAS_XROW, 4, 16, F32, 1>: the wavefronts share a feature tile and split the outputs
};
inline const char* scrf_mfma_kernel_name(int k) {
  static const char* const names[] = {"single", "ws", "plain", "db", "split"};
  return k >= 0 && k < 5 ? names[k] : "?";
}

// One kernel launch.  Its workgroup tiles own the outputs [o_base + i * o_step, o_base + (i + 1) * o_step), i < gy, cut
// at n_out; of a tile's o_step outputs the first 16 NT (scores) or 16 MT (counts) are computed.  Template arguments a
// kernel does not have are 0.  Scores: the grid is gy workgroups per 256-row tile, gx is 1.  Counts: gx workgroups of
// 48 NW feature columns (48 in the split form) per output tile and row chunk.
struct ScrfMfmaLaunch {
  int kernel;                   // ScrfMfmaKernel
  int f32;
  int nt, mw, ntw;              // scores: NT of the single-role kernel; <MW, NTW> of the wave-specialised one
  int has_xrow, nw, kc, mt, mtw, db;   // counts
  uint32_t o_base, gy, o_step, gx;
  size_t lds;                   // dynamic LDS bytes
};
#define SCRF_MFMA_MAX_LAUNCHES 4

inline ScrfMfmaLaunch scrf_mfma_score_launch(int kernel, int f32, int nt, int mw, int ntw, uint32_t o_base, uint32_t gy, uint32_t o_step, size_t lds) {
  ScrfMfmaLaunch p = {};
  p.kernel = kernel; p.f32 = f32; p.nt = nt; p.mw = mw; p.ntw = ntw;
  p.o_base = o_base; p.gy = gy; p.o_step = o_step; p.gx = 1; p.lds = lds;
  return p;
}

// launch_scores_mfma: n_out outputs over nfe features (sp.nfe).  Returns the number of launches written to out.
inline int scrf_scores_mfma_plan(const ScrfKnobs& kn, uint32_t n_out, uint32_t nfe, int f32, ScrfMfmaLaunch out[SCRF_MFMA_MAX_LAUNCHES]) {
  int n = 0;
  if (n_out == 0) return 0;
  uint32_t o_base = 0;
  // SCRF_SCORES_MFMA_WS=0 for A/B runs (from 192 features on: with only a few 32-feature chunks the role split is all prologue -- the 40-feature per-window
  // transition scores of STDSEG_NO_DUR: 5.8 ms single-role, 6.1 split)
  if (!f32 && kn.scores_mfma_ws && n_out >= SW_NO && nfe >= SW_MIN_NFE) {
    // the wave-specialised form: 16 T outputs as a tiles of 96 and b tiles of 112 (T = 6a + 7b, fewest masked outputs); when
    // the count does not split that way, the whole 96-output tiles go here and the rest to the single-role kernels below
    const uint32_t T = (n_out + 15) / 16;
    uint32_t a = n_out / SW_NO, bt = 0;
    for (uint32_t b7 = 0; b7 < 6 && 7 * b7 <= T; b7++)
      if ((T - 7 * b7) % 6 == 0) { a = (T - 7 * b7) / 6; bt = b7; break; }
    if (a) out[n++] = scrf_mfma_score_launch(SCRF_MK_WS, 0, 0, 4, 3, 0u, a, SW_NO, 2 * SW_IMG);
    if (bt) out[n++] = scrf_mfma_score_launch(SCRF_MK_WS, 0, 0, 2, 7, a * SW_NO, bt, SW_NO7, 2 * SW_IMG);
    o_base = a * SW_NO + bt * SW_NO7;
    if (o_base >= n_out) return n;
  }
  const uint32_t left = n_out - o_base;
  const uint32_t n_full = left / SM_NO, rem = left % SM_NO;
  if (n_full) out[n++] = scrf_mfma_score_launch(SCRF_MK_SINGLE, f32, 3, 0, 0, o_base, n_full, SM_NO, 0);
  // the outputs past the last full 48: a launch whose workgroups carry only the N-tiles that hold outputs
  if (rem) out[n++] = scrf_mfma_score_launch(SCRF_MK_SINGLE, f32, rem > 32 ? 3 : rem > 16 ? 2 : 1, 0, 0, o_base + n_full * SM_NO, 1u, SM_NO, 0);
  return n;
}

// wavefronts per workgroup and rows per staged chunk of the unsplit count forms, by the 48-column wave tiles the
// feature functions need.  NW = 8 covers 384 columns (the full 338-wide state block of config 2 in one workgroup, so R
// is read once); KC = 32 for the wide tile, 64 for narrow tiles so that the staging/barrier cost per MFMA stays low
// when few wavefronts share one R tile.
// (64-row chunks for the 8-wave form were tried: 256 VGPRs + 336 bytes of spills)
// (two 4-wave workgroups per CU with 64-row chunks instead: 18.1 ms against 14.4 at the TIMIT transition counts)
inline void scrf_expf_mfma_waves(uint32_t nfun, int* nw, int* kc) {
  const uint32_t tiles = (nfun + EM_NF - 1) / EM_NF;
  if (tiles <= 1) { *nw = 1; *kc = 32; }
  else if (tiles <= 4) { *nw = (int)tiles; *kc = 64; }
  else { *nw = 8; *kc = 32; }
}
// few feature functions (<= 48) and many outputs: 4 wavefronts share the feature tile and split 192 outputs
inline bool scrf_expf_mfma_is_split(uint32_t n_out, uint32_t nfun) { return nfun <= EM_NF && n_out >= EM_SPLIT_NW * EM_SPLIT_NO; }

// launch_expf_mfma: n_out outputs over nfun feature functions (sp.nfun(): the features and the bias column).
inline int scrf_expf_mfma_plan(const ScrfKnobs& kn, uint32_t n_out, uint32_t nfun, int f32, int has_xrow, ScrfMfmaLaunch out[SCRF_MFMA_MAX_LAUNCHES]) {
  int n = 0;
  if (n_out == 0) return 0;
  ScrfMfmaLaunch p = {};
  p.f32 = f32 ? 1 : 0;
  p.has_xrow = has_xrow ? 1 : 0;
  if (scrf_expf_mfma_is_split(n_out, nfun)) {
    p.kernel = SCRF_MK_SPLIT;
    p.nw = EM_SPLIT_NW; p.kc = EM_SPLIT_KC; p.mt = 3; p.mtw = 3;
    p.o_step = EM_SPLIT_NO * EM_SPLIT_NW;
    p.gx = 1; p.gy = (n_out + p.o_step - 1) / p.o_step;
    p.lds = sizeof(double) * p.kc * em_rss((int)p.o_step) + sizeof(float) * p.kc * (EM_NF + 16);
    out[n++] = p;
    return n;
  }
  scrf_expf_mfma_waves(nfun, &p.nw, &p.kc);
  p.mtw = EM_MTW(p.f32, p.nw);
  const uint32_t NO = 16 * (uint32_t)p.mtw;
  p.o_step = NO;
  p.gx = (nfun + EM_NF * p.nw - 1) / (EM_NF * p.nw);
  const size_t sm = sizeof(double) * p.kc * em_rss((int)NO) + sizeof(float) * p.kc * (EM_NF * p.nw + 16);
  // the 8-wave workgroup has its CU to itself: room for a second image pair (DB), and in f64 for the role split (which
  // always keeps two pairs and has no DB argument)
  if (p.nw == 8 && !p.f32 && p.kc == EW_KC && NO == EW_NO && kn.expf_mfma_ws) { p.kernel = SCRF_MK_WS; p.db = 0; p.lds = 2 * EW_IMG; }
  else if (p.nw == 8 && kn.expf_db) { p.kernel = SCRF_MK_DB; p.db = 1; p.lds = 2 * sm; }
  else { p.kernel = SCRF_MK_PLAIN; p.db = 0; p.lds = sm; }
  const uint32_t n_full = n_out / NO, rem = n_out % NO;
  if (n_full) {
    p.mt = p.mtw; p.o_base = 0; p.gy = n_full;
    out[n++] = p;
  }
  // the outputs past the last full tile: workgroups that carry only the M-tiles holding outputs
  // (a mixed tiling of the outputs -- 200 = 64 + 3 x 48 instead of 3 x 64 + a thin 8-output launch -- was measured at config 5:
  // 81.8 against 80.0 ms; the thin launch costs less than the thirteenth M-tile)
  if (rem) {
    p.mt = (int)((rem + 15) / 16); p.o_base = n_full * NO; p.gy = 1;
    out[n++] = p;
  }
  return n;
}

// workgroups launch_expf_mfma starts per row chunk when it takes the 8-wavefront form (one workgroup per CU), else 0:
// the engine sizes the number of row chunks so that the launch fills whole rounds of the chip's CUs
inline uint32_t expf_mfma_wide_tiles(uint32_t n_out, uint32_t nfun, int f32) {
  int nw, kc;
  scrf_expf_mfma_waves(nfun, &nw, &kc);
  if (nw < 8) return 0;   // split and narrow forms: several workgroups per CU, no round structure to fit
  const uint32_t gx = (nfun + EM_NF * 8 - 1) / (EM_NF * 8);
  const uint32_t NO = 16 * (uint32_t)EM_MTW(f32, 8);
  return gx * ((n_out + NO - 1) / NO);
}

#endif  // SCRF_MFMA_PLAN_H_
