// scrf_fused_plan.h -- which template instantiations the launchers of scrf_fused.hip start, with which grid and how much
// LDS.  Host-only (no HIP), like scrf_mfma_plan.h: every launch_* of the fused kernels calls one function below (or is
// handed its result by the engine) and switches on the fields, and tests/host/fused_plan_probe.cpp prints the same
// result without a GPU, so what the probe says about a shape is what the launcher does.  Every threshold of the choice
// lives here and only here; the tile geometry the kernels and the choice share is defined here for both.
// (<math.h>: fu_sample_step's ceilf.)
#ifndef SCRF_FUSED_PLAN_H_
#define SCRF_FUSED_PLAN_H_

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "scrf_dp_plan.h"   // SCRF_HD, walk_segments
#include "scrf_knobs.h"

// the layout fields the choice reads (ScrfLayout's, scrf_common.h; fused_shape() in scrf_kernels.h copies them)
struct ScrfFusedShape { uint32_t L, D; int32_t use_sb; };

#define SCRF_FUSED_LDS_BYTES (160 * 1024)   // LDS of a workgroup (SCRF_LDS_BYTES of scrf_common.h)

// ---- tile geometry
#define SCRF_FUSED_ROWS_SCORES 256
#define SCRF_FUSED_ROWS_EXPF 76
#define FU_GC 40        // columns per dense chunk of the score kernel
#define FU_XS 42        // float row stride of the chunk image (== 2 mod 4: conflict-free A fragments)
#define FU_WS 49        // row stride of the transposed lambda image
#define FU_ROWS SCRF_FUSED_ROWS_SCORES
#define FE_ROWS SCRF_FUSED_ROWS_EXPF
#define FE_RSF 80       // float row stride of the R image in the f32 form: == 16 (mod 32), the b32 counterpart
#define FE_RS 48        // double row stride of the R image: 96 dwords = 32 (mod 64), so the two k-rows a 32-lane half of a
                        // ds_read_b64 A-fragment covers fall on disjoint banks (50 overlapped four of them)
#define FU_DS 50        // double row stride of the P image and of the duration-weight table: 25 16-byte slots, odd, so
                        // that the rows of consecutive frames / durations a ds_read_b128 lane group gathers start on
                        // distinct slots (48 would put them on two)
#define FU_NT 512       // threads of k_scores_fused
#define FE_NT 256       // ... of k_expf_fused
#define FW_NT 512       // ... of k_expf_fused_ws
#define FW_ROWS_BIG 100
#define PF_MT 4      // output tiles per wavefront (64 outputs)
#ifndef FU_EXPTAB
#define FU_EXPTAB 0     // 1: table-based exp in the epilogue (14 instructions + a gathered LDS read instead of 21; measured
                        // equal -- the epilogue is not instruction-bound -- and the table costs 2 KB of LDS and bank conflicts)
#endif
#define FU_EXPT_N 256
#define FU_REC_BYTES 16   // a row record of the score tile (uint4)

SCRF_HD inline uint32_t fu_sample_step(uint32_t d, int k) {
  const float ot = (float)((double)d * 0.1);
  return (uint32_t)ceilf(ot * (float)(2 * k + 1)) - 1u;
}
// rows of the staged P image: block k holds the frames sample position k can reach, TB + off_k(D) of them
SCRF_HD inline uint32_t fu_p_rows(uint32_t D, uint32_t TB) {
  uint32_t n = 0;
  for (int k = 0; k < 5; k++) n += TB + (D - 1 - fu_sample_step(D, k));
  return n;
}
// (the LA form, k_scores_fused: a sixth block with the prefix sums of the frames t0 - D .. t0 + nfr - 1)
SCRF_HD inline uint32_t fu_p_rows_la(uint32_t D, uint32_t TB) { return fu_p_rows(D, TB) + TB + D; }

// ---- k_scores_fused
inline size_t fused_scores_smem_tb(uint32_t W, uint32_t D, uint32_t TB) {
  const uint32_t nfmax = TB + D - 1;
  size_t opn = sizeof(float) * (FU_ROWS + 1) * FU_XS + sizeof(double) * FU_GC * FU_WS + sizeof(float) * nfmax * W;
  const uint32_t npr = fu_p_rows_la(D, TB);   // one tile plan for every form of the kernel
  const size_t pb = sizeof(double) * npr * FU_DS;
  if (pb > opn) opn = pb;
  opn = (opn + 15) & ~(size_t)15;
  // rbase and rowmap in whole 16-byte chunks (the kernel's layout = k_tile_tables' layout in memory).  The spare at the
  // end shrinks by what that padding took over 4-entry padding (0, 8 or 16 of its 16 bytes), so the total -- and with it
  // the tile plan -- is what it was before the tables were padded.
  const size_t t4 = sizeof(uint16_t) * (((TB + 3) & ~3u) + ((npr + 3) & ~3u));
  const size_t t8 = sizeof(uint16_t) * (((TB + 7) & ~7u) + ((npr + 7) & ~7u));
  const size_t spare = 16 - (t8 - t4);
  return opn + sizeof(double) * D * FU_DS + (size_t)FU_REC_BYTES * FU_ROWS + t8 + (FU_EXPTAB ? sizeof(double) * FU_EXPT_N : 0) + spare;
}
// frames per score tile: as many whole frames as give <= 256 rows and keep the workgroup's LDS
// (the staged P rows grow with TB + D - 1) within 80 KB, i.e. two workgroups per CU; 0 = no fit
inline uint32_t fused_scores_tb(uint32_t W, uint32_t D) {
  for (uint32_t TB = FU_ROWS / D; TB >= 1; TB--)
    if (fused_scores_smem_tb(W, D, TB) <= 80 * 1024) return TB;
  // long durations with wide frames (D = 32 at W = 39): one workgroup per CU, as many frames as fit
  for (uint32_t TB = FU_ROWS / D; TB >= 1; TB--)
    if (fused_scores_smem_tb(W, D, TB) <= 156 * 1024) return TB;
  return 0;
}
inline size_t fused_tile_table_bytes(uint32_t D, uint32_t TB) {
  return (size_t)FU_REC_BYTES * FU_ROWS + sizeof(uint16_t) * (((TB + 7) & ~7u) + ((fu_p_rows_la(D, TB) + 7) & ~7u)) + 64;
}
inline size_t fused_dur_table_doubles(const ScrfFusedShape& lay) { return (size_t)((lay.L + 47) / 48) * lay.D * FU_DS; }

// the duration classes of k_scores_fused and the count kernels
inline int fused_dmax3(uint32_t D) { return D <= 12 ? 12 : D <= 25 ? 25 : 40; }
// ... and of the walks (k_lin_z, k_lin_z5, k_post_z)
inline int fused_dmax5(uint32_t D) { return D <= 8 ? 8 : D <= 16 ? 16 : D <= 25 ? 25 : D <= 32 ? 32 : 40; }

// k_scores_fused<DMAX, F32, DEC, LA, DMA> over grid (tiles, gy), `threads` threads, `lds` bytes.  tb: whole frames per
// tile (0: the shape has no plan).  smax: the epilogue can write exp(S - smax) and the row maxima (a row spans several
// workgroups when L > 48: the caller runs k_exp_rows instead).
struct ScrfFusedScoresPlan { int dmax, f32, dec, la, dma, smax; uint32_t tb, gy, threads; size_t lds; };
// la (SCRF_PREC_FASTLIN, fp64 only): P carries 6 groups per frame, the sixth summed along the utterance (k_avg_prefix).
// dec: the decode form (fp64, no la).  The LDS-DMA form (SCRF_SCORES_DMA=0: off) copies both launch tables, so it needs
// both: have_dtab / have_rtab say whether the launch has k_dur_table's and k_tile_tables' outputs.
inline ScrfFusedScoresPlan fused_scores_plan(const ScrfKnobs& kn, const ScrfFusedShape& lay, uint32_t W, int f32, int dec, int la,
                                             int have_dtab, int have_rtab) {
  ScrfFusedScoresPlan p = {};
  p.dmax = fused_dmax3(lay.D);
  p.dec = dec ? 1 : 0;
  p.la = (la && !dec) ? 1 : 0;
  p.f32 = (f32 && !dec && !la) ? 1 : 0;
  p.dma = (kn.scores_dma && have_dtab && have_rtab) ? 1 : 0;
  p.smax = (!dec && lay.L <= 48) ? 1 : 0;
  p.tb = fused_scores_tb(W, lay.D);
  p.gy = (lay.L + 47) / 48;
  p.threads = FU_NT;
  p.lds = p.tb ? fused_scores_smem_tb(W, lay.D, p.tb) : 0;
  return p;
}

// ---- the walks over an utterance: k_lin_z, k_lin_z5, k_post_z
// k_lin_z<DMAX> / k_lin_z5<DMAX> / k_post_z<DMAX, LA, RW, SPLIT> over grid (gx, gy, nz).  nz > 1: every utterance's
// walk is cut into nz segments of seg_len frames that ADD into Z, which the launcher clears first (clear_z).
struct ScrfFusedWalkPlan { int dmax, la, rw, split, seg_len, clear_z; uint32_t nz, gx, gy; };

inline ScrfFusedWalkPlan fused_lin_z_plan(const ScrfFusedShape& lay, uint32_t n_utts) {
  ScrfFusedWalkPlan p = {};
  p.dmax = fused_dmax5(lay.D);
  p.nz = 1; p.gx = n_utts; p.gy = (lay.L + 63) / 64;
  return p;
}
// frame segments per utterance so that the launch has about 1024 workgroups, none shorter than 2 D frames
inline uint32_t lin_z5_segments(uint32_t n_utts, uint32_t L, uint32_t D, uint32_t t_max, int* seg_len) {
  const uint64_t wgs = (uint64_t)n_utts * ((L + 63) / 64);
  uint32_t want = wgs >= 1024 ? 1 : (uint32_t)((1024 + wgs - 1) / wgs);
  int sl = (int)((t_max + want - 1) / (want ? want : 1));
  if (sl < (int)(2 * D)) sl = (int)(2 * D);
  if (sl < 1) sl = 1;
  *seg_len = sl;
  const uint32_t nz = (t_max + sl - 1) / sl;
  return nz ? nz : 1;
}
// (nz is also the number of blocks per utterance of k_lin_z5's duration slab)
inline ScrfFusedWalkPlan fused_lin_z5_plan(const ScrfFusedShape& lay, uint32_t n_utts, uint32_t t_max) {
  ScrfFusedWalkPlan p = fused_lin_z_plan(lay, n_utts);
  p.nz = lin_z5_segments(n_utts, lay.L, lay.D, t_max, &p.seg_len);
  p.clear_z = p.nz > 1;
  return p;
}
// RW = lanes of the Z_avg rings that exist (48 when L <= 48: 8 wavefronts per CU keep their LDS)
inline ScrfFusedWalkPlan fused_post_z_plan(const ScrfKnobs& kn, const ScrfFusedShape& lay, uint32_t n_utts, int la, uint32_t t_max) {
  ScrfFusedWalkPlan p = fused_lin_z_plan(lay, n_utts);
  p.la = la ? 1 : 0;
  p.rw = (la && lay.L <= 48) ? 48 : 64;
  // few wavefronts (a small minibatch): several segments per utterance (walk_segments; SCRF_POSTZ_SPLIT=0: never)
  int seg_len = 0;
  const uint32_t nz = kn.postz_split ? walk_segments((uint64_t)p.gx * p.gy, lay.D, t_max, &seg_len) : 1;
  if (nz > 1) { p.nz = nz; p.split = 1; p.seg_len = seg_len; p.clear_z = 1; }
  return p;
}

// ---- the two per-frame contractions of the sampled blocks
inline int pframe_supported(uint32_t W) { return W <= 80; }
// k_pframe<KS> (KS k-steps >= ceil(W / 4)) over grid (gx, gy): fpw frames per wavefront
struct ScrfPframePlan { int ks; uint64_t fpw; uint32_t gx, gy; };
inline ScrfPframePlan fused_pframe_plan(uint32_t W, uint64_t n_frames, uint32_t n_out) {
  ScrfPframePlan p = {};
  // about 2048 wavefronts per output group, whole pairs of 16-frame tiles each
  uint64_t fpw = ((n_frames + 2047) / 2048 + 31) & ~31ull;
  if (fpw < 64) fpw = 64;
  p.fpw = fpw;
  p.gx = (uint32_t)((n_frames + fpw - 1) / fpw);
  p.gy = (n_out + 16 * PF_MT - 1) / (16 * PF_MT);
  const uint32_t ks = (W + 3) / 4;
  p.ks = ks <= 4 ? 4 : ks <= 10 ? 10 : ks <= 16 ? 16 : 20;
  return p;
}
// k_ztf<NT, ZT_MT> (NT column tiles >= ceil(W / 16), ZT_MT output tiles per wavefront: 1 = the narrow form of the side
// stream) over grid (n_chunks, gy)
struct ScrfZtfPlan { int nt, mt; uint32_t gx, gy; };
inline ScrfZtfPlan fused_ztf_plan(uint32_t W, uint32_t n_out, uint32_t n_chunks, int narrow) {
  ScrfZtfPlan p = {};
  p.mt = narrow ? 1 : 4;
  p.gx = n_chunks;
  p.gy = (n_out + 16 * p.mt - 1) / (16 * p.mt);
  const uint32_t nt = (W + 15) / 16;
  p.nt = nt <= 1 ? 1 : nt >= 5 ? 5 : (int)nt;
  return p;
}

// ---- the count kernels: k_expf_fused, k_expf_fused_ws, k_expf_fused_ws_n
// column tiles needed, and the row stride of the kernel instantiation that serves them (NCT * 16)
inline uint32_t fused_expf_xs(const ScrfFusedShape& lay, uint32_t W, uint32_t* n_ct) {
  const uint32_t ncol = 3 * W + lay.D + (lay.use_sb ? 1 : 0);
  *n_ct = (ncol + 15) / 16;
  return (*n_ct <= 5 ? 5 : *n_ct <= 9 ? 9 : 13) * 16;
}
// the wave-specialised kernel: dense groups only (g0 = 1: without the average); zb: one statistic per workgroup column
inline uint32_t fused_expf_ws_xs(uint32_t W, int g0, int zb, uint32_t* n_ct) {
  const uint32_t ncol = zb ? W : (3 - g0) * W;
  *n_ct = (ncol + 15) / 16;
  return (*n_ct <= 5 ? 5 : *n_ct <= 9 ? 9 : 13) * 16;
}

// Expected-count tiles are whole frames: as many as give <= 76 rows (what two workgroups per CU can hold at config 2);
// the depth the kernel runs is the next of 52 / 64 / 76 rows (rows past the tile are staged as zeros).
// D = 25: 3 frames, 75 rows in 76; D = 10: 7 frames, 70 in 76.
inline uint32_t fused_expf_frames(uint32_t D) { return D >= FE_ROWS ? 1u : FE_ROWS / D; }
inline uint32_t fused_expf_nks(uint32_t D) {
  const uint32_t rows = fused_expf_frames(D) * D;
  return rows <= 52 ? 13u : rows <= 64 ? 16u : 19u;
}
// most raw frames a tile can need (t_last - f0 + 1)
inline uint32_t fused_expf_nfmax(uint32_t D) { return fused_expf_frames(D) + D - 1; }
inline size_t fused_expf_smem(const ScrfFusedShape& lay, uint32_t W) {
  uint32_t n_ct;
  const uint32_t xs = fused_expf_xs(lay, W, &n_ct);
  return sizeof(float) * (FE_ROWS + 1) * xs + sizeof(double) * FE_ROWS * FE_RS +
         sizeof(float) * fused_expf_nfmax(lay.D) * W + 64;
}
// the single-role count kernel (all dense columns + one-hot + bias in one image; FAST32, SCRF_EXPF_WS=0)
inline bool fused_expf_plain_fits(const ScrfFusedShape& lay, uint32_t W) {
  uint32_t n_ct;
  fused_expf_xs(lay, W, &n_ct);
  return n_ct <= 13 && fused_expf_smem(lay, W) <= 156 * 1024;   // above 80 KB: one workgroup per CU instead of two
}

// the wave-specialised kernel (one 512-thread workgroup per CU, two image pairs in LDS) serves the fp64 form whenever
// its LDS fits; SCRF_EXPF_WS=0 switches it off (A/B measurements).  Rows per tile: 100 when g0 = 1 and the narrower
// column image lets two pairs of that height into 160 KB (its own tile list, built with the batch), else 76.
// Wide streams (config 3: W = 144, config 5: W = 123) do not fit (3 - g0) W columns into 13 column tiles / 160 KB: the
// launch is then z-blocked, one statistic per workgroup column (W <= 144: two images of 9 column tiles; 13 pass 160 KB).
inline size_t fused_expf_ws_smem_rows(uint32_t W, int g0, int zb, uint32_t rows) {
  uint32_t n_ct;
  const uint32_t xs = fused_expf_ws_xs(W, g0, zb, &n_ct);
  return 2 * (sizeof(float) * (rows + 1) * xs + sizeof(double) * rows * FE_RS);
}
inline bool fused_expf_ws_fits(uint32_t W, int g0, int zb) {
  uint32_t n_ct;
  fused_expf_ws_xs(W, g0, zb, &n_ct);
  return n_ct <= 13 && fused_expf_ws_smem_rows(W, g0, zb, FE_ROWS) <= SCRF_FUSED_LDS_BYTES;
}
inline int fused_expf_ws_zb(uint32_t W, int g0) { return !fused_expf_ws_fits(W, g0, 0) && fused_expf_ws_fits(W, g0, 1) ? 1 : 0; }
// The R tiles go to LDS by DMA (16-byte pieces) when every output pair of R is 16-byte aligned: an even row length
// (and an aligned base, an input of the plan); odd L keeps the register path.  SCRF_EXPF_DMA=0 forces the register
// path (A/B measurements, tests).
inline bool fused_expf_dma(const ScrfKnobs& kn, uint32_t L) { return kn.expf_dma && !(L & 1); }
inline uint32_t fused_expf_ws_rows(const ScrfKnobs& kn, uint32_t W, int g0) {
  // Tall tiles only when the side stream is off, or on request (SCRF_EXPF_BIG=1).  On the register path 100-row tiles
  // take 245 registers and cannot share a SIMD with the side stream's narrow k_ztf (29.22 against 29.46 ms for the
  // 76-row form with that overlap; without the side stream 29.54 against 29.43).  On the DMA path both heights fit
  // beside k_ztf (178 / 184 registers) and the tall form is the faster kernel (5.8 against 6.3 ms), but a 100-row tile
  // list deals other rows to each workgroup's slab, so the counts come out in another summation order (2e-15 relative
  // on the weights after five steps): the default keeps the order the 76-row list gives.
  uint32_t n_ct;
  fused_expf_ws_xs(W, g0, 0, &n_ct);
  return (kn.expf_big && g0 == 1 && n_ct <= 5 && !fused_expf_ws_zb(W, g0) && fused_expf_ws_smem_rows(W, g0, 0, FW_ROWS_BIG) <= SCRF_FUSED_LDS_BYTES) ? FW_ROWS_BIG : FE_ROWS;
}
inline bool fused_expf_ws(const ScrfKnobs& kn, const ScrfFusedShape& lay, uint32_t W, int f32, int g0) {
  return kn.expf_ws && !f32 && (fused_expf_ws_fits(W, g0, 0) || fused_expf_ws_fits(W, g0, 1));
}

// f32: FAST32 runs the single-role count kernel only
inline int fused_supported(const ScrfKnobs& kn, const ScrfFusedShape& lay, uint32_t W, int f32 = 0) {
  if (lay.D < 2 || lay.D > 40 || W < 1) return 0;
  if (!fused_expf_plain_fits(lay, W) && !fused_expf_ws(kn, lay, W, f32, 0)) return 0;
  // wide streams with many labels (config 5: W = 123, L = 200, D = 40) are served better by the general path: every
  // 48-output block of the fused kernels repeats the window scans, the D = 40 forms spill, k_post_z walks four label
  // groups (measured 253.6 ms fused against 206.4 ms materialised per 128 utterances).  The z-blocked count kernel is for
  // one label group.
  if (!fused_expf_plain_fits(lay, W) && lay.L > 64) return 0;
  // several label groups with the D = 40 forms (k_post_z<40> and the count kernel spill): the hybrid path is faster
  // (L = 200, D = 40, W = 40, 128 x 1000 frames: 66.8 ms fused, 49.6 ms hybrid; at D <= 25 the fused kernels win: 38.5 vs
  // 46.5 ms at L = 200, W = 39)
  if (lay.L > 64 && lay.D > 32) return 0;
  return fused_scores_tb(W, lay.D) >= 1;
}
// SCRF_PREC_FASTLIN (`la`): the window average leaves both dense contractions (prefix sums of a sixth per-frame
// projection / a sixth group of Z).  It needs the wave-specialised count kernel (the only one without the avg group);
// shapes this returns 0 for run the FAST kernels (the reference's float average) under that precision.  (L > 64:
// k_post_z keeps one Z_avg ring per 64-output group, which its LDS no longer holds two of per SIMD -- left to FAST.)
inline int fused_la_supported(const ScrfKnobs& kn, const ScrfFusedShape& lay, uint32_t W) {
  return fused_supported(kn, lay, W, 0) && lay.L <= 64 && fused_expf_ws(kn, lay, W, 0, 1);
}

enum ScrfFusedExpfKernel {
  SCRF_FK_NONE,    // neither count kernel holds the shape (fused_supported is 0 there)
  SCRF_FK_PLAIN,   // k_expf_fused<NT, DMAX, F32, NKS>
  SCRF_FK_WS,      // k_expf_fused_ws<NT, DMAX, NKS, G0, ROWS, DMA>
  SCRF_FK_WS_N,    // k_expf_fused_ws_n<...>: the same body under a 208-register cap (fused_expf_ws_capped)
};
// the narrow forms of the wave-specialised kernel leave room for the side stream's kernels (constexpr: launch_expf_fused
// asks it about a template argument)
constexpr bool fused_expf_ws_capped(int nt) { return nt <= 4; }
inline const char* scrf_fused_expf_kernel_name(int k) {
  static const char* const names[] = {"none", "plain", "ws", "ws_n"};
  return k >= 0 && k < 4 ? names[k] : "?";
}
// The count launch.  Layout of its slabs: slab [blocks][L][ncol] (dense groups from g0: 0 avg, 1 max) and, when
// ndur > 0, a separate duration slab [blocks][L][ndur] (one-hot duration counts + bias; wave-specialised kernel).
// rows / frames: height of the row tiles the kernel walks (whole frames); tile_list: which of the batch's tile lists
// describes them (1: <= 76 rows, 2: <= 100 rows, built only for batches of an SCRF_PREC_FASTLIN engine).
// nz: workgroup columns of the launch (one dense statistic each when > 1: the z-blocked form).
// The launch: `kernel` with the template arguments nt (slots per consumer wavefront), dmax, nks (k-steps), g0, rows, dma,
// f32 over grid (blocks, gy, nz), `threads` threads and `lds` bytes; n_ct column tiles of the xs-float-wide image, nfmax
// raw frames per tile (single-role kernel).  blocks: persistent workgroups = slabs, the tiles of the launch up to cap (<= 512).
struct ScrfFusedExpfPlan {
  int ws; int g0; uint32_t ncol; uint32_t ndur; uint32_t rows; uint32_t frames; int tile_list; uint32_t nz;
  int kernel, nt, dmax, nks, f32, dma;
  uint32_t n_ct, xs, nfmax, cap, gy, threads;
  size_t lds;
};
// r_aligned: R's base is 16-byte aligned (a caller that wants the layout only -- the batch's tile lists -- passes 1)
inline ScrfFusedExpfPlan fused_expf_plan(const ScrfKnobs& kn, const ScrfFusedShape& lay, uint32_t W, int f32, int la, int r_aligned) {
  ScrfFusedExpfPlan p = {};
  p.ws = fused_expf_ws(kn, lay, W, f32, la ? 1 : 0) ? 1 : 0;
  p.g0 = (p.ws && la) ? 1 : 0;
  p.ncol = p.ws ? (3 - p.g0) * W : 3 * W + lay.D + (lay.use_sb ? 1 : 0);
  p.ndur = p.ws ? lay.D + (lay.use_sb ? 1 : 0) : 0;
  p.rows = p.ws ? fused_expf_ws_rows(kn, W, p.g0) : FE_ROWS;
  p.tile_list = p.rows == FE_ROWS ? 1 : 2;
  p.frames = lay.D >= p.rows ? 1u : p.rows / lay.D;
  const int zb = p.ws ? fused_expf_ws_zb(W, p.g0) : 0;
  p.nz = zb ? (uint32_t)(3 - p.g0) : 1u;
  p.gy = (lay.L + 47) / 48;
  p.dmax = fused_dmax3(lay.D);
  // the depths that occur per duration class: D <= 12 always fills more than 64 rows, 13..25 never stops at 52
  const uint32_t nks = fused_expf_nks(lay.D);
  p.nks = lay.D <= 12 ? 19 : lay.D <= 25 ? (nks == 16 ? 16 : 19) : (int)nks;
  p.cap = kn.expf_blocks;
  if (p.ws) {
    p.xs = fused_expf_ws_xs(W, p.g0, zb, &p.n_ct);
    if (p.rows == FW_ROWS_BIG) {
      // 100-row tiles (g0 = 1, n_ct <= 5): k-steps = ceil(frames * D / 4) rounded up to 21 or 25
      p.nt = 4;
      p.nks = p.frames * lay.D <= 84 ? 21 : 25;
    } else {
      // slots per consumer wavefront = ceil(3 n_ct / 4)
      p.nt = p.n_ct <= 5 ? 4 : p.n_ct <= 8 ? 6 : p.n_ct <= 9 ? 7 : 10;
    }
    p.kernel = fused_expf_ws_capped(p.nt) ? SCRF_FK_WS_N : SCRF_FK_WS;
    p.dma = (fused_expf_dma(kn, lay.L) && r_aligned) ? 1 : 0;
    p.threads = FW_NT;
    p.lds = fused_expf_ws_smem_rows(W, p.g0, zb, p.rows);
    if (p.cap > 256u) p.cap = 256u;   // one workgroup per CU there
  } else {
    p.xs = fused_expf_xs(lay, W, &p.n_ct);
    p.nt = p.n_ct <= 5 ? 4 : p.n_ct <= 9 ? 7 : 10;
    p.kernel = fused_expf_plain_fits(lay, W) ? SCRF_FK_PLAIN : SCRF_FK_NONE;
    p.f32 = f32 ? 1 : 0;
    p.nfmax = fused_expf_nfmax(lay.D);
    p.threads = FE_NT;
    p.lds = fused_expf_smem(lay, W);
  }
  return p;
}
inline uint32_t fused_expf_blocks(const ScrfFusedExpfPlan& p, uint64_t n_tiles) { return (uint32_t)(n_tiles < p.cap ? n_tiles : p.cap); }

#endif  // SCRF_FUSED_PLAN_H_
