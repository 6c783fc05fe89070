// scrf_dp_plan.h -- which kernel instantiation the launchers of the recursions, the walks and the searches start, with
// which grid, how many threads and how much LDS; and the predicates by which the engine routes a chunk to them.
// Host-only (no HIP), like scrf_fused_plan.h: every launch_* named below asks one function here for its plan and
// switches on the fields, and tests/host/dp_plan_probe.cpp prints the same plan without a GPU, so what the probe says
// about a shape is what the launcher does.  Every threshold of the choice lives here and only here.
#ifndef SCRF_DP_PLAN_H_
#define SCRF_DP_PLAN_H_

#include <stddef.h>
#include <stdint.h>

#include "scrf_knobs.h"

#ifdef __HIPCC__
#define SCRF_HD __host__ __device__
#else
#define SCRF_HD
#endif

// the layout fields the choice reads (ScrfLayout's, scrf_common.h; dp_shape() in scrf_kernels.h copies them)
struct ScrfDpShape { uint32_t L, D; int32_t use_tf, use_tb; };

// ---- LDS budgets (a workgroup has 160 KB: SCRF_LDS_BYTES)
#define SCRF_DP_LDS_BUDGET (156 * 1024)    // the wavefront-per-utterance recursions: what their workgroup may ask for
#define SCRF_WG_LDS_BUDGET (150 * 1024)    // k_fb_segtrans_w and k_sl_fb: above it the shape goes to another kernel
#define SCRF_VF_LDS_BUDGET (64 * 1024)     // k_viterbi_fast: two workgroups per CU

// ---- wavefronts / threads per workgroup the kernels are built for
#define DP_WPB 12      // k_dp_wave, k_dp_lin: 3 per SIMD, one workgroup per CU (6-wave groups do not pair up on a CU)
#define DPV_NW 4       // k_dp_lin_mv: wavefronts per sweep
#define VF_WAVES 4     // k_viterbi_fast: utterances per workgroup
#define FBW_WAVES 16   // k_fb_segtrans_w: the most wavefronts per workgroup
#define AL_WAVES 4     // k_align_wave: utterances per workgroup
#define NB_WAVES 16    // k_nbest
#define SL_NT 512      // threads of the STDSEG recursion workgroup: one per full label (nLabs <= 512)
#define SA_MG 3        // k_sl_atb: 16-row tiles of p per wavefront

// wavefronts per workgroup the LDS allows: 12 when they fit, else 8 / 4 / 2 / 1 (L = 64 with D >= 17 needs that)
inline uint32_t dp_waves_per_block(size_t shared_bytes, size_t per_wave_bytes) {
  const uint32_t opts[5] = {DP_WPB, 8, 4, 2, 1};
  for (int i = 0; i < 5; i++)
    if (shared_bytes + opts[i] * per_wave_bytes <= SCRF_DP_LDS_BUDGET) return opts[i];
  return 1;
}

// Frame segments per utterance of a walk with `waves` wavefronts in all (k_post_z, k_post_occ).  Few wavefronts (a
// small minibatch): several segments per utterance, about four wavefronts per CU in all (half the kernels' occupancy),
// no segment shorter than 2 D frames.  Returns the number of segments; *seg_len their length (0: one piece).
// Config 3, 256 utterances: k_post_z 1.21 -> 0.50 ms; config 2's shape at 64 utterances: 1.90 -> 0.38 ms
inline uint32_t walk_segments(uint64_t waves, uint32_t D, uint32_t t_max, int* seg_len) {
  *seg_len = 0;
  if (!waves || waves > 2 * 256 || t_max < 4 * D) return 1;
  const uint32_t want = (uint32_t)((4 * 256 + waves - 1) / waves);
  int sl = (int)((t_max + want - 1) / want);
  if (sl < (int)(2 * D)) sl = (int)(2 * D);
  *seg_len = sl;
  return (uint32_t)((t_max + sl - 1) / sl);
}

// ---- k_exp_m / k_exp_m_tile<NE> (NE 256-element slices of an L x L matrix; 0: k_exp_m) over n_mat workgroups
struct ScrfExpMPlan { int ne; uint32_t gx, threads; };
inline ScrfExpMPlan exp_m_plan(const ScrfKnobs& kn, uint32_t L, uint64_t n_mat) {
  ScrfExpMPlan p = {};
  const uint32_t ne = (L * L + 255) / 256;
  if (L <= 64 && kn.expm_tile) p.ne = ne <= 4 ? 4 : ne <= 9 ? 9 : 16;
  p.gx = (uint32_t)n_mat;
  p.threads = 256;
  return p;
}

// ---- k_dp_wave<DMAX, MPF>: the log-domain recursion, one wavefront per (utterance, direction)
inline int dp_wave_supported(const ScrfDpShape& lay) { return lay.L <= 64 && lay.D <= 32; }
// wpb wavefronts per workgroup; the time-invariant transition matrix (MPF = 0) is shared by the workgroup
struct ScrfDpWavePlan { int dmax, mpf; uint32_t wpb, blocks, threads; size_t lds; };
inline ScrfDpWavePlan dp_wave_plan(const ScrfDpShape& lay, uint32_t n_utts, int m_per_frame) {
  ScrfDpWavePlan p = {};
  const size_t shared = sizeof(double) * (m_per_frame ? 0 : (size_t)lay.L * lay.L);
  p.dmax = lay.D <= 1 ? 1 : lay.D <= 4 ? 4 : lay.D <= 10 ? 10 : lay.D <= 16 ? 16 : lay.D <= 25 ? 25 : 32;
  p.mpf = m_per_frame ? 1 : 0;
  p.wpb = dp_waves_per_block(shared, sizeof(double) * (size_t)lay.D * lay.L);
  p.blocks = 2 * ((n_utts + p.wpb - 1) / p.wpb);
  p.threads = p.wpb * 64;
  p.lds = shared + sizeof(double) * (size_t)p.wpb * lay.D * lay.L;
  return p;
}

// ---- the scaled linear-domain recursion: k_dp_lin, k_dp_lin_mv, k_dp_lin_mw
// the one-wavefront-per-utterance form (k_dp_lin): L <= 64, D <= 40 (the log-domain k_dp_wave stops at 32)
inline int dplin_supported(const ScrfDpShape& lay) { return lay.L <= 64 && lay.D <= 40; }
inline int dplin_mw_supported(const ScrfDpShape& lay) { return lay.L > 64 && lay.L <= 256 && lay.D <= 40; }
enum ScrfDpLinKernel {
  SCRF_DK_LIN,      // k_dp_lin<DMAX, MPF, LC>: a wavefront per sweep, wpb of them per workgroup
  SCRF_DK_LIN_MV,   // k_dp_lin_mv<DMAX, MPF>: DPV_NW wavefronts per sweep
  SCRF_DK_LIN_MW,   // k_dp_lin_mw<DMAX, MPF, LR, TAIL>: L > 64, a wavefront per 64 labels
};
inline const char* scrf_dp_lin_kernel_name(int k) {
  static const char* const names[] = {"k_dp_lin", "k_dp_lin_mv", "k_dp_lin_mw"};
  return k >= 0 && k < 3 ? names[k] : "?";
}
// lc: k_dp_lin's label count as a template argument (0: from the layout).  lr / tail: rows of the transition column
// k_dp_lin_mw keeps in registers (0: none) and whether the rows past them come from L2.  wpb: wavefronts per workgroup.
struct ScrfDpLinPlan { int kernel, dmax, mpf, lc, lr, tail; uint32_t wpb, blocks, threads; size_t lds; };
inline ScrfDpLinPlan dp_lin_plan(const ScrfKnobs& kn, const ScrfDpShape& lay, uint32_t n_utts, int m_per_frame, int n_cu) {
  ScrfDpLinPlan p = {};
  p.mpf = m_per_frame ? 1 : 0;
  if (lay.L > 64) {
    p.kernel = SCRF_DK_LIN_MW;
    p.dmax = lay.D <= 10 ? 10 : lay.D <= 25 ? 25 : 40;
    p.wpb = (lay.L + 63) / 64;
    // The matrix column in registers (SCRF_DPLIN_EREG=0: from L2 every frame).
    // Measured (ms per launch, from L2 -> in registers): L = 200, D = 25, 512 x 300 frames 17.6 -> 9.4 (LR = 208: 49 spilled
    // registers, still a gain); L = 96, D = 25, 1024 utterances 10.2 -> 6.5; L = 128, D = 10: 5.4 -> 4.3.  At DMAX = 40 the
    // duration step's 80 registers leave room for 128 rows only (L = 200 in full spills 141 registers and LOSES: 13.7 ->
    // 17.8): there 128 rows live in registers and the rest comes from L2 (TAIL).
    if (m_per_frame || !kn.dplin_ereg) p.lr = 0;
    else if (lay.L <= 128) p.lr = 128;
    else if (p.dmax <= 25 && lay.L <= 192) p.lr = 192;
    else if (p.dmax <= 25 && lay.L <= 208) p.lr = 208;
    else if (p.dmax > 25 && kn.dplin_tail) { p.lr = 128; p.tail = 1; }
    p.blocks = 2 * n_utts;
    p.threads = 64 * p.wpb;
    p.lds = sizeof(double) * ((((size_t)lay.D * lay.L + 1) & ~(size_t)1) + 64 * p.wpb + 64 + 64 * p.wpb + 16);
    return p;
  }
  // k_dp_lin_mv (four wavefronts per sweep): SCRF_DPLIN_MV=1 always, =0 never; unset: with per-frame transition matrices
  // when the launch has at most SCRF_DPLIN_MV_SWEEPS (default 3: the kernel's occupancy) sweeps per CU -- there the
  // single-wavefront kernel's step is the latency of one wavefront fetching an L x L matrix, and four fetch it in
  // parallel (config 3, 256 utterances: 1.86 -> 1.03 ms).  With time-invariant transitions it measured no faster at any
  // batch size (64 .. 4096 utterances), so it stays opt-in there.
  const bool use_mv = kn.dplin_mv == 1 || (kn.dplin_mv < 0 && m_per_frame && 2 * (uint64_t)n_utts <= (uint64_t)kn.dplin_mv_sweeps * n_cu);
  if (use_mv && lay.D >= 2) {
    p.kernel = SCRF_DK_LIN_MV;
    p.dmax = lay.D <= 10 ? 10 : lay.D <= 16 ? 16 : lay.D <= 25 ? 25 : lay.D <= 32 ? 32 : 40;
    p.wpb = DPV_NW;
    p.blocks = 2 * n_utts;
    p.threads = 64 * DPV_NW;
    p.lds = sizeof(double) * ((((size_t)lay.D * lay.L + 1) & ~(size_t)1) + 4 * DPV_NW * 64);
    return p;
  }
  p.kernel = SCRF_DK_LIN;
  p.dmax = lay.D <= 1 ? 1 : lay.D <= 4 ? 4 : lay.D <= 10 ? 10 : lay.D <= 16 ? 16 : lay.D <= 25 ? 25 : lay.D <= 32 ? 32 : 40;
  p.lc = (!m_per_frame && p.dmax == 25 && lay.L == 48) ? 48 : 0;
  const size_t shared = sizeof(double) * (m_per_frame ? 0 : (size_t)lay.L * lay.L);
  p.wpb = dp_waves_per_block(shared, sizeof(double) * ((size_t)lay.D * lay.L + 128));
  if (p.wpb > 8) {
    // Tail-aware workgroup size: one workgroup per CU, so the launch runs in ceil(workgroups / CUs) rounds of T steps,
    // and a step costs a fixed latency plus a share per resident wavefront (measured on MI355X at config 2:
    // 3.4 us + 0.31 us per wavefront).  8192 sweeps on 256 CUs: 12 wavefronts per workgroup are
    // 2.67 -> 3 rounds of 7.1 us steps, 11 are 2.91 -> 3 rounds of 6.8 us steps.
    uint32_t best = p.wpb;
    double best_cost = 1e300;
    for (uint32_t w = p.wpb; w >= 8; w--) {
      const uint64_t blocks = 2 * (((uint64_t)n_utts + w - 1) / w);
      const double cost = (double)((blocks + n_cu - 1) / n_cu) * (3.4 + 0.31 * w);
      if (cost < best_cost - 1e-9) { best_cost = cost; best = w; }
    }
    p.wpb = best;
  }
  p.blocks = 2 * ((n_utts + p.wpb - 1) / p.wpb);
  p.threads = p.wpb * 64;
  p.lds = shared + sizeof(double) * (size_t)p.wpb * (lay.D * lay.L + 128);
  return p;
}

// ---- k_atb<LT>: A^T B over row chunks, LT 16-column tiles a side (L > 64: 64 x 64 output blocks in grid.y)
inline int atb_supported(const ScrfDpShape& lay) { return lay.L <= 256; }
struct ScrfAtbPlan { int lt; uint32_t gx, gy, threads; };
inline ScrfAtbPlan atb_plan(const ScrfDpShape& lay, uint32_t n_chunks) {
  ScrfAtbPlan p = {};
  const uint32_t nb = (lay.L + 63) / 64, lt = lay.L > 64 ? 4 : (lay.L + 15) / 16;
  p.lt = lt <= 1 ? 1 : (int)lt;
  p.gx = (n_chunks + 3) / 4;
  p.gy = nb * nb;
  p.threads = 256;
  return p;
}

// ---- k_fb / k_fb_segtrans: the workgroup-per-utterance log-domain recursions; k_viterbi
inline int fb_block_threads(const ScrfDpShape& lay) { return lay.L <= 256 ? 256 : 1024; }
inline size_t fb_smem_bytes(const ScrfDpShape& lay, int NT) {
  int G = NT / (int)lay.L;
  if (G < 1) G = 1;
  return sizeof(double) * ((size_t)2 * lay.D * lay.L + 2 * lay.L + (size_t)2 * G * lay.L);
}
inline size_t fb_segtrans_smem_bytes(const ScrfDpShape& lay, int NT) {
  int G = NT / (int)lay.L;
  if (G < 1) G = 1;
  return sizeof(double) * ((size_t)3 * lay.D * lay.L + (size_t)2 * G * lay.L);
}
// a workgroup per utterance: `threads` threads, `lds` bytes
struct ScrfGroupPlan { uint32_t threads; size_t lds; };
inline ScrfGroupPlan fb_plan(const ScrfDpShape& lay) {
  ScrfGroupPlan p = {};
  p.threads = (uint32_t)fb_block_threads(lay);
  p.lds = fb_smem_bytes(lay, (int)p.threads);
  return p;
}
inline ScrfGroupPlan viterbi_plan(const ScrfDpShape& lay) {
  ScrfGroupPlan p = {};
  int NT = ((int)lay.L + 63) / 64 * 64;
  if (NT > 1024) NT = 1024;
  p.threads = (uint32_t)NT;
  p.lds = sizeof(float) * ((size_t)2 * lay.L + (size_t)lay.D * lay.L);
  return p;
}
// wave = 1: k_fb_segtrans_w, the wavefront-per-window form, while two D x L images fit; larger D * L keeps the
// column-wise k_fb_segtrans.  Wavefronts per workgroup: 16 when every CU has at most one utterance, 8 (two workgroups
// per CU) beyond that; SCRF_FBW_WAVES in [1, FBW_WAVES] sets them
struct ScrfFbSegtransPlan { int wave; uint32_t threads; size_t lds; };
inline ScrfFbSegtransPlan fb_segtrans_plan(const ScrfKnobs& kn, const ScrfDpShape& lay, uint32_t n_utts) {
  ScrfFbSegtransPlan p = {};
  const size_t smw = sizeof(double) * 2 * (size_t)lay.D * lay.L;
  if (smw <= SCRF_WG_LDS_BUDGET) {
    int nw = n_utts > 256 ? FBW_WAVES / 2 : FBW_WAVES;
    if (kn.fbw_waves >= 1 && kn.fbw_waves <= FBW_WAVES) nw = kn.fbw_waves;
    p.wave = 1;
    p.threads = 64 * (uint32_t)nw;
    p.lds = smw;
    return p;
  }
  p.threads = (uint32_t)fb_block_threads(lay);
  p.lds = fb_segtrans_smem_bytes(lay, (int)p.threads);
  return p;
}

// ---- k_viterbi_fast<DMAX, LV>: float arc weights, one wavefront per utterance (fast decode; L <= 64, constant M)
inline size_t viterbi_fast_smem_bytes(const ScrfDpShape& lay) {
  return sizeof(float) * ((size_t)lay.L * lay.L + VF_WAVES * ((size_t)lay.L + (size_t)lay.D * lay.L));
}
inline int viterbi_fast_supported(const ScrfDpShape& lay) {
  return lay.L <= 64 && lay.D >= 2 && lay.D <= 40 && !lay.use_tf && viterbi_fast_smem_bytes(lay) <= SCRF_VF_LDS_BUDGET;
}
// lv: register column + 16-byte reads of the previous node's costs, for 48 or 64 labels -- L a multiple of 4 (the LDS
// vectors stay 16-byte aligned); 0 (SCRF_VITERBI_VEC=0, other L): scalar reads
struct ScrfViterbiFastPlan { int dmax, lv; uint32_t gx, threads; size_t lds; };
inline ScrfViterbiFastPlan viterbi_fast_plan(const ScrfKnobs& kn, const ScrfDpShape& lay, uint32_t n_utts) {
  ScrfViterbiFastPlan p = {};
  p.dmax = lay.D <= 12 ? 12 : lay.D <= 25 ? 25 : 40;
  p.lv = (kn.viterbi_vec && lay.L % 4 == 0) ? (lay.L <= 48 ? 48 : 64) : 0;
  p.gx = (n_utts + VF_WAVES - 1) / VF_WAVES;
  p.threads = 64 * VF_WAVES;
  p.lds = viterbi_fast_smem_bytes(lay);
  return p;
}

// ---- k_post_occ<DMAX, RW>: the posterior walk over grid (n_utts, groups of 64 outputs, nz frame segments)
inline uint32_t post_occ_groups(const ScrfDpShape& lay) { return (lay.L + 63) / 64; }
// rw: lanes of the rings (48 when L <= 48).  seg_len: frames per segment (past any utterance when nz = 1).
// sum_groups: L > 64, the groups' partial masses are added by k_sum_groups afterwards
struct ScrfPostOccPlan { int dmax, rw, seg_len, sum_groups; uint32_t gx, gy, nz; };
inline ScrfPostOccPlan post_occ_plan(const ScrfDpShape& lay, uint32_t n_utts, uint32_t t_max, int split_ok) {
  ScrfPostOccPlan p = {};
  p.dmax = lay.D <= 8 ? 8 : lay.D <= 16 ? 16 : lay.D <= 25 ? 25 : lay.D <= 32 ? 32 : 40;
  p.rw = lay.L <= 48 ? 48 : 64;
  p.gx = n_utts;
  p.gy = post_occ_groups(lay);
  p.sum_groups = p.gy > 1;
  int sl = 0;
  p.nz = split_ok ? walk_segments((uint64_t)p.gx * p.gy, lay.D, t_max, &sl) : 1;
  p.seg_len = p.nz > 1 ? sl : 0x7fffffff / 2;
  return p;
}

// ---- k_align_wave<DMAX>: forced alignment, one wavefront per utterance (transcripts of at most 64 phones)
inline int align_wave_supported(const ScrfDpShape& lay) { return lay.D <= 40; }
inline size_t align_group_smem_bytes(const ScrfDpShape& lay, uint64_t K) { return sizeof(float) * ((size_t)lay.D + 2) * K; }
struct ScrfAlignWavePlan { int dmax; uint32_t gx, threads; size_t lds; };
inline ScrfAlignWavePlan align_wave_plan(const ScrfDpShape& lay, uint32_t n_utts) {
  ScrfAlignWavePlan p = {};
  p.dmax = lay.D <= 4 ? 4 : lay.D <= 12 ? 12 : 40;
  p.gx = (n_utts + AL_WAVES - 1) / AL_WAVES;
  p.threads = 64 * AL_WAVES;
  p.lds = sizeof(float) * AL_WAVES * (64 + (size_t)lay.D * 64);   // D <= 40: at most 41 KiB
  return p;
}

// ---- STDSEG with bias-only transitions on the training path: k_sl_fb, k_sl_atb<NT>.  lay.L = full labels, La = actual
inline size_t sl_fb_smem_bytes(const ScrfDpShape& lay) {
  return sizeof(double) * ((size_t)lay.D * lay.L + 2 * lay.D + lay.L + SL_NT / 64 + 2);
}
inline int stdseg_lin_supported(const ScrfDpShape& lay, uint32_t La) {
  return !lay.use_tf && lay.use_tb && lay.L <= SL_NT && La <= 64 && lay.D >= 1 && sl_fb_smem_bytes(lay) <= SCRF_WG_LDS_BUDGET;
}
struct ScrfSlFbPlan { uint32_t gx, threads; size_t lds; };
inline ScrfSlFbPlan sl_fb_plan(const ScrfDpShape& lay, uint32_t n_utts) {
  ScrfSlFbPlan p = {};
  p.gx = 2 * n_utts;
  p.threads = SL_NT;
  p.lds = sl_fb_smem_bytes(lay);
  return p;
}
// nt: 16-column tiles of the actual labels; a wavefront per (row chunk, duration, group of SA_MG row tiles)
struct ScrfSlAtbPlan { int nt; uint32_t gx, threads; };
inline ScrfSlAtbPlan sl_atb_plan(const ScrfDpShape& lay, uint32_t La, uint32_t n_chunks) {
  ScrfSlAtbPlan p = {};
  const uint32_t n_mt = (lay.L + 15) / 16, n_mg = (n_mt + SA_MG - 1) / SA_MG, nt = (La + 15) / 16;
  p.nt = nt <= 1 ? 1 : nt >= 4 ? 4 : (int)nt;
  p.gx = (uint32_t)((uint64_t)n_chunks * lay.D * n_mg);
  p.threads = 64;
  return p;
}

// ---- LDS of the workgroup-per-utterance searches the engine checks against SCRF_LDS_BYTES before it launches
inline size_t lat_sweep_smem_bytes(const ScrfDpShape& lay) { return sizeof(double) * ((size_t)lay.D + 2) * lay.L; }
// a workgroup whose longest transcript has K phones: (D + 2) K doubles
inline size_t transcript_smem_bytes(const ScrfDpShape& lay, uint64_t K) { return sizeof(double) * ((size_t)lay.D + 2) * K; }
// head ranks of one wavefront's merge: one 16-bit entry per list, L (boundary, final) or D + 1 (end) of them
SCRF_HD inline uint32_t nbest_heads(uint32_t L, uint32_t D) { return ((L > D + 1 ? L : D + 1) + 1) & ~1u; }
// end double-buffered and the boundary ring, (D + 2) L N floats, + the head ranks
inline size_t nbest_smem_bytes(const ScrfDpShape& lay, uint32_t n_best) {
  return sizeof(float) * ((size_t)lay.D + 2) * lay.L * n_best + sizeof(uint16_t) * NB_WAVES * (size_t)nbest_heads(lay.L, lay.D);
}

#endif  // SCRF_DP_PLAN_H_
