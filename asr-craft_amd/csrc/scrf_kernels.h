// scrf_kernels.h -- launch wrappers of the HIP kernels (scrf_kernels.hip, scrf_mfma.hip).
#ifndef SCRF_KERNELS_H_
#define SCRF_KERNELS_H_

#include "scrf_arcw.h"
#include "scrf_common.h"
#include "scrf_knobs.h"
#include "scrf_dp_plan.h"
#include "scrf_fused_plan.h"
#include "scrf_mfma_plan.h"

#include <vector>

// the recursions, the walks and the searches: which instantiation their launchers start, the predicates that route a chunk
// to them (dp_wave_supported, dplin_supported, ...) and the LDS sizes the engine checks are in scrf_dp_plan.h
inline ScrfDpShape dp_shape(const ScrfLayout& l) { return ScrfDpShape{l.L, l.D, l.use_tf, l.use_tb}; }

void launch_windows(hipStream_t st, const float* frames, const uint64_t* sframe_off, ScrfBatchView bv,
                    uint32_t u0, uint32_t u1, uint64_t n_frames, uint32_t W, uint32_t D, uint32_t lctx,
                    uint32_t rctx, int extract, float* X, uint32_t F, uint32_t out_col, int first_only = 0);
void launch_frame_rows(hipStream_t st, ScrfBatchView bv, uint32_t u0, uint32_t u1, uint32_t D,
                       uint64_t n_frames, uint64_t* xrow, int next);
void launch_scores_exact(hipStream_t st, const float* X, uint32_t F, const uint64_t* xrow, uint64_t n_rows,
                         const double* lambda, const ScrfLayout& lay, int is_trans, uint32_t n_out, double* out);
void launch_fb(hipStream_t st, const ScrfLayout& lay, ScrfBatchView bv, uint32_t u0, uint32_t n_utts,
               const double* S, const double* M, int m_per_frame, double* AD, double* alpha_g, double* beta_g,
               double* XI, double* xi_acc, double* numer, double* zx, int* status, int write_post, int frame_model = 0);
void launch_expf_gemm(hipStream_t st, const double* A, uint32_t n_out, const float* X, uint32_t F,
                      const uint64_t* xrow, uint64_t n_rows, const ScrfLayout& lay, int is_trans,
                      uint64_t rows_per_chunk, uint32_t n_chunks, double* slab);
void launch_reduce_slabs(hipStream_t st, const double* slab, uint32_t n_chunks, uint32_t n_out,
                         const ScrfLayout& lay, const ScrfGemmSpec& sp, double* grad);
void launch_reduce_xiacc(hipStream_t st, const double* xi_acc, uint32_t n_utts, const ScrfLayout& lay,
                         double* grad);
void launch_batch_sums(hipStream_t st, const double* numer, const double* zx, uint32_t n, double* sums3);
// src (here and below): the chunk's arcs, ScrfArcSrc of scrf_arcw.h
void launch_viterbi(hipStream_t st, const ScrfLayout& lay, ScrfBatchView bv, uint32_t u0, uint32_t n_utts, const ScrfArcSrc& src,
                    uint16_t* bp_b, uint16_t* bp_e, uint32_t* out_labels, uint32_t* out_n, float* out_cost);
void launch_arcs(hipStream_t st, const ScrfLayout& lay, uint32_t T, const ScrfArcSrc& src, float final_w, scrf_arc* arcs);
void launch_sgd_step(hipStream_t st, double* lambda, double* lambda_acc, double* gsa, double* grad, uint32_t n,
                     double lr, int adagrad, double eps);
void launch_scale(hipStream_t st, double* v, uint32_t n, double s, int divide);
void launch_add(hipStream_t st, double* y, const double* x, uint32_t n);

// scrf_segtrans.hip: STDSEG_NO_DUR (one transition matrix per window): workgroup-per-utterance log-domain recursion
void launch_zero_initial_rows(hipStream_t st, ScrfBatchView bv, const uint32_t* frame_u, uint32_t u0, uint64_t n_frames,
                              uint32_t D, uint32_t L, double* M2);
void launch_fb_segtrans(hipStream_t st, const ScrfKnobs& kn, const ScrfLayout& lay, ScrfBatchView bv, uint32_t u0, uint32_t n_utts,
                        const uint32_t* prev_lab, const double* S, const double* M2, double* AD, double* alpha_g,
                        double* beta_g, double* XI2, double* numer, double* zx, int* status, int write_post);

uint64_t segtrans_num_arcs(uint32_t T, uint32_t L, uint32_t D);
void launch_arcs_segtrans(hipStream_t st, const ScrfLayout& lay, uint32_t T, const double* S, const double* M2, float final_w,
                          scrf_arc* arcs);
void launch_viterbi_segtrans(hipStream_t st, const ScrfLayout& lay, ScrfBatchView bv, uint32_t u0, uint32_t n_utts,
                             const double* S, const double* M2, uint16_t* bp_p, uint16_t* bp_d, uint32_t* out_labels,
                             uint32_t* out_n, float* out_cost);

// scrf_mfma.hip: fp64 MFMA contractions (FAST training precision)
void launch_scores_mfma(hipStream_t st, const ScrfKnobs& kn, const float* X, uint32_t F, const uint64_t* xrow, uint64_t n_rows,
                        const double* lambda, const ScrfLayout& lay, const ScrfGemmSpec& sp, uint32_t n_out,
                        double* out, int f32 = 0);
void launch_expf_mfma(hipStream_t st, const ScrfKnobs& kn, const double* A, uint32_t n_out, const float* X, uint32_t F,
                      const uint64_t* xrow, uint64_t n_rows, const ScrfLayout& lay, const ScrfGemmSpec& sp,
                      uint64_t rows_per_chunk, uint32_t n_chunks, double* slab, int f32 = 0);
// (which instantiations the two launch, and expf_mfma_wide_tiles for the engine's row chunks: scrf_mfma_plan.h)

// scrf_dp.hip: wavefront-per-utterance DP and the parallel posterior kernels
void launch_exp_m(hipStream_t st, const ScrfKnobs& kn, const double* M, uint32_t L, uint64_t n_mat, double* E, double* ET,
                  double* mshift);
void launch_dp_wave(hipStream_t st, const ScrfLayout& lay, ScrfBatchView bv, uint32_t u0, uint32_t n_utts,
                    const double* S, const double* E, const double* ET, const double* mshift, int m_per_frame,
                    double* AD, double* alpha_g, double* beta_g, double* sd_g, double* zx, int* status);
void launch_post_state(hipStream_t st, const ScrfLayout& lay, ScrfBatchView bv, uint32_t u0, uint32_t u1,
                       uint64_t n_frames, const uint32_t* next_lab, const double* S, const double* M,
                       int m_per_frame, double* AD, const double* beta_g, const double* zx, double* numer_f,
                       int* status, double* mass_s);
void launch_numer_reduce(hipStream_t st, ScrfBatchView bv, uint32_t u0, uint32_t n_utts, const double* numer_f,
                         double* numer);
void launch_xi_factors(hipStream_t st, const ScrfLayout& lay, ScrfBatchView bv, uint32_t u0, uint32_t u1,
                       uint64_t n_frames, const double* alpha_g, const double* sd_g, const double* zx, double* A,
                       double* B);
void launch_atb(hipStream_t st, const ScrfLayout& lay, const double* A, const double* B, uint64_t n_frames,
                uint64_t rows_per_chunk, uint32_t n_chunks, double* slab, const double* M0, double* grad,
                const double* bscale = nullptr);   // bscale[f]: factor of row f of B (linear-domain path)
void launch_add_trans_counts(hipStream_t st, const uint32_t* counts, const ScrfLayout& lay, double* grad);
void launch_xi_full(hipStream_t st, const ScrfLayout& lay, ScrfBatchView bv, uint32_t u0, uint32_t u1,
                    uint64_t n_frames, const uint32_t* next_lab, const double* A, const double* B, const double* E,
                    const double* mshift, double* XI);

// scrf_dplin.hip: scaled linear-domain forward/backward + posteriors (training path, L <= 64)
void launch_true_scores(hipStream_t st, const ScrfLayout& lay, ScrfBatchView bv, const uint32_t* frame_u, uint32_t u0,
                        uint64_t n_frames, const double* S, double* s_true);
void launch_exp_rows(hipStream_t st, double* S, uint64_t n_rows, uint32_t L, double* smax);
void launch_dp_lin(hipStream_t st, const ScrfKnobs& kn, const ScrfLayout& lay, ScrfBatchView bv, uint32_t u0, uint32_t n_utts,
                   const double* ES, const double* smax, const double* E, const double* ET, const double* mshift,
                   int m_per_frame, const ScrfDpLin& o, double* zx, int* status);
void launch_post_lin(hipStream_t st, const ScrfLayout& lay, ScrfBatchView bv, const uint32_t* frame_u, uint32_t u0,
                     uint64_t n_frames, const uint32_t* next_lab, const double* s_true, const double* M,
                     int m_per_frame, double* ES, const double* smax, const ScrfDpLin& o, const double* zx,
                     double* numer_f, int* status, double* mass_s);
// posterior-mass self-checks per frame (state mass from the posterior kernel vs sum_c exp(alpha + beta - Zx));
// lin: a/b are mantissa vectors with log-scales ga/gb, else log-domain arrays (ga, gb unused)
void launch_mass_check(hipStream_t st, ScrfBatchView bv, const uint32_t* frame_u, uint32_t u0, uint64_t n_frames,
                       uint32_t L, int frame_model, int lin, const double* a, const double* ga, const double* b,
                       const double* gb, const double* zx, const double* mass_s, int* status);
void launch_xi_lin(hipStream_t st, const ScrfLayout& lay, ScrfBatchView bv, const uint32_t* frame_u, uint32_t u0,
                   uint64_t n_frames, const ScrfDpLin& o, const double* zx);
void launch_xi_scale(hipStream_t st, ScrfBatchView bv, const uint32_t* frame_u, uint32_t u0, uint64_t n_frames,
                     const ScrfDpLin& o, const double* zx);
void launch_lin_to_log(hipStream_t st, uint64_t n_frames, uint32_t L, const double* m, const double* g, double* out);

// scrf_post.hip: posterior output (scrf_posteriors_batch): frame posteriors occ [frames][L] (nullptr: not formed) and the
// per-frame state mass mass_s [frames] (= the boundary posterior) from the linear-domain vectors / the log-domain arrays;
// mass_part [post_occ_groups][frames] holds the per-group partial masses when L > 64 (not used with one group).
// launch_post_occ returns the number of frame segments every utterance's walk was split into (1: one piece); split_ok = 0
// keeps every walk in one piece
uint32_t launch_post_occ(hipStream_t st, const ScrfLayout& lay, ScrfBatchView bv, uint32_t u0, uint32_t n_utts, uint32_t t_max,
                         uint64_t n_frames, const double* ES, const double* smax, const ScrfDpLin& o, const double* zx,
                         int* status, double* occ, double* mass_part, double* mass_s, int split_ok);
void launch_post_occ_log(hipStream_t st, const ScrfLayout& lay, ScrfBatchView bv, const uint32_t* frame_u, uint32_t u0,
                         uint64_t n_frames, const double* AD, const double* beta, const double* zx, int* status,
                         double* occ, double* mass_s);
// gamma of the queries q0 .. q0 + nq - 1 (utterance, end frame, label + L * (duration - 1)); SA = exp(S - smax) (lin) or
// alpha_dur
void launch_seg_post(hipStream_t st, const ScrfLayout& lay, ScrfBatchView bv, uint32_t u0, const uint32_t* q_u,
                     const uint32_t* q_e, const uint32_t* q_lab, uint64_t q0, uint64_t nq, int lin, const double* SA,
                     const double* smax, const ScrfDpLin& o, const double* beta, const double* zx, double* out);
// gamma [N_seg][L] = exp(alpha_dur + beta - Zx) of one utterance (zx points at its log-partition); may run in place over AD
void launch_gamma_log(hipStream_t st, const ScrfLayout& lay, uint32_t T, const double* AD, const double* beta, const double* zx,
                      double* gamma);

// scrf_fused.hip: state contractions with the window synthesis fused in (X never materialised)
// (which instantiations the launchers below start, the tile geometry, fused_supported / fused_la_supported and the
// table sizes: scrf_fused_plan.h; the launchers that take a plan are handed the one the engine made)
inline ScrfFusedShape fused_shape(const ScrfLayout& l) { return ScrfFusedShape{l.L, l.D, l.use_sb}; }
void launch_scores_fused(hipStream_t st, const ScrfFusedScoresPlan& p, const ScrfFusedArgs& fa, const ScrfLayout& lay, const double* lambda,
                         const double* P, uint64_t n_tiles, double* S, double* smax, double* s_true, const uint32_t* labels);
void launch_tile_tables(hipStream_t st, uint32_t D, uint32_t TB, int la, void* rtab);
void launch_dur_table(hipStream_t st, const ScrfLayout& lay, uint32_t W, const double* lambda, double* dtab);
void launch_avg_prefix(hipStream_t st, ScrfBatchView bv, uint32_t u0, uint32_t n_utts, uint32_t L, double* P);
// k_viterbi on float arc weights with one wavefront per utterance (fast decode; L <= 64, constant M)
void launch_viterbi_fast(hipStream_t st, const ScrfKnobs& kn, const ScrfLayout& lay, ScrfBatchView bv, uint32_t u0, uint32_t n_utts,
                         const ScrfArcSrc& src, uint16_t* bp_b, uint16_t* bp_e, uint32_t* out_labels, uint32_t* out_n, float* out_cost);
// decode mode: float arc weights + the list of entries to recompute (ScrfDecodeOut)
void launch_scores_fused_decode(hipStream_t st, const ScrfFusedScoresPlan& p, const ScrfFusedArgs& fa, const ScrfLayout& lay,
                                const double* lambda, const double* P, uint64_t n_tiles, const ScrfDecodeOut& dz);
// w1[o] = sum of |lambda| over label o's state block (features + bias weight)
void launch_state_l1(hipStream_t st, const double* lambda, const ScrfLayout& lay, double* w1);
// reference-order recomputation of the listed (row, output) arc weights from the raw frames
void launch_decode_fixup(hipStream_t st, const float* frames, uint32_t W, ScrfBatchView bv, uint32_t u0, uint32_t u1,
                         const double* lambda, const ScrfLayout& lay, const uint32_t* cnt, const uint64_t* list,
                         uint32_t cap, float* wneg);
void launch_lin_z(hipStream_t st, const ScrfLayout& lay, ScrfBatchView bv, uint32_t u0, uint32_t n_utts,
                  const double* R, double* Z);
void launch_pframe(hipStream_t st, const float* F, uint32_t W, uint64_t n_frames, const double* lambda,
                   const ScrfLayout& lay, uint32_t n_out, double* P);
void launch_ztf(hipStream_t st, const double* Zm, uint32_t n_out, const float* F, uint32_t W, uint64_t n_frames,
                uint64_t rows_per_chunk, uint32_t n_chunks, double* slab, int narrow = 0);
void launch_lin_z5(hipStream_t st, const ScrfFusedWalkPlan& p, const ScrfLayout& lay, ScrfBatchView bv, uint32_t u0, uint64_t n_frames,
                   const double* R, double* Z, double* dslab);
void launch_add_p_exp(hipStream_t st, const ScrfLayout& lay, ScrfBatchView bv, const uint32_t* frame_u, uint32_t u0, uint64_t n_frames,
                      const double* P, double* S, double* smax, double* s_true);
void launch_post_z(hipStream_t st, const ScrfKnobs& kn, const ScrfLayout& lay, ScrfBatchView bv, uint32_t u0, uint32_t n_utts,
                   const uint32_t* next_lab, const double* s_true, const double* M, int m_per_frame, double* ES,
                   const double* smax, const ScrfDpLin& o, const double* zx, double* numer_f, int* status, double* Z,
                   double* mass_s, int la = 0, uint32_t t_max = 0, uint64_t n_frames = 0);
void launch_expf_fused(hipStream_t st, const ScrfFusedExpfPlan& p, const ScrfFusedArgs& fa, const ScrfLayout& lay, const double* R,
                       uint64_t n_tiles, double* slab, double* dslab);

// ---- STDSEG (scrf_stdseg.hip): lay is the layout over FULL labels (lay.L = nLabs), La = nActualLabs
void launch_stdseg_rowinfo(hipStream_t st, ScrfBatchView bv, const uint32_t* frame_u, uint32_t u0, uint64_t n_frames,
                           uint32_t D, uint32_t* row_t, uint32_t* row_d, uint32_t* row_u);
void launch_stdseg_scores(hipStream_t st, const ScrfLayout& lay, uint32_t La, const float* X, uint64_t n_rows,
                          const uint32_t* row_t, const uint32_t* row_d, const double* lambda, double* S, double* MX);
void launch_stdseg_fb(hipStream_t st, const ScrfLayout& lay, uint32_t La, ScrfBatchView bv, uint32_t u0, uint32_t n_utts,
                      const double* S, const double* MX, double* alpha, double* beta, double* zx, int* status);
void launch_stdseg_post(hipStream_t st, const ScrfLayout& lay, uint32_t La, ScrfBatchView bv, uint32_t u0, uint32_t n_utts,
                        uint64_t n_rows, const uint32_t* row_t, const uint32_t* row_d, const uint32_t* row_u,
                        const uint32_t* prev_lab, const double* S, const double* MX, const double* alpha, const double* beta,
                        const double* zx, double* G, double* XI, double* mass_s, double* mass_t, double* numer, int* status);
void launch_stdseg_expf(hipStream_t st, const ScrfLayout& lay, uint32_t La, ScrfBatchView bv, uint32_t u0, uint32_t n_utts, uint64_t n_rows,
                        const uint32_t* row_t, const uint32_t* row_d, const uint32_t* row_u, const uint32_t* prev_lab,
                        const float* X, const double* G, const double* XI, double* grad);
// scrf_stdseg_lin.hip: STDSEG with bias-only transitions on the training path: linear-domain recursion against one
// exp(M) table, node arrays duration-major [D][frames][La], transition counts as E o (A^T B) on the MFMA
void launch_sl_tables(hipStream_t st, const ScrfLayout& lay, const double* lambda, double* E, double* ET, double* mmax);
void launch_sl_rows(hipStream_t st, ScrfBatchView bv, const uint32_t* frame_u, uint32_t u0, uint64_t n_frames, uint32_t D, uint64_t* xrow);
void launch_sl_fb(hipStream_t st, const ScrfLayout& lay, uint32_t La, ScrfBatchView bv, uint32_t u0, uint32_t n_utts, uint64_t n_frames,
                  const double* Sd, const double* E, const double* ET, const double* mmax, double* Ad, double* Bd, double* Am,
                  double* ga, double* zx, int* status);
void launch_sl_post(hipStream_t st, const ScrfLayout& lay, uint32_t La, ScrfBatchView bv, const uint32_t* frame_u, uint32_t u0,
                    uint32_t n_utts, uint64_t n_frames, const uint32_t* prev_lab, const double* lambda, const double* Sd,
                    const double* Ad, const double* Bd, const double* ga, const double* zx, double* Rd, double* Bp,
                    double* numer_f, double* numer, int* status);
void launch_sl_trans_counts(hipStream_t st, const ScrfLayout& lay, uint32_t La, ScrfBatchView bv, const uint32_t* frame_u, uint32_t u0,
                            uint64_t n_frames, const uint32_t* prev_lab, uint64_t rows_per_chunk, uint32_t n_chunks,
                            const double* Am, const double* Bp, const double* E, const double* mmax, double* slab, double* obs,
                            double* grad);
void launch_stdseg_sums(hipStream_t st, const double* numer, const double* zx, uint32_t u0, uint32_t n, double* sums);
uint64_t stdseg_num_arcs(uint32_t T, uint32_t La, uint32_t D);
void stdseg_row_arc_offsets(uint32_t T, uint32_t La, uint32_t D, std::vector<uint64_t>* off);
void launch_stdseg_arcs(hipStream_t st, const ScrfLayout& lay, uint32_t La, uint32_t T, uint64_t n_rows, const uint64_t* row_arc,
                        const double* S, const double* MX, float final_w, scrf_arc* arcs);
void launch_stdseg_viterbi(hipStream_t st, const ScrfLayout& lay, uint32_t La, ScrfBatchView bv, uint32_t u0, uint32_t n_utts,
                           const double* S, const double* MX, float* vc, uint16_t* bp, uint32_t* out_labels, uint32_t* out_n,
                           float* out_cost);

// ---- n-state frame model (scrf_nstate.hip): lay.K > 1
void launch_ns_scores(hipStream_t st, const ScrfLayout& lay, const float* X, uint64_t n_frames, const double* lambda, double* S,
                      double* TD, double* TO, double* TE);
void launch_ns_fb(hipStream_t st, const ScrfLayout& lay, ScrfBatchView bv, uint32_t u0, uint32_t n_utts, const double* S,
                  const double* TD, const double* TO, const double* TE, double* alpha, double* beta, double* zx, int* status);
void launch_ns_post(hipStream_t st, const ScrfLayout& lay, ScrfBatchView bv, const uint32_t* frame_u, uint32_t u0, uint32_t n_utts,
                    uint64_t n_frames, const double* S, const double* TD, const double* TO, const double* TE, const double* alpha,
                    const double* beta, const double* zx, double* G, double* XD, double* XO, double* XE, double* mass_s,
                    double* mass_t, double* numer, int* status);
uint32_t ns_expf_slices(uint64_t n_frames);   // frame slices of the gradient kernel: slab is [slices][lambda_len]
void launch_ns_expf(hipStream_t st, const ScrfLayout& lay, ScrfBatchView bv, const uint32_t* frame_u, uint32_t u0, uint64_t n_frames,
                    const float* X, const double* G, const double* XD, const double* XO, const double* XE, double* slab, double* grad);
uint64_t ns_num_arcs(uint32_t T, uint32_t L, uint32_t K);
void launch_ns_arcs(hipStream_t st, const ScrfLayout& lay, uint32_t T, const double* S, const double* TD, const double* TO,
                    const double* TE, float final_w, scrf_arc* arcs);
void launch_ns_viterbi(hipStream_t st, const ScrfLayout& lay, ScrfBatchView bv, uint32_t u0, uint32_t n_utts, const double* S,
                       const double* TD, const double* TO, const double* TE, float* vc, uint16_t* bp, uint32_t* out_labels,
                       uint32_t* out_n, float* out_cost);

// ---- sparse feature maps (scrf_sparse.hip): stdsparse / stdsparsetrans.  kind 0 = state (outputs = labels, rows = windows),
// kind 1 = transitions (outputs = (p, c) pairs, rows = frames read through a row map)
struct ScrfSparseIndex {
  uint32_t* hist;     // [ntiles][nidx] per-tile counts, then their exclusive prefix over the tiles
  uint32_t* tot;      // [nidx]
  uint32_t* bstart;   // [nidx + 1] bucket starts
  uint32_t* erow;     // [entries] row of each entry, buckets in (row, k) order
  float* eval;        // [entries] value of each entry
  uint32_t* sstart;   // [nidx + 1] first count segment of each bucket
  double* slab;       // [2048][n_out] bias-count partial sums
  double* part;       // [max_segs][n_out] per-segment partial counts
  uint32_t ntiles, rpt;
  uint32_t seg;       // entries per count segment
  uint64_t max_segs;
};
void sparse_index_plan(uint64_t n_rows, uint32_t nidx, uint32_t* ntiles, uint32_t* rpt);
size_t sparse_counts_bytes(uint64_t n_rows, uint32_t F, uint32_t nidx, uint32_t n_out);
void sparse_counts_carve(void* base, uint64_t n_rows, uint32_t F, uint32_t nidx, uint32_t n_out, ScrfSparseIndex* ix);
void launch_sp_relay(hipStream_t st, const double* lambda, const ScrfLayout& l, int kind, double* lamT);
void launch_sp_scores(hipStream_t st, const float* X, uint32_t F, const uint64_t* xrow, uint64_t n_rows, const double* lamT,
                      const ScrfLayout& l, int kind, double* out);
void launch_sp_counts(hipStream_t st, const float* X, uint32_t F, const uint64_t* xrow, uint64_t n_rows, const double* R,
                      const ScrfLayout& l, int kind, const ScrfSparseIndex& ix, double* grad);

// ---- beam-pruned lattices (scrf_latprune.hip): fp64 tropical forward / backward distances of the lattice's
// states, [frames of the chunk][L] each -- boundary states (B) and end states (E); the frame model uses the E arrays only --
// and fwd[final] per utterance of the batch
struct ScrfLatBufs {
  double *fB, *fE, *bB, *bE;
  double* best;   // [U], batch-absolute
};
void launch_lat_sweep(hipStream_t st, const ScrfLayout& lay, ScrfBatchView bv, uint32_t u0, uint32_t n_utts, const ScrfArcSrc& src,
                      const ScrfLatBufs& lb);
void launch_lat_count(hipStream_t st, const ScrfLayout& lay, ScrfBatchView bv, uint32_t u0, uint32_t n_utts, uint32_t t_max,
                      const ScrfArcSrc& src, const ScrfLatBufs& lb, double beam, uint32_t* counts);
void launch_lat_scan(hipStream_t st, ScrfBatchView bv, uint32_t u0, uint32_t n_utts, const uint32_t* counts, uint64_t n_nodes,
                     uint64_t* node_off, uint64_t base, uint64_t* utt_off);
void launch_lat_emit(hipStream_t st, const ScrfLayout& lay, ScrfBatchView bv, uint32_t u0, uint32_t n_utts, uint32_t t_max,
                     const ScrfArcSrc& src, const ScrfLatBufs& lb, double beam, const uint64_t* node_off, uint64_t base, uint64_t cap,
                     scrf_arc* out);

// ---- forced alignment (scrf_align.hip)
struct ScrfAlignArgs {
  const uint32_t* phones;      // transcripts of the batch, back to back
  const uint64_t* phone_off;   // [U + 1]
  const uint64_t* bp_off;      // [U + 1] back-pointer cells before each utterance: T * K of every transcript that fits
  uint16_t* bp;                // the chunk's cells; utterance u's start at bp_off[u] - bp_off[u0]
  int mode;                    // scrf_align_mode
};
// does a transcript of K phones fit an utterance of T frames?  (host: sizes the back pointers; device: the same decision)
__host__ __device__ inline bool scrf_align_feasible(uint32_t T, uint64_t K, uint32_t D, int mode) {
  if (T == 0 || K == 0 || K > T) return false;
  return mode != SCRF_ALIGN_ONE || K * D >= T;
}
// can end(t, k) lie on a complete path?  (shared by the search and by the transcript sums of scrf_transcript.hip)
__device__ inline bool align_live(int t, int k, int T, int K, int D, int mode) {
  if (k > t || K - 1 - k > T - 1 - t) return false;
  if (mode == SCRF_ALIGN_ONE && ((long long)(k + 1) * D < t + 1 || (long long)(K - 1 - k) * D < T - 1 - t)) return false;
  return true;
}

// the same for boundary(t, k), the start of position k's next segment at frame t: k segments (ONE) cover the t frames before it
__device__ inline bool align_live_b(int t, int k, int T, int K, int D, int mode) {
  if (k > t || K - k > T - t) return false;
  if (mode == SCRF_ALIGN_ONE && ((long long)k * D < t || (long long)(K - k) * D < T - t)) return false;
  return true;
}

void launch_align_wave(hipStream_t st, const ScrfLayout& lay, ScrfBatchView bv, uint32_t u0, uint32_t n_utts, const ScrfArcSrc& src,
                       const ScrfAlignArgs& aa, uint32_t* out_labels, uint32_t* out_n, float* out_cost);
void launch_align_group(hipStream_t st, const ScrfLayout& lay, ScrfBatchView bv, uint32_t u0, uint32_t n_utts, uint32_t k_max,
                        const ScrfArcSrc& src, const ScrfAlignArgs& aa, uint32_t* out_labels, uint32_t* out_n, float* out_cost);

// ---- transcript scoring (scrf_transcript.hip)
struct ScrfTransArgs {
  const uint32_t* phones;      // transcripts of the batch, back to back
  const uint64_t* phone_off;   // [U + 1]
  const uint64_t* cell_off;    // [U + 1] (frame, position) cells before each utterance: T * K of every transcript that fits
  const uint32_t* inv_pos;     // [sum K] per utterance its positions sorted by label, ascending inside a label
  const uint32_t* inv_off;     // [U][L + 1] where each label's positions start in the utterance's part of inv_pos
  double* aB;                  // the chunk's forward cells [T][K]; utterance u's start at cell_off[u] - cell_off[u0]
  double* bE;                  // the chunk's backward cells, laid out the same
  int mode;                    // scrf_align_mode
  int lin;                     // the scores are exp(S - smax) with smax per row (the linear-domain path), not S
  int want_seg;                // segment queries follow: run the backward sweep even without frame / end output
};
// log_num [U], occ [sum T][L] (or NULL), endp [sum T] (or NULL): arrays of the whole batch.  k_max: the longest transcript
// of the chunk that fits
void launch_transcript(hipStream_t st, const ScrfLayout& lay, ScrfBatchView bv, uint32_t u0, uint32_t n_utts, uint64_t k_max,
                       const double* S, const double* smax, const double* M, int m_per_frame, const ScrfTransArgs& ta,
                       int* status, double* log_num, double* occ, double* endp);
void launch_transcript_seg(hipStream_t st, const ScrfLayout& lay, ScrfBatchView bv, uint32_t u0, const uint32_t* q_u,
                           const uint32_t* q_e, const uint32_t* q_lab, uint64_t q0, uint64_t nq, const double* S,
                           const double* smax, const ScrfTransArgs& ta, const double* log_num, double* out);


// ---- N-best decoding (scrf_nbest.hip)
struct ScrfNbestBufs {
  uint32_t N;           // list length = the n_best of the call
  uint32_t* bp_b;       // [frames of the chunk][L][N] boundary(t, l)[r] (frame model: state): predecessor label << 16 | its rank
  uint32_t* bp_e;       // [frames of the chunk][L][N] end(t, l)[r]: duration << 16 | rank in boundary(t - d + 1, l)
  float* fin_cost;      // [utterances of the chunk][N] ascending, +inf where the utterance has fewer paths
  uint32_t* fin_ptr;    // [utterances of the chunk][N] last label << 16 | its rank in end(T-1, .)
  uint32_t* cnt;        // [utterances of the chunk][N] segments of the hypothesis, 0: none
  uint64_t* lab_pos;    // [utterances * N + 1] where each hypothesis's labels start in the result
  uint64_t* hyp_pos;    // [utterances * N] index of each hypothesis in the result
  uint64_t* tot;        // {labels, hypotheses} of the chunk
};
void launch_nbest(hipStream_t st, const ScrfLayout& lay, ScrfBatchView bv, uint32_t u0, uint32_t n_utts, const ScrfArcSrc& src,
                  const ScrfNbestBufs& nb);
void launch_nbest_count(hipStream_t st, const ScrfLayout& lay, ScrfBatchView bv, uint32_t u0, uint32_t n_utts, int frame_model,
                        const ScrfNbestBufs& nb);
// lab_base / hyp_base: labels and hypotheses of the chunks done; hyp_off [U + 1]: the batch's hypothesis offsets
void launch_nbest_scan(hipStream_t st, const ScrfNbestBufs& nb, uint32_t u0, uint32_t n_utts, uint64_t lab_base, uint64_t hyp_base,
                       uint64_t* hyp_off);
// res_lab [lab_cap], res_off [hyp_cap + 1], res_cost [hyp_cap]: the result of the whole batch
void launch_nbest_trace(hipStream_t st, const ScrfLayout& lay, ScrfBatchView bv, uint32_t u0, uint32_t n_utts, int frame_model,
                        const ScrfNbestBufs& nb, uint64_t lab_cap, uint64_t hyp_cap, uint32_t* res_lab, uint64_t* res_off, float* res_cost);

#endif  // SCRF_KERNELS_H_
