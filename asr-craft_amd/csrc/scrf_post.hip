// scrf_post.hip -- posterior OUTPUT of the segmental recursion (scrf_posteriors_batch): from the segment
// posteriors gamma(t, d, l) of a label-less batch
//   occ[f][l] = sum of gamma(t, d, l) over the segments that cover frame f (t - d + 1 <= f <= t)   frame posterior
//   end[t]    = sum over d, l of gamma(t, d, l)                                                    boundary posterior
//   seg_post  = gamma(e, d, l) of listed segments                                                  segment confidence
// (the per-frame label posteriors of decoders/CRF_NewLocalPosteriorBuilder.cpp:61-188, generalised to segments).
// Nothing here needs labels, writes R or feeds the gradient.
//   k_post_occ      after the scaled linear-domain recursion (scrf_dplin.hip): one walk over exp(S - smax)
//   k_post_occ_log  after the log-domain recursions (k_fb / k_dp_wave): gamma = exp(alpha_dur + beta - Zx)
//   k_seg_post      gather of single gamma entries, either domain
#include "scrf_dp_common.h"

// ------------------------------------------------------------------------------------------
// k_post_occ: one wavefront per (utterance, 64 outputs[, frame segment]) walks the utterance once, like k_post_z
// (scrf_fused.hip), and forms
//   gamma[(t,d)][o] = p[t-d][o] * es[(t,d)][o] * b[t][o] * exp(gp[t-d] + smax[(t,d)] + gb[t] - Zx)
// in registers (t - d = -1: p = 1, gp = 0).  es is read once and not written.  The last D alpha-plus-transition
// vectors sit in an LDS ring (lane-private columns), the D scale factors of a frame are computed by lanes 0..D-1 and
// broadcast through LDS.
// occ: a segment reaches D - 1 frames back, so the open sums of the last D frames sit in a second LDS ring (slot of
// frame f = f mod D): at frame t the suffix sums u_j = sum_{d > j} gamma(t, d) are added to the slots of frames t - j,
// then frame t - D + 1 has seen its last segment and retires to memory.
// end[t] (= the node's state mass k_mass_check tests) is the wave sum of the row sums, written per 64-output group to
// mass[group][frame]: groups are added afterwards in a fixed order (k_sum_groups), no floating-point atomics anywhere.
// Frame segments (gridDim.z > 1, a launch of few utterances): segment z OWNS frames fa <= f < fb and walks on to frame
// fb + D - 2, the last whose segments cover an owned frame; what it adds to frames it does not own stays in the ring.
// Every owned frame receives the same terms in the same order as in the unsplit walk, so the two forms are
// bit-identical.  RW = lanes of the rings that exist (48 when L <= 48).
// ------------------------------------------------------------------------------------------
template <int DMAX, int RW>
__global__ __launch_bounds__(64, 2) void k_post_occ(ScrfLayout lay, ScrfBatchView bv, uint32_t u0,
                                                    const double* __restrict__ ES, const double* __restrict__ smax,
                                                    ScrfDpLin o_, const double* __restrict__ zx,
                                                    int* __restrict__ status, double* __restrict__ occ,
                                                    double* __restrict__ mass, uint64_t n_frames, int seg_len) {
  __shared__ double pring[DMAX * RW];
  __shared__ double oring[DMAX * RW];
  __shared__ double fsb[DMAX < 64 ? DMAX : 64];
  const uint32_t D = lay.D, L = lay.L;
  const uint32_t u = u0 + blockIdx.x;
  const int T = (int)bv.T[u];
  const uint32_t lane = threadIdx.x;
  const uint32_t o = blockIdx.y * 64 + lane;
  const bool act = o < L;
  const uint32_t oc = act ? o : L - 1;
  const uint64_t f_base = bv.frame_off[u] - bv.frame_off[u0], s_base = bv.seg_off[u] - bv.seg_off[u0];
  const double* ESu = ES + s_base * L + oc;
  const double* smu = smax + s_base;
  const double Zx = zx[u];
  const double LN_MAX = 709.782712893384;
  const uint32_t rl = lane < (uint32_t)RW ? lane : RW - 1;   // ring column (lanes past RW are never active)
  const bool rw_ok = lane < (uint32_t)RW;
  const int fa = (int)blockIdx.z * seg_len;                  // owned frames fa .. fb - 1 (seg_len >= T when unsplit)
  if (fa >= T) return;
  const int fb = (fa + seg_len < T) ? fa + seg_len : T;
  const int fe = (fb + (int)D - 1 < T) ? fb + (int)D - 1 : T;   // frames walked: fa .. fe - 1
#pragma unroll
  for (int j = 0; j < DMAX; j++) if (rw_ok) oring[j * RW + lane] = 0.0;
  int slot = fa % (int)D;   // ring slot of frame t (= t mod D)
  for (int j = 1; j <= (int)D && j <= fa; j++)
    if (rw_ok) pring[((fa - j) % (int)D) * RW + lane] = o_.p[(f_base + fa - j) * L + oc];
  int err = 0;
#pragma unroll 1
  for (int t = fa; t < fe; t++) {
    const uint32_t nd = scrf_node_max_dur((uint32_t)t, D), np = scrf_num_prev((uint32_t)t, D);
    const uint64_t row0 = scrf_seg_base((uint32_t)t, D);
    double r[DMAX];
#pragma unroll
    for (int d0 = 0; d0 < DMAX; d0++) r[d0] = ((uint32_t)d0 < nd) ? __builtin_nontemporal_load(&ESu[(row0 + d0) * L]) : 0.0;
    const double b = o_.b[(f_base + t) * L + oc];
    const double pnew = (t + 1 < T) ? o_.p[(f_base + t) * L + oc] : 0.0;
    {  // scale factor of duration d0 = lane
      double x = -INFINITY;
      if (lane < nd) {
        x = ((lane < np) ? o_.gp[f_base + t - 1 - lane] : 0.0) + smu[row0 + lane] + o_.gb[f_base + t] - Zx;
        if (x >= LN_MAX) err = SCRF_ERR_NUMERIC;
      }
      if (lane < (DMAX < 64 ? DMAX : 64)) fsb[lane] = (lane < nd) ? exp(x) : 0.0;
    }
    __syncthreads();   // the broadcast of fsb (both rings are lane-private: only fsb crosses lanes)
    double gs = 0.0;
#pragma unroll
    for (int d0 = 0; d0 < DMAX; d0++) {
      int ps = slot - 1 - d0;            // ring slot of p[t-1-d0]
      if (ps < 0) ps += (int)D;
      const double pv = ((uint32_t)d0 < np) ? pring[(((uint32_t)d0 < np) ? ps : 0) * RW + rl] : 1.0;
      const double g = (pv * r[d0]) * (b * fsb[d0]);   // r[d0] = 0 and fsb[d0] = 0 past nd
      r[d0] = g;
      gs += g;
    }
    if (t < fb) {
      const double m = wave_sum_f64_dpp(act ? gs : 0.0);
      if (lane == 0) mass[(uint64_t)blockIdx.y * n_frames + f_base + t] = m;
    }
    if (occ) {
      // suffix sums, durations descending; slot of frame t - d0 = (slot - d0) mod D
      double usum = 0.0;
#pragma unroll
      for (int d0 = DMAX - 1; d0 >= 0; d0--) {
        if ((uint32_t)d0 >= D) continue;
        usum += r[d0];
        int zsl = slot - d0;
        if (zsl < 0) zsl += (int)D;
        if (rw_ok) oring[zsl * RW + lane] += usum;   // every ring cell belongs to one lane
      }
      // frame t - D + 1 has seen its last segment
      const int zf = slot + 1 == (int)D ? 0 : slot + 1;
      const double zv = oring[zf * RW + rl];
      const int f = t + 1 - (int)D;
      if (act && f >= fa) __builtin_nontemporal_store(zv, &occ[(f_base + f) * L + o]);   // f < fb by the choice of fe
      if (rw_ok) oring[zf * RW + lane] = 0.0;
    }
    if (rw_ok) pring[slot * RW + lane] = pnew;
    slot = (slot + 1 == (int)D) ? 0 : slot + 1;
    __syncthreads();   // fsb is rewritten by the next frame
  }
  if (occ && act && fe == T) {
    // frames T - D + 1 .. T - 1 are still open in the ring
    for (int j = 1; j < (int)D && j <= T; j++) {
      const int f = T - j;
      if (f >= fa && f < fb) occ[(f_base + f) * L + o] = oring[(f % (int)D) * RW + rl];
    }
  }
  if (__any(err != 0) && lane == 0) atomicMax(&status[u], SCRF_ERR_NUMERIC);
}

// mass_s[f] = sum over the 64-output groups, ascending
__global__ void k_sum_groups(const double* __restrict__ part, uint32_t n_groups, uint64_t n_frames, double* __restrict__ out) {
  const uint64_t f = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= n_frames) return;
  double s = part[f];
  for (uint32_t g = 1; g < n_groups; g++) s += part[(uint64_t)g * n_frames + f];
  out[f] = s;
}

uint32_t launch_post_occ(hipStream_t st, const ScrfLayout& lay, ScrfBatchView bv, uint32_t u0, uint32_t n_utts, uint32_t t_max,
                         uint64_t n_frames, const double* ES, const double* smax, const ScrfDpLin& o, const double* zx,
                         int* status, double* occ, double* mass_part, double* mass_s, int split_ok) {
  if (n_utts == 0) return 0;
  // (the frame segments: walk_segments, launch_post_z's rule; split_ok = 0: never -- the results do not change)
  const ScrfPostOccPlan p = post_occ_plan(dp_shape(lay), n_utts, t_max, split_ok);
  double* mp = p.sum_groups ? mass_part : mass_s;
#define PO_CASE(N, R) \
  case (N) * 64 + (R): hipLaunchKernelGGL((k_post_occ<N, R>), dim3(p.gx, p.gy, p.nz), dim3(64), 0, st, lay, bv, u0, ES, smax, o, zx, status, occ, mp, n_frames, p.seg_len); break
#define PO_CASES(N) PO_CASE(N, 48); PO_CASE(N, 64)
  switch (p.dmax * 64 + p.rw) { PO_CASES(8); PO_CASES(16); PO_CASES(25); PO_CASES(32); PO_CASES(40); }
#undef PO_CASES
#undef PO_CASE
  if (p.sum_groups)
    hipLaunchKernelGGL(k_sum_groups, dim3((uint32_t)((n_frames + 255) / 256)), dim3(256), 0, st, mass_part, p.gy, n_frames, mass_s);
  return p.nz;
}

// ------------------------------------------------------------------------------------------
// k_post_occ_log: the same sums from the log-domain arrays the recursions k_fb / k_dp_wave leave behind,
//   gamma[(t,d)][l] = exp(alpha_dur[(t,d)][l] + beta[t][l] - Zx).
// The parity form (SCRF_PREC_EXACT, shapes the wavefront recursion does not take, the redo after SCRF_ERR_NUMERIC): one
// workgroup per frame f, a thread per label; the terms of occ[f][l] are added for t = f .. f + D - 1 ascending, durations
// descending inside a frame -- a fixed order.  end[f] is a tree sum over the workgroup's threads (fixed as well).
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_post_occ_log(ScrfLayout lay, ScrfBatchView bv, const uint32_t* __restrict__ frame_u,
                                                      uint32_t u0, const double* __restrict__ AD,
                                                      const double* __restrict__ beta, const double* __restrict__ zx,
                                                      int* __restrict__ status, double* __restrict__ occ,
                                                      double* __restrict__ mass_s) {
  __shared__ double red[256];
  const uint32_t L = lay.L, D = lay.D;
  const uint64_t fi = blockIdx.x;   // frame index inside the chunk
  const uint64_t gf = bv.frame_off[u0] + fi;
  const uint32_t u = frame_u[gf];
  const uint32_t t = (uint32_t)(gf - bv.frame_off[u]);
  const uint32_t T = bv.T[u];
  const uint64_t s_base = bv.seg_off[u] - bv.seg_off[u0];
  const double Zx = zx[u];
  const double LN_MAX = 709.782712893384;
  int err = 0;
  double es = 0.0;
  for (uint32_t l = threadIdx.x; l < L; l += blockDim.x) {
    if (occ) {
      double acc = 0.0;
      const uint32_t t_hi = (t + D < T) ? t + D : T;
      for (uint32_t tt = t; tt < t_hi; tt++) {
        const uint32_t nd = scrf_node_max_dur(tt, D);
        const uint64_t row0 = s_base + scrf_seg_base(tt, D);
        const double bt = beta[(fi + (tt - t)) * L + l];
        for (uint32_t d = nd; d >= tt - t + 1; d--) {
          const double x = AD[(row0 + d - 1) * L + l] + bt - Zx;
          if (!(x < LN_MAX)) err = SCRF_ERR_NUMERIC;
          acc += exp(fmin(x, 700.0));
        }
      }
      occ[fi * L + l] = acc;
    }
    {
      const uint32_t nd = scrf_node_max_dur(t, D);
      const uint64_t row0 = s_base + scrf_seg_base(t, D);
      const double bt = beta[fi * L + l];
      for (uint32_t d = nd; d >= 1; d--) {
        const double x = AD[(row0 + d - 1) * L + l] + bt - Zx;
        if (!(x < LN_MAX)) err = SCRF_ERR_NUMERIC;
        es += exp(fmin(x, 700.0));
      }
    }
  }
  red[threadIdx.x] = es;
  __syncthreads();
  for (uint32_t s = 128; s >= 1; s >>= 1) {
    if (threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) mass_s[fi] = red[0];
  if (err) atomicMax(&status[u], err);
}

void launch_post_occ_log(hipStream_t st, const ScrfLayout& lay, ScrfBatchView bv, const uint32_t* frame_u, uint32_t u0,
                         uint64_t n_frames, const double* AD, const double* beta, const double* zx, int* status,
                         double* occ, double* mass_s) {
  if (n_frames == 0) return;
  hipLaunchKernelGGL(k_post_occ_log, dim3((uint32_t)n_frames), dim3(256), 0, st, lay, bv, frame_u, u0, AD, beta, zx, status, occ, mass_s);
}

// ------------------------------------------------------------------------------------------
// k_seg_post: one thread per query (utterance, end frame e, label value l + L (d - 1)) evaluates gamma(e, d, l) from the
// arrays of the chunk's recursion (LIN: the linear-domain vectors, else alpha_dur / beta).  The host has checked that
// every (e, d) exists and every label is in range.
// ------------------------------------------------------------------------------------------
template <int LIN>
__global__ void k_seg_post(ScrfLayout lay, ScrfBatchView bv, uint32_t u0, const uint32_t* __restrict__ q_u,
                           const uint32_t* __restrict__ q_e, const uint32_t* __restrict__ q_lab, uint64_t q0, uint64_t nq,
                           const double* __restrict__ SA, const double* __restrict__ smax, ScrfDpLin o_,
                           const double* __restrict__ beta, const double* __restrict__ zx, double* __restrict__ out) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nq) return;
  const uint64_t q = q0 + i;
  const uint32_t L = lay.L, D = lay.D;
  const uint32_t u = q_u[q], e = q_e[q], lab = q_lab[q];
  const uint32_t l = lab % L, d0 = lab / L;
  const uint64_t fi = bv.frame_off[u] - bv.frame_off[u0] + e;
  const uint64_t row = bv.seg_off[u] - bv.seg_off[u0] + scrf_seg_base(e, D) + d0;
  const double Zx = zx[u];
  double g;
  if (LIN) {
    const bool prev = d0 < scrf_num_prev(e, D);
    const double x = (prev ? o_.gp[fi - 1 - d0] : 0.0) + smax[row] + o_.gb[fi] - Zx;
    const double pv = prev ? o_.p[(fi - 1 - d0) * L + l] : 1.0;
    g = (pv * SA[row * L + l]) * (o_.b[fi * L + l] * exp(fmin(x, 700.0)));
  } else {
    g = exp(fmin(SA[row * L + l] + beta[fi * L + l] - Zx, 700.0));
  }
  out[q] = g;
}

void launch_seg_post(hipStream_t st, const ScrfLayout& lay, ScrfBatchView bv, uint32_t u0, const uint32_t* q_u,
                     const uint32_t* q_e, const uint32_t* q_lab, uint64_t q0, uint64_t nq, int lin, const double* SA,
                     const double* smax, const ScrfDpLin& o, const double* beta, const double* zx, double* out) {
  if (nq == 0) return;
  const dim3 grid((uint32_t)((nq + 255) / 256));
  if (lin) hipLaunchKernelGGL(k_seg_post<1>, grid, dim3(256), 0, st, lay, bv, u0, q_u, q_e, q_lab, q0, nq, SA, smax, o, beta, zx, out);
  else hipLaunchKernelGGL(k_seg_post<0>, grid, dim3(256), 0, st, lay, bv, u0, q_u, q_e, q_lab, q0, nq, SA, smax, o, beta, zx, out);
}

// gamma [N_seg][L] of ONE utterance from its log-domain arrays (parity hook scrf_seg_posteriors): one workgroup per frame
__global__ __launch_bounds__(256) void k_gamma_log(ScrfLayout lay, uint32_t T, const double* AD,
                                                   const double* __restrict__ beta, const double* __restrict__ zx,
                                                   double* gamma) {   // gamma may be AD (in place): no restrict on the two
  const uint32_t L = lay.L, D = lay.D, t = blockIdx.x;
  const uint32_t nd = scrf_node_max_dur(t, D);
  const uint64_t row0 = scrf_seg_base(t, D);
  const double Zx = zx[0];
  for (uint32_t idx = threadIdx.x; idx < nd * L; idx += blockDim.x) {
    const uint32_t l = idx % L;
    gamma[row0 * L + idx] = exp(fmin(AD[row0 * L + idx] + beta[(uint64_t)t * L + l] - Zx, 700.0));
  }
}
void launch_gamma_log(hipStream_t st, const ScrfLayout& lay, uint32_t T, const double* AD, const double* beta, const double* zx,
                      double* gamma) {
  if (T == 0) return;
  hipLaunchKernelGGL(k_gamma_log, dim3(T), dim3(256), 0, st, lay, T, AD, beta, zx, gamma);
}
