// scrf_softnum.hip -- the numerator of the soft-alignment gradient (scrf_fb_transcript_batch), gfx950.
//
// The gradient of A(q) - Zx is E[f | x, transcript] - E[f | x].  The training pass forms the second expectation with labels
// that are all SCRF_LAB_BAD (R = -gamma, XI = -xi); these kernels form the first one from what k_transcript left behind (the
// aB / bE cells and A, scrf_transcript.hip) and add it in, so that the count contractions run once, over the difference:
//   G(row(t,d), l) = sum over the positions k with q_k = l, ascending, of exp( aB(t-d+1,k) + S(t,d,l) + bE(t,k) - A )
//   xa(t,k) = exp( aE(t-1,k-1) + M_t(q_{k-1},q_k) + bB(t,k) - A )     advance, k >= 1, boundary t >= 1
//   xs(t,k) = exp( aE(t-1,k)   + M_t(q_k,q_k)     + bB(t,k) - A )     stay, SCRF_ALIGN_RUNS only
// k_transcript keeps aE and bB in LDS only, so k_soft_trans forms them again per cell from the stored aB / bE and the scores
// (D terms each, max-shifted through LseAcc, the sweep's own order); the exponentials xa / xs are taken where they are
// consumed (k_soft_add_xi, k_soft_pos_sums), one exp per live cell and direction.
//
//   k_soft_state        one thread per (window row, label) of every utterance: G
//   k_soft_trans        one thread per (frame, position) cell: aE, bB
//   k_soft_add_r        R += G
//   k_soft_add_xi       transition features: one thread per frame row f of XI (the transition out of frame f, k_xi_full's
//                       convention), positions ascending
//   k_soft_pos_sums     bias-only transitions: one thread per position, the sums of xa / xs over the frames, ascending
//   k_soft_trans_table  bias-only transitions: per utterance an [L][L] table, one thread per (p, c), positions ascending; the
//                       tables of a chunk go into the transition-bias weights ascending by utterance (k_reduce_xiacc, the
//                       reduction of the workgroup recursion's per-utterance xi)
// k_soft_state and k_soft_trans read the scores and therefore run BEFORE the posterior walk of the linear-domain path, which
// overwrites them with R; the add kernels run behind it.  fp64 throughout, no floating-point atomic, every sum in an order
// fixed by the transcript alone: two runs and any chunking of the batch give the same G, aE, bB and per-position sums.
#include <float.h>
#include <math.h>

#include "scrf_dp_common.h"
#include "scrf_lse.h"
#include "scrf_softnum.h"

#define SN_THREADS 256

// the fp64 log score of a row, in either form the score stage leaves behind (tr_score of scrf_transcript.hip)
__device__ __forceinline__ double sn_score(const double* __restrict__ Su, const double* __restrict__ smu, int lin, uint64_t row,
                                           uint32_t L, uint32_t q) {
  const double v = Su[row * L + q];
  return lin ? smu[row] + log(v) : v;
}

// the utterance of a workgroup (blockIdx.y) and whether it has a numerator at all
struct SnUtt {
  uint32_t u;
  int T, K;
  double A;
  bool ok;
  uint64_t s_base, f_base, c_base, p_base;
  const uint32_t* ph;
};
__device__ __forceinline__ SnUtt sn_utt(const ScrfLayout& lay, const ScrfBatchView& bv, uint32_t u0, const ScrfTransArgs& ta,
                                        const ScrfSoftArgs& sa) {
  SnUtt x;
  x.u = u0 + blockIdx.y;
  x.T = (int)bv.T[x.u];
  const uint64_t K64 = ta.phone_off[x.u + 1] - ta.phone_off[x.u];
  x.K = (int)K64;
  x.A = sa.log_num[x.u];
  x.ok = scrf_align_feasible((uint32_t)x.T, K64, lay.D, ta.mode) && sa.status[x.u] == 0 && x.A > -INFINITY && x.A < INFINITY;
  x.s_base = bv.seg_off[x.u] - bv.seg_off[u0];
  x.f_base = bv.frame_off[x.u] - bv.frame_off[u0];
  x.c_base = ta.cell_off[x.u] - ta.cell_off[u0];
  x.p_base = ta.phone_off[x.u] - ta.phone_off[u0];
  x.ph = ta.phones + ta.phone_off[x.u];
  return x;
}

// ------------------------------------------------------------------------------------------
// k_soft_state: thread i of an utterance = (t, d, l), d <= min(t + 1, D); every row of the utterance is written (zeros for
// an utterance without a numerator and for a label the transcript does not hold, which costs no exp)
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SN_THREADS) void k_soft_state(ScrfLayout lay, ScrfBatchView bv, uint32_t u0, const double* __restrict__ S,
                                                           const double* __restrict__ smax, ScrfTransArgs ta, ScrfSoftArgs sa) {
  const SnUtt x = sn_utt(lay, bv, u0, ta, sa);
  const uint32_t L = lay.L, D = lay.D;
  const uint64_t n = (uint64_t)x.T * D * L;
  const double* Su = S + x.s_base * L;
  const double* smu = ta.lin ? smax + x.s_base : nullptr;
  const double* aBs = ta.aB + x.c_base;
  const double* bEs = ta.bE + x.c_base;
  const uint32_t* ioff = ta.inv_off + (size_t)x.u * (L + 1);
  const uint32_t* ipos = ta.inv_pos + ta.phone_off[x.u];
  for (uint64_t i = (uint64_t)blockIdx.x * SN_THREADS + threadIdx.x; i < n; i += (uint64_t)gridDim.x * SN_THREADS) {
    const uint32_t l = (uint32_t)(i % L), d = (uint32_t)((i / L) % D) + 1, t = (uint32_t)(i / ((uint64_t)L * D));
    if (d > t + 1) continue;   // no such window
    const uint64_t row = scrf_seg_base(t, D) + d - 1;
    double g = 0.0;
    if (x.ok && ioff[l] < ioff[l + 1]) {
      const double sc = sn_score(Su, smu, ta.lin, row, L, l);
      const uint32_t ts = t + 1 - d;
      for (uint32_t j = ioff[l]; j < ioff[l + 1]; j++) {
        const uint32_t k = ipos[j];
        const double ab = ts == 0 ? (k == 0 ? 0.0 : -INFINITY) : aBs[(size_t)ts * x.K + k];
        const double be = bEs[(size_t)t * x.K + k];
        if (ab > -INFINITY && be > -INFINITY) g += exp(ab + sc + be - x.A);   // a dead cell adds nothing
      }
    }
    sa.G[(x.s_base + row) * L + l] = g;
  }
}

void launch_soft_state(hipStream_t st, const ScrfLayout& lay, ScrfBatchView bv, uint32_t u0, uint32_t n_utts, uint32_t t_max,
                       const double* S, const double* smax, const ScrfTransArgs& ta, const ScrfSoftArgs& sa) {
  if (n_utts == 0 || t_max == 0) return;
  const uint64_t n = (uint64_t)t_max * lay.D * lay.L;
  const uint32_t gx = (uint32_t)std::min<uint64_t>((n + SN_THREADS - 1) / SN_THREADS, 4096);
  hipLaunchKernelGGL(k_soft_state, dim3(gx, n_utts), dim3(SN_THREADS), 0, st, lay, bv, u0, S, smax, ta, sa);
}

// ------------------------------------------------------------------------------------------
// k_soft_trans: thread i of an utterance = cell (t, k).  aE(t, k) in the forward sweep's order (the start term, then d
// descending); bB(t, k), t >= 1, in the backward sweep's (d ascending).  Dead cells are -inf and read nothing.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SN_THREADS) void k_soft_trans(ScrfLayout lay, ScrfBatchView bv, uint32_t u0, const double* __restrict__ S,
                                                           const double* __restrict__ smax, ScrfTransArgs ta, ScrfSoftArgs sa) {
  const SnUtt x = sn_utt(lay, bv, u0, ta, sa);
  if (!x.ok) return;   // no cells (a transcript that does not fit) or none that is read
  const int L = lay.L, D = lay.D, T = x.T, K = x.K, mode = ta.mode, lin = ta.lin;
  const double* Su = S + x.s_base * L;
  const double* smu = lin ? smax + x.s_base : nullptr;
  const double* aBs = ta.aB + x.c_base;
  const double* bEs = ta.bE + x.c_base;
  double* aEs = sa.aE + x.c_base;
  double* bBs = sa.bB + x.c_base;
  const uint64_t n = (uint64_t)T * K;
  for (uint64_t i = (uint64_t)blockIdx.x * SN_THREADS + threadIdx.x; i < n; i += (uint64_t)gridDim.x * SN_THREADS) {
    const int t = (int)(i / K), k = (int)(i % K);
    const uint32_t q = x.ph[k];
    double e = -INFINITY, b = -INFINITY;
    if (align_live(t, k, T, K, D, mode)) {
      const uint64_t base = scrf_seg_base(t, D);
      LseAcc a;
      if (k == 0 && t < D) a.add(sn_score(Su, smu, lin, base + t, L, q));
      for (int d = t < D ? t : D; d >= 1; d--) {
        const double ab = aBs[(size_t)(t - d + 1) * K + k];
        if (ab > -INFINITY) a.add(ab + sn_score(Su, smu, lin, base + d - 1, L, q));
      }
      e = a.value();
    }
    if (t >= 1 && align_live_b(t, k, T, K, D, mode)) {
      LseAcc a;
      const int nd = T - t < D ? T - t : D;
      for (int d = 1; d <= nd; d++) {
        const int te = t + d - 1;
        const double be = bEs[(size_t)te * K + k];
        if (be > -INFINITY) a.add(sn_score(Su, smu, lin, scrf_seg_base(te, D) + d - 1, L, q) + be);
      }
      b = a.value();
    }
    aEs[i] = e;
    bBs[i] = b;
  }
}

void launch_soft_trans(hipStream_t st, const ScrfLayout& lay, ScrfBatchView bv, uint32_t u0, uint32_t n_utts, uint64_t cells_max,
                       const double* S, const double* smax, const ScrfTransArgs& ta, const ScrfSoftArgs& sa) {
  if (n_utts == 0 || cells_max == 0) return;
  const uint32_t gx = (uint32_t)std::min<uint64_t>((cells_max + SN_THREADS - 1) / SN_THREADS, 4096);
  hipLaunchKernelGGL(k_soft_trans, dim3(gx, n_utts), dim3(SN_THREADS), 0, st, lay, bv, u0, S, smax, ta, sa);
}

// the two transition numerators into boundary t >= 1 at position k, from the cells; 0 for a dead cell
__device__ __forceinline__ void sn_xa_xs(const SnUtt& x, const double* __restrict__ aEs, const double* __restrict__ bBs,
                                         const double* __restrict__ Mt, int L, int mode, int t, int k, double* xa, double* xs) {
  *xa = *xs = 0.0;
  const double b = bBs[(size_t)t * x.K + k];
  if (!(b > -INFINITY)) return;
  const uint32_t q = x.ph[k];
  if (k >= 1) {
    const double e = aEs[(size_t)(t - 1) * x.K + k - 1];
    if (e > -INFINITY) *xa = exp(e + Mt[(size_t)x.ph[k - 1] * L + q] + b - x.A);
  }
  if (mode == SCRF_ALIGN_RUNS) {
    const double e = aEs[(size_t)(t - 1) * x.K + k];
    if (e > -INFINITY) *xs = exp(e + Mt[(size_t)q * L + q] + b - x.A);
  }
}

__global__ void k_soft_add_r(double* __restrict__ R, const double* __restrict__ G, uint64_t n) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) R[i] += G[i];
}
void launch_soft_add_r(hipStream_t st, double* R, const double* G, uint64_t n) {
  if (n == 0) return;
  const uint32_t gx = (uint32_t)std::min<uint64_t>((n + SN_THREADS - 1) / SN_THREADS, 65535);
  hipLaunchKernelGGL(k_soft_add_r, dim3(gx), dim3(SN_THREADS), 0, st, R, G, n);
}

// ------------------------------------------------------------------------------------------
// k_soft_add_xi: M is one matrix per frame of the chunk.  Row f of XI belongs to one thread: no two threads add into one
// element, and the positions come in ascending order.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SN_THREADS) void k_soft_add_xi(ScrfLayout lay, ScrfBatchView bv, uint32_t u0, const double* __restrict__ M,
                                                            ScrfTransArgs ta, ScrfSoftArgs sa, double* __restrict__ XI) {
  const SnUtt x = sn_utt(lay, bv, u0, ta, sa);
  if (!x.ok) return;
  const int L = lay.L;
  const size_t LL = (size_t)L * L;
  const double* aEs = sa.aE + x.c_base;
  const double* bBs = sa.bB + x.c_base;
  for (int f = blockIdx.x * SN_THREADS + threadIdx.x; f + 1 < x.T; f += gridDim.x * SN_THREADS) {
    const int t = f + 1;
    const double* Mt = M + (x.f_base + t) * LL;
    double* out = XI + (x.f_base + f) * LL;
    for (int k = 0; k < x.K; k++) {
      double xa, xs;
      sn_xa_xs(x, aEs, bBs, Mt, L, ta.mode, t, k, &xa, &xs);
      const uint32_t q = x.ph[k];
      if (xa != 0.0) out[(size_t)x.ph[k - 1] * L + q] += xa;
      if (xs != 0.0) out[(size_t)q * L + q] += xs;
    }
  }
}

void launch_soft_add_xi(hipStream_t st, const ScrfLayout& lay, ScrfBatchView bv, uint32_t u0, uint32_t n_utts, uint32_t t_max,
                        const double* M, const ScrfTransArgs& ta, const ScrfSoftArgs& sa, double* XI) {
  if (n_utts == 0 || t_max < 2) return;
  hipLaunchKernelGGL(k_soft_add_xi, dim3((t_max + SN_THREADS - 1) / SN_THREADS, n_utts), dim3(SN_THREADS), 0, st, lay, bv, u0, M, ta, sa, XI);
}

// ------------------------------------------------------------------------------------------
// bias-only transitions: one matrix M for every frame.  k_soft_pos_sums: adv[k] = sum_t xa(t, k), stay[k] = sum_t xs(t, k),
// t ascending.  k_soft_trans_table: tab[u][p][c] = sum over the positions k of utterance u, ascending, of
// adv[k] [p = q_{k-1}, c = q_k] + stay[k] [p = c = q_k] (every entry is written).  k_reduce_xiacc then adds the tables of the
// chunk, ascending by utterance, times the transition-bias value into the weight k_add_trans_counts adds the observed
// counts to.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SN_THREADS) void k_soft_pos_sums(ScrfLayout lay, ScrfBatchView bv, uint32_t u0, const double* __restrict__ M,
                                                              ScrfTransArgs ta, ScrfSoftArgs sa) {
  const SnUtt x = sn_utt(lay, bv, u0, ta, sa);
  const double* aEs = sa.aE + x.c_base;
  const double* bBs = sa.bB + x.c_base;
  for (int k = blockIdx.x * SN_THREADS + threadIdx.x; k < x.K; k += gridDim.x * SN_THREADS) {
    double a = 0.0, s = 0.0;
    if (x.ok)
      for (int t = 1; t < x.T; t++) {
        double xa, xs;
        sn_xa_xs(x, aEs, bBs, M, lay.L, ta.mode, t, k, &xa, &xs);
        a += xa;
        s += xs;
      }
    sa.adv[x.p_base + k] = a;
    sa.stay[x.p_base + k] = s;
  }
}

__global__ __launch_bounds__(SN_THREADS) void k_soft_trans_table(ScrfLayout lay, uint32_t u0, ScrfTransArgs ta, ScrfSoftArgs sa) {
  const uint32_t L = lay.L, i = blockIdx.x * SN_THREADS + threadIdx.x;
  if (i >= L * L) return;
  const uint32_t p = i / L, c = i % L, u = u0 + blockIdx.y;
  const uint64_t p0 = ta.phone_off[u0], k0 = ta.phone_off[u], k1 = ta.phone_off[u + 1];
  double v = 0.0;
  for (uint64_t k = k0; k < k1; k++) {
    if (ta.phones[k] != c) continue;
    if (k > k0 && ta.phones[k - 1] == p) v += sa.adv[k - p0];
    if (p == c) v += sa.stay[k - p0];
  }
  sa.tab[(size_t)blockIdx.y * L * L + i] = v;
}

void launch_soft_trans_table(hipStream_t st, const ScrfLayout& lay, ScrfBatchView bv, uint32_t u0, uint32_t n_utts, uint64_t k_max,
                             const double* M, const ScrfTransArgs& ta, const ScrfSoftArgs& sa, double* grad) {
  if (n_utts == 0 || !lay.use_tb) return;
  const uint32_t LL = lay.L * lay.L;
  const uint32_t gx = (uint32_t)((std::max<uint64_t>(k_max, 1) + SN_THREADS - 1) / SN_THREADS);
  hipLaunchKernelGGL(k_soft_pos_sums, dim3(gx, n_utts), dim3(SN_THREADS), 0, st, lay, bv, u0, M, ta, sa);
  hipLaunchKernelGGL(k_soft_trans_table, dim3((LL + SN_THREADS - 1) / SN_THREADS, n_utts), dim3(SN_THREADS), 0, st, lay, u0, ta, sa);
  launch_reduce_xiacc(st, sa.tab, n_utts, lay, grad);   // bias-only transitions: trans_idx(p, c) is the bias weight itself
}
