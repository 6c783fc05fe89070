// scrf_transcript.hip -- transcript scoring (scrf_transcript_batch), gfx950.
//
// The log-semiring twin of scrf_align.hip: the sum over every alignment of a phone transcript q_0 .. q_{K-1}, fp64 log
// domain, over (frame t, transcript position k).  aB / aE are the forward sums at the start / the end of a segment of
// position k, bB / bE the backward ones:
//   aB(t,k) = LSE( aE(t-1,k-1) + M_t(q_{k-1},q_k)           advance, k >= 1
//                , aE(t-1,k)   + M_t(q_k,q_k) )             stay, SCRF_ALIGN_RUNS only
//   aE(t,k) = LSE( S(t,t+1,q_0) for k = 0, t < D            the start term, first
//                , aB(t-d+1,k) + S(t,d,q_k) )               d descending from min(t, D), as the search visits them
//   A       = aE(T-1,K-1)
//   bE(T-1,K-1) = 0;  bE(t,k) = LSE( bB(t+1,k+1) + M_{t+1}(q_k,q_{k+1}),  RUNS: bB(t+1,k) + M_{t+1}(q_k,q_k) )
//   bB(t,k) = LSE_d( S(t+d-1,d,q_k) + bE(t+d-1,k) )         d ascending
//   g(t,d,k) = exp( aB(t-d+1,k) + S(t,d,q_k) + bE(t,k) - A )                (t-d+1 = 0: aB := 0 for k = 0)
// Cells that cannot lie on a complete path (align_live / align_live_b, the bounds of the search) are -inf and not computed.
// Every sum is a max-shifted one over terms in a fixed order (LseAcc, scrf_lse.h); there is no floating-point atomic, and
// nothing a cell adds depends on the launch: two runs and any chunking give the same bytes.
// On the linear path (scores kept as exp(S - row maximum)) a live term whose exponential is zero or subnormal sends the
// utterance to the log-domain redo (tr_score_live): the sum over a transcript's alignments has no right to drop it.
//
//   k_transcript      one workgroup per utterance, threads strided over k: the forward sweep, then the backward sweep with
//                     the occupancy walk of k_post_occ per position and a per-label retire
//   k_transcript_seg  one thread per segment query: sum over the positions that carry the queried label
#include <float.h>
#include <math.h>

#include "scrf_dp_common.h"
#include "scrf_kernels.h"
#include "scrf_lse.h"

#define TR_MAX_WAVES 16

// the fp64 log score of row `row`, label q, in either form the score stage leaves behind: S itself (log path) or
// smax + log(ES) with ES = exp(S - smax) (linear path; ES == 0 reads as -inf)
__device__ __forceinline__ double tr_score(const double* __restrict__ Su, const double* __restrict__ smu, int lin, uint64_t row,
                                           uint32_t L, uint32_t q) {
  const double v = Su[row * L + q];
  return lin ? smu[row] + log(v) : v;
}

// The same for a term of the forward sweep, whose other summand `with` is finite: on the linear path an ES below DBL_MIN
// (zero: the term would vanish; subnormal: its log has lost bits) sets `lost`.  A free recursion may drop
// such a term, because the label that holds the row maximum stands in the same sum; a sum over the alignments of a
// transcript may not, because that label need not be in the transcript: the alignments through the term can carry all of
// the mass, and A stays finite on those that are left.
__device__ __forceinline__ double tr_score_live(const double* __restrict__ Su, const double* __restrict__ smu, int lin, uint64_t row,
                                                uint32_t L, uint32_t q, bool with, bool& lost) {
  const double v = Su[row * L + q];
  if (!lin) return v;
  lost |= with && v < DBL_MIN;
  return smu[row] + log(v);
}

// threads that own transcript positions: K rounded up to a wavefront, at most 1024 -- a function of K alone, so that the
// order of every sum over positions does not depend on the other transcripts of the launch
__host__ __device__ inline int tr_threads(uint64_t K) {
  const uint64_t n = (K + 63) / 64 * 64;
  return n > 1024 ? 1024 : (n ? (int)n : 64);
}

__global__ __launch_bounds__(1024) void k_transcript(ScrfLayout lay, ScrfBatchView bv, uint32_t u0, const double* __restrict__ S,
                                                     const double* __restrict__ smax, const double* __restrict__ M,
                                                     int m_per_frame, ScrfTransArgs ta, int* __restrict__ status,
                                                     double* __restrict__ log_num, double* __restrict__ occ,
                                                     double* __restrict__ endp) {
  extern __shared__ double trsm[];            // [2][K] aE, then bB | [D][K] the aB ring, then the occupancy ring
  __shared__ double wsum[TR_MAX_WAVES];       // per-wavefront parts of end[t]
  const int L = lay.L, D = lay.D;
  const int tid = threadIdx.x, NB = blockDim.x;
  const uint32_t u = u0 + blockIdx.x;
  const int T = (int)bv.T[u];
  const uint64_t K64 = ta.phone_off[u + 1] - ta.phone_off[u];
  const uint64_t F0 = bv.frame_off[u];        // the outputs are arrays of the whole batch
  if (!scrf_align_feasible((uint32_t)T, K64, (uint32_t)D, ta.mode)) {   // uniform over the workgroup
    if (tid == 0) log_num[u] = -INFINITY;
    if (occ) for (uint64_t i = tid; i < (uint64_t)T * L; i += NB) occ[F0 * L + i] = 0.0;
    if (endp) for (int t = tid; t < T; t += NB) endp[F0 + t] = 0.0;
    return;
  }
  const int K = (int)K64, mode = ta.mode, lin = ta.lin;   // K <= T
  const int NT = tr_threads(K64);                         // <= NB
  const bool own = tid < NT;
  const uint64_t f_base = F0 - bv.frame_off[u0];
  const uint64_t s_base = bv.seg_off[u] - bv.seg_off[u0];
  const double* Su = S + s_base * L;
  const double* smu = lin ? smax + s_base : nullptr;
  const size_t LL = (size_t)L * L;
  const uint32_t* ph = ta.phones + ta.phone_off[u];
  const uint64_t c_base = ta.cell_off[u] - ta.cell_off[u0];
  double* aBs = ta.aB + c_base;   // [T][K], every cell of frames 1 .. T-1
  double* bEs = ta.bE + c_base;   // [T][K], every cell
  // a transcript of at most 1024 phones: the thread's one position, its neighbours and (single M) its three transition
  // scores stay in registers
  const bool one = K <= NT;
  const int k1 = tid < K ? tid : K - 1;
  const uint32_t q1 = ph[k1], qp1 = k1 >= 1 ? ph[k1 - 1] : q1, qn1 = k1 + 1 < K ? ph[k1 + 1] : q1;
  double mA1 = 0.0, mS1 = 0.0, mN1 = 0.0;
  if (!m_per_frame) { mA1 = M[(size_t)qp1 * L + q1]; mS1 = M[(size_t)q1 * L + q1]; mN1 = M[(size_t)q1 * L + qn1]; }
  const bool regs = one && !m_per_frame;

  // ---- forward.  Every term whose aB is finite is read here through tr_score_live.  The backward sweep and
  // k_transcript_seg read no other live term: a term (t, d, k) adds to g or to bB only where aB(t-d+1, k) and bE(t, k) are
  // both finite, and with no term lost a finite aB is the aB of this sweep -- so they need no guard of their own.
  bool lost = false;
  if (tid == 0) wsum[0] = 0.0;   // the workgroup's flag until the backward sweep takes wsum; the frames' barriers come before any set
  {
    double* ring = trsm + 2 * (size_t)K;   // [D][K] aB(t', .), slot t' % D, a column private to its thread
    int slot = 0;
    for (int t = 0; t < T; t++) {
      const double* e_prev = trsm + (size_t)((t + 1) & 1) * K;
      double* e_cur = trsm + (size_t)(t & 1) * K;
      const double* Mt = M + (m_per_frame ? (f_base + t) * LL : 0);
      const uint64_t base = scrf_seg_base(t, D);
      if (own)
        for (int k = tid; k < K; k += NT) {
          const uint32_t q = one ? q1 : ph[k];
          if (t >= 1) {
            double b = -INFINITY;
            if (align_live_b(t, k, T, K, D, mode)) {
              LseAcc a;
              if (k >= 1) a.add(e_prev[k - 1] + (regs ? mA1 : Mt[(size_t)(one ? qp1 : ph[k - 1]) * L + q]));
              if (mode == SCRF_ALIGN_RUNS) a.add(e_prev[k] + (regs ? mS1 : Mt[(size_t)q * L + q]));
              b = a.value();
            }
            ring[(size_t)slot * K + k] = b;
            aBs[(size_t)t * K + k] = b;
          }
          double e = -INFINITY;
          if (align_live(t, k, T, K, D, mode)) {
            LseAcc a;
            if (k == 0 && t < D) a.add(tr_score_live(Su, smu, lin, base + t, L, q, true, lost));   // from the start: duration t + 1
            for (int d = t < D ? t : D; d >= 1; d--) {
              const int s = slot - (d - 1) < 0 ? slot - (d - 1) + D : slot - (d - 1);
              const double ab = ring[(size_t)s * K + k];
              a.add(ab + tr_score_live(Su, smu, lin, base + d - 1, L, q, ab > -INFINITY, lost));
            }
            e = a.value();
          }
          e_cur[k] = e;
        }
      __syncthreads();
      if (++slot == D) slot = 0;
    }
  }
  const double A = trsm[(size_t)((T - 1) & 1) * K + K - 1];
  if (tid == 0) log_num[u] = A;
  if (lost) wsum[0] = 1.0;
  __syncthreads();
  const bool any_lost = wsum[0] != 0.0;
  if (any_lost || !(A > -INFINITY && A < INFINITY)) {
    // a live term was lost to ES < DBL_MIN: whatever A is, it is the sum over the alignments that are left.  Or A is not
    // finite: a transcript that fits has a path, so every path lost a segment (or the scores are not finite).  The call is
    // redone on the log path, or reports this utterance.
    if (tid == 0) atomicMax(&status[u], SCRF_ERR_NUMERIC);
    if (occ) for (uint64_t i = tid; i < (uint64_t)T * L; i += NB) occ[F0 * L + i] = 0.0;
    if (endp) for (int t = tid; t < T; t += NB) endp[F0 + t] = 0.0;
    return;
  }
  if (!occ && !endp && !ta.want_seg) return;
  __syncthreads();   // everyone holds A: the forward arrays are dead

  // ---- backward, with the occupancy walk
  double* oring = trsm + 2 * (size_t)K;   // [D][K] open occupancy sums of position k, slot of frame f = f % D
  if (own)
    for (int k = tid; k < K; k += NT)
      for (int j = 0; j < D; j++) oring[(size_t)j * K + k] = 0.0;
  const uint32_t* ioff = ta.inv_off + (size_t)u * (L + 1);
  const uint32_t* ipos = ta.inv_pos + ta.phone_off[u];
  const int wave = tid >> 6, n_waves = NT >> 6;
  int slot = (T - 1) % D;
  for (int t = T - 1; t >= 0; t--) {
    const double* b_next = trsm + (size_t)((t + 1) & 1) * K;
    double* b_cur = trsm + (size_t)(t & 1) * K;
    const double* Mn = M + ((m_per_frame && t + 1 < T) ? (f_base + t + 1) * LL : 0);
    const uint64_t base = scrf_seg_base(t, D);
    const int zs = slot + 1 == D ? 0 : slot + 1;   // the slot frame t+1 left = the slot of frame t-D+1, which opens now
    double esum = 0.0;
    if (own)
      for (int k = tid; k < K; k += NT) {
        const uint32_t q = one ? q1 : ph[k];
        oring[(size_t)zs * K + k] = 0.0;
        double be = -INFINITY;
        if (align_live(t, k, T, K, D, mode)) {
          if (t == T - 1) {
            be = 0.0;   // live at the last frame: k = K - 1
          } else {
            LseAcc a;
            if (k + 1 < K) a.add(b_next[k + 1] + (regs ? mN1 : Mn[(size_t)q * L + (one ? qn1 : ph[k + 1])]));
            if (mode == SCRF_ALIGN_RUNS) a.add(b_next[k] + (regs ? mS1 : Mn[(size_t)q * L + q]));
            be = a.value();
          }
        }
        bEs[(size_t)t * K + k] = be;
        double usum = 0.0;
        if (be > -INFINITY) {
          // suffix sums over d descending: the segments of duration > j cover frame t - j (k_post_occ's scheme)
          for (int d = t + 1 < D ? t + 1 : D; d >= 1; d--) {
            const int ts = t - d + 1;
            const double ab = ts == 0 ? (k == 0 ? 0.0 : -INFINITY) : aBs[(size_t)ts * K + k];
            const double x = ab + tr_score(Su, smu, lin, base + d - 1, L, q) + be - A;
            usum += exp(x);   // exp(-inf) = 0
            const int s = slot - (d - 1) < 0 ? slot - (d - 1) + D : slot - (d - 1);
            oring[(size_t)s * K + k] += usum;
          }
        }
        esum += usum;
        if (t >= 1) {
          double b = -INFINITY;
          if (align_live_b(t, k, T, K, D, mode)) {
            LseAcc a;
            const int nd = T - t < D ? T - t : D;
            for (int d = 1; d <= nd; d++) {
              const int te = t + d - 1;
              a.add(tr_score(Su, smu, lin, scrf_seg_base(te, D) + d - 1, L, q) + bEs[(size_t)te * K + k]);
            }
            b = a.value();
          }
          b_cur[k] = b;
        }
      }
    const double ws = wave_sum_f64_dpp(esum);
    if ((tid & 63) == 0 && wave < TR_MAX_WAVES) wsum[wave] = ws;
    __syncthreads();
    // frame t has seen its last segment: a thread per label adds the positions that carry it, ascending
    if (occ)
      for (int l = tid; l < L; l += NB) {
        double v = 0.0;
        for (uint32_t i = ioff[l]; i < ioff[l + 1]; i++) v += oring[(size_t)slot * K + ipos[i]];
        occ[(F0 + t) * L + l] = v;
      }
    if (endp && tid == 0) {
      double v = 0.0;
      for (int w = 0; w < n_waves; w++) v += wsum[w];
      endp[F0 + t] = v;
    }
    __syncthreads();   // the retired slot is opened again, and wsum rewritten, by the next frame
    slot = slot == 0 ? D - 1 : slot - 1;
  }
}


void launch_transcript(hipStream_t st, const ScrfLayout& lay, ScrfBatchView bv, uint32_t u0, uint32_t n_utts, uint64_t k_max,
                       const double* S, const double* smax, const double* M, int m_per_frame, const ScrfTransArgs& ta,
                       int* status, double* log_num, double* occ, double* endp) {
  if (n_utts == 0) return;
  const size_t sm = transcript_smem_bytes(dp_shape(lay), k_max ? k_max : 1);   // the chunk's longest transcript that fits
  hipFuncSetAttribute((const void*)k_transcript, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sm);
  hipLaunchKernelGGL(k_transcript, dim3(n_utts), dim3(tr_threads(k_max)), sm, st, lay, bv, u0, S, smax, M, m_per_frame, ta, status,
                     log_num, occ, endp);
}

// ------------------------------------------------------------------------------------------
// k_transcript_seg: query (utterance, end frame e, label value l + L (d - 1)) -> sum over the positions k with q_k = l,
// ascending, of g(e, d, k), from the aB / bE cells the sweep left in the chunk's scratch.  The host has checked that
// every (e, d) exists and every label is in range.
// ------------------------------------------------------------------------------------------
__global__ void k_transcript_seg(ScrfLayout lay, ScrfBatchView bv, uint32_t u0, const uint32_t* __restrict__ q_u,
                                 const uint32_t* __restrict__ q_e, const uint32_t* __restrict__ q_lab, uint64_t q0, uint64_t nq,
                                 const double* __restrict__ S, const double* __restrict__ smax, ScrfTransArgs ta,
                                 const double* __restrict__ log_num, double* __restrict__ out) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nq) return;
  const uint64_t qi = q0 + i;
  const uint32_t L = lay.L, D = lay.D;
  const uint32_t u = q_u[qi], e = q_e[qi], lab = q_lab[qi];
  const uint32_t l = lab % L, d = lab / L + 1;
  const uint32_t T = bv.T[u];
  const uint64_t K = ta.phone_off[u + 1] - ta.phone_off[u];
  const double A = log_num[u];
  double g = 0.0;
  if (scrf_align_feasible(T, K, D, ta.mode) && A > -INFINITY && A < INFINITY) {
    const uint64_t s_base = bv.seg_off[u] - bv.seg_off[u0];
    const uint64_t c_base = ta.cell_off[u] - ta.cell_off[u0];
    const double* aBs = ta.aB + c_base;
    const double* bEs = ta.bE + c_base;
    const double sc = tr_score(S + s_base * L, ta.lin ? smax + s_base : nullptr, ta.lin, scrf_seg_base(e, D) + d - 1, L, l);
    const uint32_t ts = e + 1 - d;
    const uint32_t* ioff = ta.inv_off + (size_t)u * (L + 1);
    const uint32_t* ipos = ta.inv_pos + ta.phone_off[u];
    for (uint32_t j = ioff[l]; j < ioff[l + 1]; j++) {
      const uint32_t k = ipos[j];
      const double ab = ts == 0 ? (k == 0 ? 0.0 : -INFINITY) : aBs[(size_t)ts * K + k];
      g += exp(ab + sc + bEs[(size_t)e * K + k] - A);
    }
  }
  out[qi] = g;
}

void launch_transcript_seg(hipStream_t st, const ScrfLayout& lay, ScrfBatchView bv, uint32_t u0, const uint32_t* q_u,
                           const uint32_t* q_e, const uint32_t* q_lab, uint64_t q0, uint64_t nq, const double* S,
                           const double* smax, const ScrfTransArgs& ta, const double* log_num, double* out) {
  if (nq == 0) return;
  hipLaunchKernelGGL(k_transcript_seg, dim3((uint32_t)((nq + 255) / 256)), dim3(256), 0, st, lay, bv, u0, q_u, q_e, q_lab, q0, nq,
                     S, smax, ta, log_num, out);
}
