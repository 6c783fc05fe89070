// scrf_align.hip -- batched forced alignment (scrf_align_batch), gfx950.
//
// The best path of the lattice of scrf_lattice_arcs(norm = 0) among the paths that realise a phone transcript q_0 .. q_{K-1}:
// float tropical semiring, path cost = the left-to-right float sum k_viterbi forms, strict improvement with the candidates
// in a fixed order (boundary: advance, then stay; end: the start arc, then t' ascending).  The search runs over (frame t,
// transcript position k) instead of (frame, label):
//   boundary(t,k) <- end(t-1,k-1) + w_boundary(M_t, q_{k-1}, q_k)          advance, k >= 1
//                 <- end(t-1,k)   + w_boundary(M_t, q_k, q_k)              stay, SCRF_ALIGN_RUNS only
//   end(t,k)      <- 0.0f + w_seg(t, t+1, q_0) for k = 0, t < D ;  boundary(t-d+1,k) + w_seg(t, d, q_k)
//   frame model:  state(t,k) <- state(t-1,k') + scrf_w_frame(M_t, S, t, q_k', q_k), k' = k-1 | k
// Cells that cannot lie on a complete path (k > t, K-1-k > T-1-t, in SCRF_ALIGN_ONE the duration bounds) stay +inf.
// One back pointer of 16 bits per cell: bits 0..14 the duration chosen by end(t,k), bit 15 set when boundary(t,k) chose
// "stay".  The backtrace runs in the kernel on one lane.  No atomics: the result does not depend on chunking.
//
//   k_align_wave   one wavefront per utterance, lane = transcript position (K <= 64)
//   k_align_group  one workgroup per utterance, threads strided over k (any K <= T)
#include <math.h>

#include "scrf_arcw.h"
#include "scrf_kernels.h"

#define AL_STAY 0x8000u

// the path from end(T-1, K-1) back to frame 0, written first to last; returns the number of segments (0: no path).
// Only cells with a finite cost are visited: their back pointers were written and point at finite cells.
__device__ inline uint32_t align_backtrace(const uint16_t* __restrict__ bp, const uint32_t* __restrict__ ph, int T, int K, int L,
                                           uint32_t* __restrict__ outl) {
  uint32_t n = 0;
  for (int pass = 0; pass < 2; pass++) {
    int t = T - 1, k = K - 1;
    uint32_t i = 0;
    while (true) {
      const int d = bp[(size_t)t * K + k] & 0x7fff;
      if (d < 1 || d > t + 1 || (int)i >= T) return 0;   // cannot happen on a finite path; never walk out of the arrays
      if (pass) outl[n - 1 - i] = ph[k] + (uint32_t)L * (uint32_t)(d - 1);
      i++;
      const int ts = t - d + 1;   // first frame of the segment
      if (ts == 0) break;
      if (!(bp[(size_t)ts * K + k] & AL_STAY)) k--;
      if (k < 0) return 0;
      t = ts - 1;
    }
    n = i;
  }
  return n;
}

// ------------------------------------------------------------------------------------------
// k_align_wave: lane = transcript position.  q_k, q_{k-1} and (single M) the lane's two transition weights stay in
// registers; end(t-1, .) and the D-deep ring of boundary values sit in LDS, the ring private to the lane's column -- the one
// cross-lane read is end(t-1, k-1).  No workgroup barrier.  The frame's D segment weights (column q_k of D consecutive rows)
// are requested a frame ahead, as k_viterbi_fast does.  It reads the weights through the scrf_w_* functions directly, not
// through ScrfArcView as k_align_group does: with the view its D <= 40 variant measured 0.8 % slower at 4096 utterances x 300
// frames (profiles/EXPERIMENTS.md), so its body stays as it was.
// ------------------------------------------------------------------------------------------
template <int DMAX>
__global__ __launch_bounds__(64 * AL_WAVES) void k_align_wave(ScrfLayout lay, ScrfBatchView bv, uint32_t u0, uint32_t n_utts,
                                                              const double* __restrict__ S, const float* __restrict__ Wn,
                                                              const double* __restrict__ M, int m_per_frame, int frame_model,
                                                              ScrfAlignArgs aa, uint32_t* __restrict__ out_labels,
                                                              uint32_t* __restrict__ out_n, float* __restrict__ out_cost) {
  extern __shared__ float alsm[];
  const int L = lay.L, D = lay.D;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float* e_prev = alsm + (size_t)wave * (64 + D * 64);   // [64] end(t-1, .)
  float* ring = e_prev + 64;                             // [D][64] boundary(t', .), slot t' % D
  const uint32_t ui = blockIdx.x * AL_WAVES + wave;
  if (ui >= n_utts) return;
  const uint32_t u = u0 + ui;
  const int T = (int)bv.T[u];
  const uint64_t K64 = aa.phone_off[u + 1] - aa.phone_off[u];
  if (!scrf_align_feasible((uint32_t)T, K64, (uint32_t)D, aa.mode) || K64 > 64) {
    if (lane == 0) { out_n[u] = 0; out_cost[u] = INFINITY; }
    return;
  }
  const int K = (int)K64, mode = aa.mode;
  const uint64_t f_base = bv.frame_off[u] - bv.frame_off[u0];
  const uint64_t s_base = bv.seg_off[u] - bv.seg_off[u0];
  const double* Su = S ? S + s_base * L : nullptr;
  const float* Wu = Wn ? Wn + s_base * L : nullptr;   // float(-1 * score) already formed (segment model)
  const size_t LL = (size_t)L * L;
  const uint32_t* ph = aa.phones + aa.phone_off[u];
  uint16_t* bp = aa.bp + (aa.bp_off[u] - aa.bp_off[u0]);
  const bool act = lane < K;
  const int k = act ? lane : K - 1;   // idle lanes shadow the last position; they are never live
  const uint32_t q = ph[k], qp = k >= 1 ? ph[k - 1] : q;
  float wA = 0.0f, wS = 0.0f;
  if (!m_per_frame && !frame_model) { wA = scrf_w_boundary(M, L, qp, q); wS = scrf_w_boundary(M, L, q, q); }
  float wv_n[DMAX];
  auto fetch_w = [&](int t, float (&w)[DMAX]) {
    const bool live = act && t < T && align_live(t, k, T, K, D, mode);
    const int tt = t < T ? t : T - 1;
    const uint64_t base = scrf_seg_base(tt, D);
    const int nd = tt + 1 < D ? tt + 1 : D;
#pragma unroll
    for (int i = 0; i < DMAX; i++)
      w[i] = (live && i < nd) ? (Wu ? Wu[(base + i) * L + q] : scrf_w_segment(Su, base, i + 1, L, q)) : 0.0f;
  };
  if (!frame_model) fetch_w(0, wv_n);
  int slot = 0;   // t % D
  for (int t = 0; t < T; t++) {
    const bool live = act && align_live(t, k, T, K, D, mode);
    float best = INFINITY;
    uint32_t arg = 0, flag = 0;
    if (frame_model) {
      if (t == 0) {
        if (live) { best = 0.0f + scrf_w_segment(Su, 0, 1, L, q); arg = 1; }
      } else if (live) {
        const double* Mt = M + (m_per_frame ? (f_base + t) * LL : 0);
        if (k >= 1) {
          const float c = e_prev[k - 1] + scrf_w_frame(Mt, Su, t, L, qp, q);
          if (c < best) best = c;
        }
        if (mode == SCRF_ALIGN_RUNS) {
          const float c = e_prev[k] + scrf_w_frame(Mt, Su, t, L, q, q);
          if (c < best) { best = c; flag = AL_STAY; }
        }
        arg = 1;
      }
    } else {
      const int nd = t + 1 < D ? t + 1 : D;
      float wv[DMAX];
#pragma unroll
      for (int i = 0; i < DMAX; i++) wv[i] = wv_n[i];
      fetch_w(t + 1, wv_n);
      if (t >= 1) {
        float b = INFINITY;
        if (act && align_live_b(t, k, T, K, D, mode)) {
          if (m_per_frame) {
            const double* Mt = M + (f_base + t) * LL;
            wA = scrf_w_boundary(Mt, L, qp, q); wS = scrf_w_boundary(Mt, L, q, q);
          }
          if (k >= 1) {
            const float c = e_prev[k - 1] + wA;
            if (c < b) b = c;
          }
          if (mode == SCRF_ALIGN_RUNS) {
            const float c = e_prev[k] + wS;
            if (c < b) { b = c; flag = AL_STAY; }
          }
        }
        ring[slot * 64 + lane] = b;
      }
      if (live) {
        if (k == 0 && t < D) {   // from the start state: duration t+1
#pragma unroll
          for (int i = 0; i < DMAX; i++)
            if (i == t) { const float c = 0.0f + wv[i]; if (c < best) { best = c; arg = t + 1; } }
        }
        // tp ascending = d descending
#pragma unroll
        for (int i = DMAX - 1; i >= 0; i--) {
          const int d = i + 1, tp = t - i;
          if (d <= nd && tp >= 1) {
            const int s = slot - i < 0 ? slot - i + D : slot - i;
            const float c = ring[s * 64 + lane] + wv[i];
            if (c < best) { best = c; arg = d; }
          }
        }
      }
    }
    // every lane has read end(t-1, .) before any lane replaces it
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    e_prev[lane] = best;
    if (act) bp[(size_t)t * K + k] = (uint16_t)(arg | flag);   // every cell: a boundary can be live where its end is not
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    if (++slot == D) slot = 0;
  }
  __threadfence_block();
  if (lane == 0) {
    float cost = e_prev[K - 1] + (frame_model ? 0.0f : -0.0f);
    uint32_t n = 0;
    if (cost < INFINITY) {
      n = align_backtrace(bp, ph, T, K, L, out_labels + bv.frame_off[u]);
      cost = n ? cost + 0.0f : INFINITY;   // Times(distance, Final = One)
    } else {
      cost = INFINITY;
    }
    out_n[u] = n;
    out_cost[u] = cost;
  }
}

void launch_align_wave(hipStream_t st, const ScrfLayout& lay, ScrfBatchView bv, uint32_t u0, uint32_t n_utts, const ScrfArcSrc& src,
                       const ScrfAlignArgs& aa, uint32_t* out_labels, uint32_t* out_n, float* out_cost) {
  if (n_utts == 0) return;
  const ScrfAlignWavePlan p = align_wave_plan(dp_shape(lay), n_utts);
#define AL_CASE(N)                                                                                                          \
  case N:                                                                                                                   \
    hipLaunchKernelGGL((k_align_wave<N>), dim3(p.gx), dim3(p.threads), p.lds, st, lay, bv, u0, n_utts, src.S, src.Wn, src.M, \
                       src.m_per_frame, src.frame_model, aa, out_labels, out_n, out_cost);                                  \
    break
  switch (p.dmax) { AL_CASE(4); AL_CASE(12); AL_CASE(40); }
#undef AL_CASE
}

// ------------------------------------------------------------------------------------------
// k_align_group: one workgroup per utterance, threads strided over k.  LDS: end double-buffered [2][K] and the boundary ring
// [D][K], the ring again private to a column -- one barrier per frame.
// ------------------------------------------------------------------------------------------
__global__ void k_align_group(ScrfLayout lay, ScrfBatchView bv, uint32_t u0, const double* __restrict__ S,
                              const float* __restrict__ Wn, const double* __restrict__ M, int m_per_frame, int frame_model,
                              ScrfAlignArgs aa, uint32_t* __restrict__ out_labels, uint32_t* __restrict__ out_n,
                              float* __restrict__ out_cost) {
  extern __shared__ float agsm[];
  const int L = lay.L, D = lay.D;
  const int tid = threadIdx.x, NT = blockDim.x;
  const uint32_t u = u0 + blockIdx.x;
  const ScrfArcView v(ScrfArcSrc{S, Wn, M, m_per_frame, frame_model}, lay, bv, u0, u);
  const int T = (int)v.T;
  const uint64_t K64 = aa.phone_off[u + 1] - aa.phone_off[u];
  if (!scrf_align_feasible((uint32_t)T, K64, (uint32_t)D, aa.mode)) {   // uniform over the workgroup
    if (tid == 0) { out_n[u] = 0; out_cost[u] = INFINITY; }
    return;
  }
  const int K = (int)K64, mode = aa.mode;   // K <= T
  const uint32_t* ph = aa.phones + aa.phone_off[u];
  uint16_t* bp = aa.bp + (aa.bp_off[u] - aa.bp_off[u0]);
  float* ring = agsm + 2 * (size_t)K;   // [D][K]
  int slot = 0;                         // t % D
  for (int t = 0; t < T; t++) {
    const float* e_prev = agsm + (size_t)((t + 1) & 1) * K;
    float* e_cur = agsm + (size_t)(t & 1) * K;
    const double* Mt = v.Mt(t);
    const uint64_t base = scrf_seg_base(t, D);
    for (int k = tid; k < K; k += NT) {
      const bool live = align_live(t, k, T, K, D, mode);
      float best = INFINITY;
      uint32_t arg = 0, flag = 0;
      if (frame_model) {
        if (live) {
          const uint32_t q = ph[k];
          if (t == 0) {
            best = 0.0f + v.start(q);
          } else {
            if (k >= 1) {
              const float c = e_prev[k - 1] + v.frame(Mt, t, ph[k - 1], q);
              if (c < best) best = c;
            }
            if (mode == SCRF_ALIGN_RUNS) {
              const float c = e_prev[k] + v.frame(Mt, t, q, q);
              if (c < best) { best = c; flag = AL_STAY; }
            }
          }
          arg = 1;
        }
      } else {
        const uint32_t q = ph[k];
        if (t >= 1) {
          float b = INFINITY;
          if (align_live_b(t, k, T, K, D, mode)) {
            if (k >= 1) {
              const float c = e_prev[k - 1] + v.boundary(Mt, ph[k - 1], q);
              if (c < b) b = c;
            }
            if (mode == SCRF_ALIGN_RUNS) {
              const float c = e_prev[k] + v.boundary(Mt, q, q);
              if (c < b) { b = c; flag = AL_STAY; }
            }
          }
          ring[(size_t)slot * K + k] = b;
        }
        if (live) {
          if (k == 0 && t < D) {   // from the start state: duration t+1
            const float c = 0.0f + v.segment(base, t + 1, q);
            if (c < best) { best = c; arg = t + 1; }
          }
          // tp ascending = d descending from min(t, D), eight weights requested at a time so that their loads overlap
          for (int d0 = t < D ? t : D; d0 >= 1; d0 -= 8) {
            float w[8];
#pragma unroll
            for (int j = 0; j < 8; j++) {
              const int d = d0 - j > 1 ? d0 - j : 1;
              w[j] = v.segment(base, d, q);
            }
#pragma unroll
            for (int j = 0; j < 8; j++) {
              const int d = d0 - j;
              if (d >= 1) {
                const int s = slot - (d - 1) < 0 ? slot - (d - 1) + D : slot - (d - 1);
                const float c = ring[(size_t)s * K + k] + w[j];
                if (c < best) { best = c; arg = d; }
              }
            }
          }
        }
      }
      e_cur[k] = best;
      bp[(size_t)t * K + k] = (uint16_t)(arg | flag);   // every cell: a boundary can be live where its end is not
    }
    __syncthreads();
    if (++slot == D) slot = 0;
  }
  if (tid == 0) {
    float cost = agsm[(size_t)((T - 1) & 1) * K + K - 1] + (frame_model ? 0.0f : -0.0f);
    uint32_t n = 0;
    if (cost < INFINITY) {
      n = align_backtrace(bp, ph, T, K, L, out_labels + bv.frame_off[u]);
      cost = n ? cost + 0.0f : INFINITY;   // Times(distance, Final = One)
    } else {
      cost = INFINITY;
    }
    out_n[u] = n;
    out_cost[u] = cost;
  }
}


void launch_align_group(hipStream_t st, const ScrfLayout& lay, ScrfBatchView bv, uint32_t u0, uint32_t n_utts, uint32_t k_max,
                        const ScrfArcSrc& src, const ScrfAlignArgs& aa, uint32_t* out_labels, uint32_t* out_n, float* out_cost) {
  if (n_utts == 0) return;
  int NT = ((int)(k_max ? k_max : 1) + 63) / 64 * 64;
  if (NT > 1024) NT = 1024;
  const size_t sm = align_group_smem_bytes(dp_shape(lay), k_max ? k_max : 1);   // the chunk's longest transcript
  hipFuncSetAttribute((const void*)k_align_group, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sm);
  hipLaunchKernelGGL(k_align_group, dim3(n_utts), dim3(NT), sm, st, lay, bv, u0, src.S, src.Wn, src.M, src.m_per_frame, src.frame_model,
                     aa, out_labels, out_n, out_cost);
}
