// scrf_nbest.hip -- batched N-best decoding (scrf_nbest_batch), gfx950.
//
// The n least-cost complete paths of the lattice of scrf_lattice_arcs(norm = 0), pairwise distinct and ascending by cost:
// float tropical semiring, path cost = the left-to-right float sum k_viterbi forms.  k_viterbi's recursion with a sorted list
// of up to N costs per state instead of one value:
//   boundary(t,l)[0..N) <- the N least of { end(t-1,p)[r] + w_boundary(M_t,p,l) }        ordered by (cost, p, r)
//   end(t,l)[0..N)      <- the N least of { 0.0f + w_seg(t,t+1,l) (t < D) ; boundary(t',l)[r] + w_seg(t,t-t'+1,l) }
//                                                                  ordered by (cost, the start arc first, then t' ascending, r)
//   final[0..N)         <- the N least of { (end(T-1,l)[r] + (-0.0f)) + 0.0f }           ordered by (cost, l, r)
//   frame model:  state(t,c)[0..N) <- the N least of { state(t-1,p)[r] + scrf_w_frame(M_t,S,t,p,c) }, ordered by (cost, p, r)
// A list is sorted, and adding one arc weight keeps it sorted (float addition is monotone), so a state's new list is the first N
// outputs of a stable multi-way merge of its predecessors' lists.  Lists shorter than N are padded with +inf; an +inf entry is
// never a hypothesis.  With N = 1 the merge is k_viterbi's strict-improvement scan.  No atomics.
//
//   k_nbest        one workgroup per utterance, one wavefront per (t, l) merge
//   k_nbest_count  one thread per (utterance, rank): the hypothesis's number of segments
//   k_nbest_scan   one workgroup: label and hypothesis offsets of the chunk
//   k_nbest_trace  one thread per (utterance, rank): labels first to last, cost and label offset into the result
#include <math.h>

#include "scrf_arcw.h"
#include "scrf_kernels.h"

#define NB_NOLIST 0x7fffffff

// the lists a merge draws from, in the order of the tie rule: list(j) = the N sorted costs of predecessor j (nullptr: the
// single entry 0.0f), w(j) = the arc's weight, tag(j) = the high half of the back pointer
struct NbBoundary {   // end(t-1, p) -> boundary(t, l) ; frame model: state(t-1, p) -> state(t, l)
  const float* prev; const ScrfArcView& v; const double* Mt; int N, l, t, frame_model;
  __device__ const float* list(int p) const { return prev + (size_t)p * N; }
  __device__ float w(int p) const { return frame_model ? v.frame(Mt, t, p, l) : v.boundary(Mt, p, l); }
  __device__ uint32_t tag(int p) const { return (uint32_t)p << 16; }
};
struct NbEnd {   // j = 0: the start arc (t < D) ; j >= 1: boundary(t - d + 1, l) with d = dmax - j + 1, d descending
  const float* ring; const ScrfArcView& v; uint64_t base; int L, D, N, l, t, dmax;
  __device__ int dur(int j) const { return j == 0 ? t + 1 : dmax - j + 1; }
  __device__ const float* list(int j) const { return j == 0 ? nullptr : ring + ((size_t)((t - dur(j) + 1) % D) * L + l) * N; }
  __device__ float w(int j) const {
    if (j == 0 && t >= D) return INFINITY;   // no start arc of this length
    return v.segment(base, dur(j), l);
  }
  __device__ uint32_t tag(int j) const { return (uint32_t)dur(j) << 16; }
};
struct NbFinal {   // end(T-1, l) -> final
  const float* last; int N; float wf;
  __device__ const float* list(int l) const { return last + (size_t)l * N; }
  __device__ float w(int) const { return wf; }
  __device__ uint32_t tag(int l) const { return (uint32_t)l << 16; }
};

// The first N outputs of the stable merge of n_lists sorted lists, by one wavefront.  Lane j % 64 owns list j: its head rank
// hd[j] (LDS, private to the wavefront), and the least (cost, j) among the heads of the lists it owns.  N times: the wavefront's
// arg-min over (cost, j), the owner writes cost and back pointer (tag | rank) and advances that head.  Inside a list the head is
// the least rank left, so equal costs come out by (j, rank) ascending.  Ends early once only +inf is left.
template <class Src>
__device__ inline void nb_merge(const Src& src, int n_lists, int N, int lane, uint16_t* hd, float* out, uint32_t* bp) {
  const float w0 = lane < n_lists ? src.w(lane) : INFINITY;   // the lane's first list: the only one when n_lists <= 64
  const float* l0 = lane < n_lists ? src.list(lane) : nullptr;
  for (int j = lane; j < n_lists; j += 64) hd[j] = 0;
  float bc;
  int bj;
  auto head = [&](int j) -> float {
    const int r = hd[j];
    const float* lst = j == lane ? l0 : src.list(j);
    const float w = j == lane ? w0 : src.w(j);
    if (!lst) return r == 0 ? 0.0f + w : INFINITY;
    return r < N ? lst[r] + w : INFINITY;
  };
  auto local = [&]() {
    bc = INFINITY;
    bj = NB_NOLIST;
    for (int j = lane; j < n_lists; j += 64) {
      const float c = head(j);
      if (bj == NB_NOLIST || c < bc) { bc = c; bj = j; }   // j ascending: the first of equal costs stays
    }
  };
  local();
  int s = 0;
  for (; s < N; s++) {
    float wc = bc;
    int wj = bj;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
      const float oc = __shfl_xor(wc, m, 64);
      const int oj = __shfl_xor(wj, m, 64);
      if (oc < wc || (oc == wc && oj < wj)) { wc = oc; wj = oj; }
    }
    if (!(wc < INFINITY)) break;   // the same in every lane
    if (wj == bj && bj != NB_NOLIST) {
      const int r = hd[wj];
      out[s] = wc;
      bp[s] = src.tag(wj) | (uint32_t)r;
      hd[wj] = (uint16_t)(r + 1);   // r < N <= 65535: a finite head
      local();
    }
  }
  for (int i = s + lane; i < N; i += 64) out[i] = INFINITY;
}

__global__ __launch_bounds__(64 * NB_WAVES) void k_nbest(ScrfLayout lay, ScrfBatchView bv, uint32_t u0, const double* __restrict__ S,
                                                         const float* __restrict__ Wn, const double* __restrict__ M,
                                                         int m_per_frame, int frame_model, ScrfNbestBufs nb) {
  extern __shared__ float nbsm[];
  const int L = lay.L, D = lay.D, N = (int)nb.N;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n_waves = blockDim.x >> 6;
  const uint32_t ui = blockIdx.x, u = u0 + ui;
  const ScrfArcView v(ScrfArcSrc{S, Wn, M, m_per_frame, frame_model}, lay, bv, u0, u);
  const int T = (int)v.T;
  const uint64_t f_base = v.f_base;
  const size_t LN = (size_t)L * N;
  float* ring = nbsm + 2 * LN;                                        // [D][L][N] boundary(t', .), slot t' % D
  uint16_t* hd = (uint16_t*)(ring + (size_t)D * LN) + (size_t)wave * nbest_heads(L, D);
  uint32_t* bpb = nb.bp_b + f_base * LN;
  uint32_t* bpe = nb.bp_e + f_base * LN;
  float* fin_cost = nb.fin_cost + (size_t)ui * N;
  uint32_t* fin_ptr = nb.fin_ptr + (size_t)ui * N;
  if (T == 0) {   // uniform over the workgroup
    for (int i = threadIdx.x; i < N; i += blockDim.x) fin_cost[i] = INFINITY;
    return;
  }
  for (int t = 0; t < T; t++) {
    const float* e_prev = nbsm + (size_t)((t + 1) & 1) * LN;
    float* e_cur = nbsm + (size_t)(t & 1) * LN;
    const double* Mt = v.Mt(t);
    if (frame_model) {
      for (int l = wave; l < L; l += n_waves) {
        float* out = e_cur + (size_t)l * N;
        if (t == 0) {
          for (int i = lane; i < N; i += 64) out[i] = i == 0 ? 0.0f + v.start(l) : INFINITY;
        } else {
          const NbBoundary src{e_prev, v, Mt, N, l, t, 1};
          nb_merge(src, L, N, lane, hd, out, bpb + ((size_t)t * L + l) * N);
        }
      }
      __syncthreads();
      continue;
    }
    if (t >= 1) {
      for (int l = wave; l < L; l += n_waves) {
        const NbBoundary src{e_prev, v, Mt, N, l, t, 0};
        nb_merge(src, L, N, lane, hd, ring + ((size_t)(t % D) * L + l) * N, bpb + ((size_t)t * L + l) * N);
      }
    }
    __syncthreads();
    const int dmax = t < D ? t : D;
    for (int l = wave; l < L; l += n_waves) {
      const NbEnd src{ring, v, scrf_seg_base(t, D), L, D, N, l, t, dmax};
      nb_merge(src, 1 + dmax, N, lane, hd, e_cur + (size_t)l * N, bpe + ((size_t)t * L + l) * N);
    }
    __syncthreads();
  }
  if (wave == 0) {
    const float* last = nbsm + (size_t)((T - 1) & 1) * LN;
    float* out = nbsm + (size_t)(T & 1) * LN;   // the other end buffer: dead now
    const NbFinal src{last, N, frame_model ? 0.0f : -0.0f};
    nb_merge(src, L, N, lane, hd, out, fin_ptr);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    for (int i = lane; i < N; i += 64) fin_cost[i] = out[i] + 0.0f;   // Times(distance, Final = One)
  }
}

// the hypothesis of rank r of chunk utterance ui, walked from the final state back to frame 0.  out == nullptr: returns the
// number of segments; otherwise writes the n labels first to last.  A pointer that would leave the arrays (it cannot on a
// finite entry) ends the walk with 0.
__device__ inline uint32_t nb_walk(const ScrfNbestBufs& nb, int T, int L, int frame_model, uint64_t f_base, uint32_t ui, uint32_t r,
                                   uint32_t* out, uint32_t n) {
  const uint32_t N = nb.N;
  const size_t LN = (size_t)L * N;
  const uint32_t* bpb = nb.bp_b + f_base * LN;
  const uint32_t* bpe = nb.bp_e + f_base * LN;
  uint32_t w = nb.fin_ptr[(size_t)ui * N + r];
  uint32_t l = w >> 16, rk = w & 0xffffu, i = 0;
  int t = T - 1;
  while (true) {
    if (l >= (uint32_t)L || rk >= N || (int)i >= T) return 0;
    if (frame_model) {
      if (out) out[n - 1 - i] = l;
      i++;
      if (t == 0) break;
      w = bpb[((size_t)t * L + l) * N + rk];
      l = w >> 16; rk = w & 0xffffu;
      t--;
    } else {
      w = bpe[((size_t)t * L + l) * N + rk];
      const int d = (int)((w >> 16) & 0x7fffu);
      rk = w & 0xffffu;
      if (d < 1 || d > t + 1) return 0;
      if (out) out[n - 1 - i] = l + (uint32_t)L * (uint32_t)(d - 1);
      i++;
      const int ts = t - d + 1;   // first frame of the segment
      if (ts == 0) break;
      if (rk >= N) return 0;
      w = bpb[((size_t)ts * L + l) * N + rk];
      l = w >> 16; rk = w & 0xffffu;
      t = ts - 1;
    }
  }
  return i;
}

__global__ void k_nbest_count(ScrfLayout lay, ScrfBatchView bv, uint32_t u0, uint32_t n_utts, int frame_model, ScrfNbestBufs nb) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (uint64_t)n_utts * nb.N) return;
  const uint32_t ui = (uint32_t)(i / nb.N), r = (uint32_t)(i % nb.N), u = u0 + ui;
  uint32_t n = 0;
  if (nb.fin_cost[i] < INFINITY)
    n = nb_walk(nb, (int)bv.T[u], lay.L, frame_model, bv.frame_off[u] - bv.frame_off[u0], ui, r, nullptr, 0);
  nb.cnt[i] = n;
}

// exclusive prefix sums of the chunk's n = n_utts * N counts (labels) and of their non-zero flags (hypotheses: a prefix of
// every utterance's N ranks), the totals, and the batch's hypothesis offsets of the chunk's utterances
#define NB_SCAN_NT 1024
__global__ __launch_bounds__(NB_SCAN_NT) void k_nbest_scan(ScrfNbestBufs nb, uint32_t u0, uint32_t n_utts, uint64_t lab_base,
                                                           uint64_t hyp_base, uint64_t* __restrict__ hyp_off) {
  __shared__ uint64_t sl[NB_SCAN_NT], sh[NB_SCAN_NT];
  const uint32_t tid = threadIdx.x;
  const uint64_t n = (uint64_t)n_utts * nb.N, per = (n + NB_SCAN_NT - 1) / NB_SCAN_NT;
  const uint64_t lo = min(n, tid * per), hi = min(n, lo + per);
  uint64_t a = 0, b = 0;
  for (uint64_t i = lo; i < hi; i++) { a += nb.cnt[i]; b += nb.cnt[i] ? 1 : 0; }
  sl[tid] = a; sh[tid] = b;
  __syncthreads();
  for (uint32_t off = 1; off < NB_SCAN_NT; off <<= 1) {
    const uint64_t va = tid >= off ? sl[tid - off] : 0, vb = tid >= off ? sh[tid - off] : 0;
    __syncthreads();
    sl[tid] += va; sh[tid] += vb;
    __syncthreads();
  }
  uint64_t ra = lab_base + sl[tid] - a, rb = hyp_base + sh[tid] - b;
  for (uint64_t i = lo; i < hi; i++) {
    nb.lab_pos[i] = ra; nb.hyp_pos[i] = rb;
    ra += nb.cnt[i]; rb += nb.cnt[i] ? 1 : 0;
  }
  if (tid == NB_SCAN_NT - 1) {
    nb.tot[0] = sl[tid]; nb.tot[1] = sh[tid];
    nb.lab_pos[n] = lab_base + sl[tid];
    hyp_off[u0 + n_utts] = hyp_base + sh[tid];
  }
  __syncthreads();
  for (uint32_t k = tid; k < n_utts; k += NB_SCAN_NT) hyp_off[u0 + k] = nb.hyp_pos[(uint64_t)k * nb.N];
}

__global__ void k_nbest_trace(ScrfLayout lay, ScrfBatchView bv, uint32_t u0, uint32_t n_utts, int frame_model, ScrfNbestBufs nb,
                              uint64_t lab_cap, uint64_t hyp_cap, uint32_t* __restrict__ res_lab, uint64_t* __restrict__ res_off,
                              float* __restrict__ res_cost) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, n_all = (uint64_t)n_utts * nb.N;
  if (i == 0) {   // the end of the result so far; the next chunk's first hypothesis writes the same value there
    const uint64_t h_end = nb.hyp_pos[n_all - 1] + (nb.cnt[n_all - 1] ? 1 : 0);
    if (h_end <= hyp_cap) res_off[h_end] = nb.lab_pos[n_all];
  }
  if (i >= n_all) return;
  const uint32_t n = nb.cnt[i];
  if (n == 0) return;
  const uint64_t hp = nb.hyp_pos[i], lp = nb.lab_pos[i];
  if (hp >= hyp_cap || lp + n > lab_cap) return;   // the host reserved both from the scan's totals
  const uint32_t ui = (uint32_t)(i / nb.N), r = (uint32_t)(i % nb.N), u = u0 + ui;
  res_cost[hp] = nb.fin_cost[i];
  res_off[hp] = lp;
  nb_walk(nb, (int)bv.T[u], lay.L, frame_model, bv.frame_off[u] - bv.frame_off[u0], ui, r, res_lab + lp, n);
}

void launch_nbest(hipStream_t st, const ScrfLayout& lay, ScrfBatchView bv, uint32_t u0, uint32_t n_utts, const ScrfArcSrc& src,
                  const ScrfNbestBufs& nb) {
  if (n_utts == 0) return;
  const int n_waves = lay.L < NB_WAVES ? (int)lay.L : NB_WAVES;
  const size_t sm = nbest_smem_bytes(dp_shape(lay), nb.N);
  hipFuncSetAttribute((const void*)k_nbest, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sm);
  hipLaunchKernelGGL(k_nbest, dim3(n_utts), dim3(64 * n_waves), sm, st, lay, bv, u0, src.S, src.Wn, src.M, src.m_per_frame,
                     src.frame_model, nb);
}

void launch_nbest_count(hipStream_t st, const ScrfLayout& lay, ScrfBatchView bv, uint32_t u0, uint32_t n_utts, int frame_model,
                        const ScrfNbestBufs& nb) {
  if (n_utts == 0) return;
  const uint64_t n = (uint64_t)n_utts * nb.N;
  hipLaunchKernelGGL(k_nbest_count, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, st, lay, bv, u0, n_utts, frame_model, nb);
}

void launch_nbest_scan(hipStream_t st, const ScrfNbestBufs& nb, uint32_t u0, uint32_t n_utts, uint64_t lab_base, uint64_t hyp_base,
                       uint64_t* hyp_off) {
  if (n_utts == 0) return;
  hipLaunchKernelGGL(k_nbest_scan, dim3(1), dim3(NB_SCAN_NT), 0, st, nb, u0, n_utts, lab_base, hyp_base, hyp_off);
}

void launch_nbest_trace(hipStream_t st, const ScrfLayout& lay, ScrfBatchView bv, uint32_t u0, uint32_t n_utts, int frame_model,
                        const ScrfNbestBufs& nb, uint64_t lab_cap, uint64_t hyp_cap, uint32_t* res_lab, uint64_t* res_off, float* res_cost) {
  if (n_utts == 0) return;
  const uint64_t n = (uint64_t)n_utts * nb.N;
  hipLaunchKernelGGL(k_nbest_trace, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, st, lay, bv, u0, n_utts, frame_model, nb, lab_cap,
                     hyp_cap, res_lab, res_off, res_cost);
}
