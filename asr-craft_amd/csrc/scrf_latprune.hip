// scrf_latprune.hip -- beam-pruned lattices, batched.
//
// The lattice is the one k_arcs_seg / k_arcs_frame emit: both take a node's arcs -- states, order and float weights -- from
// scrf_node_arc (scrf_arcw.h); it is never materialised here.  With wd = (double)w:
//   fwd[0] = 0,      fwd[s] = min over arcs into s  of fwd[src] + wd
//   bwd[final] = 0,  bwd[s] = min over arcs out of s of wd + bwd[dst]
//   an arc is kept iff (fwd[src] + wd) + bwd[dst] <= fwd[final] + beam          (fp64, that association)
// min is exact and every + rounds once (-ffp-contract=off), so the kept set does not depend on the order of evaluation.
//
//   k_lat_sweep   one workgroup per (utterance, direction): labels on threads, the D-deep window of the recursion in LDS
//   k_lat_count   one workgroup per (utterance, node): kept arcs of the node (T + 1 nodes, the last = the final arcs)
//   k_lat_scan    exclusive scan of the node counts of a chunk (integers)
//   k_lat_emit    the grid of k_lat_count: recomputes the test and compacts the node's arcs in arc order
// No atomics anywhere: two runs give the same bytes.
#include "scrf_kernels.h"
#include "scrf_arcw.h"

#include <math.h>

#define LAT_NT 256
#define LAT_SCAN_NT 1024

static __device__ inline double lat_min(double a, double b) { return b < a ? b : a; }

// State kinds of the segmental lattice: boundary states (t, l), t >= 1 ("a segment of label l starts at frame t") and end
// states (t, l) ("a segment of label l ended at frame t"); the frame model has one state (t, c) per frame and label, kept
// in the E arrays.  Arrays are [frames of the chunk][L].
__global__ void k_lat_sweep(ScrfLayout lay, ScrfBatchView bv, uint32_t u0, const double* __restrict__ S,
                            const double* __restrict__ M, int m_per_frame, int frame_model, ScrfLatBufs lb) {
  extern __shared__ double lsm[];
  const int L = lay.L, D = lay.D;
  const int tid = threadIdx.x, NT = blockDim.x;
  const uint32_t u = u0 + blockIdx.x;
  const ScrfArcView v(ScrfArcSrc{S, nullptr, M, m_per_frame, frame_model}, lay, bv, u0, u);
  const int T = (int)v.T;
  const uint64_t f_base = v.f_base;
  const double wfin = (double)(frame_model ? 0.0f : -0.0f);
  double* sh = lsm;            // [2][L]: the vector every label reads (end states forward, boundary states backward)
  double* ring = lsm + 2 * L;  // [D][L]: the vector a label reads only its own column of
  if (T == 0) return;
  if (blockIdx.y == 0) {  // ---- forward
    double* fB = lb.fB + f_base * L;
    double* fE = lb.fE + f_base * L;
    for (int t = 0; t < T; t++) {
      double* cur = sh + (t & 1) * L;
      const double* prev = sh + ((t + 1) & 1) * L;
      const double* Mt = v.Mt(t);
      const uint64_t base = scrf_seg_base(t, D);
      const int np = (int)scrf_num_prev(t, D), nd = (int)scrf_node_max_dur(t, D);
      for (int l = tid; l < L; l += NT) {
        double e = INFINITY;
        if (frame_model) {
          if (t == 0) e = 0.0 + (double)v.start(l);
          else
            for (int p = 0; p < L; p++) e = lat_min(e, prev[p] + (double)v.frame(Mt, t, p, l));
        } else {
          if (t >= 1) {
            double b = INFINITY;
            for (int p = 0; p < L; p++) b = lat_min(b, prev[p] + (double)v.boundary(Mt, p, l));
            ring[(t % D) * L + l] = b;
            fB[(size_t)t * L + l] = b;
          }
          for (int d = 1; d <= nd; d++) {
            const double src = d <= np ? ring[((t - d + 1) % D) * L + l] : 0.0;
            e = lat_min(e, src + (double)v.segment(base, d, l));
          }
        }
        cur[l] = e;
        fE[(size_t)t * L + l] = e;
      }
      __syncthreads();
    }
    if (tid == 0) {
      const double* last = sh + ((T - 1) & 1) * L;
      double best = INFINITY;
      for (int p = 0; p < L; p++) best = lat_min(best, last[p] + wfin);
      lb.best[u] = best;
    }
  } else {  // ---- backward
    double* bB = lb.bB + f_base * L;
    double* bE = lb.bE + f_base * L;
    for (int t = T - 1; t >= 0; t--) {
      double* cur = sh + (t & 1) * L;
      const double* nxt = sh + ((t + 1) & 1) * L;
      const double* Mn = v.Mt(t + 1);   // read only when t + 1 < T
      for (int l = tid; l < L; l += NT) {
        double e = INFINITY;
        if (t == T - 1) e = wfin + 0.0;
        else if (frame_model)
          for (int c = 0; c < L; c++) e = lat_min(e, (double)v.frame(Mn, t + 1, l, c) + nxt[c]);
        else
          for (int c = 0; c < L; c++) e = lat_min(e, (double)v.boundary(Mn, l, c) + nxt[c]);
        bE[(size_t)t * L + l] = e;
        if (frame_model) {
          cur[l] = e;
        } else {
          ring[(t % D) * L + l] = e;
          if (t >= 1) {   // segments of label l starting at frame t: durations 1 .. min(D, T - t)
            double b = INFINITY;
            const int dmax = T - t < D ? T - t : D;
            for (int d = 1; d <= dmax; d++) {
              const int te = t + d - 1;
              b = lat_min(b, (double)v.segment(scrf_seg_base(te, D), d, l) + ring[(te % D) * L + l]);
            }
            cur[l] = b;
            bB[(size_t)t * L + l] = b;
          }
        }
      }
      __syncthreads();
    }
  }
}

// everything a (utterance, node) workgroup needs to walk its arcs: the node (scrf_arcw.h) and the utterance's sweeps
struct LatNode {
  ScrfArcNode a;
  const double *fB, *fE, *bB, *bE;
  double limit;
};

static __device__ inline LatNode lat_node(const ScrfLayout& lay, const ScrfBatchView& bv, uint32_t u0, uint32_t u, uint32_t t,
                                          const ScrfArcSrc& src, const ScrfLatBufs& lb, double beam) {
  const ScrfArcView v(src, lay, bv, u0, u);
  const size_t fl = v.f_base * v.L;
  return LatNode{scrf_arc_node(v, lay.D, t, src.frame_model, src.frame_model ? 0.0f : -0.0f),
                 lb.fB + fl, lb.fE + fl, lb.bB + fl, lb.bE + fl, lb.best[u] + beam};
}

// arc `idx` of the node and whether the beam keeps it: fwd of its source state, bwd of its destination
static __device__ inline bool lat_arc(const LatNode& n, uint32_t idx, scrf_arc* a) {
  ScrfArcEnd s, d;
  *a = scrf_node_arc(n.a, idx, &s, &d);
  const size_t L = n.a.v.L;
  const double fs = s.kind == SCRF_ARC_TERM ? 0.0 : (s.kind == SCRF_ARC_BOUNDARY ? n.fB : n.fE)[s.t * L + s.l];
  const double bd = d.kind == SCRF_ARC_TERM ? 0.0 : (d.kind == SCRF_ARC_BOUNDARY ? n.bB : n.bE)[d.t * L + d.l];
  return (fs + (double)a->w) + bd <= n.limit;
}

// node index inside the chunk: every utterance has T + 1 nodes
static __device__ inline uint64_t lat_node_index(const ScrfBatchView& bv, uint32_t u0, uint32_t u, uint32_t t) {
  return bv.frame_off[u] - bv.frame_off[u0] + (u - u0) + t;
}

__global__ __launch_bounds__(LAT_NT) void k_lat_count(ScrfLayout lay, ScrfBatchView bv, uint32_t u0, const double* __restrict__ S,
                                                     const double* __restrict__ M, int m_per_frame, int frame_model,
                                                     ScrfLatBufs lb, double beam, uint32_t* __restrict__ counts) {
  __shared__ uint32_t red[LAT_NT];
  const uint32_t u = u0 + blockIdx.y, t = blockIdx.x;
  if (t > bv.T[u]) return;
  const LatNode n = lat_node(lay, bv, u0, u, t, ScrfArcSrc{S, nullptr, M, m_per_frame, frame_model}, lb, beam);
  uint32_t c = 0;
  scrf_arc a;
  for (uint32_t idx = threadIdx.x; idx < n.a.n_arcs; idx += LAT_NT) c += lat_arc(n, idx, &a) ? 1u : 0u;
  red[threadIdx.x] = c;
  __syncthreads();
  for (uint32_t s = LAT_NT / 2; s > 0; s >>= 1) {
    if (threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) counts[lat_node_index(bv, u0, u, t)] = red[0];
}

// node_off[i] = kept arcs of the chunk before node i (node_off[n] = all of them); utt_off[u] = base + those before
// utterance u, base = kept arcs of the chunks before this one.  One workgroup: every thread sums a contiguous run.
__global__ __launch_bounds__(LAT_SCAN_NT) void k_lat_scan(const uint32_t* __restrict__ counts, uint64_t n, uint64_t* __restrict__ node_off,
                                                         ScrfBatchView bv, uint32_t u0, uint32_t n_utts, uint64_t base,
                                                         uint64_t* __restrict__ utt_off) {
  __shared__ uint64_t sh[LAT_SCAN_NT];
  const uint32_t tid = threadIdx.x;
  const uint64_t per = (n + LAT_SCAN_NT - 1) / LAT_SCAN_NT;
  const uint64_t lo = (uint64_t)tid * per < n ? (uint64_t)tid * per : n, hi = lo + per < n ? lo + per : n;
  uint64_t s = 0;
  for (uint64_t i = lo; i < hi; i++) s += counts[i];
  sh[tid] = s;
  __syncthreads();
  for (uint32_t off = 1; off < LAT_SCAN_NT; off <<= 1) {
    const uint64_t v = tid >= off ? sh[tid - off] : 0;
    __syncthreads();
    sh[tid] += v;
    __syncthreads();
  }
  uint64_t run = sh[tid] - s;
  for (uint64_t i = lo; i < hi; i++) { node_off[i] = run; run += counts[i]; }
  if (tid == LAT_SCAN_NT - 1) node_off[n] = sh[tid];
  __syncthreads();
  for (uint32_t k = tid; k <= n_utts; k += LAT_SCAN_NT) {
    const uint64_t i = k < n_utts ? lat_node_index(bv, u0, u0 + k, 0) : n;
    utt_off[u0 + k] = base + node_off[i];
  }
}

__global__ __launch_bounds__(LAT_NT) void k_lat_emit(ScrfLayout lay, ScrfBatchView bv, uint32_t u0, const double* __restrict__ S,
                                                    const double* __restrict__ M, int m_per_frame, int frame_model,
                                                    ScrfLatBufs lb, double beam, const uint64_t* __restrict__ node_off,
                                                    uint64_t base, uint64_t cap, scrf_arc* __restrict__ out) {
  __shared__ uint32_t wcnt[LAT_NT / SCRF_WAVE];
  const uint32_t u = u0 + blockIdx.y, t = blockIdx.x;
  if (t > bv.T[u]) return;
  const uint64_t ni = lat_node_index(bv, u0, u, t);
  const uint64_t o0 = node_off[ni], o1 = node_off[ni + 1];
  if (o0 == o1) return;   // nothing of this node survives
  const LatNode n = lat_node(lay, bv, u0, u, t, ScrfArcSrc{S, nullptr, M, m_per_frame, frame_model}, lb, beam);
  const uint32_t lane = threadIdx.x % SCRF_WAVE, wv = threadIdx.x / SCRF_WAVE;
  uint64_t run = base + o0;
  // the node's arcs in index order, a workgroup's width at a time: rank inside the wavefront from the ballot, the
  // wavefronts' bases through LDS
  for (uint32_t r0 = 0; r0 < n.a.n_arcs; r0 += LAT_NT) {
    const uint32_t idx = r0 + threadIdx.x;
    scrf_arc a;
    const bool keep = idx < n.a.n_arcs && lat_arc(n, idx, &a);
    const unsigned long long bal = __ballot(keep);
    if (lane == 0) wcnt[wv] = (uint32_t)__popcll(bal);
    __syncthreads();
    uint32_t wb = 0, tot = 0;
    for (uint32_t w = 0; w < LAT_NT / SCRF_WAVE; w++) {
      const uint32_t c = wcnt[w];
      if (w < wv) wb += c;
      tot += c;
    }
    if (keep) {
      const uint64_t pos = run + wb + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull));
      if (pos < cap) out[pos] = a;
    }
    run += tot;
    __syncthreads();
  }
}


void launch_lat_sweep(hipStream_t st, const ScrfLayout& lay, ScrfBatchView bv, uint32_t u0, uint32_t n_utts, const ScrfArcSrc& src,
                      const ScrfLatBufs& lb) {
  if (n_utts == 0) return;
  int NT = ((int)lay.L + 63) / 64 * 64;
  if (NT > 256) NT = 256;
  const size_t sm = lat_sweep_smem_bytes(dp_shape(lay));
  hipFuncSetAttribute((const void*)k_lat_sweep, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sm);
  hipLaunchKernelGGL(k_lat_sweep, dim3(n_utts, 2), dim3(NT), sm, st, lay, bv, u0, src.S, src.M, src.m_per_frame, src.frame_model, lb);
}

void launch_lat_count(hipStream_t st, const ScrfLayout& lay, ScrfBatchView bv, uint32_t u0, uint32_t n_utts, uint32_t t_max,
                      const ScrfArcSrc& src, const ScrfLatBufs& lb, double beam, uint32_t* counts) {
  if (n_utts == 0) return;
  hipLaunchKernelGGL(k_lat_count, dim3(t_max + 1, n_utts), dim3(LAT_NT), 0, st, lay, bv, u0, src.S, src.M, src.m_per_frame, src.frame_model,
                     lb, beam, counts);
}

void launch_lat_scan(hipStream_t st, ScrfBatchView bv, uint32_t u0, uint32_t n_utts, const uint32_t* counts, uint64_t n_nodes,
                     uint64_t* node_off, uint64_t base, uint64_t* utt_off) {
  if (n_utts == 0) return;
  hipLaunchKernelGGL(k_lat_scan, dim3(1), dim3(LAT_SCAN_NT), 0, st, counts, n_nodes, node_off, bv, u0, n_utts, base, utt_off);
}

void launch_lat_emit(hipStream_t st, const ScrfLayout& lay, ScrfBatchView bv, uint32_t u0, uint32_t n_utts, uint32_t t_max,
                     const ScrfArcSrc& src, const ScrfLatBufs& lb, double beam, const uint64_t* node_off, uint64_t base, uint64_t cap,
                     scrf_arc* out) {
  if (n_utts == 0) return;
  hipLaunchKernelGGL(k_lat_emit, dim3(t_max + 1, n_utts), dim3(LAT_NT), 0, st, lay, bv, u0, src.S, src.M, src.m_per_frame, src.frame_model,
                     lb, beam, node_off, base, cap, out);
}
