// scrf_sparse.hip -- the sparse feature maps stdsparse / stdsparsetrans (ftrmaps/CRF_StdSparseFeatureMap.cpp): a window
// vector of num_feas floats read as (index, value) pairs (x[2k], x[2k+1]).  Weight layout = the dense map's (ScrfLayout);
// a pair adds value * lambda[block + index].  DESIGN.md 4.12.
//
//   k_sp_relay     lambda re-laid index-major per call: lamT[f][o] = lambda[woff(o) + f], the bias as row nfe, so the
//                  lanes of one pair read one contiguous row (the native layout puts the labels `stride` doubles apart)
//   k_sp_scores    S / M: one wavefront per window row, lanes over outputs, pairs in the reference's order (k ascending,
//                  each product rounded, then added; bias last) -- bit-identical to computeStateArrayValue /
//                  computeTransMatrixValue in every precision tier
//   k_sp_hist, k_sp_colscan, k_sp_bscan, k_sp_scatter
//                  inverted index of a chunk: entries (row, value) bucketed by index, inside a bucket in (row, k) order
//                  -- a deterministic counting sort (per-tile histograms, scans, a ranked scatter; no atomics whose
//                  order could matter)
//   k_sp_counts, k_sp_counts_reduce
//                  per index bucket, lanes over outputs: grad[woff(o) + index] += sum_entries R[row][o] * value, in the
//                  bucket's fixed order (R = Y - gamma for states, Y - xi for transitions): segments of a bucket summed
//                  by separate workgroups, then added segment by segment
//   k_sp_colsum, k_sp_colsum_commit
//                  bias counts sum_rows R[row][o] (unit value) through fixed row blocks and an ordered reduction
// Everything adds into the staged gradient the caller passes; nothing uses floating-point atomics, so every tier is
// bit-reproducible from run to run.
#include "scrf_kernels.h"

#define SP_WIN 8192u    // indices per LDS counter window of the counting sort (32 KB)
#define SP_WIN_BITS 13
#define SP_NA 16        // outputs per thread of k_sp_counts

// (QNUInt32) x of the reference where that is defined; a negative, NaN or >= 2^32 index float is out of range
// (the reference's conversion is undefined there).  The range start is 0 (scrf_create refuses another).
__device__ __forceinline__ bool sp_index(float x, uint32_t hi, uint32_t* idx) {
  if (!(x >= 0.0f) || !(x < 4294967296.0f)) return false;
  const uint32_t i = (uint32_t)x;
  *idx = i;
  return i <= hi;
}

__device__ __forceinline__ uint32_t sp_woff(const ScrfLayout& l, int kind, uint32_t o) {
  return kind == 0 ? l.state_idx(o) : l.trans_idx(o / l.L, o % l.L);
}

__device__ __forceinline__ const float* sp_row(const float* X, uint32_t F, const uint64_t* xrow, uint64_t r) {
  return X + (xrow ? xrow[r] : r) * (uint64_t)F;
}

// ---- lambda, index-major --------------------------------------------------------------------------------------------
__global__ void k_sp_relay(const double* __restrict__ lambda, ScrfLayout l, int kind, uint32_t nrow, uint32_t n_out,
                           double* __restrict__ lamT) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (uint64_t)nrow * n_out) return;
  const uint32_t f = (uint32_t)(i / n_out), o = (uint32_t)(i % n_out);
  lamT[i] = lambda[sp_woff(l, kind, o) + f];
}

// ---- scores ---------------------------------------------------------------------------------------------------------
// One wavefront per row.  The row's pairs are held one per lane and broadcast with readlane: index, value and range flag
// are wave-uniform, the weight read is one contiguous lamT row per pair.  The first 64 pairs are loaded and range-checked
// once per row, before the loop over 64-output groups (36 of them for L = 48 transitions); a window of more than 64
// pairs reloads its further groups per output group.
__global__ __launch_bounds__(256) void k_sp_scores(const float* __restrict__ X, uint32_t F, const uint64_t* __restrict__ xrow,
                                                   uint64_t n_rows, const double* __restrict__ lamT, uint32_t nfe, uint32_t hi,
                                                   int use_b, uint32_t n_out, double* __restrict__ out) {
  const uint64_t r = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const uint32_t lane = threadIdx.x & 63;
  if (r >= n_rows) return;
  const float* x = sp_row(X, F, xrow, r);
  const uint32_t np = F / 2;
  uint32_t idx0 = 0;   // the row's first 64 pairs, staged once
  float v0 = 0.0f;
  int ok0 = 0;
  if (nfe && lane < np) {
    ok0 = sp_index(x[2 * lane], hi, &idx0) ? 1 : 0;
    v0 = x[2 * lane + 1];
  }
  for (uint32_t o0 = 0; o0 < n_out; o0 += 64) {
    const uint32_t o = o0 + lane;
    const bool live = o < n_out;
    double acc = 0.0;
    if (nfe) {
      for (uint32_t k0 = 0; k0 < np; k0 += 64) {
        const uint32_t k = k0 + lane;
        uint32_t idx = idx0;
        float v = v0;
        int ok = ok0;
        if (k0 > 0) {
          idx = 0; v = 0.0f; ok = 0;
          if (k < np) {
            ok = sp_index(x[2 * k], hi, &idx) ? 1 : 0;
            v = x[2 * k + 1];
          }
        }
        const uint32_t n = np - k0 < 64 ? np - k0 : 64;
        for (uint32_t j = 0; j < n; j++) {
          if (__builtin_amdgcn_readlane(ok, j)) {
            const uint32_t ij = (uint32_t)__builtin_amdgcn_readlane((int)idx, j);
            const float vj = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), j));
            if (live) acc += (double)vj * lamT[(uint64_t)ij * n_out + o];
          }
        }
      }
    }
    if (use_b && live) acc += lamT[(uint64_t)nfe * n_out + o];
    if (live) out[r * n_out + o] = acc;
  }
}

// ---- inverted index (deterministic counting sort) -------------------------------------------------------------------
// Rows are cut into tiles of rpt rows, one wavefront per (tile, window of SP_WIN indices).  Each index window rereads
// its tile's rows: the window bytes these two kernels read grow with ceil(index space / 8192) (one pass up to 8192
// indices, the shapes measured in DESIGN.md 4.12; 20000 indices read the windows three times).
__global__ __launch_bounds__(64) void k_sp_hist(const float* __restrict__ X, uint32_t F, const uint64_t* __restrict__ xrow,
                                                uint64_t n_rows, uint32_t rpt, uint32_t nidx, uint32_t* __restrict__ hist) {
  __shared__ uint32_t cnt[SP_WIN];
  const uint32_t lane = threadIdx.x, tile = blockIdx.x, w0 = blockIdx.y * SP_WIN;
  for (uint32_t i = lane; i < SP_WIN; i += 64) cnt[i] = 0;
  __syncthreads();
  const uint64_t r0 = (uint64_t)tile * rpt, r1 = r0 + rpt < n_rows ? r0 + rpt : n_rows;
  const uint32_t np = F / 2;
  for (uint64_t r = r0; r < r1; r++) {
    const float* x = sp_row(X, F, xrow, r);
    for (uint32_t k = lane; k < np; k += 64) {
      uint32_t idx;
      if (sp_index(x[2 * k], nidx - 1, &idx) && idx >= w0 && idx - w0 < SP_WIN) atomicAdd(&cnt[idx - w0], 1u);
    }
  }
  __syncthreads();
  for (uint32_t i = lane; i < SP_WIN && w0 + i < nidx; i += 64) hist[(uint64_t)tile * nidx + w0 + i] = cnt[i];
}

// per index: exclusive prefix over the tiles (in place), total per index
__global__ void k_sp_colscan(uint32_t* __restrict__ hist, uint32_t ntiles, uint32_t nidx, uint32_t* __restrict__ tot) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nidx) return;
  uint32_t run = 0, t = 0;
  for (; t + 8 <= ntiles; t += 8) {   // eight loads in flight, then the running sum
    uint32_t c[8];
#pragma unroll
    for (int j = 0; j < 8; j++) c[j] = hist[(uint64_t)(t + j) * nidx + i];
#pragma unroll
    for (int j = 0; j < 8; j++) { hist[(uint64_t)(t + j) * nidx + i] = run; run += c[j]; }
  }
  for (; t < ntiles; t++) {
    const uint32_t c = hist[(uint64_t)t * nidx + i];
    hist[(uint64_t)t * nidx + i] = run;
    run += c;
  }
  tot[i] = run;
}

// bucket starts: exclusive prefix of the totals, bstart[nidx] = number of entries (one workgroup)
// (seg > 0: the same over ceil(tot / seg), the segments of each bucket)
__global__ __launch_bounds__(1024) void k_sp_bscan(const uint32_t* __restrict__ tot, uint32_t nidx, uint32_t seg, uint32_t* __restrict__ bstart) {
  __shared__ uint32_t s[1024];
  __shared__ uint32_t carry;
  const uint32_t tid = threadIdx.x;
  if (tid == 0) carry = 0;
  __syncthreads();
  for (uint32_t b = 0; b < nidx; b += 1024) {
    uint32_t v = b + tid < nidx ? tot[b + tid] : 0;
    if (seg) v = (v + seg - 1) / seg;
    s[tid] = v;
    __syncthreads();
    for (uint32_t d = 1; d < 1024; d <<= 1) {   // inclusive Hillis-Steele scan
      const uint32_t a = tid >= d ? s[tid - d] : 0;
      __syncthreads();
      s[tid] += a;
      __syncthreads();
    }
    if (b + tid < nidx) bstart[b + tid] = carry + s[tid] - v;
    __syncthreads();
    if (tid == 1023) carry += s[1023];
    __syncthreads();
  }
  if (tid == 0) bstart[nidx] = carry;
}

// entries of each tile in (row, k) order: lanes holding the same index in one 64-pair group are ranked by lane (k
// ascending), the group's first lane advances the index's counter
__global__ __launch_bounds__(64) void k_sp_scatter(const float* __restrict__ X, uint32_t F, const uint64_t* __restrict__ xrow,
                                                   uint64_t n_rows, uint32_t rpt, uint32_t nidx, const uint32_t* __restrict__ hist,
                                                   const uint32_t* __restrict__ bstart, uint32_t* __restrict__ erow,
                                                   float* __restrict__ eval) {
  __shared__ uint32_t cnt[SP_WIN];
  const uint32_t lane = threadIdx.x, tile = blockIdx.x, w0 = blockIdx.y * SP_WIN;
  for (uint32_t i = lane; i < SP_WIN && w0 + i < nidx; i += 64) cnt[i] = bstart[w0 + i] + hist[(uint64_t)tile * nidx + w0 + i];
  __syncthreads();
  const uint64_t r0 = (uint64_t)tile * rpt, r1 = r0 + rpt < n_rows ? r0 + rpt : n_rows;
  const uint32_t np = F / 2;
  const uint64_t lt = (1ull << lane) - 1;
  for (uint64_t r = r0; r < r1; r++) {
    const float* x = sp_row(X, F, xrow, r);
    for (uint32_t k0 = 0; k0 < np; k0 += 64) {
      const uint32_t k = k0 + lane;
      uint32_t idx = 0;
      float v = 0.0f;
      bool ok = false;
      if (k < np) {
        ok = sp_index(x[2 * k], nidx - 1, &idx) && idx >= w0 && idx - w0 < SP_WIN;
        v = x[2 * k + 1];
      }
      const uint32_t key = ok ? idx - w0 : 0;
      uint64_t m = __ballot(ok);
      for (int b = 0; b < SP_WIN_BITS; b++) {
        const bool bit = (key >> b) & 1;
        const uint64_t bal = __ballot(ok && bit);
        m &= bit ? bal : ~bal;
      }
      uint32_t base = 0;
      if (ok) base = cnt[key];
      __syncthreads();   // every lane has read its counter before a group's first lane advances it
      if (ok) {
        const uint32_t rank = (uint32_t)__popcll(m & lt);
        erow[base + rank] = (uint32_t)r;
        eval[base + rank] = v;
        if (rank == 0) cnt[key] = base + (uint32_t)__popcll(m);
      }
      __syncthreads();
    }
  }
}

// ---- counts ---------------------------------------------------------------------------------------------------------
// A bucket is cut into segments of `seg` entries (its last one shorter); one workgroup per segment sums
// R[row][o] * value over its entries in order into part[segment][o], k_sp_counts_reduce adds a bucket's segments in
// order into the gradient.  The segments keep a long bucket from becoming one latency-bound serial walk.
template <int NA>
__global__ __launch_bounds__(256) void k_sp_counts(const double* __restrict__ R, uint32_t n_out, uint32_t nidx, uint32_t seg,
                                                   const uint32_t* __restrict__ bstart, const uint32_t* __restrict__ sstart,
                                                   const uint32_t* __restrict__ erow, const float* __restrict__ eval,
                                                   double* __restrict__ part) {
  const uint32_t sg = blockIdx.x;
  if (sg >= sstart[nidx]) return;
  uint32_t lo = 0, hi = nidx;   // bucket: the last idx with sstart[idx] <= sg
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) / 2;
    if (sstart[mid] <= sg) lo = mid; else hi = mid;
  }
  const uint32_t idx = lo;
  const uint32_t e0 = bstart[idx] + (sg - sstart[idx]) * seg;
  const uint32_t e1 = e0 + seg < bstart[idx + 1] ? e0 + seg : bstart[idx + 1];
  const uint32_t nt = blockDim.x;
  for (uint32_t o0 = 0; o0 < n_out; o0 += NA * nt) {
    double acc[NA];
#pragma unroll
    for (int j = 0; j < NA; j++) acc[j] = 0.0;
    for (uint32_t e = e0; e < e1; e++) {
      const double* Rr = R + (uint64_t)erow[e] * n_out;
      const double v = (double)eval[e];
#pragma unroll
      for (int j = 0; j < NA; j++) {
        const uint32_t o = o0 + j * nt + threadIdx.x;
        if (o < n_out) acc[j] += Rr[o] * v;
      }
    }
#pragma unroll
    for (int j = 0; j < NA; j++) {
      const uint32_t o = o0 + j * nt + threadIdx.x;
      if (o < n_out) part[(uint64_t)sg * n_out + o] = acc[j];
    }
  }
}

__global__ __launch_bounds__(256) void k_sp_counts_reduce(const double* __restrict__ part, uint32_t n_out, const uint32_t* __restrict__ sstart,
                                                          ScrfLayout l, int kind, double* __restrict__ grad) {
  const uint32_t idx = blockIdx.x;
  const uint32_t s0 = sstart[idx], s1 = sstart[idx + 1];
  if (s0 == s1) return;
  for (uint32_t o = threadIdx.x; o < n_out; o += blockDim.x) {
    double acc = 0.0;
    for (uint32_t q = s0; q < s1; q++) acc += part[(uint64_t)q * n_out + o];
    grad[sp_woff(l, kind, o) + idx] += acc;
  }
}

__global__ __launch_bounds__(256) void k_sp_colsum(const double* __restrict__ R, uint64_t n_rows, uint32_t n_out, uint64_t rpb,
                                                   double* __restrict__ slab) {
  const uint64_t r0 = (uint64_t)blockIdx.x * rpb, r1 = r0 + rpb < n_rows ? r0 + rpb : n_rows;
  for (uint32_t o = threadIdx.x; o < n_out; o += blockDim.x) {
    double acc = 0.0;
    uint64_t r = r0;
    for (; r + 4 <= r1; r += 4) {   // four rows' loads in flight, then added in row order
      const double a0 = R[r * n_out + o], a1 = R[(r + 1) * n_out + o], a2 = R[(r + 2) * n_out + o], a3 = R[(r + 3) * n_out + o];
      acc += a0; acc += a1; acc += a2; acc += a3;
    }
    for (; r < r1; r++) acc += R[r * n_out + o];
    slab[(uint64_t)blockIdx.x * n_out + o] = acc;
  }
}

__global__ void k_sp_colsum_commit(const double* __restrict__ slab, uint32_t nblk, uint32_t n_out, ScrfLayout l, int kind,
                                   uint32_t fno, double* __restrict__ grad) {
  const uint32_t o = blockIdx.x * blockDim.x + threadIdx.x;
  if (o >= n_out) return;
  double s = 0.0;
  for (uint32_t b = 0; b < nblk; b++) s += slab[(uint64_t)b * n_out + o];
  grad[sp_woff(l, kind, o) + fno] += s;
}

// ---- host side ------------------------------------------------------------------------------------------------------
static uint32_t sp_block_threads(uint32_t n_out) { return n_out <= 64 ? 64 : 256; }

void sparse_index_plan(uint64_t n_rows, uint32_t nidx, uint32_t* ntiles, uint32_t* rpt) {
  // tiles of >= 64 rows, at most 8192 of them (a wavefront each: several per SIMD) and at most 16 M histogram cells (64 MB)
  uint64_t max_t = std::min<uint64_t>(8192, std::max<uint64_t>(1, (16ull << 20) / std::max<uint32_t>(1, nidx)));
  uint64_t r = std::max<uint64_t>(64, (n_rows + max_t - 1) / max_t);
  *rpt = (uint32_t)r;
  *ntiles = (uint32_t)std::max<uint64_t>(1, (n_rows + r - 1) / r);
}

static size_t pad256s(size_t b) { return (b + 255) & ~(size_t)255; }
#define SP_COLSUM_BLOCKS 2048u

// entries per count segment: >= 128, and the partial rows of all segments within about 256 MB
static uint32_t sp_seg_len(uint64_t ne, uint32_t n_out) {
  return (uint32_t)std::max<uint64_t>(128, (ne * n_out * 8 + (1ull << 28) - 1) >> 28);
}
static uint32_t sp_colsum_blocks(uint64_t n_rows) {
  return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(SP_COLSUM_BLOCKS, (n_rows + 63) / 64));
}
static uint64_t sp_max_segs(uint64_t ne, uint32_t nidx, uint32_t n_out) {
  return ne / sp_seg_len(ne, n_out) + std::min<uint64_t>(nidx, ne) + 1;
}

size_t sparse_counts_bytes(uint64_t n_rows, uint32_t F, uint32_t nidx, uint32_t n_out) {
  uint32_t nt, rpt;
  sparse_index_plan(n_rows, nidx, &nt, &rpt);
  const uint64_t ne = n_rows * (F / 2);
  return pad256s((size_t)nt * nidx * 4) + pad256s((size_t)nidx * 4) + 2 * pad256s(((size_t)nidx + 1) * 4) + 2 * pad256s(ne * 4) +
         pad256s((size_t)sp_colsum_blocks(n_rows) * n_out * 8) + pad256s(sp_max_segs(ne, nidx, n_out) * n_out * 8);
}

void sparse_counts_carve(void* base, uint64_t n_rows, uint32_t F, uint32_t nidx, uint32_t n_out, ScrfSparseIndex* ix) {
  char* p = (char*)base;
  sparse_index_plan(n_rows, nidx, &ix->ntiles, &ix->rpt);
  const uint64_t ne = n_rows * (F / 2);
  ix->hist = (uint32_t*)p;   p += pad256s((size_t)ix->ntiles * nidx * 4);
  ix->tot = (uint32_t*)p;    p += pad256s((size_t)nidx * 4);
  ix->bstart = (uint32_t*)p; p += pad256s(((size_t)nidx + 1) * 4);
  ix->sstart = (uint32_t*)p; p += pad256s(((size_t)nidx + 1) * 4);
  ix->erow = (uint32_t*)p;   p += pad256s(ne * 4);
  ix->eval = (float*)p;      p += pad256s(ne * 4);
  ix->slab = (double*)p;      p += pad256s((size_t)sp_colsum_blocks(n_rows) * n_out * 8);
  ix->part = (double*)p;
  ix->seg = sp_seg_len(ne, n_out);
  ix->max_segs = sp_max_segs(ne, nidx, n_out);
}

void launch_sp_relay(hipStream_t st, const double* lambda, const ScrfLayout& l, int kind, double* lamT) {
  const uint32_t nfe = kind ? l.ntfe : l.nsfe, use_b = kind ? l.use_tb : l.use_sb;
  const uint32_t n_out = kind ? l.L * l.L : l.L, nrow = nfe + use_b;
  const uint64_t n = (uint64_t)nrow * n_out;
  if (n == 0) return;
  hipLaunchKernelGGL(k_sp_relay, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, st, lambda, l, kind, nrow, n_out, lamT);
}

void launch_sp_scores(hipStream_t st, const float* X, uint32_t F, const uint64_t* xrow, uint64_t n_rows, const double* lamT,
                      const ScrfLayout& l, int kind, double* out) {
  if (n_rows == 0) return;
  const uint32_t nfe = kind ? l.ntfe : l.nsfe, use_b = kind ? l.use_tb : l.use_sb;
  const uint32_t hi = kind ? l.tfe : l.sfe, n_out = kind ? l.L * l.L : l.L;
  hipLaunchKernelGGL(k_sp_scores, dim3((uint32_t)((n_rows + 3) / 4)), dim3(256), 0, st, X, F, xrow, n_rows, lamT, nfe, hi,
                     (int)use_b, n_out, out);
}

void launch_sp_counts(hipStream_t st, const float* X, uint32_t F, const uint64_t* xrow, uint64_t n_rows, const double* R,
                      const ScrfLayout& l, int kind, const ScrfSparseIndex& ix, double* grad) {
  if (n_rows == 0) return;
  const uint32_t nfe = kind ? l.ntfe : l.nsfe, use_b = kind ? l.use_tb : l.use_sb;
  const uint32_t n_out = kind ? l.L * l.L : l.L;
  if (nfe) {
    const uint32_t nwin = (nfe + SP_WIN - 1) / SP_WIN;
    hipLaunchKernelGGL(k_sp_hist, dim3(ix.ntiles, nwin), dim3(64), 0, st, X, F, xrow, n_rows, ix.rpt, nfe, ix.hist);
    hipLaunchKernelGGL(k_sp_colscan, dim3((nfe + 255) / 256), dim3(256), 0, st, ix.hist, ix.ntiles, nfe, ix.tot);
    hipLaunchKernelGGL(k_sp_bscan, dim3(1), dim3(1024), 0, st, ix.tot, nfe, 0u, ix.bstart);
    hipLaunchKernelGGL(k_sp_bscan, dim3(1), dim3(1024), 0, st, ix.tot, nfe, ix.seg, ix.sstart);
    hipLaunchKernelGGL(k_sp_scatter, dim3(ix.ntiles, nwin), dim3(64), 0, st, X, F, xrow, n_rows, ix.rpt, nfe, ix.hist, ix.bstart,
                       ix.erow, ix.eval);
    if (n_out <= 64)
      hipLaunchKernelGGL(k_sp_counts<1>, dim3((uint32_t)ix.max_segs), dim3(64), 0, st, R, n_out, nfe, ix.seg, ix.bstart, ix.sstart,
                         ix.erow, ix.eval, ix.part);
    else
      hipLaunchKernelGGL(k_sp_counts<SP_NA>, dim3((uint32_t)ix.max_segs), dim3(256), 0, st, R, n_out, nfe, ix.seg, ix.bstart, ix.sstart,
                         ix.erow, ix.eval, ix.part);
    hipLaunchKernelGGL(k_sp_counts_reduce, dim3(nfe), dim3(sp_block_threads(n_out)), 0, st, ix.part, n_out, ix.sstart, l, kind, grad);
  }
  if (use_b) {
    const uint32_t nblk = sp_colsum_blocks(n_rows);
    const uint64_t rpb = (n_rows + nblk - 1) / nblk;
    hipLaunchKernelGGL(k_sp_colsum, dim3(nblk), dim3(sp_block_threads(n_out)), 0, st, R, n_rows, n_out, rpb, ix.slab);
    hipLaunchKernelGGL(k_sp_colsum_commit, dim3((n_out + 255) / 256), dim3(256), 0, st, ix.slab, nblk, n_out, l, kind, nfe, grad);
  }
}
