// scrf_arcw.h -- the float arc weights of the lattice, one expression per arc kind.  Shared by the arc emission
// (k_arcs_seg / k_arcs_frame, scrf_kernels.hip) and the lattice beam (scrf_latprune.hip), which must see exactly the
// weights the full lattice carries: w = (float)(-1.0 * score), formed in fp64 and rounded once.
#ifndef SCRF_ARCW_H_
#define SCRF_ARCW_H_

#include "scrf_common.h"

// boundary arc end(t-1, pl) -> boundary(t, lab); Mt = the transition matrix of frame t (or the only one)
__device__ inline float scrf_w_boundary(const double* __restrict__ Mt, uint32_t L, uint32_t pl, uint32_t lab) {
  return (float)(-1.0 * Mt[(size_t)pl * L + lab]);
}
// segment arc of duration d ending at the frame whose first window row is `base` (scrf_seg_base); Su = the utterance's scores
__device__ inline float scrf_w_segment(const double* __restrict__ Su, uint64_t base, uint32_t d, uint32_t L, uint32_t lab) {
  return (float)(-1.0 * Su[(base + d - 1) * L + lab]);
}
// frame model: state(t-1, p) -> state(t, c), t >= 1; the arcs out of the start state carry scrf_w_segment(Su, 0, 1, L, c)
__device__ inline float scrf_w_frame(const double* __restrict__ Mt, const double* __restrict__ Su, uint32_t t, uint32_t L,
                                     uint32_t p, uint32_t c) {
  return (float)(-1.0 * (Mt[(size_t)p * L + c] + Su[(size_t)t * L + c]));
}

#endif  // SCRF_ARCW_H_
