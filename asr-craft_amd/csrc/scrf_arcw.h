// scrf_arcw.h -- the arcs of the lattice as every search sees them: where a chunk's arc weights come from (ScrfArcSrc),
// one utterance's view of them (ScrfArcView) and the arcs of one lattice node in the reference's order (ScrfArcNode).
// Shared by the arc emission (scrf_kernels.hip), the lattice beam (scrf_latprune.hip), forced alignment's workgroup kernel
// (scrf_align.hip) and N-best (scrf_nbest.hip), which must all see exactly the weights the full lattice carries:
// w = (float)(-1.0 * score), formed in fp64 and rounded once.  k_viterbi and k_align_wave write the same expressions out
// (the view cost them 0.5 - 0.8 %, profiles/EXPERIMENTS.md); their launchers take the ScrfArcSrc like the others.
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

// A chunk's arcs (host side; the engine's arc_src() builds it).  Exactly one of S (fp64 scores) and Wn (their float arc
// weights, already formed: fast decode, segment model only) is set.  M: one matrix (m_per_frame 0) or one per frame of the
// chunk (1); the per-window matrices of STDSEG_NO_DUR (2) have kernels of their own.  A launcher unpacks the struct into
// the kernel's `const ... * __restrict__` parameters -- the compiler takes no-alias and read-only from those, not from
// pointers inside a struct -- and the kernel forms the view below from them.
struct ScrfArcSrc {
  const double* S;
  const float* Wn;
  const double* M;
  int m_per_frame, frame_model;
};

// one utterance of the chunk
struct ScrfArcView {
  const double* Su;   // the utterance's scores, or nullptr
  const float* Wu;    // the utterance's float segment weights, or nullptr
  const double* M;    // the chunk's first matrix
  size_t m_stride;    // L * L with a matrix per frame, else 0
  uint32_t L, T;
  uint64_t f_base, s_base;   // frames / score rows of the chunk before the utterance

  // utterance u of the chunk that starts at u0
  __device__ ScrfArcView(const ScrfArcSrc& src, const ScrfLayout& lay, const ScrfBatchView& bv, uint32_t u0, uint32_t u)
      : ScrfArcView(src, lay, bv.T[u], bv.frame_off[u] - bv.frame_off[u0], bv.seg_off[u] - bv.seg_off[u0]) {}
  // the only utterance of its chunk: u0 = u
  __device__ ScrfArcView(const ScrfArcSrc& src, const ScrfLayout& lay, uint32_t T_, uint64_t fb = 0, uint64_t sb = 0)
      : Su(src.S ? src.S + sb * lay.L : nullptr), Wu(src.Wn ? src.Wn + sb * lay.L : nullptr), M(src.M),
        m_stride(src.m_per_frame ? (size_t)lay.L * lay.L : 0), L(lay.L), T(T_), f_base(fb), s_base(sb) {}

  __device__ const double* Mt(uint32_t t) const { return M + (f_base + t) * m_stride; }
  __device__ float boundary(const double* mt, uint32_t p, uint32_t l) const { return scrf_w_boundary(mt, L, p, l); }
  // the one place that prefers the formed weights to the scores
  __device__ float segment(uint64_t base, uint32_t d, uint32_t l) const {
    return Wu ? Wu[(base + d - 1) * L + l] : scrf_w_segment(Su, base, d, L, l);
  }
  __device__ float frame(const double* mt, uint32_t t, uint32_t p, uint32_t c) const { return scrf_w_frame(mt, Su, t, L, p, c); }
  __device__ float start(uint32_t l) const { return scrf_w_segment(Su, 0, 1, L, l); }   // frame model: start -> state(0, l)
};

// ---------------------------------------------------------------------------------------------
// The arcs of one lattice node, at the index the reference's AddArc call order gives them inside the node.  Node t < T holds
// the arcs added while visiting frame t, node T the L final arcs (index = the label).
//   segment model  t >= 1: L * L boundary arcs end(t-1, pl) -> boundary(t, lab), "for lab, for prev_lab" (:260-296); then
//                  L * nd segment arcs boundary(t-d+1, lab) | start -> end(t, lab), "for lab, for dur" (:300-325)
//   frame model    t = 0: L arcs start -> state(0, c); t >= 1: L * L arcs state(t-1, p) -> state(t, c), "for c, for p"
// States: 0 = start; segment model: node t has its L boundary states (t >= 1) from scrf_node_start_state(t), its L end states
// behind them, final = scrf_node_start_state(T); frame model: state(t, c) = L t + c + 1 (kept as end states), final = L T + 1.
// ---------------------------------------------------------------------------------------------
enum { SCRF_ARC_TERM, SCRF_ARC_BOUNDARY, SCRF_ARC_END };   // start (as source) or final (as destination) | boundary(t, l) | end(t, l)
struct ScrfArcEnd {
  int kind;
  uint32_t t, l;
};
struct ScrfArcNode {
  ScrfArcView v;
  uint32_t D, t, nb, np, nd, n_arcs;   // nb boundary arcs ahead of the segment arcs; np, nd: scrf_num_prev, scrf_node_max_dur
  int frame_model;
  const double* Mt;
  uint64_t base;    // scrf_seg_base(t)
  float final_w;
};

__device__ inline ScrfArcNode scrf_arc_node(const ScrfArcView& v, uint32_t D, uint32_t t, int frame_model, float final_w) {
  ScrfArcNode n{v, D, t, 0, 0, 0, v.L, frame_model, v.M, 0, final_w};
  if (t == v.T) return n;
  n.Mt = v.Mt(t);
  n.base = scrf_seg_base(t, D);
  n.np = scrf_num_prev(t, D);
  n.nd = scrf_node_max_dur(t, D);
  if (frame_model) { n.nb = t > 0 ? v.L * v.L : 0; n.n_arcs = t > 0 ? n.nb : v.L; }
  else { n.nb = n.np > 0 ? v.L * v.L : 0; n.n_arcs = n.nb + v.L * n.nd; }
  return n;
}

__device__ inline int32_t scrf_arc_state(const ScrfArcNode& n, const ScrfArcEnd& e, bool dst) {
  const uint32_t L = n.v.L;
  if (n.frame_model) return e.kind == SCRF_ARC_TERM ? (dst ? (int32_t)(L * n.v.T + 1) : 0) : (int32_t)(L * e.t + e.l + 1);
  if (e.kind == SCRF_ARC_TERM) return dst ? scrf_node_start_state(n.v.T, L) : 0;
  return scrf_node_start_state(e.t, L) + (int32_t)((e.kind == SCRF_ARC_END && e.t > 0) ? L : 0) + (int32_t)e.l;
}

// arc idx < n.n_arcs of the node; src / dst: its two states, for what a caller keeps per state
__device__ inline scrf_arc scrf_node_arc(const ScrfArcNode& n, uint32_t idx, ScrfArcEnd* src, ScrfArcEnd* dst) {
  const uint32_t L = n.v.L, t = n.t;
  int32_t lbl = 0;
  float w;
  if (t == n.v.T) {   // final arcs (:366-399)
    *src = ScrfArcEnd{SCRF_ARC_END, t - 1, idx}; *dst = ScrfArcEnd{SCRF_ARC_TERM, 0, 0};
    w = n.final_w;
  } else if (n.frame_model && t == 0) {
    *src = ScrfArcEnd{SCRF_ARC_TERM, 0, 0}; *dst = ScrfArcEnd{SCRF_ARC_END, 0, idx};
    lbl = (int32_t)idx + 1;
    w = n.v.start(idx);
  } else if (n.frame_model) {
    const uint32_t c = idx / L, p = idx % L;
    *src = ScrfArcEnd{SCRF_ARC_END, t - 1, p}; *dst = ScrfArcEnd{SCRF_ARC_END, t, c};
    lbl = (int32_t)c + 1;
    w = n.v.frame(n.Mt, t, p, c);
  } else if (idx < n.nb) {
    const uint32_t lab = idx / L, pl = idx % L;
    *src = ScrfArcEnd{SCRF_ARC_END, t - 1, pl}; *dst = ScrfArcEnd{SCRF_ARC_BOUNDARY, t, lab};
    w = n.v.boundary(n.Mt, pl, lab);
  } else {
    const uint32_t j = idx - n.nb, lab = j / n.nd, d = j % n.nd + 1;
    *src = d <= n.np ? ScrfArcEnd{SCRF_ARC_BOUNDARY, t - d + 1, lab} : ScrfArcEnd{SCRF_ARC_TERM, 0, 0};
    *dst = ScrfArcEnd{SCRF_ARC_END, t, lab};
    lbl = (int32_t)(lab + L * (d - 1) + 1);
    w = n.v.segment(n.base, d, lab);
  }
  return scrf_arc{scrf_arc_state(n, *src, false), lbl, lbl, w, scrf_arc_state(n, *dst, true)};
}

#endif  // SCRF_ARCW_H_
