// scrf_knobs.h -- every SCRF_* environment switch of the kernel library, in one table.  Host-only (no HIP): the engine
// reads the table once, in scrf_create, into scrf_engine_s::kn, and planners, tile builders and launchers all take that
// one struct, so they cannot disagree about a switch.  DESIGN.md "Knobs" is the same list with the kernels each touches.
#ifndef SCRF_KNOBS_H_
#define SCRF_KNOBS_H_

#include <stdint.h>
#include <stdlib.h>

// X(type, field, default, environment name, value when set (from the string e), what it switches)
#define SCRF_KNOBS(X)                                                                                                                    \
  X(int, lanes, 1, "SCRF_LANES", atoi(e) > 1 ? 2 : 1, "2: alternate chunks of a batch on two streams")                                   \
  X(bool, fuse, true, "SCRF_FUSE", atoi(e) != 0, "0: materialise the windows even where the fused kernels fit")                          \
  X(bool, side, true, "SCRF_SIDE", atoi(e) != 0, "0: no side stream (k_ztf + transition counts) under the count kernel")                 \
  X(bool, dtab, true, "SCRF_DTAB", atoi(e) != 0, "0: the score kernel builds its duration-weight table per tile")                        \
  X(bool, fuse_mixed, true, "SCRF_FUSE_MIXED", atoi(e) != 0, "0: two-stream batches keep the general path for the state part")           \
  X(bool, comm_overlap, true, "SCRF_COMM_OVERLAP", atoi(e) != 0, "0: the fused call issues both all-reduce blocks after the batch")      \
  X(bool, lindp, true, "SCRF_LINDP", atoi(e) != 0, "0: log-domain recursion instead of the scaled linear-domain one")                    \
  X(bool, stdseg_lin, true, "SCRF_STDSEG_LIN", atoi(e) != 0, "0: STDSEG trains on the reference-order kernels under every precision")    \
  X(bool, postocc_split, true, "SCRF_POSTOCC_SPLIT", atoi(e) != 0, "0: k_post_occ walks every utterance in one piece")                   \
  X(bool, fast_decode, true, "SCRF_FAST_DECODE", atoi(e) != 0, "0: decode through the reference-order score kernel only")                \
  X(bool, align_wave, true, "SCRF_ALIGN_WAVE", atoi(e) != 0, "0: every alignment chunk through the workgroup kernel")                    \
  X(int, batch_pool, 1, "SCRF_BATCH_POOL", atoi(e), "0: hipMalloc / hipFree per batch; 2: pool on, uploads on the engine stream")        \
  X(int, hybrid, 1, "SCRF_HYBRID", atoi(e), "0: no hybrid path; 2: L > 64 takes it even where the fused kernels fit")                    \
  X(double, decode_bound_scale, 1.0, "SCRF_DECODE_BOUND_SCALE", atof(e) > 1.0 ? atof(e) : 1.0, "widens the fast decode's screen (>= 1)") \
  X(bool, postz_split, true, "SCRF_POSTZ_SPLIT", atoi(e) != 0, "0: k_post_z never splits an utterance's walk into frame segments")       \
  X(bool, expf_dma, true, "SCRF_EXPF_DMA", atoi(e) != 0, "0: the count kernel stages its R tiles through registers")                     \
  X(bool, expf_big, false, "SCRF_EXPF_BIG", atoi(e) != 0, "100-row count tiles where they fit; unset: only with SCRF_SIDE=0")            \
  X(bool, expf_ws, true, "SCRF_EXPF_WS", atoi(e) != 0, "0: the single-role count kernel instead of the wave-specialised one")            \
  X(uint32_t, expf_blocks, 512u, "SCRF_EXPF_BLOCKS", (uint32_t)atoi(e), "persistent workgroups of the count kernel (<= 512)")            \
  X(bool, dplin_ereg, true, "SCRF_DPLIN_EREG", atoi(e) != 0, "0: k_dp_lin_mw reads the transition column from L2 every frame")           \
  X(bool, dplin_tail, true, "SCRF_DPLIN_TAIL", atoi(e) != 0, "0: L > 128 at D > 25 keeps no transition rows in registers")               \
  X(int, dplin_mv, -1, "SCRF_DPLIN_MV", atoi(e) != 0 ? 1 : 0, "k_dp_lin_mv: 0 never, nonzero always; unset: by sweeps per CU")           \
  X(int, dplin_mv_sweeps, 3, "SCRF_DPLIN_MV_SWEEPS", atoi(e), "sweeps per CU below which k_dp_lin_mv is chosen")                         \
  X(bool, scores_mfma_ws, true, "SCRF_SCORES_MFMA_WS", atoi(e) != 0, "0: single-role k_scores_mfma from 192 features on too")            \
  X(bool, expf_db, true, "SCRF_EXPF_DB", atoi(e) != 0, "0: the 8-wave k_expf_mfma keeps one image pair in LDS")                          \
  X(bool, expf_mfma_ws, true, "SCRF_EXPF_MFMA_WS", atoi(e) != 0, "0: single-role k_expf_mfma where the role split applies")              \
  X(bool, expm_tile, true, "SCRF_EXPM_TILE", atoi(e) != 0, "0: k_exp_m without the tiled form for L <= 64")                              \
  X(bool, viterbi_vec, true, "SCRF_VITERBI_VEC", atoi(e) != 0, "0: k_viterbi_fast without the 16-byte cost reads (L % 4 == 0)")          \
  X(int, trans_chunks, 0, "SCRF_TRANS_CHUNKS", atoi(e), "row chunks of the per-frame transition contraction (0: not forced)")            \
  X(bool, rtab, true, "SCRF_RTAB", atoi(e) != 0, "0: the score kernel derives its row records per tile")                                 \
  X(bool, scores_dma, true, "SCRF_SCORES_DMA", atoi(e) != 0, "0: the score kernel stages tables, frames and P through registers")        \
  X(int, fbw_waves, 0, "SCRF_FBW_WAVES", atoi(e), "wavefronts per workgroup of k_fb_segtrans_w (0 / out of range: by batch size)")       \
  X(double, comm_timeout_s, 300.0, "SCRF_COMM_TIMEOUT_S", atof(e) > 0 ? atof(e) : 300.0,                                                 \
    "seconds a collective may wait; operational, so wait_collective reads it at every wait, not from this struct")

struct ScrfKnobs {
#define X(T, f, d, name, parse, doc) T f = d;
  SCRF_KNOBS(X)
#undef X
  bool pool_on() const { return batch_pool != 0; }
  bool pool_up() const { return batch_pool != 2; }   // uploads on their own stream
  bool hybrid_on() const { return hybrid != 0; }
  bool hybrid_first() const { return hybrid == 2; }
};

struct ScrfKnobDoc { const char *name, *dflt, *doc; };
static const ScrfKnobDoc scrf_knob_docs[] = {
#define X(T, f, d, name, parse, doc) {name, #d, doc},
    SCRF_KNOBS(X)
#undef X
};

inline ScrfKnobs scrf_knobs_read(const char* (*get)(const char*)) {
  ScrfKnobs k;
#define X(T, f, d, name, parse, doc) if (const char* e = get(name)) k.f = (parse);
  SCRF_KNOBS(X)
#undef X
  if (!get("SCRF_EXPF_BIG")) k.expf_big = !k.side;   // tall tiles by default only when the side stream is off
  return k;
}
inline const char* scrf_env(const char* name) { return getenv(name); }   // what scrf_create passes to scrf_knobs_read

#endif  // SCRF_KNOBS_H_
