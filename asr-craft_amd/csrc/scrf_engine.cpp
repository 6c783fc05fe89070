// scrf_engine.cpp -- host side of libscrf_amd.so: the C ABI of include/scrf_abi.h on top of
// the HIP kernels.  One engine = one GPU, one HIP stream; batches live in HBM; scratch is a
// single device arena carved per chunk of utterances.  There is NO CPU compute path here:
// without a HIP device scrf_create fails with SCRF_ERR_NO_DEVICE.
#include <dlfcn.h>
#include <time.h>
#include <unistd.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <functional>
#include <string>
#include <unordered_map>
#include <vector>

#include "scrf_kernels.h"
#include "scrf_own.h"
#include "scrf_softnum.h"

// ---------------------------------------------------------------------------------------------
// RCCL, bound lazily (so that loading the library never drags a second RCCL into a process
// that already has one, e.g. under torch.distributed)
// ---------------------------------------------------------------------------------------------
typedef struct { char internal[128]; } scrf_nccl_uid;
typedef void* scrf_nccl_comm;
struct RcclApi {
  void* lib = nullptr;
  int (*GetUniqueId)(scrf_nccl_uid*) = nullptr;
  int (*CommInitRank)(scrf_nccl_comm*, int, scrf_nccl_uid, int) = nullptr;
  int (*AllReduce)(const void*, void*, size_t, int, int, scrf_nccl_comm, hipStream_t) = nullptr;
  int (*CommDestroy)(scrf_nccl_comm) = nullptr;
  int (*GroupStart)() = nullptr;
  int (*GroupEnd)() = nullptr;
  int (*CommAbort)(scrf_nccl_comm) = nullptr;
  int (*CommGetAsyncError)(scrf_nccl_comm, int*) = nullptr;
  const char* (*GetErrorString)(int) = nullptr;
};
static RcclApi g_rccl;
static bool rccl_load(std::string* why) {
  if (g_rccl.lib) return true;
  const char* names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
  for (const char* n : names) {
    g_rccl.lib = dlopen(n, RTLD_NOW | RTLD_GLOBAL);
    if (g_rccl.lib) break;
  }
  if (!g_rccl.lib) {
    *why = std::string("cannot load RCCL: ") + dlerror();
    return false;
  }
  g_rccl.GetUniqueId = (int (*)(scrf_nccl_uid*))dlsym(g_rccl.lib, "ncclGetUniqueId");
  g_rccl.CommInitRank = (int (*)(scrf_nccl_comm*, int, scrf_nccl_uid, int))dlsym(g_rccl.lib, "ncclCommInitRank");
  g_rccl.AllReduce = (int (*)(const void*, void*, size_t, int, int, scrf_nccl_comm, hipStream_t))dlsym(g_rccl.lib, "ncclAllReduce");
  g_rccl.CommDestroy = (int (*)(scrf_nccl_comm))dlsym(g_rccl.lib, "ncclCommDestroy");
  g_rccl.GroupStart = (int (*)())dlsym(g_rccl.lib, "ncclGroupStart");
  g_rccl.GroupEnd = (int (*)())dlsym(g_rccl.lib, "ncclGroupEnd");
  g_rccl.CommAbort = (int (*)(scrf_nccl_comm))dlsym(g_rccl.lib, "ncclCommAbort");
  g_rccl.CommGetAsyncError = (int (*)(scrf_nccl_comm, int*))dlsym(g_rccl.lib, "ncclCommGetAsyncError");
  g_rccl.GetErrorString = (const char* (*)(int))dlsym(g_rccl.lib, "ncclGetErrorString");
  if (!g_rccl.GetUniqueId || !g_rccl.CommInitRank || !g_rccl.AllReduce) {
    *why = "RCCL symbols missing";
    return false;
  }
  return true;
}
enum { SCRF_NCCL_DOUBLE = 8, SCRF_NCCL_SUM = 0 };  // ncclFloat64, ncclSum (rccl.h)

// ---------------------------------------------------------------------------------------------
// What the handle owns (scrf_own.h).  These types, like the owning ones, lie in namespace scrf_eng: whatever of them the
// library exports carries that name.
namespace scrf_eng {

// Batch arrays (scrf_batch_create / scrf_batch_destroy) come from a pool and are uploaded on a stream of their own:
// a trainer that makes one batch per minibatch used to synchronise the device at every destroy (hipFree) and to wait
// for the previous minibatch's kernels at every upload.  A freed block carries the epoch of its destroy call; the
// engine stream's event of that epoch says when the last kernel that could read it has finished, and only then is the
// block handed out again (otherwise a fresh one is allocated).  SCRF_BATCH_POOL=0: hipMalloc / hipFree as before.
struct BatchPool {
  struct Block { void* p; size_t cap; uint64_t epoch; };
  std::vector<Block> free;
  std::unordered_map<void*, size_t> live;    // blocks held by batches
  Stream up_stream;
  Event ev[8];
  uint64_t epoch = 0, done = 0;              // destroy calls so far / epochs known to be finished
  size_t bytes = 0;                          // bytes sitting in `free`
  BatchPool() = default;
  BatchPool(const BatchPool&) = delete;
  BatchPool& operator=(const BatchPool&) = delete;
  ~BatchPool() {   // (scrf_destroy has drained the streams)
    for (auto& bl : free) hipFree(bl.p);
    for (auto& kv : live) hipFree(kv.first);
  }
};

// The per-feature state of the handle: each struct owns its buffers and its counters.
// k_tile_tables: row records / row bases / rowmap of a steady-state score tile.  The tables depend on (D, TB, la) alone:
// launched when that key changes or the buffer moves, on `stream`; a call on another stream waits for `ev`
struct TileTables {
  DevArray<char> tab;
  uint32_t key[3] = {0, 0, 0};
  bool valid = false;
  hipStream_t stream = nullptr;
  Event ev;
};

// result buffers of scrf_viterbi_batch and scrf_align_batch, kept across calls (a hipMalloc / hipFree pair per call is a
// device-wide synchronisation each) and their pinned host images (the labels come back in one asynchronous copy)
struct DecodeOut {
  DevArray<uint32_t> lab, n;      // [sum T], [U]
  DevArray<float> cost;           // [U]
  PinnedArray<uint32_t> hlab, hn;
  PinnedArray<float> hcost;
  uint64_t n_fix = 0, n_fallback = 0;   // entries recomputed / chunks sent back to the EXACT path
  hipError_t reserve(size_t n_frames, size_t n_utts) {   // room for the results of one batch
    hipError_t e = lab.reserve(n_frames);
    if (e == hipSuccess) e = hlab.reserve(n_frames);
    if (e == hipSuccess) e = n.reserve(n_utts);
    if (e == hipSuccess) e = cost.reserve(n_utts);
    if (e == hipSuccess) e = hn.reserve(n_utts);
    if (e == hipSuccess) e = hcost.reserve(n_utts);
    return e;
  }
};

// result of scrf_lattice_prune_batch: the kept arcs of the whole batch, back to back, outside the scratch
// budget; grows geometrically, kept across calls.  One result, tied to the batch and the weights it was computed from
struct PrunedLattice {
  DevArray<scrf_arc> arcs;
  DevArray<char> meta;          // best [U] doubles | utterance offsets [U + 1]
  scrf_batch batch = nullptr;   // the batch of the valid result, or nullptr
  std::vector<uint64_t> off;    // [U + 1] host image of the offsets
  uint64_t n_calls = 0, n_chunks = 0;
};

// result of scrf_nbest_batch: the labels of every hypothesis of the batch back to back, where each
// hypothesis's labels start and its cost, sized by what the searches found; outside the scratch budget, grows geometrically,
// kept across calls.  One result, tied to the batch and the weights, as the pruned lattice is
struct NBestResult {
  DevArray<uint32_t> lab;       // [labels of all hypotheses]
  DevArray<uint64_t> lab_off;   // [hypotheses + 1]
  DevArray<float> cost;         // [hypotheses]
  DevArray<uint64_t> hyp_off;   // [U + 1] hypotheses before each utterance
  scrf_batch batch = nullptr;   // the batch of the valid result, or nullptr
  std::vector<uint64_t> off;    // [U + 1] host image of hyp_off
  uint64_t n_labels = 0;
  uint64_t n_calls = 0, n_chunks = 0, n_fast_chunks = 0;
};

// scrf_align_batch: the transcripts of the call on the device (phones | phone_off, back-pointer offsets),
// kept across calls; bp_off is the host image chunk_layout sizes a chunk's back pointers with.
// scrf_transcript_batch: the transcripts go into ph / off as well; inv holds each transcript's positions
// sorted by label and where each label's start (inv_pos [sum K] | inv_off [U][L + 1]); cell_off is the host image
// chunk_layout sizes a chunk's forward / backward cells with
struct Transcripts {
  DevArray<uint32_t> ph, inv;
  DevArray<uint64_t> off;
  std::vector<uint64_t> bp_off, cell_off;
  std::vector<uint32_t> inv_h;
  uint64_t n_al_calls = 0, n_al_chunks = 0, n_al_wave = 0, n_al_group = 0;   // calls; searches launched, and by which kernel
  uint64_t n_tr_calls = 0, n_tr_chunks = 0, n_tr_redone = 0;   // calls; chunks swept (both passes of a redone call); calls redone
};

// scrf_fb_transcript_batch: the transcripts go into tx as scrf_transcript_batch's do.  bad: label arrays that
// are all SCRF_LAB_BAD, sized to the largest batch seen -- the training kernels read them where a labelled batch has its
// labels, and so form the free expectation alone.  log_num [U]: A of every utterance.  ph_off: the host image of phone_off
// chunk_layout sizes a chunk's per-position sums with.
struct SoftGrad {
  DevArray<uint32_t> bad;
  DevArray<double> log_num;
  std::vector<uint64_t> ph_off;
  uint64_t n_calls = 0, n_chunks = 0, n_redone = 0;   // calls; chunks run (both passes of a redone call); calls redone
};

// HIP-event times of the last timed call: per phase (scrf_last_timing) and per kernel (scrf_kernel_timing)
struct KTime { std::string name; double ms; uint32_t n; };
struct Timing {
  bool on = false;
  std::vector<KTime> ktimes;
  Event kev[2];
  Event ev[SCRF_N_PHASES + 1][2];
  float ms[SCRF_N_PHASES] = {};
  uint32_t nlaunch[SCRF_N_PHASES] = {};
};

}  // namespace scrf_eng
using namespace scrf_eng;

// Everything the handle holds of the device is a member of an owning type: a new buffer is one member, reserved where it is
// first needed, and scrf_destroy never hears of it.  Who waits for what before a buffer of the handle is dropped for a larger
// one (DevArray::reserve itself waits for nothing):
//   ensure_scratch                               both streams
//   reserve_drained (post_buf, lp.meta, tx.*, nb.hyp_off)   the engine stream
//   dec.*, rtab.tab, d_pack                      nothing
struct __attribute__((visibility("hidden"))) scrf_engine_s {   // (hidden: its constructor and destructor are not for export)
  scrf_config cfg;
  ScrfKnobs kn;   // the SCRF_* environment switches as scrf_create found them (scrf_knobs.h, DESIGN.md "Knobs")
  ScrfLayout lay;
  // K states per label on a segmental model (nodes/CRF_StdSegNStateNode_WithoutDurLab_WithoutSegTransFtr.cpp): the
  // kernels run the dense one-state layout `lay` with the bias of every transition the topology lacks pinned at
  // log 0 (mask_w); the callers see the reference's compact layout `xlay` (CRF_StdFeatureMap.cpp:293-312), and every
  // weight-length vector crossing the ABI is scattered / gathered through s2d (compact index -> dense index)
  bool shadow = false;
  ScrfLayout xlay;
  std::vector<uint32_t> s2d, masked;
  double mask_w = 0.0;
  std::vector<double> xbuf;
  int device = 0;
  Stream stream;              // the engine's own, or the caller's (scrf_set_stream)
  DevArray<double> d_lambda, d_lambda_acc, d_gsa;
  DevArray<double> d_grad;    // the engine's own, or the caller's (scrf_set_grad_buffer)
  DevArray<double> d_m0;      // [L*L] time-invariant transition scores (bias-only transitions)
  DevArray<double> d_e0, d_et0, d_msh0;   // exp(M0 - shift), its transpose and the shift (linear-domain DP)
  bool m0_valid = false;
  DevArray<double> d_sums;    // {numer, zx, n_utts, active}
  // a batch's gradient and sums are built in a staging buffer and committed to d_grad / d_sums by a kernel
  // that is a no-op when an utterance of the batch failed (d_latch): a failed scrf_fb_batch leaves the
  // gradient as it was, and a NUMERIC failure of the linear-domain recursion can be redone in the log domain
  DevArray<double> d_stage;
  // sparse maps (scrf_sparse.hip): lambda re-laid index-major per call, [0] state block, [1] transition block
  DevArray<double> d_lamT[2];
  DevArray<double> d_sums_stage;
  DevArray<int> d_latch;      // {status code, utterance} of the first failed utterance of the batch in flight
  PinnedArray<int> h_latch;   // pinned copy, valid once ev_status has completed
  PinnedArray<double> h_sums; // pinned image of the batch sums (scrf_queue_batch_sums / scrf_take_batch_sums)
  Event ev_sums;
  bool sums_queued = false;
  Event ev_status;
  uint64_t n_lin_fallback = 0;   // batches redone through the log-domain recursion
  // second lane: alternate chunks of a batch run on a second stream so that the VALU-bound DP
  // kernels of one chunk overlap the MFMA-bound contractions of the other
  Stream stream2;
  DevArray<char> scratch[2];  // the scratch arena of each lane (ensure_scratch)
  DevArray<double> d_grad2, d_sums2;
  Event ev_fork, ev_join;
  BatchPool pool;
  // all-reduce / compute overlap (scrf_fb_batch_allreduce): inside the fused call the transition
  // contraction runs first and the all-reduce of the transition weights (98.7 % of the TIMIT-demo gradient) is issued on
  // the second stream as soon as they are committed, under the state contraction
  bool overlap_comm = false;  // set for the duration of a scrf_fb_batch_allreduce call
  bool early_done = false;    // the transition block of this step has been all-reduced already
  uint64_t n_collectives = 0, n_overlapped = 0;   // scrf_comm_stats
  DevArray<double> d_pack;    // [L * nsf + 8]: the state weights of every label + the 8 scalars, one small message
  TileTables rtab;
  DevArray<double> d_dtab;      // k_dur_table: duration weight + bias per output block, for the fused score kernel
  DevArray<double> d_sl_tab;    // STDSEG, bias-only transitions: E, E^T (nLabs^2 each) and max M (scrf_stdseg_lin.hip)
  bool frame_mass = false;   // posterior-mass self-checks with the frame model's bounds (scrf_set_frame_mass_check)
  uint64_t n_post_split = 0, n_post_whole = 0;   // k_post_occ launches in frame segments / in one piece (scrf_posterior_stats)
  // the workgroup-per-utterance log-domain recursion (k_fb: column-wise max-shifted log-sum-exp, the
  // reference's LogMath) instead of the wavefront kernels, whose transition step works on exp(M - max M):
  // set for the automatic redo of a batch / hook call that raised SCRF_ERR_NUMERIC there
  bool force_fb = false;
  // decode from the fused score kernel's float arc weights + reference-order fix-ups (bit-identical
  // to the EXACT path by a rounding-error bound, ScrfDecodeOut; kn.fast_decode)
  DevArray<double> d_w1;
  DecodeOut dec;
  // result arrays of scrf_posteriors_batch (whole batch: chunking stays invisible), kept across calls like the decode buffers
  DevArray<char> post_buf;
  PrunedLattice lp;
  NBestResult nb;
  Transcripts tx;
  SoftGrad soft;
  std::string err;
  Timing tm;
  scrf_nccl_comm comm = nullptr;
  int rank = 0, nranks = 1;
};

struct scrf_batch_s {
  uint32_t U = 0;
  int mode = 0;  // 0 = windows resident, 1 = frames + recipe
  std::vector<uint32_t> T;
  std::vector<uint64_t> frame_off, seg_off, arc_off;
  // every device array below is a view into one of these blocks of the engine's pool (upload); they are what the batch owns
  std::vector<void*> blocks;
  uint32_t* d_T = nullptr;
  uint64_t* d_frame_off = nullptr;
  uint64_t* d_seg_off = nullptr;
  uint64_t* d_arc_off = nullptr;
  uint32_t* d_labels = nullptr;
  uint32_t* d_next_lab = nullptr;      // [sum T] label of the next labelled frame (gradbuilder :436-444)
  uint32_t* d_prev_lab = nullptr;      // [sum T] label of the nearest EARLIER labelled frame (CRF_NewGradBuilder_StdSeg.cpp, STDSEG_NO_DUR)
  uint32_t* d_trans_counts = nullptr;  // [L*L] observed (c -> n) transitions of the whole batch
  uint32_t* d_frame_u = nullptr;       // [sum T] utterance of each frame
  float* d_xm_f = nullptr;             // [sum T] max(|x|, 1, |state bias value|) over the frame's utterance (fused path)
  float* d_windows = nullptr;
  uint32_t n_streams = 0;
  scrf_stream_recipe recipe[SCRF_MAX_STREAMS];
  uint32_t width[SCRF_MAX_STREAMS];
  float* d_frames[SCRF_MAX_STREAMS] = {nullptr, nullptr, nullptr};
  uint64_t* d_sframe_off[SCRF_MAX_STREAMS] = {nullptr, nullptr, nullptr};
  double* d_numer = nullptr;
  double* d_zx = nullptr;
  int* d_status = nullptr;
  // fused window synthesis: row tiles of the score kernel [0] and of the expected-count kernel [1]
  bool fused_ok = false;
  bool hybrid_ok = false;   // one segment-recipe stream the fused kernels do not take (L > 64): sampled blocks through P / Z, dense statistics materialised
  bool mixed = false;   // fused state part (stream 0) + materialised transition-feature streams (config 3's shape)
  std::vector<uint64_t> tile_off[3];   // 0: score tiles, 1: expected-count tiles (<= 76 rows), 2: <= 100 rows (FASTLIN)
  ScrfTileDesc* d_tiles[3] = {nullptr, nullptr, nullptr};
  ScrfBatchView view() const {
    ScrfBatchView v;
    v.U = U; v.T = d_T; v.frame_off = d_frame_off; v.seg_off = d_seg_off; v.arc_off = d_arc_off;
    v.labels = d_labels;
    return v;
  }
};

static std::string g_create_err;

static int fail(scrf_handle h, int code, const char* fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  if (h) h->err = buf; else g_create_err = buf;
  return code;
}

#define HIPCHK(h, call)                                                                   \
  do {                                                                                    \
    hipError_t e_ = (call);                                                               \
    if (e_ != hipSuccess)                                                                 \
      return fail(h, SCRF_ERR_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), \
                  __FILE__, __LINE__);                                                    \
  } while (0)
// the same for a call that returns one of the engine's own codes (it has set the error text)
#define RCCHK(...)                     \
  do {                                 \
    int rc_ = (__VA_ARGS__);           \
    if (rc_ != SCRF_OK) return rc_;    \
  } while (0)

static uint32_t window_width(const scrf_stream_recipe& r, uint32_t D) {
  // io/CRF_InFtrStream_SeqMultiWindow.cpp:50-125
  if (D == 1) return (r.left_ctx + 1 + r.right_ctx) * r.in_width;
  if (r.extract_seg_ftr) return 8 * r.in_width + D + (r.left_ctx + r.right_ctx) * r.in_width;
  return (r.left_ctx + 1 + r.right_ctx) * r.in_width;
}

static int build_layout(const scrf_config& c, ScrfLayout* l, std::string* why) {
  if (c.abi_version != SCRF_ABI_VERSION) { *why = "abi_version mismatch"; return SCRF_ERR_INVALID; }
  if (c.num_states == 0) { *why = "num_states must be >= 1"; return SCRF_ERR_INVALID; }
  if (c.num_states > 1 && c.model_type != SCRF_STDFRAME && c.model_type != SCRF_STDSEG_NO_DUR_NO_TRANSFTR && c.model_type != SCRF_STDSEG_NO_DUR_NO_SEGTRANSFTR) {
    // nodes/CRF_StateNode.cpp:496-507: "CRF_StdSegNStateNode has not been implemented yet"
    *why = "crf_states > 1: CRF_StdSegNStateNode / CRF_StdSegNStateNode_WithoutDurLab have not been implemented (the reference has stdframe and stdseg_no_dur_no_segtransftr n-state nodes only)";
    return SCRF_ERR_INVALID;
  }
  if (c.num_states > 1 && c.model_type != SCRF_STDFRAME && (!c.use_trans_bias || !(c.trans_bias_val > 0.0f))) {
    *why = "crf_states > 1 on a segmental model needs the transition bias (crf_use_trans_bias, a positive bias value): the topology is held by it";
    return SCRF_ERR_INVALID;
  }
  if (c.num_states > 1 && c.num_labs % c.num_states != 0) { *why = "Invalid state/label combination while computing transitions"; return SCRF_ERR_INVALID; }  // CRF_StdFeatureMap.cpp:476-479
  if (c.num_labs == 0 || c.lab_max_dur == 0 || c.num_feas == 0) { *why = "num_labs, lab_max_dur, num_feas must be > 0"; return SCRF_ERR_INVALID; }
  if (c.model_type == SCRF_STDSEG && c.num_labs % c.lab_max_dur != 0) { *why = "stdseg: the number of all labels and the maximum duration of labels do not correspond (nLabs = nActualLabs * labMaxDur)"; return SCRF_ERR_INVALID; }
  if (c.model_type > SCRF_STDSEG_NO_DUR_NO_SEGTRANSFTR) { *why = "unknown model_type"; return SCRF_ERR_INVALID; }
  if (c.model_type == SCRF_STDFRAME && c.lab_max_dur != 1) { *why = "the maximum duration of labels must be 1 for \"stdframe\" CRF model."; return SCRF_ERR_INVALID; }  // CRFTrain/src/Main.cpp:574-578
  if (c.map_type > SCRF_STDSPARSETRANS) { *why = "unknown map_type"; return SCRF_ERR_INVALID; }
  const bool sparse = c.map_type == SCRF_STDSPARSE || c.map_type == SCRF_STDSPARSETRANS;
  if (sparse) {   // CRF_StdSparseFeatureMap: the frame model and the TIMIT-demo model, one state per label
    if (c.model_type == SCRF_STDSEG_NO_DUR_NO_TRANSFTR) { *why = "crf_featuremap must be \"stdstate\" for \"stdseg_no_dur_no_transftr\" CRF model."; return SCRF_ERR_INVALID; }
    if (c.model_type == SCRF_STDSEG) { *why = "sparse feature maps (stdsparse/stdsparsetrans) are not built for the \"stdseg\" CRF model; use \"stdframe\" or \"stdseg_no_dur_no_segtransftr\""; return SCRF_ERR_INVALID; }
    if (c.model_type == SCRF_STDSEG_NO_DUR) { *why = "sparse feature maps (stdsparse/stdsparsetrans) are not built for the \"stdseg_no_dur\" CRF model; use \"stdframe\" or \"stdseg_no_dur_no_segtransftr\""; return SCRF_ERR_INVALID; }
    if (c.num_states != 1) { *why = "sparse feature maps (stdsparse/stdsparsetrans) are built for crf_states = 1 only"; return SCRF_ERR_INVALID; }
    if (c.num_feas % 2) { *why = "a sparse feature map reads (index, value) pairs: num_feas must be even (the reference reads past the window otherwise)"; return SCRF_ERR_INVALID; }
    if ((c.use_state_ftrs && c.state_fidx_start != 0) || (c.use_trans_ftrs && c.trans_fidx_start != 0)) {
      *why = "a sparse feature map needs feature index start 0: the reference adds the index to the label's block without subtracting the start, so another start reads outside the label's weights";
      return SCRF_ERR_INVALID;
    }
  }
  if (c.model_type == SCRF_STDSEG_NO_DUR_NO_TRANSFTR && (c.map_type != SCRF_STDSTATE || c.use_trans_ftrs)) {   // CRFTrain/src/Main.cpp:465-468
    *why = "crf_featuremap must be \"stdstate\" for \"stdseg_no_dur_no_transftr\" CRF model.";
    return SCRF_ERR_INVALID;
  }
  if (c.num_labs > 1024) { *why = "num_labs > 1024 unsupported"; return SCRF_ERR_INVALID; }
  memset(l, 0, sizeof(*l));
  l->L = c.num_labs; l->D = c.lab_max_dur; l->F = c.num_feas;
  l->use_sf = c.use_state_ftrs != 0; l->use_tf = c.use_trans_ftrs != 0;
  l->use_sb = c.use_state_bias != 0; l->use_tb = c.use_trans_bias != 0;
  l->sfs = c.state_fidx_start; l->sfe = c.state_fidx_end; l->tfs = c.trans_fidx_start; l->tfe = c.trans_fidx_end;
  l->sbv = c.state_bias_val; l->tbv = c.trans_bias_val;
  if (sparse) {
    // the ranges bound the pair INDEX; the biases are added unscaled (CRF_StdSparseFeatureMap.cpp:74-79, :113-118)
    l->sbv = l->tbv = 1.0;
    if (l->use_sf && l->sfe >= 0x3fffffffu) { *why = "state feature index range too large"; return SCRF_ERR_INVALID; }
    if (l->use_tf && l->tfe >= 0x3fffffffu) { *why = "transition feature index range too large"; return SCRF_ERR_INVALID; }
  } else if (l->use_sf && (l->sfe < l->sfs || l->sfe >= l->F)) { *why = "state feature range outside the window vector"; return SCRF_ERR_INVALID; }
  if (!sparse && l->use_tf && (l->tfe < l->tfs || l->tfe >= l->F)) { *why = "transition feature range outside the window vector"; return SCRF_ERR_INVALID; }
  l->nsfe = l->use_sf ? l->sfe - l->sfs + 1 : 0;
  l->ntfe = l->use_tf ? l->tfe - l->tfs + 1 : 0;
  l->nsf = l->nsfe + (l->use_sb ? 1 : 0);
  l->ntf = l->ntfe + (l->use_tb ? 1 : 0);
  l->stride = l->nsf + l->L * l->ntf;
  l->K = c.num_states;
  uint64_t ll = (uint64_t)l->L * l->stride;
  if (l->K > 1) {   // :480-485: end->start + self + next-state transitions
    const uint64_t P = l->L / l->K;
    ll = (uint64_t)l->L * l->nsf + (P * P + 2 * (uint64_t)l->L - P) * l->ntf;
  }
  if (ll == 0 || ll > 0xfffffff0ull) { *why = "lambda_len out of range"; return SCRF_ERR_INVALID; }
  l->lambda_len = (uint32_t)ll;
  return SCRF_OK;
}

// ---------------------------------------------------------------------------------------------
// lifetime
// ---------------------------------------------------------------------------------------------
extern "C" int scrf_create(const scrf_config* cfg, scrf_handle* out) {
  if (!cfg || !out) return fail(nullptr, SCRF_ERR_INVALID, "scrf_create: null argument");
  *out = nullptr;
  ScrfLayout lay;
  std::string why;
  int rc = build_layout(*cfg, &lay, &why);
  if (rc != SCRF_OK) return fail(nullptr, rc, "scrf_create: %s", why.c_str());
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev <= 0)
    return fail(nullptr, SCRF_ERR_NO_DEVICE, "scrf_create: no HIP device (%s); this library has no CPU path",
                e != hipSuccess ? hipGetErrorString(e) : "device count 0");
  if (cfg->device_id < 0 || cfg->device_id >= ndev)
    return fail(nullptr, SCRF_ERR_INVALID, "scrf_create: device_id %d out of range [0,%d)", cfg->device_id, ndev);
  scrf_handle h = new scrf_engine_s();
  h->cfg = *cfg;
  h->lay = lay;
  h->xlay = lay;
  if (lay.K > 1 && cfg->model_type != SCRF_STDFRAME) {
    const uint64_t dense = (uint64_t)lay.L * lay.stride;
    if (dense > 0xfffffff0ull) { delete h; return fail(nullptr, SCRF_ERR_INVALID, "scrf_create: lambda_len out of range"); }
    h->shadow = true;
    h->lay.K = 1;
    h->lay.lambda_len = (uint32_t)dense;
    lay = h->lay;
    h->mask_w = -1e30 / (double)cfg->trans_bias_val;
    h->s2d.assign(h->xlay.lambda_len, 0);
    for (uint32_t c = 0; c < lay.L; c++) {
      for (uint32_t f = 0; f < lay.nsf; f++) h->s2d[h->xlay.state_idx_k(c) + f] = lay.state_idx(c) + f;
      for (uint32_t p = 0; p < lay.L; p++) {
        const uint32_t x = h->xlay.trans_idx_k(p, c);
        if (x == 0xffffffffu) h->masked.push_back(lay.trans_idx(p, c) + lay.ntf - 1);   // the bias is the last transition function
        else for (uint32_t f = 0; f < lay.ntf; f++) h->s2d[x + f] = lay.trans_idx(p, c) + f;
      }
    }
  }
  h->device = cfg->device_id;
  if (h->cfg.scratch_bytes == 0) h->cfg.scratch_bytes = 8ull << 30;
  h->kn = scrf_knobs_read(scrf_env);
  // a failing call leaves through scrf_destroy, like a finished engine: what was made before it is given back
#define CRCHK(call)                                                                          \
  do {                                                                                       \
    hipError_t e_ = (call);                                                                  \
    if (e_ != hipSuccess) {                                                                  \
      fail(nullptr, SCRF_ERR_HIP, "scrf_create: %s failed: %s", #call, hipGetErrorString(e_)); \
      scrf_destroy(h);                                                                       \
      return SCRF_ERR_HIP;                                                                   \
    }                                                                                        \
  } while (0)
  CRCHK(hipSetDevice(h->device));
  CRCHK(h->stream.create(hipStreamNonBlocking));
  const size_t n_lam = lay.lambda_len, LL = (size_t)lay.L * lay.L, nb = sizeof(double) * n_lam;
  CRCHK(h->d_lambda.reserve(n_lam));
  CRCHK(h->d_lambda_acc.reserve(n_lam));
  CRCHK(h->d_gsa.reserve(n_lam));
  CRCHK(h->d_grad.reserve(n_lam));
  CRCHK(h->d_m0.reserve(LL));
  CRCHK(h->d_w1.reserve(lay.L));
  if (lay.D <= 40) CRCHK(h->d_dtab.reserve(fused_dur_table_doubles(fused_shape(lay))));
  if (cfg->map_type >= SCRF_STDSPARSE) {
    CRCHK(h->d_lamT[0].reserve(((size_t)lay.nsfe + lay.use_sb) * lay.L));
    CRCHK(h->d_lamT[1].reserve(((size_t)lay.ntfe + lay.use_tb) * LL));
  }
  if (cfg->model_type == SCRF_STDSEG && !lay.use_tf) CRCHK(h->d_sl_tab.reserve(2 * LL + 8));
  CRCHK(h->d_e0.reserve(LL));
  CRCHK(h->d_et0.reserve(LL));
  CRCHK(h->d_msh0.reserve(1));
  CRCHK(h->d_sums.reserve(8));
  CRCHK(h->d_stage.reserve(n_lam));
  CRCHK(h->d_sums_stage.reserve(4));
  CRCHK(h->d_latch.reserve(2));
  CRCHK(h->h_latch.reserve(2));
  h->h_latch[0] = h->h_latch[1] = 0;
  CRCHK(h->h_sums.reserve(4));
  CRCHK(h->ev_sums.create(hipEventDisableTiming));
  CRCHK(h->ev_status.create(hipEventDisableTiming));
  CRCHK(h->tm.kev[0].create());
  CRCHK(h->tm.kev[1].create());
  CRCHK(h->d_grad2.reserve(n_lam));
  CRCHK(h->d_sums2.reserve(4));
  CRCHK(h->stream2.create(hipStreamNonBlocking));
  CRCHK(h->pool.up_stream.create(hipStreamNonBlocking));
  CRCHK(h->ev_fork.create(hipEventDisableTiming));
  CRCHK(h->ev_join.create(hipEventDisableTiming));
  CRCHK(h->rtab.ev.create(hipEventDisableTiming));
  CRCHK(hipMemsetAsync(h->d_lambda, 0, nb, h->stream));
  CRCHK(hipMemsetAsync(h->d_lambda_acc, 0, nb, h->stream));
  CRCHK(hipMemsetAsync(h->d_gsa, 0, nb, h->stream));
  CRCHK(hipMemsetAsync(h->d_grad, 0, nb, h->stream));
  CRCHK(hipMemsetAsync(h->d_sums, 0, sizeof(double) * 8, h->stream));
  for (int i = 0; i <= SCRF_N_PHASES; i++) {
    CRCHK(h->tm.ev[i][0].create());
    CRCHK(h->tm.ev[i][1].create());
  }
  CRCHK(hipStreamSynchronize(h->stream));
  if (h->shadow) {
    std::vector<double> z(h->xlay.lambda_len, 0.0);
    if (scrf_set_lambda(h, z.data(), h->xlay.lambda_len) != SCRF_OK) { g_create_err = h->err; scrf_destroy(h); return SCRF_ERR_HIP; }
  }
#undef CRCHK
  *out = h;
  return SCRF_OK;
}

extern "C" int scrf_destroy(scrf_handle h) {
  if (!h) return SCRF_OK;
  hipSetDevice(h->device);
  // nothing is released while a stream may still use it; the members give back what they own (scrf_own.h)
  for (hipStream_t s : {h->stream.get(), h->stream2.get(), h->pool.up_stream.get()})
    if (s) hipStreamSynchronize(s);
  if (h->comm && g_rccl.CommDestroy) g_rccl.CommDestroy(h->comm);
  delete h;
  return SCRF_OK;
}

extern "C" const char* scrf_last_error(scrf_handle h) { return h ? h->err.c_str() : g_create_err.c_str(); }

extern "C" int scrf_set_stream(scrf_handle h, void* s) {
  if (!h) return SCRF_ERR_INVALID;
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (s) h->stream.borrow((hipStream_t)s);
  else HIPCHK(h, h->stream.create(hipStreamNonBlocking));
  return SCRF_OK;
}

extern "C" int scrf_synchronize(scrf_handle h) {
  if (!h) return SCRF_ERR_INVALID;
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream2));
  return SCRF_OK;
}

// ---------------------------------------------------------------------------------------------
// layout hooks / model state
// ---------------------------------------------------------------------------------------------
extern "C" int scrf_lambda_len(scrf_handle h, uint32_t* n) { if (!h || !n) return SCRF_ERR_INVALID; *n = h->xlay.lambda_len; return SCRF_OK; }
extern "C" int scrf_num_state_funcs(scrf_handle h, uint32_t* n) { if (!h || !n) return SCRF_ERR_INVALID; *n = h->lay.nsf; return SCRF_OK; }
extern "C" int scrf_num_trans_funcs(scrf_handle h, uint32_t* n) { if (!h || !n) return SCRF_ERR_INVALID; *n = h->lay.ntf; return SCRF_OK; }
extern "C" int scrf_state_idx(scrf_handle h, uint32_t clab, uint32_t fno, uint32_t* idx) {
  if (!h || !idx) return SCRF_ERR_INVALID;
  if (clab >= h->lay.L) return fail(h, SCRF_ERR_INVALID, "scrf_state_idx: label %u >= %u", clab, h->lay.L);
  *idx = h->xlay.state_idx_k(clab) + fno;  // getStateFeatureIdx :421-423
  return SCRF_OK;
}
extern "C" int scrf_trans_idx(scrf_handle h, uint32_t plab, uint32_t clab, uint32_t fno, uint32_t* idx) {
  if (!h || !idx) return SCRF_ERR_INVALID;
  if (clab >= h->lay.L || plab >= h->lay.L) return fail(h, SCRF_ERR_INVALID, "scrf_trans_idx: label out of range");
  {
    const uint32_t v = h->xlay.trans_idx_k(plab, clab);   // getTransFeatureIdx :435-437; 0xffffffff: no such transition (n-state topology)
    *idx = v == 0xffffffffu ? v : v + fno;
  }
  return SCRF_OK;
}

static int vec_io(scrf_handle h, double* dev, const double* in, double* out, uint32_t n, const char* what) {
  if (!h || (!in && !out)) return SCRF_ERR_INVALID;
  if (n != h->xlay.lambda_len) return fail(h, SCRF_ERR_INVALID, "%s: length %u != lambda_len %u", what, n, h->xlay.lambda_len);
  HIPCHK(h, hipSetDevice(h->device));
  if (h->shadow) {   // compact (caller) <-> dense (device)
    const uint32_t nd = h->lay.lambda_len;
    h->xbuf.assign(nd, 0.0);
    if (in) {
      for (uint32_t i = 0; i < n; i++) h->xbuf[h->s2d[i]] = in[i];
      if (dev == h->d_lambda) for (uint32_t m : h->masked) h->xbuf[m] = h->mask_w;
      HIPCHK(h, hipMemcpyAsync(dev, h->xbuf.data(), sizeof(double) * nd, hipMemcpyHostToDevice, h->stream));
      HIPCHK(h, hipStreamSynchronize(h->stream));
    } else {
      HIPCHK(h, hipMemcpyAsync(h->xbuf.data(), dev, sizeof(double) * nd, hipMemcpyDeviceToHost, h->stream));
      HIPCHK(h, hipStreamSynchronize(h->stream));
      for (uint32_t i = 0; i < n; i++) out[i] = h->xbuf[h->s2d[i]];
    }
    return SCRF_OK;
  }
  if (in) HIPCHK(h, hipMemcpyAsync(dev, in, sizeof(double) * n, hipMemcpyHostToDevice, h->stream));
  else HIPCHK(h, hipMemcpyAsync(out, dev, sizeof(double) * n, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return SCRF_OK;
}
extern "C" int scrf_set_lambda(scrf_handle h, const double* v, uint32_t n) {
  int rc = vec_io(h, h ? h->d_lambda : nullptr, v, nullptr, n, "scrf_set_lambda");
  if (rc == SCRF_OK) { h->m0_valid = false; h->lp.batch = nullptr; h->nb.batch = nullptr; }
  return rc;
}
extern "C" int scrf_get_lambda(scrf_handle h, double* v, uint32_t n) { return vec_io(h, h ? h->d_lambda : nullptr, nullptr, v, n, "scrf_get_lambda"); }
extern "C" int scrf_set_lambda_acc(scrf_handle h, const double* v, uint32_t n) { return vec_io(h, h ? h->d_lambda_acc : nullptr, v, nullptr, n, "scrf_set_lambda_acc"); }
extern "C" int scrf_get_lambda_acc(scrf_handle h, double* v, uint32_t n) { return vec_io(h, h ? h->d_lambda_acc : nullptr, nullptr, v, n, "scrf_get_lambda_acc"); }
extern "C" int scrf_set_grad_sqr_acc(scrf_handle h, const double* v, uint32_t n) { return vec_io(h, h ? h->d_gsa : nullptr, v, nullptr, n, "scrf_set_grad_sqr_acc"); }
extern "C" int scrf_get_grad_sqr_acc(scrf_handle h, double* v, uint32_t n) { return vec_io(h, h ? h->d_gsa : nullptr, nullptr, v, n, "scrf_get_grad_sqr_acc"); }
extern "C" int scrf_get_grad(scrf_handle h, double* v, uint32_t n) { return vec_io(h, h ? h->d_grad : nullptr, nullptr, v, n, "scrf_get_grad"); }

extern "C" int scrf_zero_grad(scrf_handle h) {
  if (!h) return SCRF_ERR_INVALID;
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipMemsetAsync(h->d_grad, 0, sizeof(double) * h->lay.lambda_len, h->stream));
  HIPCHK(h, hipMemsetAsync(h->d_sums, 0, sizeof(double) * 4, h->stream));
  return SCRF_OK;
}

static const char* k_shadow_devptr = "%s: with crf_states > 1 on a segmental model the device gradient is kept in the dense one-state layout; use scrf_get_grad / scrf_add_grad / scrf_allreduce_grad";
extern "C" int scrf_grad_device_ptr(scrf_handle h, void** p) {
  if (!h || !p) return SCRF_ERR_INVALID;
  if (h->shadow) return fail(h, SCRF_ERR_INVALID, k_shadow_devptr, "scrf_grad_device_ptr");
  *p = h->d_grad;
  return SCRF_OK;
}

extern "C" int scrf_set_grad_buffer(scrf_handle h, void* dptr) {
  // accumulate into caller-owned device memory (e.g. a torch tensor that torch.distributed
  // all-reduces over RCCL); NULL restores the engine's own buffer
  if (!h) return SCRF_ERR_INVALID;
  if (h->shadow) return fail(h, SCRF_ERR_INVALID, k_shadow_devptr, "scrf_set_grad_buffer");
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (dptr) {
    h->d_grad.borrow((double*)dptr, h->lay.lambda_len);
  } else if (!h->d_grad.owned()) {
    h->d_grad.reset();
    HIPCHK(h, h->d_grad.reserve(h->lay.lambda_len));
    HIPCHK(h, hipMemsetAsync(h->d_grad, 0, sizeof(double) * h->lay.lambda_len, h->stream));
  }
  return SCRF_OK;
}

extern "C" int scrf_get_batch_sums(scrf_handle h, double* sums3) {
  if (!h || !sums3) return SCRF_ERR_INVALID;
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipMemcpyAsync(sums3, h->d_sums, sizeof(double) * 3, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return SCRF_OK;
}

// The same without stopping the host: the copy is queued behind the work issued so far and read later (a trainer reads
// minibatch k's sums after it has issued minibatch k + 1, whose batch it can then prepare while k's count kernels run).
extern "C" int scrf_queue_batch_sums(scrf_handle h) {
  if (!h) return SCRF_ERR_INVALID;
  HIPCHK(h, hipSetDevice(h->device));
  // (a copy queued before and never taken -- a caller that gave up on its minibatch -- is superseded: the image is
  // written in stream order)
  HIPCHK(h, hipMemcpyAsync(h->h_sums, h->d_sums, sizeof(double) * 3, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipEventRecord(h->ev_sums, h->stream));
  h->sums_queued = true;
  return SCRF_OK;
}
extern "C" int scrf_take_batch_sums(scrf_handle h, double* sums3) {
  if (!h || !sums3) return SCRF_ERR_INVALID;
  if (!h->sums_queued) return fail(h, SCRF_ERR_INVALID, "scrf_take_batch_sums: nothing queued");
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipEventSynchronize(h->ev_sums));
  for (int i = 0; i < 3; i++) sums3[i] = h->h_sums[i];
  h->sums_queued = false;
  return SCRF_OK;
}

// ---------------------------------------------------------------------------------------------
// scratch arena
// ---------------------------------------------------------------------------------------------
static size_t pad256(size_t b) { return (b + 255) & ~(size_t)255; }
// A null base is the measuring mode: take() advances `off` by the same padded amounts and hands out nullptr, so the walk
// that carves a chunk's buffers also gives the chunk's size (its final `off`) -- the layout is written once.
struct Arena {
  char* base;
  size_t cap, off;
  template <class Tp> Tp* take(size_t n) {
    Tp* p = base ? (Tp*)(base + off) : nullptr;
    off += pad256(n * sizeof(Tp));
    return p;
  }
};

static int ensure_scratch(scrf_handle h, size_t bytes, int lane = 0) {
  if (bytes <= h->scratch[lane].cap()) return SCRF_OK;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream2));
  hipError_t e = h->scratch[lane].reserve(bytes);
  if (e != hipSuccess) return fail(h, SCRF_ERR_HIP, "scratch allocation of %zu bytes failed: %s", bytes, hipGetErrorString(e));
  return SCRF_OK;
}

// ---------------------------------------------------------------------------------------------
// batches
// ---------------------------------------------------------------------------------------------
// ---- the batch-array pool (BatchPool, above the handle) ----
static size_t pool_class(size_t bytes) {   // size classes: powers of two from 64 KB (a minibatch's arrays vary in size from step to step)
  size_t c = 64u << 10;
  while (c < bytes) c *= 2;
  return c;
}
static void pool_poll(scrf_handle h) {   // which destroy epochs have finished on the device
  while (h->pool.done < h->pool.epoch) {
    hipEvent_t ev = h->pool.ev[(h->pool.done + 1) % 8];
    if (!ev || hipEventQuery(ev) != hipSuccess) break;
    h->pool.done++;
  }
}
static int pool_alloc(scrf_handle h, size_t bytes, void** out) {
  *out = nullptr;
  if (!h->kn.pool_on()) { HIPCHK(h, hipMalloc(out, bytes)); return SCRF_OK; }
  const size_t cap = pool_class(bytes);
  pool_poll(h);
  for (size_t i = 0; i < h->pool.free.size(); i++) {
    const auto& bl = h->pool.free[i];
    if (bl.cap == cap && bl.epoch <= h->pool.done) {
      *out = bl.p;
      h->pool.bytes -= bl.cap;
      h->pool.free[i] = h->pool.free.back();
      h->pool.free.pop_back();
      h->pool.live[*out] = cap;
      return SCRF_OK;
    }
  }
  HIPCHK(h, hipMalloc(out, cap));
  h->pool.live[*out] = cap;
  return SCRF_OK;
}
static void pool_release(scrf_handle h, void* p) {   // inside a destroy call: the block carries the epoch being closed
  if (!p) return;
  auto it = h ? h->pool.live.find(p) : decltype(h->pool.live.find(p))();
  if (!h || !h->kn.pool_on() || it == h->pool.live.end()) { hipFree(p); return; }
  h->pool.free.push_back({p, it->second, h->pool.epoch + 1});
  h->pool.bytes += it->second;
  h->pool.live.erase(it);
}
static void pool_close_epoch(scrf_handle h) {   // after the releases of one destroy call
  const uint64_t e = h->pool.epoch + 1;
  Event& ev = h->pool.ev[e % 8];
  if (ev) { hipEventSynchronize(ev); if (h->pool.done < e - 8 && e >= 8) h->pool.done = e - 8; }   // the slot's old epoch (e - 8) is long past
  else ev.create(hipEventDisableTiming);
  hipEventRecord(ev, h->stream);
  h->pool.epoch = e;
  // keep the pool bounded: beyond 8 GiB of idle blocks, give the finished ones back
  if (h->pool.bytes > ((size_t)8 << 30)) {
    pool_poll(h);
    for (size_t i = 0; i < h->pool.free.size();) {
      if (h->pool.free[i].epoch <= h->pool.done) {
        h->pool.bytes -= h->pool.free[i].cap;
        hipFree(h->pool.free[i].p);
        h->pool.free[i] = h->pool.free.back();
        h->pool.free.pop_back();
      } else i++;
    }
  }
}

static hipStream_t upload_stream(scrf_handle h) { return (h->kn.pool_on() && h->kn.pool_up()) ? h->pool.up_stream.get() : h->stream.get(); }
// A device array of batch `b`: a block of the pool, recorded in b->blocks (scrf_batch_destroy gives those back), with `src`
// queued into it on the upload stream.  *d is the typed view the kernels read.
template <class Tp>
static int upload(scrf_handle h, scrf_batch b, Tp** d, const Tp* src, size_t n) {
  *d = nullptr;
  if (n == 0) n = 1;
  void* p = nullptr;
  RCCHK(pool_alloc(h, sizeof(Tp) * n, &p));
  b->blocks.push_back(p);
  *d = (Tp*)p;
  if (src) HIPCHK(h, hipMemcpyAsync(*d, src, sizeof(Tp) * n, hipMemcpyHostToDevice, upload_stream(h)));
  return SCRF_OK;
}

// K states per label on the segmental model: P*P + 2L - P boundary arcs per frame after the first instead of L*L
// (decoders/CRF_LatticeBuilder_StdSeg_WithoutDurLab_WithoutSegTransFtr.h:563-597)
static uint64_t shadow_num_arcs(scrf_handle h, uint32_t T) {
  const uint64_t L = h->xlay.L, P = L / h->xlay.K;
  return (uint64_t)(T - 1) * (P * P + 2 * L - P) + scrf_seg_base(T, h->xlay.D) * L + L;
}

extern "C" int scrf_batch_destroy(scrf_handle h, scrf_batch b) {
  if (!b) return SCRF_OK;
  if (h) hipSetDevice(h->device);
  if (h && h->lp.batch == b) h->lp.batch = nullptr;
  if (h && h->nb.batch == b) h->nb.batch = nullptr;
  if (h && !h->kn.pool_on()) hipStreamSynchronize(h->stream);
  // (pool: no synchronisation here -- the blocks wait in the pool until the engine stream has passed this point)
  for (void* p : b->blocks) pool_release(h, p);
  if (h && h->kn.pool_on()) pool_close_epoch(h);
  delete b;
  return SCRF_OK;
}

extern "C" int scrf_batch_create(scrf_handle h, const scrf_utt* utts, uint32_t n, uint32_t n_streams,
                                 const scrf_stream_recipe* recipes, scrf_batch* out) {
  if (!h || !out || (!utts && n)) return SCRF_ERR_INVALID;
  *out = nullptr;
  HIPCHK(h, hipSetDevice(h->device));
  const ScrfLayout& lay = h->lay;
  if (n == 0) return fail(h, SCRF_ERR_EMPTY, "scrf_batch_create: empty batch");
  if (n >= (1u << 23)) return fail(h, SCRF_ERR_INVALID, "scrf_batch_create: at most 8388607 utterances per batch (the failure latch packs utterance and code into 31 bits)");
  const bool by_windows = utts[0].windows != nullptr;
  if (!by_windows) {
    if (n_streams == 0 || n_streams > SCRF_MAX_STREAMS || !recipes)
      return fail(h, SCRF_ERR_INVALID, "scrf_batch_create: frame input needs 1..%d stream recipes", SCRF_MAX_STREAMS);
    uint32_t tot = 0;
    for (uint32_t s = 0; s < n_streams; s++) {
      if (recipes[s].in_width == 0) return fail(h, SCRF_ERR_INVALID, "scrf_batch_create: stream %u has in_width 0", s);
      tot += window_width(recipes[s], lay.D);
    }
    if (tot != lay.F)
      return fail(h, SCRF_ERR_INVALID, "scrf_batch_create: joined window width %u != num_feas %u", tot, lay.F);
  }
  // built inside a guard: every early return below destroys the half-built batch, blocks taken so far included
  struct Guard {
    scrf_handle h;
    scrf_batch b;
    ~Guard() { if (b) scrf_batch_destroy(h, b); }
  } guard{h, new scrf_batch_s()};
  scrf_batch b = guard.b;
  b->U = n;
  b->mode = by_windows ? 0 : 1;
  b->n_streams = by_windows ? 0 : n_streams;
  b->T.resize(n);
  b->frame_off.assign(n + 1, 0); b->seg_off.assign(n + 1, 0); b->arc_off.assign(n + 1, 0);
  bool have_labels = utts[0].labels != nullptr;
  for (uint32_t u = 0; u < n; u++) {
    const scrf_utt& q = utts[u];
    if ((q.windows != nullptr) != by_windows) return fail(h, SCRF_ERR_INVALID, "scrf_batch_create: utterance %u mixes window and frame input", u);
    if ((q.labels != nullptr) != have_labels) return fail(h, SCRF_ERR_INVALID, "scrf_batch_create: labels given for some utterances only");
    if (q.T == 0) return fail(h, SCRF_ERR_EMPTY, "scrf_batch_create: utterance %u: No features read from this sentence.", u);
    b->T[u] = q.T;
    b->frame_off[u + 1] = b->frame_off[u] + q.T;
    b->seg_off[u + 1] = b->seg_off[u] + scrf_seg_base(q.T, lay.D);
    uint64_t na = lay.K > 1 ? ns_num_arcs(q.T, lay.L, lay.K)
                  : (lay.D == 1 && h->cfg.model_type == SCRF_STDFRAME)
                      ? (uint64_t)lay.L + (uint64_t)(q.T - 1) * lay.L * lay.L + lay.L
                      : h->cfg.model_type == SCRF_STDSEG ? stdseg_num_arcs(q.T, lay.L / lay.D, lay.D)
                      : h->cfg.model_type == SCRF_STDSEG_NO_DUR ? segtrans_num_arcs(q.T, lay.L, lay.D)
                                                                : scrf_arc_base(q.T, lay.L, lay.D) + lay.L;
    b->arc_off[u + 1] = b->arc_off[u] + na;
  }
  const uint64_t NF = b->frame_off[n], NS = b->seg_off[n];
#define BSYNC() do { hipError_t e_ = hipStreamSynchronize(upload_stream(h)); if (e_ != hipSuccess) return fail(h, SCRF_ERR_HIP, "scrf_batch_create: %s", hipGetErrorString(e_)); } while (0)
  RCCHK(upload(h, b, &b->d_T, b->T.data(), n));
  RCCHK(upload(h, b, &b->d_frame_off, b->frame_off.data(), n + 1));
  RCCHK(upload(h, b, &b->d_seg_off, b->seg_off.data(), n + 1));
  RCCHK(upload(h, b, &b->d_arc_off, b->arc_off.data(), n + 1));
  {
    std::vector<uint32_t> fu(NF);
    for (uint32_t u = 0; u < n; u++) std::fill(fu.begin() + b->frame_off[u], fu.begin() + b->frame_off[u + 1], u);
    RCCHK(upload(h, b, &b->d_frame_u, fu.data(), NF));
    BSYNC();
  }
  if (have_labels) {
    std::vector<uint32_t> lab(NF);
    for (uint32_t u = 0; u < n; u++) memcpy(&lab[b->frame_off[u]], utts[u].labels, sizeof(uint32_t) * utts[u].T);
    RCCHK(upload(h, b, &b->d_labels, lab.data(), NF));
    std::vector<uint32_t> nxt(NF), cnt((size_t)lay.L * lay.L, 0);
    for (uint32_t u = 0; u < n; u++) {
      uint32_t cur = SCRF_LAB_BAD;
      for (uint32_t t = b->T[u]; t-- > 0;) {
        const uint64_t f = b->frame_off[u] + t;
        nxt[f] = cur;
        const uint32_t lb = lab[f];
        if (lb != SCRF_LAB_BAD) {
          // K states per label: a labelled transition the topology lacks matches none of the node's transition
          // terms (nodes/CRF_StdSegNStateNode_WithoutDurLab_WithoutSegTransFtr.cpp:822-876) and adds nothing
          if (h->shadow && cur != SCRF_LAB_BAD && lb < lay.L * lay.D && cur < lay.L * lay.D &&
              h->xlay.trans_idx_k(lb % lay.L, cur % lay.L) == 0xffffffffu)
            nxt[f] = SCRF_LAB_BAD;
          else if (t + 1 < b->T[u] && cur != SCRF_LAB_BAD && lb < lay.L * lay.D && cur < lay.L * lay.D && h->cfg.model_type != SCRF_STDSEG)
            cnt[(size_t)(lb % lay.L) * lay.L + cur % lay.L]++;
          cur = lb;
        }
      }
    }
    RCCHK(upload(h, b, &b->d_next_lab, nxt.data(), NF));
    if (h->cfg.model_type == SCRF_STDSEG_NO_DUR || h->cfg.model_type == SCRF_STDSEG) {
      std::vector<uint32_t> prv(NF);
      for (uint32_t u = 0; u < n; u++) {
        uint32_t cur = SCRF_LAB_BAD;
        for (uint32_t t = 0; t < b->T[u]; t++) {
          const uint64_t f = b->frame_off[u] + t;
          prv[f] = cur;
          if (lab[f] != SCRF_LAB_BAD) cur = lab[f];
        }
      }
      RCCHK(upload(h, b, &b->d_prev_lab, prv.data(), NF));
    }
    RCCHK(upload(h, b, &b->d_trans_counts, cnt.data(), cnt.size()));
    BSYNC();
  }
  if (by_windows) {
    RCCHK(upload<float>(h, b, &b->d_windows, nullptr, NS * lay.F + 64));  // tail pad: wide loads may over-read 12 B
    for (uint32_t u = 0; u < n; u++) {
      hipError_t e = hipMemcpyAsync(b->d_windows + b->seg_off[u] * lay.F, utts[u].windows,
                                    sizeof(float) * (b->seg_off[u + 1] - b->seg_off[u]) * lay.F, hipMemcpyHostToDevice, upload_stream(h));
      if (e != hipSuccess) return fail(h, SCRF_ERR_HIP, "window upload failed: %s", hipGetErrorString(e));
    }
  } else {
    for (uint32_t s = 0; s < n_streams; s++) {
      b->recipe[s] = recipes[s];
      b->width[s] = window_width(recipes[s], lay.D);
      const uint32_t pad = recipes[s].left_ctx + recipes[s].right_ctx;
      std::vector<uint64_t> so(n + 1, 0);
      for (uint32_t u = 0; u < n; u++) {
        if (!utts[u].frames[s]) return fail(h, SCRF_ERR_INVALID, "scrf_batch_create: utterance %u has no frames for stream %u", u, s);
        so[u + 1] = so[u] + utts[u].T + pad;
      }
      RCCHK(upload(h, b, &b->d_sframe_off[s], so.data(), n + 1));
      RCCHK(upload<float>(h, b, &b->d_frames[s], nullptr, so[n] * recipes[s].in_width + 64));  // tail pad: wide loads may over-read 12 B
      BSYNC();
      for (uint32_t u = 0; u < n; u++) {
        hipError_t e = hipMemcpyAsync(b->d_frames[s] + so[u] * recipes[s].in_width, utts[u].frames[s],
                                      sizeof(float) * (so[u + 1] - so[u]) * recipes[s].in_width, hipMemcpyHostToDevice, upload_stream(h));
        if (e != hipSuccess) return fail(h, SCRF_ERR_HIP, "frame upload failed: %s", hipGetErrorString(e));
      }
    }
  }
  // fused window synthesis: one segment-recipe stream without context whose window is exactly
  // the state feature range, no transition features
  const int f32_cfg = h->cfg.train_precision == SCRF_PREC_FAST32;
  const bool sparse_map = h->cfg.map_type >= SCRF_STDSPARSE;   // the general path only
  const bool hybrid_first = !sparse_map && h->kn.hybrid_first() && lay.L > 64 && n_streams == 1 && !lay.use_tf;
  const bool seg_stream0 = !sparse_map && !hybrid_first && !by_windows && n_streams >= 1 && h->cfg.model_type != SCRF_STDSEG_NO_DUR && h->cfg.model_type != SCRF_STDSEG && lay.use_sf &&
                           recipes[0].extract_seg_ftr && !recipes[0].left_ctx && !recipes[0].right_ctx && lay.sfs == 0 &&
                           lay.nsfe == 8 * recipes[0].in_width + lay.D && fused_supported(h->kn, fused_shape(lay), recipes[0].in_width, f32_cfg);
  // "mixed" (round 4, BASELINE config 3's shape): the state features are exactly stream 0's segment-recipe window and the
  // transition features live in the other streams' columns -- the state part takes the fused kernels, the transition
  // part keeps the materialised first-row windows and the dense contractions
  // "hybrid" (round 4, BASELINE config 5's shape): the same stream structure where the fused kernels' LDS images do not
  // fit (L > 64).  The window vectors stay materialised, but the five sampled blocks -- 5 W of the 8 W + D columns, copies
  // of raw frames -- leave the two dense contractions: scores get their share from the per-frame projections P (k_add_p),
  // counts through the per-frame sums Z (k_lin_z, Z^T F), exactly as on the fused path.
  b->hybrid_ok = !sparse_map && !by_windows && n_streams == 1 && h->cfg.model_type != SCRF_STDSEG_NO_DUR && h->cfg.model_type != SCRF_STDSEG && lay.use_sf &&
                 !lay.use_tf && recipes[0].extract_seg_ftr && !recipes[0].left_ctx && !recipes[0].right_ctx && lay.sfs == 0 && lay.D >= 2 &&
                 lay.nsfe == 8 * recipes[0].in_width + lay.D && (hybrid_first || !fused_supported(h->kn, fused_shape(lay), recipes[0].in_width, f32_cfg));
  const bool mixed_ok = seg_stream0 && n_streams >= 2 && lay.use_tf && lay.tfs >= lay.nsfe && h->kn.fuse_mixed;
  if ((seg_stream0 && n_streams == 1 && !lay.use_tf && lay.nsfe == lay.F) || mixed_ok) {
    b->fused_ok = true;
    b->mixed = mixed_ok;
    {
      std::vector<float> xm(NF);
      const uint32_t W0 = recipes[0].in_width;
      for (uint32_t u = 0; u < n; u++) {
        float m = fmaxf(1.0f, (float)fabs(lay.sbv));
        const float* x = utts[u].frames[0];
        for (size_t i = 0; i < (size_t)utts[u].T * W0; i++) m = fmaxf(m, fabsf(x[i]));
        m = nextafterf(m, INFINITY);   // |sbv| was rounded to float
        std::fill(xm.begin() + b->frame_off[u], xm.begin() + b->frame_off[u + 1], m);
      }
      RCCHK(upload(h, b, &b->d_xm_f, xm.data(), NF));
      BSYNC();
    }
    // score tiles: the windows of TB whole frames; expected-count tiles: those of TBE whole frames (<= 64 windows)
    const uint32_t D = lay.D, TB = fused_scores_tb(recipes[0].in_width, D);
    const uint32_t TBE = fused_expf_plan(h->kn, fused_shape(lay), recipes[0].in_width, f32_cfg, 0, 1).frames;   // (tile list 1 without the linear average)
    // a third list when the engine trains with the linear window average and its count kernel walks taller tiles
    uint32_t TBL = 0;
    if (h->cfg.train_precision == SCRF_PREC_FASTLIN && fused_la_supported(h->kn, fused_shape(lay), recipes[0].in_width)) {
      const ScrfFusedExpfPlan plan = fused_expf_plan(h->kn, fused_shape(lay), recipes[0].in_width, 0, 1, 1);
      if (plan.tile_list == 2) TBL = plan.frames;
    }
    for (int k = 0; k < (TBL ? 3 : 2); k++) {
      std::vector<ScrfTileDesc> td;
      b->tile_off[k].assign(n + 1, 0);
      for (uint32_t u = 0; u < n; u++) {
        const uint32_t T = b->T[u];
        const uint64_t nseg = scrf_seg_base(T, D);
        uint32_t t = 0;
        for (uint64_t r0 = 0; r0 < nseg;) {
          ScrfTileDesc q;
          memset(&q, 0, sizeof(q));
          uint32_t t_end;   // one past the last frame touched
          uint64_t r1;
          t_end = std::min(T, t + (k == 0 ? TB : k == 1 ? TBE : TBL));
          r1 = scrf_seg_base(t_end, D);
          q.r0 = (uint32_t)r0; q.t0 = t; q.back = (uint16_t)std::min(t, D - 1);
          q.nfr = (uint16_t)(t_end - t); q.nrows = (uint16_t)(r1 - r0);
          q.row_abs = b->seg_off[u] + r0;
          q.fr_abs = b->frame_off[u] + t - q.back;
          td.push_back(q);
          r0 = r1;
          t = t_end;
        }
        b->tile_off[k][u + 1] = td.size();
      }
      RCCHK(upload(h, b, &b->d_tiles[k], td.data(), td.size()));
      BSYNC();
    }
  }
  RCCHK(upload<double>(h, b, &b->d_numer, nullptr, n));
  RCCHK(upload<double>(h, b, &b->d_zx, nullptr, n));
  RCCHK(upload<int>(h, b, &b->d_status, nullptr, n));
  BSYNC();
#undef BSYNC
  guard.b = nullptr;
  *out = b;
  return SCRF_OK;
}

extern "C" int scrf_batch_info(scrf_handle h, scrf_batch b, uint32_t* n_utts, uint64_t* n_frames, uint64_t* n_segs, uint64_t* n_arcs) {
  if (!h || !b) return SCRF_ERR_INVALID;
  if (n_utts) *n_utts = b->U;
  if (n_frames) *n_frames = b->frame_off[b->U];
  if (n_segs) *n_segs = b->seg_off[b->U];
  if (n_arcs) {
    *n_arcs = b->arc_off[b->U];
    if (h->shadow) {
      *n_arcs = 0;
      for (uint32_t u = 0; u < b->U; u++) *n_arcs += shadow_num_arcs(h, b->T[u]);
    }
  }
  return SCRF_OK;
}

// ---------------------------------------------------------------------------------------------
// chunk planning and the per-chunk pipeline
// ---------------------------------------------------------------------------------------------
enum { PH_WIN = 0, PH_SCORE = 1, PH_FB = 2, PH_EXPF = 3, PH_REDUCE = 4, PH_VIT = 5, PH_ALL = 6, PH_K_SCORE = 7, PH_K_DP = 8, PH_K_EXPF = 9 };
#define EXPF_ROWS_PER_CHUNK 4096ull
// split-K plan of the state expected-count contraction: about 1024 K-chunks (2 per CU-slot
// of the 512-thread MFMA kernel), at least 4096 rows each
static uint64_t expf_rows_per_chunk(uint64_t nseg) {
  uint64_t rpc = (nseg + 1023) / 1024;
  rpc = (rpc + 31) & ~31ull;
  return rpc < EXPF_ROWS_PER_CHUNK ? EXPF_ROWS_PER_CHUNK : rpc;
}

// K-chunks of the per-window transition contraction (STDSEG_NO_DUR: [N_seg][L*L] posteriors x a few feature functions):
// one per 2048 rows while the partial-sum slabs stay within 128 MB (at least 4)
static uint32_t segtrans_chunks(uint64_t nseg, size_t LL, uint32_t ntf) {
  // (ntf = 0: neither transition features nor a transition bias -- the slabs are empty)
  const uint64_t cap = std::max<uint64_t>(4, (128ull << 20) / (LL * std::max<uint32_t>(1, ntf) * sizeof(double)));
  return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(cap, (nseg + 2047) / 2048));
}

// K-chunks (row chunks) of the per-frame transition contraction (stdtrans: [frames][L*L] posteriors x the transition
// feature functions).  The wide form of k_expf_mfma holds one 8-wavefront workgroup per CU, so the launch runs in rounds
// of 256 workgroups: with the TIMIT demo's 240 tiles per chunk, 4 chunks are 3.75 rounds (the last one three quarters
// full), 16 chunks are 15 whole rounds.  Smallest count from 4 up to 16 (at least 1024 rows each) whose last round is >= 97 %
// full, else the fullest; SCRF_TRANS_CHUNKS overrides (A/B runs).
static uint32_t transframe_chunks(const ScrfKnobs& kn, uint64_t nfr, uint32_t n_out, uint32_t nfun, int f32) {
  const uint32_t base = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(4, (nfr + 2047) / 2048));
  if (kn.trans_chunks > 0) return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)kn.trans_chunks, std::max<uint64_t>(1, nfr / 64)));
  const uint32_t tiles = expf_mfma_wide_tiles(n_out, nfun, f32);
  if (tiles == 0 || base < 4) return base;
  const uint32_t cus = 256;
  uint32_t best = base;
  double best_fill = 0.0;
  // every chunk owns a slab of partial sums [n_out][nfun]: no more chunks than keep the slabs within 1 GB (the TIMIT
  // demo: 34.5 MB each)
  const uint64_t slab_bytes = (uint64_t)n_out * nfun * sizeof(double);
  const uint32_t n_max = (uint32_t)std::min<uint64_t>(16, std::max<uint64_t>(base, (1ull << 30) / std::max<uint64_t>(1, slab_bytes)));
  for (uint32_t n = base; n <= n_max && nfr / n >= 1024; n++) {
    const uint64_t wg = (uint64_t)tiles * n;
    const double fill = (double)wg / (double)(((wg + cus - 1) / cus) * cus);
    if (fill > best_fill + 1e-9) { best_fill = fill; best = n; }
    if (fill >= 0.97) { best = n; break; }
  }
  return best;
}

// K-chunks of the transition-bias contraction: one wavefront each, about 4096 of them (four per SIMD: a wavefront's
// next operands are only one 576-cycle group of MFMAs ahead, the others cover the rest of the load latency)
static uint64_t atb_rows_per_chunk(uint64_t nfr) {
  uint64_t rpc = ((nfr + 4095) / 4096 + 3) & ~3ull;
  return rpc < 64 ? 64 : rpc;
}

struct ChunkBufs {
  hipStream_t st = nullptr;  // stream of the lane this chunk runs on
  double* grad = nullptr;    // gradient / batch sums this lane accumulates into
  double* sums = nullptr;
  float* X = nullptr;        // window vectors of the chunk (scratch, or a view into the batch)
  double* S = nullptr;       // [nseg][L]
  double* M = nullptr;       // [nfr][L*L] or engine M0
  int m_per_frame = 0;
  double* AD = nullptr;      // [nseg][L]
  double* alpha = nullptr;   // [nfr][L]
  double* beta = nullptr;    // [nfr][L] (parity hooks only)
  double* XI = nullptr;      // [nfr][L*L]
  double* xi_acc = nullptr;  // [nutt][L*L]
  uint64_t* xrow_cur = nullptr;
  uint64_t* xrow_next = nullptr;
  double* slab_s = nullptr;
  double* slab_t = nullptr;
  uint16_t* bp_b = nullptr;
  uint16_t* bp_e = nullptr;
  // fast decode: float arc weights of the fused score kernel + the entries to recompute
  float* Wn = nullptr;       // [nseg][L]
  uint64_t* fix_list = nullptr;
  uint32_t* fix_cnt = nullptr;
  uint32_t fix_cap = 0;
  uint32_t nch_s = 0, nch_t = 0;
  uint64_t rpc_s = 0, rpc_t = 0;
  // wavefront-per-utterance DP
  bool wave = false;
  double* E = nullptr;       // exp(M - shift) per frame, or the engine's E0
  double* ET = nullptr;
  double* msh = nullptr;
  double* sd = nullptr;      // [nfr][L]
  double* fA = nullptr;      // [nfr][L] xi factors
  double* fB = nullptr;
  double* numer_f = nullptr; // [nfr]
  double* mass_s = nullptr;  // [nfr] state posterior mass per node (reference self-check, computeExpF :917-947)
  double* mass_part = nullptr;  // [groups][nfr] its partial sums per 64 outputs (posterior output, L > 64)
  // scaled linear-domain recursion (training path of the wavefront DP)
  bool lin = false;
  bool es_ready = false;     // cb.S already holds exp(S - smax) (written by the fused score kernel)
  bool z_ready = false;      // cb.Z already holds the per-frame sums of R (written by k_post_z)
  ScrfDpLin dl = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  double* smax = nullptr;    // [nseg] row maxima of the scores
  double* s_true = nullptr;  // [nfr] score of the labelled window ending at each frame
  double* R = nullptr;       // [nseg][L] Y - gamma: cb.S (linear path) or cb.AD
  double* slab_atb = nullptr;
  uint32_t nch_atb = 0;
  uint64_t rpc_atb = 0;
  bool fused = false;        // window synthesis fused into the contractions (no X)
  double* P = nullptr;       // [nfr][5L] per-frame projections of the sampled blocks
  double* Z = nullptr;       // [nfr][5L] per-frame sums of R over the windows sampling the frame
  double* slab_l = nullptr;
  uint32_t nch_l = 0;
  uint64_t rpc_l = 0;
  bool hybrid = false;       // materialised X, but the sampled blocks through P / Z (scrf_batch::hybrid_ok)
  bool la = false;           // SCRF_PREC_FASTLIN: linear window average (6 groups in P / Z, no avg group in the dense parts)
  double* slab_d = nullptr;  // duration + bias counts of the wave-specialised count kernel (behind slab_s)
  ScrfFusedExpfPlan expf_plan = {0, 0, 0, 0, 0, 0, 1, 1};   // the fused count kernel's plan for this chunk (tile list, slab columns)
  ScrfSparseIndex spx[2];    // sparse maps: inverted index + bias slab of the state [0] / transition [1] counts
  ScrfLatBufs lat = {nullptr, nullptr, nullptr, nullptr, nullptr};   // lattice beam: distances of the chunk's states
  uint32_t* lat_counts = nullptr;   // [nodes of the chunk] kept arcs per node
  uint64_t* lat_node_off = nullptr; // [nodes + 1]
  uint16_t* al_bp = nullptr;        // forced alignment: sum of T * K back pointers over the chunk's transcripts that fit
  double *tr_aB = nullptr, *tr_bE = nullptr;   // transcript scoring: the same cells, forward (segment start) and backward (segment end) sums
  // soft-alignment gradient: the state numerators [nseg][L], the cells' forward sums at a segment's end / backward sums at
  // its start, and (bias-only transitions) the per-position sums of the transition numerators
  double *sn_G = nullptr, *sn_aE = nullptr, *sn_bB = nullptr, *sn_adv = nullptr, *sn_stay = nullptr, *sn_tab = nullptr;
  ScrfNbestBufs nb = {0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};   // N-best: back pointers, final lists, offsets
  bool lamT_ready = false;   // sparse maps: h->d_lamT already re-laid for this call (scrf_fb_batch: once, before the lanes fork)
};

// The arcs of a scored chunk for the lattice searches (scrf_arcw.h).  The one place that knows which weights a search reads:
// a fast-decode chunk carries the formed float weights cb.Wn and no scores; the frame model never has Wn.
static ScrfArcSrc arc_src(scrf_handle h, const ChunkBufs& cb, bool fast = false) {
  const int frame_model = h->cfg.model_type == SCRF_STDFRAME;
  const bool formed = fast && !frame_model;
  return ScrfArcSrc{formed ? nullptr : cb.S, formed ? cb.Wn : nullptr, cb.M, cb.m_per_frame, frame_model};
}

// ponly (scrf_posteriors_batch): the recursion of the training path without anything that needs labels or feeds the
// gradient -- the linear-domain vectors (or alpha_dur / beta) and the per-frame state mass, no count buffers
struct Need {
  bool fb = false, post = false, beta = false, vit = false;
  bool fused = false, vitfast = false, la = false, hybrid = false;   // the batch's form (set_batch_form, decode_chunks)
  bool ponly = false, plog = false, lat = false, align = false, trans = false, soft = false;
  uint32_t nbest = 0;   // scrf_nbest_batch: the list length
  // one constructor per kind of pass, so that no call site depends on the order of the fields
  static Need scores() { return Need(); }                                              // windows and scores only
  static Need recursion() { Need n; n.fb = n.beta = true; return n; }                  // + the log-domain node values (hooks)
  static Need alpha_sum(bool on) { Need n; n.fb = on; return n; }                      // scores (+ Zx, for a normalised lattice)
  static Need training() { Need n; n.fb = n.post = true; return n; }
  static Need posterior(bool fast) { Need n = recursion(); n.ponly = true; n.plog = !fast; return n; }
  static Need transcript(bool fast) { Need n = posterior(fast); n.trans = true; return n; }
  static Need soft_training() { Need n = training(); n.trans = n.soft = true; return n; }   // scrf_fb_transcript_batch
  static Need viterbi() { Need n; n.vit = true; return n; }
  static Need lattice() { Need n; n.lat = true; return n; }
  static Need alignment() { Need n; n.align = true; return n; }
  static Need nbest_of(uint32_t n_best) { Need n; n.nbest = n_best; return n; }
};
// trans (scrf_transcript_batch): two doubles per (frame, transcript position) cell of the chunk
// soft (scrf_fb_transcript_batch): two more per cell, a double per (window row, label), and with bias-only transitions two
// per transcript position and an [L][L] table per utterance
// nbest (scrf_nbest_batch): two 32-bit back pointers per (frame, label, rank), and per (utterance, rank) the final list and
// the offsets of the backtrace
// align (scrf_align_batch): the back pointers of the chunk's (frame, transcript position) cells
// lat (scrf_lattice_prune_batch): four distance arrays over the chunk's frames and the node counts / offsets
// plog: ponly through the log-domain recursion (SCRF_PREC_EXACT: no FAST precision)
static bool need_lin(const Need& nd) { return nd.post || (nd.ponly && !nd.plog); }

// entries the decode screen may list per chunk before the chunk falls back to the EXACT path
static uint32_t decode_fix_cap(uint64_t nseg, uint32_t L) {
  const uint64_t c = nseg * L / 64 + 4096;
  return (uint32_t)std::min<uint64_t>(c, 1u << 26);
}

// does the recursion run on the wavefront kernels?  L <= 64: always (log-domain kernels for the
// hooks, linear-domain for training); 64 < L <= 256: the multi-wavefront linear-domain kernel,
// training path only
// STDSEG_NO_DUR: one transition matrix per window (scrf_segtrans.hip); its own workgroup recursion
static bool segtrans(scrf_handle h) { return h->cfg.model_type == SCRF_STDSEG_NO_DUR; }

// stdsparse / stdsparsetrans (scrf_sparse.hip): always the general path, scores and counts by the sparse kernels
static bool sparse(scrf_handle h) { return h->cfg.map_type >= SCRF_STDSPARSE; }

static bool wave_path(scrf_handle h, bool post) {
  if (h->force_fb || segtrans(h)) return false;
  return dp_wave_supported(dp_shape(h->lay)) || (post && h->kn.lindp && (dplin_mw_supported(dp_shape(h->lay)) || dplin_supported(dp_shape(h->lay))));
}

// fused path: the five sampled blocks as per-frame projections (outputs (k, label), k < 5), and
// the dense column groups [avg | max | min | onehot(d)] + bias
static ScrfGemmSpec spec_samples(uint32_t W) { return ScrfGemmSpec{2, 0, W, 0, 0.0, 0, W}; }
static ScrfGemmSpec spec_dense(const ScrfLayout& l, uint32_t W) {
  return ScrfGemmSpec{0, 0, 3 * W + l.D, (uint32_t)l.use_sb, l.sbv, 5 * W, 0};
}
// hybrid path: the materialised row holds [avg | max | min | onehot(d)] only (k_windows without the sampled blocks), padded
// to whole 16-byte groups
static uint32_t hybrid_row_floats(const ScrfLayout& l, uint32_t W) { return (3 * W + l.D + 3) & ~3u; }
static ScrfGemmSpec spec_stats_x(const ScrfLayout& l, uint32_t W) {   // [avg | max | min] of that row
  (void)l;
  return ScrfGemmSpec{0, 0, 3 * W, 0, 0.0, 5 * W, 0};
}
static ScrfGemmSpec spec_dense_x(const ScrfLayout& l, uint32_t W) {   // the whole row + bias
  return ScrfGemmSpec{0, 0, 3 * W + l.D, (uint32_t)l.use_sb, l.sbv, 5 * W, 0};
}

// The scratch layout of chunk [u0, u1) under `nd`, written once: every buffer of the chunk is taken from `a` in a fixed order
// and recorded in *cb.  On a measuring arena the same walk sizes the chunk (chunk_size, the planner); on the lane's scratch
// it carves it (carve).  A new buffer is one more take here.
static void chunk_layout(scrf_handle h, scrf_batch b, uint32_t u0, uint32_t u1, const Need& nd, Arena& a, ChunkBufs* cb) {
  const ScrfLayout& l = h->lay;
  const size_t LL = (size_t)l.L * l.L;
  const uint64_t nutt = u1 - u0, nfr = b->frame_off[u1] - b->frame_off[u0], nseg = b->seg_off[u1] - b->seg_off[u0];
  if (nd.fused) {
    const uint32_t W0 = b->recipe[0].in_width;
    cb->X = b->mixed ? a.take<float>(nseg * l.F) : nullptr;
    cb->la = nd.la;
    const size_t ng = nd.la ? 6 : 5;
    cb->P = a.take<double>(nfr * ng * l.L);
    cb->Z = cb->P;  // the projections are dead once the scores exist
    if (nd.post) {
      cb->rpc_l = ((nfr + 511) / 512 + 31) & ~31ull;   // <= 512 K-chunks of whole 4-frame groups
      cb->nch_l = (uint32_t)((nfr + cb->rpc_l - 1) / cb->rpc_l);
      cb->slab_l = a.take<double>((size_t)512 * ng * l.L * W0);
    }
  } else if (b->mode == 1) cb->X = a.take<float>(nseg * (nd.hybrid ? hybrid_row_floats(l, b->recipe[0].in_width) : l.F));
  else cb->X = b->d_windows + b->seg_off[u0] * l.F;
  if (nd.hybrid) {
    cb->hybrid = true;
    cb->P = a.take<double>(nfr * 5 * l.L);
    cb->Z = cb->P;  // the projections are dead once they are added to the scores
    cb->rpc_l = ((nfr + 511) / 512 + 31) & ~31ull;
    cb->nch_l = (uint32_t)((nfr + cb->rpc_l - 1) / cb->rpc_l);
    cb->slab_l = a.take<double>((size_t)512 * 5 * l.L * b->recipe[0].in_width);
    cb->slab_d = a.take<double>((size_t)(nutt + 1024) * l.L * (l.D + 1));
  }
  cb->fused = nd.fused;
  if (nd.vitfast) {
    cb->Wn = a.take<float>(nseg * l.L);
    cb->fix_cap = decode_fix_cap(nseg, l.L);
    cb->fix_list = a.take<uint64_t>(cb->fix_cap);
    cb->fix_cnt = a.take<uint32_t>(64);
  } else {
    cb->S = a.take<double>(nseg * l.L);
  }
  if (segtrans(h)) {
    cb->M = a.take<double>(nseg * LL);
    cb->m_per_frame = 2;   // per window
  } else if (l.use_tf) {
    cb->M = a.take<double>(nfr * LL);
    cb->xrow_cur = a.take<uint64_t>(nfr);
    cb->m_per_frame = 1;
  } else {
    cb->M = h->d_m0;
    cb->m_per_frame = 0;
  }
  if (nd.fb) {
    cb->wave = wave_path(h, need_lin(nd));
    cb->lin = cb->wave && need_lin(nd) && h->kn.lindp;
    if (cb->lin) {
      cb->smax = a.take<double>(nseg);
      cb->s_true = a.take<double>(nfr);
      cb->dl.a = a.take<double>(nfr * l.L);  cb->dl.ga = a.take<double>(nfr);
      cb->dl.p = a.take<double>(nfr * l.L);  cb->dl.gp = a.take<double>(nfr);
      cb->dl.b = a.take<double>(nfr * l.L);  cb->dl.gb = a.take<double>(nfr);
      cb->dl.sd = a.take<double>(nfr * l.L); cb->dl.gsd = a.take<double>(nfr);
      cb->R = cb->S;              // R = Y - gamma overwrites the exponentiated scores
      cb->fA = cb->dl.a;          // xi factors: a, and sd rescaled in place
      cb->fB = cb->dl.sd;
    } else {
      cb->AD = a.take<double>(nseg * l.L);
      cb->R = cb->AD;
      cb->alpha = a.take<double>(nfr * l.L);
      if (nd.beta || cb->wave || segtrans(h)) cb->beta = a.take<double>(nfr * l.L);
      if (cb->wave) cb->sd = a.take<double>(nfr * l.L);
      if (cb->wave && nd.post) {
        cb->fA = a.take<double>(nfr * l.L);
        cb->fB = a.take<double>(nfr * l.L);
      }
    }
    if (cb->wave) {
      if (l.use_tf) {
        cb->E = a.take<double>(nfr * LL);
        cb->ET = a.take<double>(nfr * LL);
        cb->msh = a.take<double>(nfr);
      } else {
        cb->E = h->d_e0; cb->ET = h->d_et0; cb->msh = h->d_msh0;
      }
      if (nd.post) {
        cb->numer_f = a.take<double>(nfr);
        if (!l.use_tf) {
          cb->rpc_atb = atb_rows_per_chunk(nfr);
          cb->nch_atb = (uint32_t)((nfr + cb->rpc_atb - 1) / cb->rpc_atb);
          cb->slab_atb = a.take<double>((size_t)cb->nch_atb * LL);
        }
      }
    }
    if (nd.ponly) {
      cb->mass_s = a.take<double>(nfr);
      // [groups][nfr], read as one array; sized one padded row per group, as the planner has always counted it
      if (post_occ_groups(dp_shape(l)) > 1) {
        cb->mass_part = a.take<double>(nfr);
        for (uint32_t g = 1; g < post_occ_groups(dp_shape(l)); g++) a.take<double>(nfr);
      }
    }
    if (nd.post) {
      cb->mass_s = a.take<double>(nfr);
      if (segtrans(h)) {
        cb->XI = a.take<double>(nseg * LL);
        cb->nch_t = segtrans_chunks(nseg, LL, l.ntf);
        cb->rpc_t = (nseg + cb->nch_t - 1) / cb->nch_t;
        cb->slab_t = a.take<double>((size_t)cb->nch_t * LL * l.ntf);
      } else if (l.use_tf) {
        cb->XI = a.take<double>(nfr * LL);
        cb->xrow_next = a.take<uint64_t>(nfr);
        if (!sparse(h)) {   // the sparse transition counts have their own slab (below)
          cb->nch_t = transframe_chunks(h->kn, nfr, (uint32_t)LL, scrf_spec_trans(l).nfun(), h->cfg.train_precision == SCRF_PREC_FAST32);
          cb->rpc_t = (nfr + cb->nch_t - 1) / cb->nch_t;
          cb->slab_t = a.take<double>((size_t)cb->nch_t * LL * l.ntf);
        }
      } else if (!cb->wave) {
        cb->xi_acc = a.take<double>(nutt * LL);
      }
      if (sparse(h)) {
        char* sp = a.take<char>(sparse_counts_bytes(nseg, l.F, l.nsfe, l.L));
        if (sp) sparse_counts_carve(sp, nseg, l.F, l.nsfe, l.L, &cb->spx[0]);
        sp = l.use_tf ? a.take<char>(sparse_counts_bytes(nfr, l.F, l.ntfe, (uint32_t)LL)) : nullptr;
        if (sp) sparse_counts_carve(sp, nfr, l.F, l.ntfe, (uint32_t)LL, &cb->spx[1]);
      }
      cb->rpc_s = expf_rows_per_chunk(nseg);
      cb->nch_s = (uint32_t)((nseg + cb->rpc_s - 1) / cb->rpc_s);
      if (!sparse(h)) cb->slab_s = a.take<double>((size_t)(nd.fused ? 512 : cb->nch_s) * l.L * l.nsf);
      if (nd.fused && cb->slab_s) {   // the fused count kernel's plan lives inside its 512 slabs: nothing of it is measured
        const ScrfFusedExpfPlan& plan = cb->expf_plan = fused_expf_plan(h->kn, fused_shape(l), b->recipe[0].in_width, h->cfg.train_precision == SCRF_PREC_FAST32,
                                                                        nd.la, ((uintptr_t)cb->R & 15) == 0);
        cb->nch_s = fused_expf_blocks(plan, b->tile_off[plan.tile_list][u1] - b->tile_off[plan.tile_list][u0]);
        // dense columns + durations + bias <= nsf: the duration slab fits behind the dense one
        cb->slab_d = cb->slab_s + (size_t)cb->nch_s * l.L * plan.ncol;
      }
    }
  }
  if (nd.vit) {
    cb->bp_b = a.take<uint16_t>(nfr * l.L);
    cb->bp_e = a.take<uint16_t>(nfr * l.L);
  }
  if (nd.lat) {
    cb->lat.fB = a.take<double>(nfr * l.L); cb->lat.fE = a.take<double>(nfr * l.L);
    cb->lat.bB = a.take<double>(nfr * l.L); cb->lat.bE = a.take<double>(nfr * l.L);
    cb->lat_counts = a.take<uint32_t>(nfr + nutt);
    cb->lat_node_off = a.take<uint64_t>(nfr + nutt + 1);
  }
  if (nd.align) cb->al_bp = a.take<uint16_t>(h->tx.bp_off[u1] - h->tx.bp_off[u0]);
  if (nd.nbest) {
    const size_t n = (size_t)nutt * nd.nbest;
    cb->nb.N = nd.nbest;
    cb->nb.bp_b = a.take<uint32_t>(nfr * l.L * nd.nbest);
    cb->nb.bp_e = a.take<uint32_t>(nfr * l.L * nd.nbest);
    cb->nb.fin_cost = a.take<float>(n);
    cb->nb.fin_ptr = a.take<uint32_t>(n);
    cb->nb.cnt = a.take<uint32_t>(n);
    cb->nb.lab_pos = a.take<uint64_t>(n + 1);
    cb->nb.hyp_pos = a.take<uint64_t>(n);
    cb->nb.tot = a.take<uint64_t>(2);
  }
  if (nd.trans) {
    cb->tr_aB = a.take<double>(h->tx.cell_off[u1] - h->tx.cell_off[u0]);
    cb->tr_bE = a.take<double>(h->tx.cell_off[u1] - h->tx.cell_off[u0]);
  }
  if (nd.soft) {
    cb->sn_G = a.take<double>(nseg * l.L);
    cb->sn_aE = a.take<double>(h->tx.cell_off[u1] - h->tx.cell_off[u0]);
    cb->sn_bB = a.take<double>(h->tx.cell_off[u1] - h->tx.cell_off[u0]);
    if (!l.use_tf) {
      cb->sn_adv = a.take<double>(h->soft.ph_off[u1] - h->soft.ph_off[u0]);
      cb->sn_stay = a.take<double>(h->soft.ph_off[u1] - h->soft.ph_off[u0]);
      cb->sn_tab = a.take<double>(nutt * LL);
    }
  }
}

// (*tmp takes the walk's pointers, which a measurement does not use: the planner passes the same one for every candidate)
static size_t chunk_size(scrf_handle h, scrf_batch b, uint32_t u0, uint32_t u1, const Need& nd, ChunkBufs* tmp) {
  Arena m{nullptr, 0, 0};
  chunk_layout(h, b, u0, u1, nd, m, tmp);
  return m.off + 4096;
}

// largest u1 > u0 whose chunk fits the budget (always at least one utterance)
static uint32_t plan_chunk(scrf_handle h, scrf_batch b, uint32_t u0, const Need& nd) {
  uint32_t u1 = u0 + 1;
  const uint32_t max_utts = 65535;  // grid.x of the per-frame kernels stays small enough anyway
  ChunkBufs tmp;
  while (u1 < b->U && u1 - u0 < max_utts) {
    uint64_t nfr = b->frame_off[u1 + 1] - b->frame_off[u0], nseg = b->seg_off[u1 + 1] - b->seg_off[u0];
    if (chunk_size(h, b, u0, u1 + 1, nd, &tmp) > h->cfg.scratch_bytes) break;
    if (nfr > 0x7fffffffull) break;
    if (sparse(h) && nseg * (h->lay.F / 2) > 0xffffffffull) break;   // the sparse index's entry positions are 32-bit
    u1++;
  }
  return u1;
}

static int carve(scrf_handle h, scrf_batch b, uint32_t u0, uint32_t u1, const Need& nd, ChunkBufs* cb, int lane = 0) {
  RCCHK(ensure_scratch(h, chunk_size(h, b, u0, u1, nd, cb), lane));
  Arena a{h->scratch[lane], h->scratch[lane].cap(), 0};
  cb->st = lane ? h->stream2.get() : h->stream.get();
  cb->grad = lane ? h->d_grad2.get() : h->d_grad.get();
  cb->sums = lane ? h->d_sums2.get() : h->d_sums.get();
  chunk_layout(h, b, u0, u1, nd, a, cb);
  if (a.off > a.cap) return fail(h, SCRF_ERR_INVALID, "internal: scratch arena overflow");
  return SCRF_OK;
}

struct PhaseTimer {
  scrf_handle h;
  int ph;
  hipStream_t st;
  PhaseTimer(scrf_handle h_, int p, hipStream_t s_ = nullptr) : h(h_), ph(p), st(s_ ? s_ : h_->stream) {
    if (h->tm.on) hipEventRecord(h->tm.ev[ph][0], st);
  }
  void stop(uint32_t launches) {
    if (!h->tm.on) return;
    hipEventRecord(h->tm.ev[ph][1], st);
    hipEventSynchronize(h->tm.ev[ph][1]);
    float ms = 0;
    hipEventElapsedTime(&ms, h->tm.ev[ph][0], h->tm.ev[ph][1]);
    h->tm.ms[ph] += ms;
    h->tm.nlaunch[ph] += launches;
  }
};

// HIP-event time of one kernel launch (or a few belonging together), accumulated by name; only when
// timing is enabled (the stop waits for the kernel, so it serialises the host with the device)
struct KernelTimer {
  scrf_handle h;
  const char* name;
  hipStream_t st;
  KernelTimer(scrf_handle h_, const char* n, hipStream_t s_) : h(h_), name(n), st(s_) {
    if (h->tm.on) hipEventRecord(h->tm.kev[0], st);
  }
  void stop(uint32_t launches = 1) {
    if (!h->tm.on) return;
    hipEventRecord(h->tm.kev[1], st);
    hipEventSynchronize(h->tm.kev[1]);
    float ms = 0;
    hipEventElapsedTime(&ms, h->tm.kev[0], h->tm.kev[1]);
    for (auto& k : h->tm.ktimes)
      if (k.name == name) { k.ms += ms; k.n += launches; return; }
    h->tm.ktimes.push_back({name, ms, launches});
  }
};
#define KT_RUN(name, st, ...) do { KernelTimer kt_(h, name, st); __VA_ARGS__; kt_.stop(); } while (0)

// the bracket of a timed batch call (scrf_enable_timing): clears the phase and kernel times, then times the whole call on
// the engine stream; each entry point closes it where its timed region ends
struct CallTimer {
  scrf_handle h;
  explicit CallTimer(scrf_handle h_) : h(h_) {
    if (!h->tm.on) return;
    memset(h->tm.ms, 0, sizeof(h->tm.ms)); memset(h->tm.nlaunch, 0, sizeof(h->tm.nlaunch)); h->tm.ktimes.clear();
    hipEventRecord(h->tm.ev[SCRF_N_PHASES][0], h->stream);
  }
  void stop() {
    if (!h->tm.on) return;
    hipEventRecord(h->tm.ev[SCRF_N_PHASES][1], h->stream);
    hipEventSynchronize(h->tm.ev[SCRF_N_PHASES][1]);
    hipEventElapsedTime(&h->tm.ms[PH_ALL], h->tm.ev[SCRF_N_PHASES][0], h->tm.ev[SCRF_N_PHASES][1]);
  }
};

static ScrfFusedArgs fused_args(scrf_handle h, scrf_batch b, uint32_t u0, int which) {
  ScrfFusedArgs fa;
  memset(&fa, 0, sizeof(fa));
  fa.frames = b->d_frames[0];
  fa.tiles = b->d_tiles[which];
  fa.tile0 = b->tile_off[which][u0];
  fa.row_base = b->seg_off[u0];
  fa.frame_base = b->frame_off[u0];
  fa.W = b->recipe[0].in_width;
  return fa;
}

// window vectors of chunk [u0, u1) into X, stream by stream (batches made from frames).  skip0: stream 0 is synthesised
// inside the fused kernels; hybrid: rows of hybrid_row_floats without the sampled blocks
static void launch_chunk_windows(scrf_handle h, scrf_batch b, uint32_t u0, uint32_t u1, hipStream_t st, float* X, bool skip0 = false,
                                 bool fast = false, bool hybrid = false) {
  const ScrfLayout& l = h->lay;
  const uint64_t nfr = b->frame_off[u1] - b->frame_off[u0];
  ScrfBatchView bv = b->view();
  uint32_t col = 0;
  for (uint32_t s = 0; s < b->n_streams; col += b->width[s++]) {
    const scrf_stream_recipe& r = b->recipe[s];
    if (skip0 && s == 0) continue;
    // FAST training path with per-frame transition features: a stream whose columns hold no state feature is read through
    // the frame rows (k_frame_rows: the node's first window) only -- its other window rows are not written (the TIMIT
    // demo's +-6-frame context stream: 5.8 GB of the 9.3 GB window image).  The window hook (scrf_windows) and EXACT
    // precision materialise every row.
    const bool first_only = fast && !sparse(h) && l.use_tf && !segtrans(h) && l.D > 1 && (col > l.sfe || col + b->width[s] <= l.sfs);
    KT_RUN("k_windows", st, launch_windows(st, b->d_frames[s], b->d_sframe_off[s], bv, u0, u1, nfr, r.in_width, l.D, r.left_ctx, r.right_ctx,
                                           r.extract_seg_ftr, X, hybrid ? hybrid_row_floats(l, r.in_width) : l.F, col,
                                           (first_only ? 1 : 0) | (hybrid ? 2 : 0)));
  }
}

// bias-only transitions: the one L x L matrix of every frame (the bias value) and its exponential, unless the current
// weights' are there already; true when it was launched.  No feature is read (ntfe = 0), so no window pointer is passed.
static bool ensure_m0(scrf_handle h, hipStream_t st) {
  if (h->m0_valid) return false;
  const ScrfLayout& l = h->lay;
  launch_scores_exact(st, nullptr, l.F, nullptr, 1, h->d_lambda, l, 1, l.L * l.L, h->d_m0);
  launch_exp_m(st, h->kn, h->d_m0, l.L, 1, h->d_e0, h->d_et0, h->d_msh0);
  h->m0_valid = true;
  return true;
}

// sparse maps: lambda index-major, once per batch call on the engine stream (before the lanes fork): every chunk's score
// kernel reads it
static void relay_sparse_lambda(scrf_handle h, hipStream_t st) {
  launch_sp_relay(st, h->d_lambda, h->lay, 0, h->d_lamT[0]);
  if (h->lay.use_tf) launch_sp_relay(st, h->d_lambda, h->lay, 1, h->d_lamT[1]);
}

// windows + exact scores of a chunk (both training and decode start here)
static int run_scores(scrf_handle h, scrf_batch b, uint32_t u0, uint32_t u1, ChunkBufs& cb, bool fast = false, int f32 = 0) {
  const ScrfLayout& l = h->lay;
  const uint64_t nfr = b->frame_off[u1] - b->frame_off[u0], nseg = b->seg_off[u1] - b->seg_off[u0];
  ScrfBatchView bv = b->view();
  if (cb.fused) {
    PhaseTimer tm(h, PH_SCORE, cb.st);
    const uint32_t W0 = b->recipe[0].in_width;
    ScrfFusedArgs fa = fused_args(h, b, u0, 0);
    const bool tabs = h->d_dtab && h->kn.dtab;   // the launch tables: k_dur_table's and (SCRF_RTAB) k_tile_tables'
    const ScrfFusedScoresPlan sp = fused_scores_plan(h->kn, fused_shape(l), W0, f32, cb.Wn ? 1 : 0, cb.la ? 1 : 0, tabs, tabs && h->kn.rtab);
    fa.TB = sp.tb;
    if (tabs) {
      launch_dur_table(cb.st, l, W0, h->d_lambda, h->d_dtab);
      fa.dtab = h->d_dtab;
      const size_t nb = fused_tile_table_bytes(l.D, fa.TB);
      if (nb > h->rtab.tab.cap()) h->rtab.valid = false;   // the buffer moves
      HIPCHK(h, h->rtab.tab.reserve(nb));
      const uint32_t key[3] = {l.D, fa.TB, (cb.la && !cb.Wn) ? 1u : 0u};
      if (!h->rtab.valid || memcmp(key, h->rtab.key, sizeof(key)) != 0) {
        launch_tile_tables(cb.st, key[0], key[1], (int)key[2], h->rtab.tab);
        HIPCHK(h, hipEventRecord(h->rtab.ev, cb.st));
        memcpy(h->rtab.key, key, sizeof(key));
        h->rtab.valid = true;
        h->rtab.stream = cb.st;
      } else if (cb.st != h->rtab.stream) HIPCHK(h, hipStreamWaitEvent(cb.st, h->rtab.ev, 0));
      if (h->kn.rtab) fa.rtab = h->rtab.tab;
    }
    // per-frame projections of the five sampled blocks, then the dense part + gather
    if (pframe_supported(W0))
      KT_RUN("k_pframe", cb.st, launch_pframe(cb.st, b->d_frames[0] + b->frame_off[u0] * W0, W0, nfr, h->d_lambda, l, (cb.la ? 6 : 5) * l.L, cb.P));
    else
      KT_RUN("k_scores_mfma(samples)", cb.st, launch_scores_mfma(cb.st, h->kn, b->d_frames[0] + b->frame_off[u0] * W0, W0, nullptr, nfr, h->d_lambda, l,
                         spec_samples(W0), (cb.la ? 6 : 5) * l.L, cb.P));
    if (cb.la) KT_RUN("k_avg_prefix", cb.st, launch_avg_prefix(cb.st, bv, u0, u1 - u0, l.L, cb.P));
    if (cb.Wn) {
      // decode: float arc weights + the rounding screen
      launch_state_l1(cb.st, h->d_lambda, l, h->d_w1);
      HIPCHK(h, hipMemsetAsync(cb.fix_cnt, 0, sizeof(uint32_t), cb.st));
      ScrfDecodeOut dz;
      dz.wneg = cb.Wn; dz.w1 = h->d_w1; dz.xm_f = b->d_xm_f + b->frame_off[u0];
      dz.cnt = cb.fix_cnt; dz.list = cb.fix_list; dz.cap = cb.fix_cap;
      // |fused - reference order| <= (gamma_n + gamma_m) * sum_f |x_f lambda_f|, u = 2^-53: n = nsfe + 1
      // separately rounded products added one by one; m <= 3 W + 8 roundings on any term's way through
      // the fused evaluation (MFMA accumulation of the 3W dense columns or a W-term P dot, gather and
      // epilogue adds).  1 % covers gamma's denominator and the rounding of the bound itself.
      dz.bound_scale = h->kn.decode_bound_scale * 1.01 * 0x1p-53 * (double)(l.nsfe + 1 + 3 * W0 + 8);
      PhaseTimer tk(h, PH_K_SCORE, cb.st);
      KT_RUN("k_scores_fused(decode)", cb.st, launch_scores_fused_decode(cb.st, sp, fa, l, h->d_lambda, cb.P, b->tile_off[0][u1] - b->tile_off[0][u0], dz));
      tk.stop(1);
      tm.stop(3);
      HIPCHK(h, hipGetLastError());
      return SCRF_OK;
    }
    // on the linear-domain path the epilogue already exponentiates the rows (L <= 48)
    cb.es_ready = cb.lin && sp.smax;
    {
      PhaseTimer tk(h, PH_K_SCORE, cb.st);
      KT_RUN("k_scores_fused", cb.st, launch_scores_fused(cb.st, sp, fa, l, h->d_lambda, cb.P, b->tile_off[0][u1] - b->tile_off[0][u0], cb.S,
                          cb.es_ready ? cb.smax : nullptr, cb.s_true, b->d_labels));
      tk.stop(1);
    }
    tm.stop(2);
    HIPCHK(h, hipGetLastError());
    if (!b->mixed) return SCRF_OK;
    // mixed: the transition part below (windows of the other streams, per-frame transition scores)
  }
  if (b->mode == 1) {
    PhaseTimer tm(h, PH_WIN, cb.st);
    launch_chunk_windows(h, b, u0, u1, cb.st, cb.X, cb.fused, fast, cb.hybrid);
    tm.stop(b->n_streams);
  }
  PhaseTimer tm(h, PH_SCORE, cb.st);
  uint32_t nl = 1;
  if (!cb.fused && cb.hybrid) {
    // dense statistics [avg | max | min | onehot(d)] + bias from X (3 W + D of its 8 W + D columns), the five sampled blocks
    // as per-frame projections added by row
    const uint32_t W0 = b->recipe[0].in_width;
    if (pframe_supported(W0)) KT_RUN("k_pframe", cb.st, launch_pframe(cb.st, b->d_frames[0] + b->frame_off[u0] * W0, W0, nfr, h->d_lambda, l, 5 * l.L, cb.P));
    else KT_RUN("k_scores_mfma(samples)", cb.st, launch_scores_mfma(cb.st, h->kn, b->d_frames[0] + b->frame_off[u0] * W0, W0, nullptr, nfr, h->d_lambda, l,
                                                                     spec_samples(W0), 5 * l.L, cb.P, f32));
    PhaseTimer tk(h, PH_K_SCORE, cb.st);
    KT_RUN("k_scores_mfma(state)", cb.st, launch_scores_mfma(cb.st, h->kn, cb.X, hybrid_row_floats(l, W0), nullptr, nseg, h->d_lambda, l, spec_dense_x(l, W0), l.L, cb.S, f32));
    // + the labelled windows' scores, the row maxima and exp(S - smax) for the linear-domain recursion (cb.lin)
    KT_RUN("k_add_p_exp", cb.st, launch_add_p_exp(cb.st, l, bv, b->d_frame_u, u0, nfr, cb.P, cb.S, cb.smax, cb.s_true));
    cb.es_ready = true;
    tk.stop(2);
    nl += 2;
  } else if (sparse(h)) {
    // stdsparse / stdsparsetrans: the reference's pair order in every tier (bit-identical scores), lambda index-major
    PhaseTimer tk(h, PH_K_SCORE, cb.st);
    if (!cb.lamT_ready) launch_sp_relay(cb.st, h->d_lambda, l, 0, h->d_lamT[0]);
    KT_RUN("k_sp_scores(state)", cb.st, launch_sp_scores(cb.st, cb.X, l.F, nullptr, nseg, h->d_lamT[0], l, 0, cb.S));
    tk.stop(2);
    nl += 1;
    if (l.use_tf) {
      if (!cb.lamT_ready) launch_sp_relay(cb.st, h->d_lambda, l, 1, h->d_lamT[1]);
      launch_frame_rows(cb.st, bv, u0, u1, l.D, nfr, cb.xrow_cur, 0);
      KT_RUN("k_sp_scores(trans)", cb.st, launch_sp_scores(cb.st, cb.X, l.F, cb.xrow_cur, nfr, h->d_lamT[1], l, 1, cb.M));
      nl += 3;
    }
  } else if (!cb.fused) {
    PhaseTimer tk(h, PH_K_SCORE, cb.st);
    if (fast) KT_RUN("k_scores_mfma(state)", cb.st, launch_scores_mfma(cb.st, h->kn, cb.X, l.F, nullptr, nseg, h->d_lambda, l, scrf_spec_state(l), l.L, cb.S, f32));
    else KT_RUN("k_scores_exact(state)", cb.st, launch_scores_exact(cb.st, cb.X, l.F, nullptr, nseg, h->d_lambda, l, 0, l.L, cb.S));
    tk.stop(1);
  }
  if (sparse(h)) {
    if (!l.use_tf && ensure_m0(h, cb.st)) nl += 2;   // the dense path's M0 (the bias value is 1 here)
  } else if (segtrans(h)) {
    // one transition matrix per window: the same contraction over every row of X; the rows of the
    // utterance-initial segments (no predecessor) are zeroed like the reference leaves them unused
    if (fast) KT_RUN("k_scores_mfma(trans)", cb.st, launch_scores_mfma(cb.st, h->kn, cb.X, l.F, nullptr, nseg, h->d_lambda, l, scrf_spec_trans(l), l.L * l.L, cb.M, f32));
    else KT_RUN("k_scores_exact(trans)", cb.st, launch_scores_exact(cb.st, cb.X, l.F, nullptr, nseg, h->d_lambda, l, 1, l.L * l.L, cb.M));
    launch_zero_initial_rows(cb.st, bv, b->d_frame_u, u0, nfr, l.D, l.L, cb.M);
    nl += 2;
  } else if (l.use_tf) {
    launch_frame_rows(cb.st, bv, u0, u1, l.D, nfr, cb.xrow_cur, 0);
    if (fast) KT_RUN("k_scores_mfma(trans)", cb.st, launch_scores_mfma(cb.st, h->kn, cb.X, l.F, cb.xrow_cur, nfr, h->d_lambda, l, scrf_spec_trans(l), l.L * l.L, cb.M, f32));
    else KT_RUN("k_scores_exact(trans)", cb.st, launch_scores_exact(cb.st, cb.X, l.F, cb.xrow_cur, nfr, h->d_lambda, l, 1, l.L * l.L, cb.M));
    nl += 2;
  } else if (ensure_m0(h, cb.st)) nl += 2;
  tm.stop(nl);
  HIPCHK(h, hipGetLastError());
  return SCRF_OK;
}

// the longest utterance of chunk [u0, u1): a launch of few utterances splits each into segments of frames
static uint32_t longest_utt(scrf_batch b, uint32_t u0, uint32_t u1) { return *std::max_element(b->T.begin() + u0, b->T.begin() + u1); }

// carve + scores: the head of every chunk.  SCORE_EXACT: the hooks and the decode paths (reference-order scores, sparse
// maps re-lay lambda per chunk); SCORE_PASS: a training or label-free pass (the handle's precision; the pass re-laid lambda
// once, before its first chunk)
enum ScoreMode { SCORE_EXACT, SCORE_PASS };
static bool prec_fast(scrf_handle h) { return h->cfg.train_precision >= SCRF_PREC_FAST; }
static int prec_f32(scrf_handle h) { return h->cfg.train_precision == SCRF_PREC_FAST32; }
static int score_chunk(scrf_handle h, scrf_batch b, uint32_t u0, uint32_t u1, const Need& nd, ChunkBufs* cb, ScoreMode mode = SCORE_EXACT, int lane = 0) {
  RCCHK(carve(h, b, u0, u1, nd, cb, lane));
  if (mode == SCORE_EXACT) return run_scores(h, b, u0, u1, *cb);
  cb->lamT_ready = sparse(h);
  return run_scores(h, b, u0, u1, *cb, prec_fast(h), prec_f32(h));
}

// Where a chunk of the training pass runs (fb_route): its lane; whether it is the batch's last; whether the transition block
// is counted first and all-reduced early, under the state contraction (overlap); whether the engine's second stream takes
// the recursion's check kernels, the status copy, k_ztf and k_atb (side).
struct FbRoute { int lane = 0; bool two_lanes = false, last = false, overlap = false, side = false; };

// What a caller wants of run_dp.  The hooks take the default: the log-domain node values of the chunk.
struct DpOpts {
  bool post = false;    // + posteriors, numerators and xi: leaves R = Y - gamma in cb.R
  bool ponly = false;   // the recursion alone: the caller's posterior-output kernels take it from there
  FbRoute route;        // training pass: side sends the linear-domain path's check kernels to the second stream
  // Launches that read the chunk's scores beside the pass (scrf_fb_transcript_batch's numerators).  run_dp queues them at the
  // last point at which the scores exist: on the linear-domain path between the recursion and the posterior walk, which
  // overwrites them with R (dp_wave_lin); on every other path, where S stays beside R = AD, behind the recursion's launches.
  std::function<int()> reads_scores;
  static DpOpts training(const FbRoute& rt) { DpOpts o; o.post = true; o.route = rt; return o; }
  static DpOpts recursion_only() { DpOpts o; o.ponly = true; return o; }
};

// (only the posterior-mass self-checks look at it in the recursion kernels)
static int frame_mass_model(scrf_handle h) { return h->cfg.model_type == SCRF_STDFRAME || h->frame_mass; }

static int queue_status(scrf_handle h, scrf_batch b, hipStream_t st);

// STDSEG_NO_DUR: one transition matrix per window, its own workgroup recursion
static int dp_segtrans(scrf_handle h, scrf_batch b, uint32_t u0, uint32_t u1, ChunkBufs& cb, bool post, uint32_t* nl) {
  const ScrfLayout& l = h->lay;
  if (fb_segtrans_smem_bytes(dp_shape(l), fb_block_threads(dp_shape(l))) > SCRF_LDS_BYTES)
    return fail(h, SCRF_ERR_INVALID, "labels x maximum duration = %u x %u is too large for the stdseg_no_dur recursion "
                "(its three [D][L] rings must fit 160 KB of LDS)", l.L, l.D);
  KT_RUN("k_fb_segtrans", cb.st, launch_fb_segtrans(cb.st, h->kn, l, b->view(), u0, u1 - u0, b->d_prev_lab, cb.S, cb.M, cb.AD, cb.alpha, cb.beta,
                     post ? cb.XI : nullptr, b->d_numer, b->d_zx, b->d_status, post ? 1 : 0));
  *nl += 1;
  return SCRF_OK;
}

// the workgroup-per-utterance kernel: column-wise max-shifted log-sum-exp like the reference's LogMath
static int dp_group(scrf_handle h, scrf_batch b, uint32_t u0, uint32_t u1, ChunkBufs& cb, bool post, uint32_t* nl) {
  const ScrfLayout& l = h->lay;
  const uint32_t nutt = u1 - u0;
  if (fb_smem_bytes(dp_shape(l), fb_block_threads(dp_shape(l))) > SCRF_LDS_BYTES)
    return fail(h, SCRF_ERR_INVALID, "labels x maximum duration = %u x %u is too large for the workgroup-per-utterance recursion "
                "(its two [D][L] rings must fit 160 KB of LDS; the wavefront kernels cover L <= 256 with D <= 40)", l.L, l.D);
  if (post && cb.xi_acc) HIPCHK(h, hipMemsetAsync(cb.xi_acc, 0, sizeof(double) * nutt * l.L * l.L, cb.st));
  KT_RUN("k_fb", cb.st, launch_fb(cb.st, l, b->view(), u0, nutt, cb.S, cb.M, cb.m_per_frame, cb.AD, cb.alpha, cb.beta, post ? cb.XI : nullptr,
            post ? cb.xi_acc : nullptr, b->d_numer, b->d_zx, b->d_status, post ? 1 : 0, frame_mass_model(h)));
  *nl += 1;
  return SCRF_OK;
}

// Behind the posterior walk of either wavefront recursion: the reference's posterior-mass self-checks (computeExpF :917-947),
// the numerators and the xi factors on `ck`, then -- with transition features -- the full xi on the chunk's stream.  The two
// recursions check different vectors and form their factors with different kernels: each passes its own launches.
template <class MassCheck, class XiFactors>
static uint32_t post_tail(scrf_handle h, scrf_batch b, uint32_t u0, uint32_t u1, ChunkBufs& cb, hipStream_t ck, MassCheck mass_check,
                          XiFactors xi_factors) {
  const ScrfLayout& l = h->lay;
  const uint64_t nfr = b->frame_off[u1] - b->frame_off[u0];
  KT_RUN("k_mass_check", ck, mass_check());
  KT_RUN("k_numer_reduce", ck, launch_numer_reduce(ck, b->view(), u0, u1 - u0, cb.numer_f, b->d_numer));
  xi_factors();
  if (!l.use_tf) return 3;
  KT_RUN("k_xi_full", cb.st, launch_xi_full(cb.st, l, b->view(), u0, u1, nfr, b->d_next_lab, cb.fA, cb.fB, cb.E, cb.msh, cb.XI));
  return 4;
}

// the scaled linear-domain wavefront recursion (training and label-free passes)
static int dp_wave_lin(scrf_handle h, scrf_batch b, uint32_t u0, uint32_t u1, ChunkBufs& cb, const DpOpts& o, uint32_t* nl) {
  const ScrfLayout& l = h->lay;
  const uint32_t nutt = u1 - u0;
  const uint64_t nfr = b->frame_off[u1] - b->frame_off[u0], nseg = b->seg_off[u1] - b->seg_off[u0];
  ScrfBatchView bv = b->view();
  if (!cb.es_ready) {
    if (!o.ponly) KT_RUN("k_true_scores", cb.st, launch_true_scores(cb.st, l, bv, b->d_frame_u, u0, nfr, cb.S, cb.s_true));
    KT_RUN("k_exp_rows", cb.st, launch_exp_rows(cb.st, cb.S, nseg, l.L, cb.smax));
    *nl += o.ponly ? 1 : 2;
  }
  {
    PhaseTimer tk(h, PH_K_DP, cb.st);
    KT_RUN(l.L > 64 ? "k_dp_lin_mw" : "k_dp_lin", cb.st, launch_dp_lin(cb.st, h->kn, l, bv, u0, nutt, cb.S, cb.smax, cb.E, cb.ET, cb.msh, cb.m_per_frame, cb.dl,
                    b->d_zx, b->d_status));
    tk.stop(1);
  }
  *nl += 1;
  if (o.ponly) return SCRF_OK;
  if (o.reads_scores) RCCHK(o.reads_scores());   // the walk below overwrites the scores
  if (cb.fused) {
    // posterior pass and the per-frame sums of R in one walk (R is not read back for Z)
    if (l.L > 64) HIPCHK(h, hipMemsetAsync(cb.mass_s, 0, sizeof(double) * nfr, cb.st));   // summed over the 64-output groups
    const uint32_t t_max = longest_utt(b, u0, u1);
    KT_RUN("k_post_z", cb.st, launch_post_z(cb.st, h->kn, l, bv, u0, nutt, b->d_next_lab, cb.s_true, cb.M, cb.m_per_frame, cb.S, cb.smax,
                  cb.dl, b->d_zx, cb.numer_f, b->d_status, cb.Z, cb.mass_s, cb.la ? 1 : 0, t_max, nfr));
    cb.z_ready = true;
  } else {
    KT_RUN("k_post_lin", cb.st, launch_post_lin(cb.st, l, bv, b->d_frame_u, u0, nfr, b->d_next_lab, cb.s_true, cb.M, cb.m_per_frame, cb.S,
                    cb.smax, cb.dl, b->d_zx, cb.numer_f, b->d_status, cb.mass_s));
  }
  // Nothing the count kernel reads comes from the check kernels (it takes R, the frames and the tile list): on a side
  // route they leave the main stream, which goes from the posterior walk straight to the count kernel.  The second stream
  // keeps their order, and what they write is read behind the join of the count phase (k_batch_sums: d_numer; k_commit:
  // the latch) or by that stream's own k_atb (the rescaled gsd).
  hipStream_t ck = cb.st;
  if (o.route.side) {
    HIPCHK(h, hipEventRecord(h->ev_fork, cb.st));
    HIPCHK(h, hipStreamWaitEvent(h->stream2, h->ev_fork, 0));
    ck = h->stream2;
  }
  *nl += 1 + post_tail(h, b, u0, u1, cb, ck,
      [&] {   // before sd / gsd are rescaled below
        launch_mass_check(ck, bv, b->d_frame_u, u0, nfr, l.L, frame_mass_model(h), 1, cb.dl.a, cb.dl.ga, cb.dl.b, cb.dl.gb, b->d_zx, cb.mass_s, b->d_status);
      },
      [&] {   // with transition features the rescaled sd rows are needed as an array; with bias-only transitions only their
              // per-frame factor is, applied inside the A^T B contraction
        if (l.use_tf) KT_RUN("k_xi_lin", ck, launch_xi_lin(ck, l, bv, b->d_frame_u, u0, nfr, cb.dl, b->d_zx));
        else KT_RUN("k_xi_scale", ck, launch_xi_scale(ck, bv, b->d_frame_u, u0, nfr, cb.dl, b->d_zx));
      });
  // every status of the batch is final behind the last chunk's k_mass_check (a side route has no transition features: no k_xi_full)
  if (o.route.side && o.route.last) return queue_status(h, b, ck);
  return SCRF_OK;
}

// the log-domain wavefront recursion (hooks, SCRF_PREC_EXACT passes, training without the linear-domain kernels)
static int dp_wave_log(scrf_handle h, scrf_batch b, uint32_t u0, uint32_t u1, ChunkBufs& cb, bool post, uint32_t* nl) {
  const ScrfLayout& l = h->lay;
  const uint32_t nutt = u1 - u0;
  const uint64_t nfr = b->frame_off[u1] - b->frame_off[u0];
  ScrfBatchView bv = b->view();
  {
    PhaseTimer tk(h, PH_K_DP, cb.st);
    KT_RUN("k_dp_wave", cb.st, launch_dp_wave(cb.st, l, bv, u0, nutt, cb.S, cb.E, cb.ET, cb.msh, cb.m_per_frame, cb.AD, cb.alpha,
                   cb.beta, cb.sd, b->d_zx, b->d_status));
    tk.stop(1);
  }
  *nl += 1;
  if (!post) return SCRF_OK;
  KT_RUN("k_post_state", cb.st, launch_post_state(cb.st, l, bv, u0, u1, nfr, b->d_next_lab, cb.S, cb.M, cb.m_per_frame, cb.AD, cb.beta,
                    b->d_zx, cb.numer_f, b->d_status, cb.mass_s));
  *nl += 1 + post_tail(h, b, u0, u1, cb, cb.st,
      [&] { launch_mass_check(cb.st, bv, b->d_frame_u, u0, nfr, l.L, frame_mass_model(h), 0, cb.alpha, nullptr, cb.beta, nullptr, b->d_zx, cb.mass_s, b->d_status); },
      [&] { KT_RUN("k_xi_factors", cb.st, launch_xi_factors(cb.st, l, bv, u0, u1, nfr, cb.alpha, cb.sd, b->d_zx, cb.fA, cb.fB)); });
  return SCRF_OK;
}

// forward + backward (+ posteriors with o.post) of chunk [u0, u1) by the recursion its carve chose: wavefront-per-utterance
// kernels for L <= 64 (and the multi-wavefront linear-domain one up to 256), the workgroup-per-utterance kernel otherwise.
// Leaves R = Y - gamma in cb.R (post) or alpha-with-duration in cb.AD (no post), alpha in cb.alpha, beta in cb.beta (wave
// path or nd.beta).  *nl_out: the launches queued.
static int run_dp(scrf_handle h, scrf_batch b, uint32_t u0, uint32_t u1, ChunkBufs& cb, const DpOpts& o, uint32_t* nl_out) {
  uint32_t nl = 0;
  if (segtrans(h)) RCCHK(dp_segtrans(h, b, u0, u1, cb, o.post, &nl));
  else if (!cb.wave) RCCHK(dp_group(h, b, u0, u1, cb, o.post, &nl));
  else {
    if (cb.m_per_frame) {
      KT_RUN("k_exp_m", cb.st, launch_exp_m(cb.st, h->kn, cb.M, h->lay.L, b->frame_off[u1] - b->frame_off[u0], cb.E, cb.ET, cb.msh));
      nl++;
    }
    RCCHK(cb.lin ? dp_wave_lin(h, b, u0, u1, cb, o, &nl) : dp_wave_log(h, b, u0, u1, cb, o.post, &nl));
  }
  if (o.reads_scores && !cb.lin) RCCHK(o.reads_scores());   // cb.lin: dp_wave_lin has queued them before its posterior walk
  if (nl_out) *nl_out = nl;
  HIPCHK(h, hipGetLastError());
  return SCRF_OK;
}

// ---------------------------------------------------------------------------------------------
// status of a batch: first failed utterance -> {code, utterance} (d_latch), copied to pinned host memory;
// the commit of the staged gradient is a no-op when the latch is set
// ---------------------------------------------------------------------------------------------
// latch[0]: non-zero iff an utterance failed (what k_commit tests); latch[1]: min over the failed utterances of
// (utterance << 8 | code), so the LOWEST failing utterance is the one reported, whichever thread gets there first --
// the order in which the reference's per-utterance loop would have thrown.  latch_reset arms it.
#define SCRF_LATCH_IDLE 0x7fffffff
__global__ void k_latch_status(const int* __restrict__ status, uint32_t n, int* __restrict__ latch) {
  const uint32_t u = blockIdx.x * blockDim.x + threadIdx.x;
  if (u >= n) return;
  const int s = status[u];
  if (s != 0) {
    atomicMin(&latch[1], (int)((u << 8) | ((uint32_t)s & 0xffu)));
    atomicOr(&latch[0], 1);
  }
}
__global__ void k_latch_reset(int* __restrict__ latch) {
  latch[0] = 0;
  latch[1] = SCRF_LATCH_IDLE;
}
// arms the latch on the engine stream, at the head of a pass (training or label-free)
static void latch_reset(scrf_handle h) { hipLaunchKernelGGL(k_latch_reset, dim3(1), dim3(1), 0, h->stream, h->d_latch.get()); }
// {code, utterance} from the pinned copy of the latch
static void latch_decode(const int* h_latch, int out[2]) {
  out[0] = out[1] = 0;
  if (h_latch[0] != 0 && h_latch[1] != SCRF_LATCH_IDLE) {
    out[0] = h_latch[1] & 0xff;
    out[1] = (int)((uint32_t)h_latch[1] >> 8);
  }
}
__global__ void k_commit(double* __restrict__ grad, const double* __restrict__ stage, uint32_t n,
                         double* __restrict__ sums, const double* __restrict__ sums_stage,
                         const int* __restrict__ latch) {
  if (latch[0] != 0) return;   // a failed batch contributes nothing
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) grad[i] += stage[i];
  if (i < 3) sums[i] += sums_stage[i];
}

// the same for one block of the weight vector: part 1 = the transition weights of every label ([nsf, stride) of its
// block), part 0 = the state weights ([0, nsf)) and the batch sums
__global__ void k_commit_part(double* __restrict__ grad, const double* __restrict__ stage, uint32_t n, uint32_t stride, uint32_t nsf,
                              int part, double* __restrict__ sums, const double* __restrict__ sums_stage,
                              const int* __restrict__ latch) {
  if (latch[0] != 0) return;
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n && ((i % stride >= nsf) ? 1 : 0) == part) grad[i] += stage[i];
  if (part == 0 && i < 3) sums[i] += sums_stage[i];
}

static const char* status_text(int code) {
  return code == SCRF_ERR_BAD_LABEL ? "the label is larger than nActualLabs*labMaxDur"
         : code == SCRF_ERR_EMPTY   ? "No features read from this sentence."
                                    : "overflow / NaN / log of zero in the recursion, or posterior-mass check failed";
}

static int queue_status(scrf_handle h, scrf_batch b, hipStream_t st) {
  hipLaunchKernelGGL(k_latch_status, dim3((b->U + 255) / 256), dim3(256), 0, st, b->d_status, b->U, h->d_latch);
  HIPCHK(h, hipMemcpyAsync(h->h_latch, h->d_latch, sizeof(int) * 2, hipMemcpyDeviceToHost, st));
  HIPCHK(h, hipEventRecord(h->ev_status, st));
  return SCRF_OK;
}
static int queue_status(scrf_handle h, scrf_batch b) { return queue_status(h, b, h->stream); }

// ---------------------------------------------------------------------------------------------
// STDSEG (duration-labelled, scrf_stdseg.hip): its own small pipeline -- windows, scores, workgroup recursion,
// posteriors, per-weight gradient -- in chunks of utterances that fit the scratch budget.  h->lay is the layout over
// the FULL labels (lay.L = nLabs); La = nActualLabs.
// ---------------------------------------------------------------------------------------------
static bool stdseg(scrf_handle h) { return h->cfg.model_type == SCRF_STDSEG; }
static uint32_t stdseg_La(scrf_handle h) { return h->lay.L / h->lay.D; }

// The small pipelines (STDSEG log-domain, STDSEG linear-domain, n-state) each have a layout function: one walk over an Arena
// for sizing and carving, like chunk_layout.  What differs between them besides the layout is carried here, as it has always
// been (tests/test_gpu_chunk_plan.py pins every cut): the bytes of slack a chunk's size adds and the most utterances a chunk
// may hold (0: no cap).
template <class Bufs>
struct SmallPipe {
  void (*layout)(scrf_handle, scrf_batch, uint32_t, uint32_t, bool, Arena&, Bufs*);
  size_t slack;
  uint32_t max_utts;
  size_t chunk_size(scrf_handle h, scrf_batch b, uint32_t u0, uint32_t u1, bool post) const {
    Arena m{nullptr, 0, 0};
    Bufs sb;
    layout(h, b, u0, u1, post, m, &sb);
    return m.off + slack;
  }
  // carves the chunk on the engine's scratch and queues its window vectors (batches made from frames)
  int begin_chunk(scrf_handle h, scrf_batch b, uint32_t u0, uint32_t u1, bool post, Bufs* sb) const {
    RCCHK(ensure_scratch(h, chunk_size(h, b, u0, u1, post)));
    Arena a{h->scratch[0], h->scratch[0].cap(), 0};
    layout(h, b, u0, u1, post, a, sb);
    if (a.off > a.cap) return fail(h, SCRF_ERR_INVALID, "internal: scratch arena overflow");
    if (b->mode == 1) launch_chunk_windows(h, b, u0, u1, h->stream, sb->X);
    return SCRF_OK;
  }
  // largest u1 > u0 whose chunk fits the budget (always at least one utterance)
  uint32_t plan(scrf_handle h, scrf_batch b, uint32_t u0, bool post) const {
    uint32_t u1 = u0 + 1;
    while (u1 < b->U && (!max_utts || u1 - u0 < max_utts) && chunk_size(h, b, u0, u1 + 1, post) <= h->cfg.scratch_bytes) u1++;
    return u1;
  }
};

struct StdsegBufs {
  float* X; uint32_t *row_t, *row_d, *row_u;
  double *S, *MX, *alpha, *beta, *G, *XI, *mass_s, *mass_t;
};
// scratch layout of a chunk (one walk for sizing and carving, like chunk_layout)
static void stdseg_layout(scrf_handle h, scrf_batch b, uint32_t u0, uint32_t u1, bool post, Arena& a, StdsegBufs* sb) {
  const ScrfLayout& l = h->lay;
  const uint32_t La = stdseg_La(h);
  const uint64_t nfr = b->frame_off[u1] - b->frame_off[u0], nseg = b->seg_off[u1] - b->seg_off[u0];
  memset(sb, 0, sizeof(*sb));
  sb->X = b->mode == 1 ? a.take<float>(nseg * l.F) : b->d_windows + b->seg_off[u0] * l.F;
  sb->row_t = a.take<uint32_t>(nseg); sb->row_d = a.take<uint32_t>(nseg); sb->row_u = a.take<uint32_t>(nseg);
  sb->S = a.take<double>(nseg * La); sb->alpha = a.take<double>(nseg * La); sb->beta = a.take<double>(nseg * La);
  sb->MX = a.take<double>(nseg * (size_t)l.L * La);
  if (post) {
    sb->G = a.take<double>(nseg * La); sb->XI = a.take<double>(nseg * (size_t)l.L * La);
    sb->mass_s = a.take<double>(nfr); sb->mass_t = a.take<double>(nfr);
  }
}
static const SmallPipe<StdsegBufs> stdseg_pipe = {stdseg_layout, 0, 0};   // no slack, no cap
// ---- STDSEG, bias-only transitions, FAST precisions, training path: scrf_stdseg_lin.hip (not during a log-domain redo,
// force_fb: that one runs k_stdseg_fb, the reference's order)
static bool stdseg_lin(scrf_handle h) {
  return h->kn.stdseg_lin && !h->force_fb && h->cfg.train_precision != SCRF_PREC_EXACT && h->lay.use_sf && stdseg_lin_supported(dp_shape(h->lay), stdseg_La(h));
}
static uint64_t sl_rows_per_chunk(uint64_t nfr) {   // K-chunks of the count contractions: <= 256 of them, multiples of 32 frames
  uint64_t rpc = ((nfr + 255) / 256 + 31) & ~31ull;
  return rpc < 64 ? 64 : rpc;
}
struct StdsegLinBufs {
  float* X; uint64_t* xrow;
  double *Sd, *Ad, *Bd, *Rd, *Bp, *Am, *ga, *numer_f;
  double *slab_s, *slab_t, *obs;   // state-count slabs (one duration at a time), transition slabs, observed transitions
  uint64_t rpc; uint32_t nch;
};
static void stdseg_lin_layout(scrf_handle h, scrf_batch b, uint32_t u0, uint32_t u1, bool /*post: always*/, Arena& a, StdsegLinBufs* sb) {
  const ScrfLayout& l = h->lay;
  const uint32_t La = stdseg_La(h);
  const uint64_t nfr = b->frame_off[u1] - b->frame_off[u0], nseg = b->seg_off[u1] - b->seg_off[u0];
  const size_t nn = (size_t)l.D * nfr * La;
  sb->X = b->mode == 1 ? a.take<float>(nseg * l.F) : b->d_windows + b->seg_off[u0] * l.F;
  sb->xrow = a.take<uint64_t>((size_t)l.D * nfr);
  sb->Sd = a.take<double>(nn); sb->Ad = a.take<double>(nn); sb->Bd = a.take<double>(nn);
  sb->Rd = a.take<double>(nn); sb->Bp = a.take<double>(nn);
  sb->Am = a.take<double>(nfr * (size_t)l.L);
  sb->ga = a.take<double>(nfr); sb->numer_f = a.take<double>(nfr);
  sb->rpc = sl_rows_per_chunk(nfr);
  sb->nch = (uint32_t)((nfr + sb->rpc - 1) / sb->rpc);
  sb->slab_s = a.take<double>((size_t)sb->nch * La * l.nsf);
  sb->slab_t = a.take<double>((size_t)sb->nch * l.L * l.L);
  sb->obs = a.take<double>((size_t)l.L * l.L);
}
static const SmallPipe<StdsegLinBufs> stdseg_lin_pipe = {stdseg_lin_layout, 4096, 32767};   // 4 KB of slack, at most 32,767 utterances
static int stdseg_lin_run_chunk(scrf_handle h, scrf_batch b, uint32_t u0, uint32_t u1, double* grad) {
  const ScrfLayout& l = h->lay;
  const uint32_t La = stdseg_La(h);
  const uint64_t nfr = b->frame_off[u1] - b->frame_off[u0];
  StdsegLinBufs sb;
  RCCHK(stdseg_lin_pipe.begin_chunk(h, b, u0, u1, true, &sb));
  ScrfBatchView bv = b->view();
  hipStream_t st = h->stream;
  const int f32 = h->cfg.train_precision == SCRF_PREC_FAST32;
  // the transition table and its exponential (once per call: lambda may have changed)
  double* E = h->d_sl_tab; double* ET = E + (size_t)l.L * l.L; double* mmax = ET + (size_t)l.L * l.L;
  launch_sl_tables(st, l, h->d_lambda, E, ET, mmax);
  launch_sl_rows(st, bv, b->d_frame_u, u0, nfr, l.D, sb.xrow);
  {
    KernelTimer kt(h, "k_scores_mfma(state, per duration)", st);
    for (uint32_t d0 = 0; d0 < l.D; d0++) {
      const ScrfGemmSpec sp{0, l.sfs, l.nsfe, (uint32_t)l.use_sb, l.sbv, d0 * La * l.stride, 0};
      launch_scores_mfma(st, h->kn, sb.X, l.F, sb.xrow + (size_t)d0 * nfr, nfr, h->d_lambda, l, sp, La, sb.Sd + (size_t)d0 * nfr * La, f32);
    }
    kt.stop(l.D);
  }
  KT_RUN("k_sl_fb", st, launch_sl_fb(st, l, La, bv, u0, u1 - u0, nfr, sb.Sd, E, ET, mmax, sb.Ad, sb.Bd, sb.Am, sb.ga, b->d_zx, b->d_status));
  KT_RUN("k_sl_post", st, launch_sl_post(st, l, La, bv, b->d_frame_u, u0, u1 - u0, nfr, b->d_prev_lab, h->d_lambda, sb.Sd, sb.Ad, sb.Bd, sb.ga, b->d_zx,
                                         sb.Rd, sb.Bp, sb.numer_f, b->d_numer, b->d_status));
  {
    KernelTimer kt(h, "k_expf_mfma(state, per duration)", st);
    for (uint32_t d0 = 0; d0 < l.D; d0++) {
      const ScrfGemmSpec sp{0, l.sfs, l.nsfe, (uint32_t)l.use_sb, l.sbv, d0 * La * l.stride, 0};
      launch_expf_mfma(st, h->kn, sb.Rd + (size_t)d0 * nfr * La, La, sb.X, l.F, sb.xrow + (size_t)d0 * nfr, nfr, l, sp, sb.rpc, sb.nch, sb.slab_s, f32);
      launch_reduce_slabs(st, sb.slab_s, sb.nch, La, l, sp, grad);
    }
    kt.stop(2 * l.D);
  }
  HIPCHK(h, hipMemsetAsync(sb.obs, 0, sizeof(double) * l.L * l.L, st));
  KT_RUN("k_sl_atb", st, launch_sl_trans_counts(st, l, La, bv, b->d_frame_u, u0, nfr, b->d_prev_lab, sb.rpc, sb.nch, sb.Am, sb.Bp, E, mmax, sb.slab_t,
                                                sb.obs, grad));
  HIPCHK(h, hipGetLastError());
  return SCRF_OK;
}

// chunk [u0, u1): scores and recursion (and, with post, posteriors, numerators, the gradient into `grad`)
static int stdseg_run_chunk(scrf_handle h, scrf_batch b, uint32_t u0, uint32_t u1, bool post, double* grad, StdsegBufs* out) {
  if (post && !out && stdseg_lin(h)) return stdseg_lin_run_chunk(h, b, u0, u1, grad);
  const ScrfLayout& l = h->lay;
  const uint32_t La = stdseg_La(h);
  const uint64_t nfr = b->frame_off[u1] - b->frame_off[u0], nseg = b->seg_off[u1] - b->seg_off[u0];
  StdsegBufs sb;
  RCCHK(stdseg_pipe.begin_chunk(h, b, u0, u1, post, &sb));
  ScrfBatchView bv = b->view();
  hipStream_t st = h->stream;
  launch_stdseg_rowinfo(st, bv, b->d_frame_u, u0, nfr, l.D, sb.row_t, sb.row_d, sb.row_u);
  KT_RUN("k_stdseg_scores", st, launch_stdseg_scores(st, l, La, sb.X, nseg, sb.row_t, sb.row_d, h->d_lambda, sb.S, sb.MX));
  KT_RUN("k_stdseg_fb", st, launch_stdseg_fb(st, l, La, bv, u0, u1 - u0, sb.S, sb.MX, sb.alpha, sb.beta, b->d_zx, b->d_status));
  if (post) {
    HIPCHK(h, hipMemsetAsync(sb.mass_s, 0, sizeof(double) * nfr, st));
    HIPCHK(h, hipMemsetAsync(sb.mass_t, 0, sizeof(double) * nfr, st));
    KT_RUN("k_stdseg_post", st, launch_stdseg_post(st, l, La, bv, u0, u1 - u0, nseg, sb.row_t, sb.row_d, sb.row_u, b->d_prev_lab, sb.S, sb.MX, sb.alpha, sb.beta,
                                                   b->d_zx, sb.G, sb.XI, sb.mass_s, sb.mass_t, b->d_numer, b->d_status));
    KT_RUN("k_stdseg_expf", st, launch_stdseg_expf(st, l, La, bv, u0, u1 - u0, nseg, sb.row_t, sb.row_d, sb.row_u, b->d_prev_lab, sb.X, sb.G, sb.XI, grad));
  }
  HIPCHK(h, hipGetLastError());
  if (out) *out = sb;
  return SCRF_OK;
}

// ---------------------------------------------------------------------------------------------
// n-state frame model (crf_states > 1, scrf_nstate.hip): the same small pipeline shape as STDSEG
// ---------------------------------------------------------------------------------------------
static bool nstate(scrf_handle h) { return h->lay.K > 1; }
struct NstateBufs {
  float* X;
  double *S, *TD, *TO, *TE, *alpha, *beta, *G, *XD, *XO, *XE, *mass_s, *mass_t;
  double* slab;   // the gradient's frame-slice partials
};
static void nstate_layout(scrf_handle h, scrf_batch b, uint32_t u0, uint32_t u1, bool post, Arena& a, NstateBufs* nb) {
  const ScrfLayout& l = h->lay;
  const uint64_t P = l.L / l.K;
  const uint64_t nfr = b->frame_off[u1] - b->frame_off[u0];
  memset(nb, 0, sizeof(*nb));
  nb->X = b->mode == 1 ? a.take<float>(nfr * l.F) : b->d_windows + b->seg_off[u0] * l.F;
  nb->S = a.take<double>(nfr * l.L); nb->TD = a.take<double>(nfr * l.L); nb->TO = a.take<double>(nfr * l.L);
  nb->alpha = a.take<double>(nfr * l.L); nb->beta = a.take<double>(nfr * l.L);
  nb->TE = a.take<double>(nfr * P * P);
  if (post) {
    nb->G = a.take<double>(nfr * l.L); nb->XD = a.take<double>(nfr * l.L); nb->XO = a.take<double>(nfr * l.L);
    nb->XE = a.take<double>(nfr * P * P);
    nb->mass_s = a.take<double>(nfr); nb->mass_t = a.take<double>(nfr);
    nb->slab = a.take<double>((size_t)ns_expf_slices(nfr) * l.lambda_len);
  }
}
static const SmallPipe<NstateBufs> nstate_pipe = {nstate_layout, 0, 0};   // no slack, no cap
static int nstate_run_chunk(scrf_handle h, scrf_batch b, uint32_t u0, uint32_t u1, bool post, double* grad, NstateBufs* out) {
  const ScrfLayout& l = h->lay;
  const uint64_t nfr = b->frame_off[u1] - b->frame_off[u0];
  NstateBufs nb;
  RCCHK(nstate_pipe.begin_chunk(h, b, u0, u1, post, &nb));
  ScrfBatchView bv = b->view();
  hipStream_t st = h->stream;
  KT_RUN("k_ns_scores", st, launch_ns_scores(st, l, nb.X, nfr, h->d_lambda, nb.S, nb.TD, nb.TO, nb.TE));
  KT_RUN("k_ns_fb", st, launch_ns_fb(st, l, bv, u0, u1 - u0, nb.S, nb.TD, nb.TO, nb.TE, nb.alpha, nb.beta, b->d_zx, b->d_status));
  if (post) {
    HIPCHK(h, hipMemsetAsync(nb.mass_s, 0, sizeof(double) * nfr, st));
    HIPCHK(h, hipMemsetAsync(nb.mass_t, 0, sizeof(double) * nfr, st));
    KT_RUN("k_ns_post", st, launch_ns_post(st, l, bv, b->d_frame_u, u0, u1 - u0, nfr, nb.S, nb.TD, nb.TO, nb.TE, nb.alpha, nb.beta, b->d_zx, nb.G, nb.XD, nb.XO,
                                           nb.XE, nb.mass_s, nb.mass_t, b->d_numer, b->d_status));
    KT_RUN("k_ns_expf", st, launch_ns_expf(st, l, bv, b->d_frame_u, u0, nfr, nb.X, nb.G, nb.XD, nb.XO, nb.XE, nb.slab, grad));
  }
  HIPCHK(h, hipGetLastError());
  if (out) *out = nb;
  return SCRF_OK;
}
// the next chunk of the small pipeline this model and pass run
static uint32_t small_plan_chunk(scrf_handle h, scrf_batch b, uint32_t u0, bool post) {
  if (nstate(h)) return nstate_pipe.plan(h, b, u0, post);
  if (post && stdseg_lin(h)) return stdseg_lin_pipe.plan(h, b, u0, post);
  return stdseg_pipe.plan(h, b, u0, post);
}

// The form a batch's training and posterior passes take, by ingredient (scrf_batch_is_fused reports them as they are):
// fusable: window synthesis inside the fused kernels (a training pass also needs a FAST precision for it); hybrid: materialised
// dense statistics, sampled blocks through the per-frame projections; la: SCRF_PREC_FASTLIN on a shape whose kernels take the
// linear window average -- it needs the fused kernels and the linear-domain recursion (k_post_z builds Z_avg), anything else
// runs as FAST.  wave_path is false during a log-domain redo (force_fb), which therefore runs neither hybrid nor la.
struct BatchForm { bool fusable, hybrid, la; };
static BatchForm batch_form(scrf_handle h, scrf_batch b) {
  const uint32_t prec = h->cfg.train_precision;
  BatchForm f;
  f.fusable = b->fused_ok && h->kn.fuse;
  f.hybrid = !f.fusable && b->hybrid_ok && h->kn.hybrid_on() && h->kn.fuse && prec >= SCRF_PREC_FAST && prec != SCRF_PREC_FAST32 && h->kn.lindp &&
             wave_path(h, true);
  f.la = prec == SCRF_PREC_FASTLIN && h->kn.lindp && wave_path(h, true) && fused_la_supported(h->kn, fused_shape(h->lay), b->recipe[0].in_width);
  return f;
}
static void set_batch_form(scrf_handle h, scrf_batch b, Need* nd) {
  const BatchForm f = batch_form(h, b);
  nd->fused = f.fusable && h->cfg.train_precision >= SCRF_PREC_FAST;
  nd->hybrid = f.hybrid;
  nd->la = nd->fused && f.la;
}

// ---------------------------------------------------------------------------------------------
// the training pass (scrf_fb_batch): one pass of the forward-backward pipeline over the batch into the staging gradient,
// in phases -- fb_begin, then per chunk (fb_chunk) scores, recursion, counts and their reductions, then fb_commit
// ---------------------------------------------------------------------------------------------
static int allreduce_block(scrf_handle h, hipStream_t st, int part);
static bool two_block_reduce(scrf_handle h) { return h->comm && h->lay.use_tf && h->cfg.model_type != SCRF_STDSEG_NO_DUR && h->cfg.model_type != SCRF_STDSEG && h->lay.K <= 1 && !h->shadow; }

// arms the status latch and clears the staging gradient and sums
static int fb_begin(scrf_handle h, scrf_batch b) {
  HIPCHK(h, hipMemsetAsync(b->d_status, 0, sizeof(int) * b->U, h->stream));
  latch_reset(h);
  HIPCHK(h, hipMemsetAsync(h->d_stage, 0, sizeof(double) * h->lay.lambda_len, h->stream));
  HIPCHK(h, hipMemsetAsync(h->d_sums_stage, 0, sizeof(double) * 4, h->stream));
  return SCRF_OK;
}

// the staged gradient into the engine's (a no-op on a latched batch): all of it, or one block of the weight vector
// (k_commit_part: 1 = the transition weights, 0 = the state weights and the batch sums)
enum { COMMIT_STATE = 0, COMMIT_TRANS = 1, COMMIT_ALL = 2 };
static void commit_staged(scrf_handle h, int part) {
  const ScrfLayout& l = h->lay;
  const dim3 grid((l.lambda_len + 255) / 256), block(256);
  if (part == COMMIT_ALL)
    hipLaunchKernelGGL(k_commit, grid, block, 0, h->stream, h->d_grad, h->d_stage, l.lambda_len, h->d_sums, h->d_sums_stage, h->d_latch);
  else
    hipLaunchKernelGGL(k_commit_part, grid, block, 0, h->stream, h->d_grad, h->d_stage, l.lambda_len, l.stride, l.nsf, part, h->d_sums,
                       h->d_sums_stage, h->d_latch);
}

// commits what the early all-reduce has not, and waits for the batch's status: latch[2] receives {status code, utterance} of
// the first failed utterance (0 = clean, gradient committed)
static int fb_commit(scrf_handle h, int latch[2]) {
  commit_staged(h, h->early_done ? COMMIT_STATE : COMMIT_ALL);   // early_done: the transition block was committed (and sent) already
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipEventSynchronize(h->ev_status));
  latch_decode(h->h_latch, latch);
  return SCRF_OK;
}

// STDSEG and the n-state frame model: their own small pipelines, chunk by chunk on the engine stream
static int fb_run_small(scrf_handle h, scrf_batch b, int latch[2]) {
  RCCHK(fb_begin(h, b));
  for (uint32_t u0 = 0; u0 < b->U;) {
    const uint32_t u1 = small_plan_chunk(h, b, u0, true);
    RCCHK(nstate(h) ? nstate_run_chunk(h, b, u0, u1, true, h->d_stage, nullptr) : stdseg_run_chunk(h, b, u0, u1, true, h->d_stage, nullptr));
    launch_stdseg_sums(h->stream, b->d_numer, b->d_zx, u0, u1 - u0, h->d_sums_stage);
    u0 = u1;
  }
  RCCHK(queue_status(h, b));
  return fb_commit(h, latch);
}

// The chunks of a training pass: each must fit the scratch budget; with two lanes a batch is cut into at least four chunks
// (none above a quarter of the utterances) so that both streams always have work.  Chunk i is [cuts[i], cuts[i + 1]).
struct FbPlan {
  std::vector<uint32_t> cuts;
  bool use2 = false;   // two lanes: odd chunks on the second stream, into a gradient of their own
  size_t n_chunks() const { return cuts.size() - 1; }
  int lane(size_t ci) const { return use2 ? (int)(ci & 1) : 0; }
};
static FbPlan fb_plan(scrf_handle h, scrf_batch b, const Need& nd) {
  FbPlan p;
  p.cuts.push_back(0);
  const bool two_lanes = h->kn.lanes > 1 && !h->tm.on && b->U >= 64;
  const uint32_t cap = two_lanes ? (b->U + 3) / 4 : b->U;
  for (uint32_t u0 = 0; u0 < b->U;) {
    const uint32_t u1 = std::min(plan_chunk(h, b, u0, nd), u0 + cap);
    p.cuts.push_back(u1);
    u0 = u1;
  }
  p.use2 = two_lanes && p.n_chunks() >= 2;
  return p;
}

// The route of chunk ci, once it is carved.  overlap (fused call only, scrf_fb_batch_allreduce): it waits for the status on
// the host, on the main stream.  side: the fused count kernel's wave-specialised form leaves room for a narrow k_ztf beside
// it, so k_ztf, its reduction and the transition counts A^T B run on the second stream -- and so do the recursion's check
// kernels and the status copy.  That needs the linear-domain fused branch of the recursion (dp_wave_lin: it forms Z in the
// posterior walk) and bias-only transitions.  Off while kernels are timed one by one (scrf_enable_timing), with two lanes
// (the second stream is a lane then) and with SCRF_SIDE=0.
static FbRoute fb_route(scrf_handle h, scrf_batch b, const ChunkBufs& cb, const FbPlan& plan, size_t ci) {
  FbRoute rt;
  rt.lane = plan.lane(ci);
  rt.two_lanes = plan.use2;
  rt.last = ci + 1 == plan.n_chunks();
  rt.overlap = h->overlap_comm && h->kn.comm_overlap && two_block_reduce(h) && !plan.use2 && !h->tm.on && !sparse(h);
  rt.side = h->kn.side && !plan.use2 && !h->tm.on && !rt.overlap && cb.fused && cb.lin && cb.wave && !h->lay.use_tf && !segtrans(h) &&
            pframe_supported(b->recipe[0].in_width) && cb.expf_plan.ws;
  return rt;
}

// The count launches of a chunk and the slab reductions they owe.  Each count function states the ScrfGemmSpec of a slab
// next to the launch that fills it; the reduce phase applies them, in launch order, behind all the count launches.
struct SlabSum { const double* slab; uint32_t nch, n_out; ScrfGemmSpec spec; };
struct ChunkCounts {
  SlabSum owed[4];   // at most three state slabs and one transition slab
  uint32_t n_owed = 0;
  uint32_t launches = 1;   // what PH_EXPF reports
  void owe(const double* slab, uint32_t nch, uint32_t n_out, const ScrfGemmSpec& spec) { owed[n_owed++] = SlabSum{slab, nch, n_out, spec}; }
};
static void reduce_owed(scrf_handle h, const ChunkBufs& cb, const ChunkCounts& cc) {
  for (uint32_t i = 0; i < cc.n_owed; i++)
    launch_reduce_slabs(cb.st, cc.owed[i].slab, cc.owed[i].nch, cc.owed[i].n_out, h->lay, cc.owed[i].spec, cb.grad);
}
// one-hot duration + bias counts from a slab of their own (the fused kernel's wave-specialised form, k_lin_z5)
static ScrfGemmSpec spec_dur_bias(const ScrfLayout& l, uint32_t W) { return ScrfGemmSpec{0, 0, l.D, (uint32_t)l.use_sb, l.sbv, 8 * W, 0}; }

// fused form: R's contraction with the synthesised windows, the sampled blocks through the per-frame sums Z
static int count_fused(scrf_handle h, scrf_batch b, uint32_t u0, uint32_t u1, ChunkBufs& cb, const FbRoute& rt, ChunkCounts* cc) {
  const ScrfLayout& l = h->lay;
  const uint32_t W0 = b->recipe[0].in_width, nz = (cb.la ? 6 : 5) * l.L;
  const uint64_t nfr = b->frame_off[u1] - b->frame_off[u0];
  const auto* fr0 = b->d_frames[0] + b->frame_off[u0] * W0;
  const ScrfFusedExpfPlan& plan = cb.expf_plan;
  ScrfFusedArgs fa = fused_args(h, b, u0, plan.tile_list);
  if (rt.side) {
    // k_ztf, its reduction and A^T B need Z / the recursion's vectors, not R's contraction: they run on the second stream
    // UNDER k_expf_fused_ws, whose one workgroup per CU leaves 80 registers per SIMD lane and the wave slots for a narrow
    // k_ztf (one output tile per wavefront).  The two sides add into disjoint weights; the streams join in the reduce phase.
    // The second stream was forked behind k_post_z (dp_wave_lin) and holds the check kernels already: no second fork.
    launch_ztf(h->stream2, cb.Z, nz, fr0, W0, nfr, cb.rpc_l, cb.nch_l, cb.slab_l, 1);
    launch_reduce_slabs(h->stream2, cb.slab_l, cb.nch_l, nz, l, spec_samples(W0), cb.grad);
    launch_atb(h->stream2, l, cb.fA, cb.fB, nfr, cb.rpc_atb, cb.nch_atb, cb.slab_atb, h->d_m0, cb.grad, cb.lin ? cb.dl.gsd : nullptr);
    HIPCHK(h, hipEventRecord(h->ev_join, h->stream2));
  }
  {
    PhaseTimer tk(h, PH_K_EXPF, cb.st);
    KT_RUN("k_expf_fused", cb.st, launch_expf_fused(cb.st, plan, fa, l, cb.R, b->tile_off[plan.tile_list][u1] - b->tile_off[plan.tile_list][u0], cb.slab_s, cb.slab_d));
    tk.stop(1);
  }
  if (plan.ndur) {
    // dense groups [avg |] max | min at columns (5 + g0) W ..; one-hot duration + bias counts from their own slab
    cc->owe(cb.slab_s, cb.nch_s, l.L, ScrfGemmSpec{0, 0, plan.ncol, 0, 0.0, (5 + plan.g0) * W0, 0});
    cc->owe(cb.slab_d, cb.nch_s, l.L, spec_dur_bias(l, W0));
  } else cc->owe(cb.slab_s, cb.nch_s, l.L, spec_dense(l, W0));
  if (!cb.z_ready) KT_RUN("k_lin_z", cb.st, launch_lin_z(cb.st, l, b->view(), u0, u1 - u0, cb.R, cb.Z));
  if (!rt.side) {
    if (pframe_supported(W0)) KT_RUN("k_ztf", cb.st, launch_ztf(cb.st, cb.Z, nz, fr0, W0, nfr, cb.rpc_l, cb.nch_l, cb.slab_l));
    else KT_RUN("k_expf_mfma(samples)", cb.st, launch_expf_mfma(cb.st, h->kn, cb.Z, nz, fr0, W0, nullptr, nfr, l, spec_samples(W0), cb.rpc_l, cb.nch_l, cb.slab_l));
    cc->owe(cb.slab_l, cb.nch_l, nz, spec_samples(W0));
  }
  cc->launches += 2;
  return SCRF_OK;
}

// hybrid form: materialised dense statistics, the sampled blocks through Z
static void count_hybrid(scrf_handle h, scrf_batch b, uint32_t u0, uint32_t u1, ChunkBufs& cb, ChunkCounts* cc) {
  const ScrfLayout& l = h->lay;
  const uint32_t W0 = b->recipe[0].in_width, nutt = u1 - u0;
  const uint64_t nfr = b->frame_off[u1] - b->frame_off[u0], nseg = b->seg_off[u1] - b->seg_off[u0];
  const auto* fr0 = b->d_frames[0] + b->frame_off[u0] * W0;
  const uint32_t t_max = longest_utt(b, u0, u1);   // k_lin_z5's segments, and so the blocks of its slab
  {
    PhaseTimer tk(h, PH_K_EXPF, cb.st);
    // [avg | max | min] only: the one-hot duration and bias counts are sums of R (k_lin_z5), and 3 W columns are one
    // 384-column tile of the count kernel where 3 W + D + 1 were two
    KT_RUN("k_expf_mfma(state)", cb.st, launch_expf_mfma(cb.st, h->kn, cb.R, l.L, cb.X, hybrid_row_floats(l, W0), nullptr, nseg, l, spec_stats_x(l, W0), cb.rpc_s, cb.nch_s, cb.slab_s, prec_f32(h)));
    tk.stop(1);
  }
  cc->owe(cb.slab_s, cb.nch_s, l.L, spec_stats_x(l, W0));
  const ScrfFusedWalkPlan zp = fused_lin_z5_plan(fused_shape(l), nutt, t_max);
  KT_RUN("k_lin_z5", cb.st, launch_lin_z5(cb.st, zp, l, b->view(), u0, nfr, cb.R, cb.Z, cb.slab_d));
  cc->owe(cb.slab_d, nutt * zp.nz, l.L, spec_dur_bias(l, W0));
  if (pframe_supported(W0)) KT_RUN("k_ztf", cb.st, launch_ztf(cb.st, cb.Z, 5 * l.L, fr0, W0, nfr, cb.rpc_l, cb.nch_l, cb.slab_l));
  else KT_RUN("k_expf_mfma(samples)", cb.st, launch_expf_mfma(cb.st, h->kn, cb.Z, 5 * l.L, fr0, W0, nullptr, nfr, l, spec_samples(W0), cb.rpc_l, cb.nch_l, cb.slab_l));
  cc->owe(cb.slab_l, cb.nch_l, 5 * l.L, spec_samples(W0));
  cc->launches += 2;
}

// sparse maps: inverted index of the chunk's windows, per-index sums of R, bias sums; then the transition counts of the
// next node's first window (the dense path's xrow_next) over Y - xi.  The sparse kernels add into the gradient themselves.
static void count_sparse(scrf_handle h, scrf_batch b, uint32_t u0, uint32_t u1, ChunkBufs& cb, ChunkCounts* cc) {
  const ScrfLayout& l = h->lay;
  const uint64_t nfr = b->frame_off[u1] - b->frame_off[u0], nseg = b->seg_off[u1] - b->seg_off[u0];
  PhaseTimer tk(h, PH_K_EXPF, cb.st);
  KT_RUN("sparse state counts", cb.st, launch_sp_counts(cb.st, cb.X, l.F, nullptr, nseg, cb.R, l, 0, cb.spx[0], cb.grad));
  tk.stop(1);
  if (!l.use_tf) return;
  launch_frame_rows(cb.st, b->view(), u0, u1, l.D, nfr, cb.xrow_next, 1);
  KT_RUN("sparse transition counts", cb.st, launch_sp_counts(cb.st, cb.X, l.F, cb.xrow_next, nfr, cb.XI, l, 1, cb.spx[1], cb.grad));
  cc->launches += 2;
}

// dense form: R's contraction with the materialised windows
static void count_dense(scrf_handle h, scrf_batch b, uint32_t u0, uint32_t u1, ChunkBufs& cb, ChunkCounts* cc) {
  const ScrfLayout& l = h->lay;
  const uint64_t nseg = b->seg_off[u1] - b->seg_off[u0];
  PhaseTimer tk(h, PH_K_EXPF, cb.st);
  if (prec_fast(h)) KT_RUN("k_expf_mfma(state)", cb.st, launch_expf_mfma(cb.st, h->kn, cb.R, l.L, cb.X, l.F, nullptr, nseg, l, scrf_spec_state(l), cb.rpc_s, cb.nch_s, cb.slab_s, prec_f32(h)));
  else KT_RUN("k_expf_gemm(state)", cb.st, launch_expf_gemm(cb.st, cb.R, l.L, cb.X, l.F, nullptr, nseg, l, 0, cb.rpc_s, cb.nch_s, cb.slab_s));
  tk.stop(1);
  cc->owe(cb.slab_s, cb.nch_s, l.L, scrf_spec_state(l));
}

// transition counts over the transition features.  by_window (STDSEG_NO_DUR): XI's rows are windows, contracted with the
// segment's own window, no row map; otherwise its rows are frames, contracted with the next node's first window.
static void count_trans(scrf_handle h, scrf_batch b, uint32_t u0, uint32_t u1, ChunkBufs& cb, bool by_window, ChunkCounts* cc) {
  const ScrfLayout& l = h->lay;
  const uint64_t nfr = b->frame_off[u1] - b->frame_off[u0], nseg = b->seg_off[u1] - b->seg_off[u0];
  const uint64_t* rows = by_window ? nullptr : cb.xrow_next;
  const uint64_t n_rows = by_window ? nseg : nfr;
  if (!by_window) launch_frame_rows(cb.st, b->view(), u0, u1, l.D, nfr, cb.xrow_next, 1);
  if (prec_fast(h)) KT_RUN("k_expf_mfma(trans)", cb.st, launch_expf_mfma(cb.st, h->kn, cb.XI, l.L * l.L, cb.X, l.F, rows, n_rows, l, scrf_spec_trans(l), cb.rpc_t, cb.nch_t, cb.slab_t, prec_f32(h)));
  else KT_RUN("k_expf_gemm(trans)", cb.st, launch_expf_gemm(cb.st, cb.XI, l.L * l.L, cb.X, l.F, rows, n_rows, l, 1, cb.rpc_t, cb.nch_t, cb.slab_t));
  cc->owe(cb.slab_t, cb.nch_t, l.L * l.L, scrf_spec_trans(l));
  cc->launches += by_window ? 1 : 2;
}

// All-reduce / compute overlap: the chunk's transition counts first, reduced at once; once the last chunk's are in they are
// committed and their all-reduce goes to the second stream, under the state contraction.  A NUMERIC failure of the recursion
// is retried with the log-domain kernels by the caller: that has to be known BEFORE a collective is issued (the peers issue
// theirs exactly once), so the host waits for the status here.  *redo: the caller reruns; nothing committed, nothing sent.
static int fb_early_trans(scrf_handle h, scrf_batch b, uint32_t u0, uint32_t u1, ChunkBufs& cb, const FbRoute& rt, int latch[2], bool* redo) {
  if (rt.last) {
    HIPCHK(h, hipEventSynchronize(h->ev_status));
    latch_decode(h->h_latch, latch);
    if (latch[0] == SCRF_ERR_NUMERIC && wave_path(h, true)) { *redo = true; return SCRF_OK; }
  }
  ChunkCounts tc;
  count_trans(h, b, u0, u1, cb, false, &tc);
  reduce_owed(h, cb, tc);
  if (!rt.last) return SCRF_OK;
  commit_staged(h, COMMIT_TRANS);
  HIPCHK(h, hipEventRecord(h->ev_fork, h->stream));
  HIPCHK(h, hipStreamWaitEvent(h->stream2, h->ev_fork, 0));
  RCCHK(allreduce_block(h, h->stream2, 1));
  HIPCHK(h, hipEventRecord(h->ev_join, h->stream2));
  h->early_done = true;
  return SCRF_OK;
}

// the count phase of a chunk: the state counts of its form, then the transition counts over transition features (unless the
// early all-reduce took them, or the sparse kernels did)
static int fb_count(scrf_handle h, scrf_batch b, uint32_t u0, uint32_t u1, ChunkBufs& cb, const FbRoute& rt, ChunkCounts* cc) {
  PhaseTimer tm(h, PH_EXPF, cb.st);
  if (cb.fused) RCCHK(count_fused(h, b, u0, u1, cb, rt, cc));
  else if (cb.hybrid) count_hybrid(h, b, u0, u1, cb, cc);
  else if (sparse(h)) count_sparse(h, b, u0, u1, cb, cc);
  else count_dense(h, b, u0, u1, cb, cc);
  if (segtrans(h)) count_trans(h, b, u0, u1, cb, true, cc);
  else if (!sparse(h) && h->lay.use_tf && !rt.overlap) count_trans(h, b, u0, u1, cb, false, cc);
  tm.stop(cc->launches);
  return SCRF_OK;
}

// the reduce phase: the owed slabs into the lane's gradient, the transition counts of bias-only transitions (no slab of
// split-K sums: A^T B over the xi factors, or the workgroup recursion's per-utterance xi), the batch sums
static int fb_reduce(scrf_handle h, scrf_batch b, uint32_t u0, uint32_t u1, ChunkBufs& cb, const FbRoute& rt, const ChunkCounts& cc) {
  const ScrfLayout& l = h->lay;
  const uint32_t nutt = u1 - u0;
  PhaseTimer tm(h, PH_REDUCE, cb.st);
  KernelTimer kt(h, "reductions (k_reduce_slabs, k_atb, k_batch_sums)", cb.st);
  reduce_owed(h, cb, cc);
  if (rt.side) HIPCHK(h, hipStreamWaitEvent(cb.st, h->ev_join, 0));   // the side stream's weights (k_ztf's, A^T B's) are in
  else if (l.use_tf || segtrans(h)) {}
  else if (cb.wave) launch_atb(cb.st, l, cb.fA, cb.fB, b->frame_off[u1] - b->frame_off[u0], cb.rpc_atb, cb.nch_atb, cb.slab_atb, h->d_m0, cb.grad,
                               cb.lin ? cb.dl.gsd : nullptr);
  else launch_reduce_xiacc(cb.st, cb.xi_acc, nutt, l, cb.grad);
  launch_batch_sums(cb.st, b->d_numer + u0, b->d_zx + u0, nutt, cb.sums);
  kt.stop(4);
  tm.stop(3);
  return SCRF_OK;
}

// chunk ci of the pass, on its lane.  *redo: see fb_early_trans.
static int fb_chunk(scrf_handle h, scrf_batch b, const FbPlan& plan, size_t ci, const Need& nd, int latch[2], bool* redo) {
  const uint32_t u0 = plan.cuts[ci], u1 = plan.cuts[ci + 1];
  ChunkBufs cb;
  RCCHK(score_chunk(h, b, u0, u1, nd, &cb, SCORE_PASS, plan.lane(ci)));
  if (!plan.lane(ci)) { cb.grad = h->d_stage; cb.sums = h->d_sums_stage; }
  const FbRoute rt = fb_route(h, b, cb, plan, ci);
  {
    PhaseTimer tm(h, PH_FB, cb.st);
    uint32_t nl = 0;
    RCCHK(run_dp(h, b, u0, u1, cb, DpOpts::training(rt), &nl));
    tm.stop(nl);
  }
  // every per-utterance status of the batch is final once the last chunk's posterior kernels are queued: its copy to the
  // host travels under the expected-count kernels (side: run_dp queued it on the second stream; two lanes: behind the join)
  if (rt.last && !rt.two_lanes && !rt.side) RCCHK(queue_status(h, b));
  if (rt.overlap) {
    RCCHK(fb_early_trans(h, b, u0, u1, cb, rt, latch, redo));
    if (*redo) return SCRF_OK;
  }
  ChunkCounts cc;
  RCCHK(fb_count(h, b, u0, u1, cb, rt, &cc));
  RCCHK(fb_reduce(h, b, u0, u1, cb, rt, cc));
  HIPCHK(h, hipGetLastError());
  return SCRF_OK;
}

static int fb_run(scrf_handle h, scrf_batch b, int latch[2]) {
  const ScrfLayout& l = h->lay;
  RCCHK(fb_begin(h, b));
  Need nd = Need::training();
  set_batch_form(h, b, &nd);
  const FbPlan plan = fb_plan(h, b, nd);
  if (!l.use_tf && !segtrans(h)) ensure_m0(h, h->stream);   // before the lanes fork
  if (sparse(h)) relay_sparse_lambda(h, h->stream);
  if (plan.use2) {
    HIPCHK(h, hipMemsetAsync(h->d_grad2, 0, sizeof(double) * l.lambda_len, h->stream));
    HIPCHK(h, hipMemsetAsync(h->d_sums2, 0, sizeof(double) * 4, h->stream));
    HIPCHK(h, hipEventRecord(h->ev_fork, h->stream));
    HIPCHK(h, hipStreamWaitEvent(h->stream2, h->ev_fork, 0));
  }
  for (size_t ci = 0; ci < plan.n_chunks(); ci++) {
    bool redo = false;
    RCCHK(fb_chunk(h, b, plan, ci, nd, latch, &redo));
    if (redo) return SCRF_OK;
  }
  if (plan.use2) {
    // join: lane 1's partial gradient and sums are added once, in a fixed order
    HIPCHK(h, hipEventRecord(h->ev_join, h->stream2));
    HIPCHK(h, hipStreamWaitEvent(h->stream, h->ev_join, 0));
    launch_add(h->stream, h->d_stage, h->d_grad2, l.lambda_len);
    launch_add(h->stream, h->d_sums_stage, h->d_sums2, 3);
    RCCHK(queue_status(h, b));
  }
  if (!l.use_tf && wave_path(h, true)) launch_add_trans_counts(h->stream, b->d_trans_counts, l, h->d_stage);
  return fb_commit(h, latch);
}

// One pass over a batch and, where it raised NUMERIC on the wavefront kernels, a second one.  The wavefront recursions take
// their transition step on exp(M - max M) (and the linear-domain one flushes what lies ~700 nats below a frame's maximum);
// where that empties a vector, leaves a transition sum below DBL_MIN or breaks a posterior-mass check, the batch is redone
// with the workgroup kernel, a column-wise max-shifted log-sum-exp like the reference's LogMath.  Nothing of the first pass
// survives: its staged gradient was dropped, its outputs are overwritten.  STDSEG and the n-state frame model have pipelines
// of their own: of those only STDSEG's linear-domain path (k_sl_fb, any number of full labels) has a log-domain second pass.
static bool first_pass_was_linear(scrf_handle h) { return stdseg(h) || nstate(h) ? stdseg(h) && stdseg_lin(h) : wave_path(h, true); }
template <class Pass>
static int run_with_redo(scrf_handle h, const int latch[2], Pass pass) {
  int rc = pass();
  if (rc != SCRF_OK || latch[0] != SCRF_ERR_NUMERIC || !first_pass_was_linear(h)) return rc;
  h->n_lin_fallback++;
  h->force_fb = true;
  rc = pass();
  h->force_fb = false;
  return rc;
}

extern "C" int scrf_fb_batch(scrf_handle h, scrf_batch b, double* numer, double* zx) {
  if (!h || !b) return SCRF_ERR_INVALID;
  HIPCHK(h, hipSetDevice(h->device));
  if (!b->d_labels) return fail(h, SCRF_ERR_INVALID, "scrf_fb_batch: the batch carries no labels");
  CallTimer call(h);
  int latch[2] = {0, 0};
  RCCHK(run_with_redo(h, latch, [&] { return stdseg(h) || nstate(h) ? fb_run_small(h, b, latch) : fb_run(h, b, latch); }));
  call.stop();
  if (latch[0] != 0) return fail(h, latch[0], "utterance %d: %s", latch[1], status_text(latch[0]));
  if (numer || zx) {
    if (numer) HIPCHK(h, hipMemcpyAsync(numer, b->d_numer, sizeof(double) * b->U, hipMemcpyDeviceToHost, h->stream));
    if (zx) HIPCHK(h, hipMemcpyAsync(zx, b->d_zx, sizeof(double) * b->U, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
  }
  return SCRF_OK;
}


// ---------------------------------------------------------------------------------------------
// posterior output: frame, boundary and segment posteriors of a label-less batch
// ---------------------------------------------------------------------------------------------
static const char* model_type_name(uint32_t mt) {
  return mt == SCRF_STDFRAME ? "stdframe" : mt == SCRF_STDSEG ? "stdseg" : mt == SCRF_STDSEG_NO_DUR ? "stdseg_no_dur"
         : mt == SCRF_STDSEG_NO_DUR_NO_TRANSFTR ? "stdseg_no_dur_no_transftr" : "stdseg_no_dur_no_segtransftr";
}
// room for n elements in a result array of the handle; the engine stream drains before a smaller one is dropped
template <class Tp>
static int reserve_drained(scrf_handle h, DevArray<Tp>& a, size_t n) {
  if (n > a.cap()) HIPCHK(h, hipStreamSynchronize(h->stream));
  HIPCHK(h, a.reserve(n));
  return SCRF_OK;
}

// The entry points that serve one transition matrix per frame (or one in all) and one state per label refuse the other
// models here; `what` names what the entry point computes.
static int model_ok(scrf_handle h, const char* fn, const char* what) {
  if (h->cfg.model_type == SCRF_STDSEG || h->cfg.model_type == SCRF_STDSEG_NO_DUR)
    return fail(h, SCRF_ERR_INVALID, "%s: %s is not built for the \"%s\" CRF model; use \"stdframe\", "
                "\"stdseg_no_dur_no_transftr\" or \"stdseg_no_dur_no_segtransftr\"", fn, what, model_type_name(h->cfg.model_type));
  if (h->cfg.num_states > 1)
    return fail(h, SCRF_ERR_INVALID, "%s: %s is built for crf_states = 1 only (this \"%s\" model has crf_states = %u)",
                fn, what, model_type_name(h->cfg.model_type), h->cfg.num_states);
  return SCRF_OK;
}

// The chunk driver of the label-free passes (scrf_posteriors_batch, scrf_transcript_batch): scores and the recursion of the
// handle's precision, chunk by chunk on the engine stream; body(cb, u0, u1, &nl) queues the pass's own kernels behind the
// recursion and adds their launches to nl.  Nothing that needs labels or feeds the gradient runs: no true scores, numerator,
// xi, R, counts, staging or commit.  latch[2]: as fb_commit's.
template <class Body>
static int label_free_run(scrf_handle h, scrf_batch b, Need nd, int latch[2], Body body) {
  HIPCHK(h, hipMemsetAsync(b->d_status, 0, sizeof(int) * b->U, h->stream));
  latch_reset(h);
  set_batch_form(h, b, &nd);   // the batch forms of scrf_fb_batch
  if (!h->lay.use_tf) ensure_m0(h, h->stream);
  if (sparse(h)) relay_sparse_lambda(h, h->stream);
  for (uint32_t u0 = 0; u0 < b->U;) {
    const uint32_t u1 = plan_chunk(h, b, u0, nd);
    ChunkBufs cb;
    RCCHK(score_chunk(h, b, u0, u1, nd, &cb, SCORE_PASS));
    PhaseTimer tm(h, PH_FB, cb.st);
    uint32_t nl = 0;
    RCCHK(run_dp(h, b, u0, u1, cb, DpOpts::recursion_only(), &nl));
    RCCHK(body(cb, u0, u1, &nl));
    tm.stop(nl);
    HIPCHK(h, hipGetLastError());
    u0 = u1;
  }
  RCCHK(queue_status(h, b));
  HIPCHK(h, hipEventSynchronize(h->ev_status));
  latch_decode(h->h_latch, latch);
  return SCRF_OK;
}

struct PostOut {
  double* occ = nullptr;    // [sum T][L]
  double* end = nullptr;    // [sum T]
  double* seg = nullptr;    // [n queries]
  const uint32_t *q_u = nullptr, *q_e = nullptr, *q_lab = nullptr;
  const uint64_t* lab_off = nullptr;   // host
};
// The result buffer of a posterior / transcript call (the handle's, scrf_abi.h), carved as [occ | end | n_extra doubles |
// seg | the queries q]: *po receives the parts the caller wants, *extra the extra doubles; the queries are uploaded.
static int post_out_carve(scrf_handle h, scrf_batch b, bool occ, bool end, bool seg, const std::vector<uint32_t>& q, uint64_t nq,
                          const uint64_t* lab_off, uint64_t n_extra, PostOut* po, double** extra) {
  const uint64_t nF = b->frame_off[b->U];
  const size_t by_occ = occ ? pad256(sizeof(double) * nF * h->lay.L) : 0, by_end = end ? pad256(sizeof(double) * nF) : 0;
  const size_t by_seg = pad256(sizeof(double) * nq), by_q = pad256(sizeof(uint32_t) * 3 * nq), by_x = pad256(sizeof(double) * n_extra);
  RCCHK(reserve_drained(h, h->post_buf, by_occ + by_end + by_x + by_seg + by_q + 256));
  char* pb = h->post_buf;
  if (occ) po->occ = (double*)pb;
  pb += by_occ;
  if (end) po->end = (double*)pb;
  pb += by_end;
  if (extra) *extra = (double*)pb;
  pb += by_x;
  if (seg && nq) {
    po->seg = (double*)pb;
    uint32_t* dq = (uint32_t*)(pb + by_seg);
    HIPCHK(h, hipMemcpyAsync(dq, q.data(), sizeof(uint32_t) * 3 * nq, hipMemcpyHostToDevice, h->stream));
    po->q_u = dq; po->q_e = dq + nq; po->q_lab = dq + 2 * nq;
    po->lab_off = lab_off;
  }
  return SCRF_OK;
}

// the posterior-output kernels of a chunk, behind its recursion: the free occupancy walk, the mass check, the segment queries
static int post_chunk(scrf_handle h, scrf_batch b, const PostOut& po, ChunkBufs& cb, uint32_t u0, uint32_t u1, uint32_t* nl) {
  const ScrfLayout& l = h->lay;
  const uint32_t nutt = u1 - u0;
  const uint64_t nfr = b->frame_off[u1] - b->frame_off[u0];
  ScrfBatchView bv = b->view();
  double* occ = po.occ ? po.occ + b->frame_off[u0] * l.L : nullptr;
  if (cb.lin) {
    const uint32_t t_max = longest_utt(b, u0, u1);
    uint32_t nz = 1;
    KT_RUN("k_post_occ", cb.st, nz = launch_post_occ(cb.st, l, bv, u0, nutt, t_max, nfr, cb.S, cb.smax, cb.dl, b->d_zx, b->d_status, occ,
                    cb.mass_part, cb.mass_s, h->kn.postocc_split ? 1 : 0));
    if (nz > 1) h->n_post_split++; else h->n_post_whole++;
    if (post_occ_groups(dp_shape(l)) > 1) *nl += 1;   // k_sum_groups
    KT_RUN("k_mass_check", cb.st, launch_mass_check(cb.st, bv, b->d_frame_u, u0, nfr, l.L, frame_mass_model(h), 1, cb.dl.a, cb.dl.ga, cb.dl.b, cb.dl.gb,
                      b->d_zx, cb.mass_s, b->d_status));
  } else {   // SCRF_PREC_EXACT, or the redo of a pass that raised NUMERIC
    KT_RUN("k_post_occ_log", cb.st, launch_post_occ_log(cb.st, l, bv, b->d_frame_u, u0, nfr, cb.AD, cb.beta, b->d_zx, b->d_status, occ, cb.mass_s));
    KT_RUN("k_mass_check", cb.st, launch_mass_check(cb.st, bv, b->d_frame_u, u0, nfr, l.L, frame_mass_model(h), 0, cb.alpha, nullptr, cb.beta, nullptr,
                      b->d_zx, cb.mass_s, b->d_status));
  }
  *nl += 2;
  if (po.end) HIPCHK(h, hipMemcpyAsync(po.end + b->frame_off[u0], cb.mass_s, sizeof(double) * nfr, hipMemcpyDeviceToDevice, cb.st));
  if (po.seg) {
    const uint64_t q0 = po.lab_off[u0], nq = po.lab_off[u1] - q0;
    KT_RUN("k_seg_post", cb.st, launch_seg_post(cb.st, l, bv, u0, po.q_u, po.q_e, po.q_lab, q0, nq, cb.lin ? 1 : 0, cb.lin ? cb.S : cb.AD, cb.smax,
                    cb.dl, cb.beta, b->d_zx, po.seg));
    *nl += 1;
  }
  return SCRF_OK;
}

// the segment queries of a call (scrf_posteriors_batch, scrf_transcript_batch): the segments of a path, back to back per
// utterance, label value l + L (d - 1) -> q [3][nq]: utterance, end frame, label value
static int seg_queries(scrf_handle h, scrf_batch b, const char* fn, const uint32_t* seg_labels, const uint64_t* lab_off, bool want,
                       std::vector<uint32_t>* qv, uint64_t* nq_out) {
  const ScrfLayout& l = h->lay;
  const uint64_t nF = b->frame_off[b->U];
  std::vector<uint32_t>& q = *qv;
  uint64_t nq = 0;
  if (want) {
    if (!seg_labels || !lab_off) return fail(h, SCRF_ERR_INVALID, "%s: seg_post needs seg_labels and lab_off", fn);
    nq = lab_off[b->U];
    if (lab_off[0] != 0 || nq > nF) return fail(h, SCRF_ERR_INVALID, "%s: lab_off does not describe back-to-back segments of this batch", fn);
    q.resize(3 * (size_t)nq + 1);
    for (uint32_t u = 0; u < b->U; u++) {
      if (lab_off[u + 1] < lab_off[u] || lab_off[u + 1] > nq) return fail(h, SCRF_ERR_INVALID, "%s: lab_off is not ascending at utterance %u", fn, u);
      uint64_t e = 0;   // frames consumed so far
      for (uint64_t i = lab_off[u]; i < lab_off[u + 1]; i++) {
        const uint32_t v = seg_labels[i];
        if (v >= l.L * l.D) return fail(h, SCRF_ERR_INVALID, "%s: utterance %u, segment %llu: label %u is out of range (labels x maximum duration = %u)",
                                        fn, u, (unsigned long long)(i - lab_off[u]), v, l.L * l.D);
        e += v / l.L + 1;
        if (e > b->T[u]) return fail(h, SCRF_ERR_INVALID, "%s: utterance %u, segment %llu ends at frame %llu, past the utterance's %u frames",
                                     fn, u, (unsigned long long)(i - lab_off[u]), (unsigned long long)(e - 1), b->T[u]);
        q[i] = u; q[nq + i] = (uint32_t)(e - 1); q[2 * nq + i] = v;
      }
    }
  }
  *nq_out = nq;
  return SCRF_OK;
}

extern "C" int scrf_posteriors_batch(scrf_handle h, scrf_batch b, double* zx, double* frame_post, double* end_post,
                                     const uint32_t* seg_labels, const uint64_t* lab_off, double* seg_post) {
  if (!h || !b) return SCRF_ERR_INVALID;
  RCCHK(model_ok(h, "scrf_posteriors_batch", "posterior output"));
  HIPCHK(h, hipSetDevice(h->device));
  const ScrfLayout& l = h->lay;
  const uint64_t nF = b->frame_off[b->U];
  std::vector<uint32_t> q;   // [3][nq]: utterance, end frame, label value
  uint64_t nq = 0;
  RCCHK(seg_queries(h, b, "scrf_posteriors_batch", seg_labels, lab_off, seg_post != nullptr, &q, &nq));
  PostOut po;
  RCCHK(post_out_carve(h, b, frame_post, end_post, seg_post, q, nq, lab_off, 0, &po, nullptr));
  CallTimer call(h);
  int latch[2] = {0, 0};
  RCCHK(run_with_redo(h, latch, [&] {   // the redo runs k_post_occ_log
    return label_free_run(h, b, Need::posterior(prec_fast(h)), latch, [&](ChunkBufs& cb, uint32_t u0, uint32_t u1, uint32_t* nl) { return post_chunk(h, b, po, cb, u0, u1, nl); });
  }));
  call.stop();
  if (latch[0] != 0) return fail(h, latch[0], "utterance %d: %s", latch[1], status_text(latch[0]));
  if (zx) HIPCHK(h, hipMemcpyAsync(zx, b->d_zx, sizeof(double) * b->U, hipMemcpyDeviceToHost, h->stream));
  if (frame_post) HIPCHK(h, hipMemcpyAsync(frame_post, po.occ, sizeof(double) * nF * l.L, hipMemcpyDeviceToHost, h->stream));
  if (end_post) HIPCHK(h, hipMemcpyAsync(end_post, po.end, sizeof(double) * nF, hipMemcpyDeviceToHost, h->stream));
  if (po.seg) HIPCHK(h, hipMemcpyAsync(seg_post, po.seg, sizeof(double) * nq, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return SCRF_OK;
}

extern "C" int scrf_add_grad(scrf_handle h, const double* g, uint32_t n) {
  if (!h || !g) return SCRF_ERR_INVALID;
  if (n != h->xlay.lambda_len) return fail(h, SCRF_ERR_INVALID, "scrf_add_grad: length mismatch");
  HIPCHK(h, hipSetDevice(h->device));
  if (h->shadow) {
    h->xbuf.assign(h->lay.lambda_len, 0.0);
    for (uint32_t i = 0; i < n; i++) h->xbuf[h->s2d[i]] = g[i];
    g = h->xbuf.data();
    n = h->lay.lambda_len;
  }
  RCCHK(ensure_scratch(h, sizeof(double) * n));
  HIPCHK(h, hipMemcpyAsync(h->scratch[0], g, sizeof(double) * n, hipMemcpyHostToDevice, h->stream));
  launch_add(h->stream, h->d_grad, (const double*)h->scratch[0].get(), n);
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return SCRF_OK;
}

// ---------------------------------------------------------------------------------------------
// parity hooks (single utterance)
// ---------------------------------------------------------------------------------------------
static int check_u(scrf_handle h, scrf_batch b, uint32_t u, const char* fn) {
  if (!h || !b) return SCRF_ERR_INVALID;
  if (u >= b->U) return fail(h, SCRF_ERR_INVALID, "%s: utterance %u >= %u", fn, u, b->U);
  return SCRF_OK;
}

// the n-state / STDSEG pipelines through one call: scores and recursion of chunk [u0, u1), no posteriors
struct SmallBufs { NstateBufs ns; StdsegBufs sg; };
static int run_small_chunk(scrf_handle h, scrf_batch b, uint32_t u0, uint32_t u1, SmallBufs* sb) {
  return nstate(h) ? nstate_run_chunk(h, b, u0, u1, false, nullptr, &sb->ns) : stdseg_run_chunk(h, b, u0, u1, false, nullptr, &sb->sg);
}
// ... of one utterance, for the hooks
static int hook_small_chunk(scrf_handle h, scrf_batch b, uint32_t u, SmallBufs* sb) {
  HIPCHK(h, hipMemsetAsync(b->d_status, 0, sizeof(int) * b->U, h->stream));
  return run_small_chunk(h, b, u, u + 1, sb);
}

// Zx = -computeAlphaSum() of utterance u, read back (the final arcs of a normalised lattice carry it)
static int read_zx(scrf_handle h, scrf_batch b, uint32_t u, double* Zx) {
  double asum = 0;
  HIPCHK(h, hipMemcpyAsync(&asum, b->d_zx + u, sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  *Zx = -1 * asum;
  return SCRF_OK;
}

// One utterance through carve, EXACT scores and the log-domain recursion, for hook `fn`: *cb holds the node values on success.
// Second attempt: the workgroup kernel (reference LogMath) when the wavefront recursion gave up.  A label out of range
// does not stop a hook that reads no label.
static int hook_fb(scrf_handle h, scrf_batch b, uint32_t u, const char* fn, ChunkBufs* cb) {
  for (;;) {
    *cb = ChunkBufs();
    int rc = score_chunk(h, b, u, u + 1, Need::recursion(), cb);
    if (rc == SCRF_OK && hipMemsetAsync(b->d_status, 0, sizeof(int) * b->U, h->stream) != hipSuccess) rc = fail(h, SCRF_ERR_HIP, "%s: memset failed", fn);
    if (rc == SCRF_OK) rc = run_dp(h, b, u, u + 1, *cb, DpOpts(), nullptr);
    int st = 0;
    if (rc == SCRF_OK && hipMemcpyAsync(&st, b->d_status + u, sizeof(int), hipMemcpyDeviceToHost, h->stream) != hipSuccess) rc = fail(h, SCRF_ERR_HIP, "%s: status copy failed", fn);
    if (rc == SCRF_OK && hipStreamSynchronize(h->stream) != hipSuccess) rc = fail(h, SCRF_ERR_HIP, "%s: synchronize failed", fn);
    if (rc == SCRF_OK && st == SCRF_ERR_NUMERIC && !h->force_fb && wave_path(h, false)) { h->force_fb = true; continue; }
    h->force_fb = false;
    if (rc != SCRF_OK) return rc;
    if (st != SCRF_OK && st != SCRF_ERR_BAD_LABEL) return fail(h, st, "utterance %u: numeric failure in forward-backward", u);
    return SCRF_OK;
  }
}

extern "C" int scrf_windows(scrf_handle h, scrf_batch b, uint32_t u, float* out) {
  RCCHK(check_u(h, b, u, "scrf_windows"));
  if (!out) return SCRF_ERR_INVALID;
  HIPCHK(h, hipSetDevice(h->device));
  ChunkBufs cb;
  RCCHK(score_chunk(h, b, u, u + 1, Need::scores(), &cb));
  uint64_t nseg = b->seg_off[u + 1] - b->seg_off[u];
  HIPCHK(h, hipMemcpyAsync(out, cb.X, sizeof(float) * nseg * h->lay.F, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return SCRF_OK;
}

static int copy_M(scrf_handle h, const ChunkBufs& cb, uint32_t T, double* M) {
  const size_t LL = (size_t)h->lay.L * h->lay.L;
  // matrices on the device: one per window (STDSEG_NO_DUR), one per frame, or one in all (copied out T times)
  const size_t n = cb.m_per_frame == 2 ? scrf_seg_base(T, h->lay.D) : cb.m_per_frame ? T : 1;
  HIPCHK(h, hipMemcpyAsync(M, cb.M, sizeof(double) * n * LL, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (!cb.m_per_frame) for (uint32_t t = 1; t < T; t++) memcpy(M + t * LL, M, sizeof(double) * LL);
  return SCRF_OK;
}

extern "C" int scrf_scores(scrf_handle h, scrf_batch b, uint32_t u, double* S, double* M) {
  RCCHK(check_u(h, b, u, "scrf_scores"));
  HIPCHK(h, hipSetDevice(h->device));
  if (nstate(h)) {   // S [T][nLabs]; M [T][2*nLabs + P*P]: self transitions | c -> c+1 | end state of p -> start state of q
    SmallBufs sm;
    RCCHK(hook_small_chunk(h, b, u, &sm));
    const NstateBufs& nb = sm.ns;
    const uint64_t T = b->T[u], L = h->lay.L, P = L / h->lay.K, w = 2 * L + P * P;
    if (S) HIPCHK(h, hipMemcpyAsync(S, nb.S, sizeof(double) * T * L, hipMemcpyDeviceToHost, h->stream));
    if (M) {
      HIPCHK(h, hipMemcpy2DAsync(M, sizeof(double) * w, nb.TD, sizeof(double) * L, sizeof(double) * L, T, hipMemcpyDeviceToHost, h->stream));
      HIPCHK(h, hipMemcpy2DAsync(M + L, sizeof(double) * w, nb.TO, sizeof(double) * L, sizeof(double) * L, T, hipMemcpyDeviceToHost, h->stream));
      HIPCHK(h, hipMemcpy2DAsync(M + 2 * L, sizeof(double) * w, nb.TE, sizeof(double) * P * P, sizeof(double) * P * P, T, hipMemcpyDeviceToHost, h->stream));
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return SCRF_OK;
  }
  if (stdseg(h)) {   // S [N_seg][nActualLabs], M [N_seg][nLabs][nActualLabs]
    SmallBufs sm;
    RCCHK(hook_small_chunk(h, b, u, &sm));
    const StdsegBufs& sb = sm.sg;
    const uint64_t ns = b->seg_off[u + 1] - b->seg_off[u];
    const uint32_t La = stdseg_La(h);
    if (S) HIPCHK(h, hipMemcpyAsync(S, sb.S, sizeof(double) * ns * La, hipMemcpyDeviceToHost, h->stream));
    if (M) HIPCHK(h, hipMemcpyAsync(M, sb.MX, sizeof(double) * ns * h->lay.L * La, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return SCRF_OK;
  }
  ChunkBufs cb;
  RCCHK(score_chunk(h, b, u, u + 1, Need::scores(), &cb));
  uint64_t nseg = b->seg_off[u + 1] - b->seg_off[u];
  if (S) HIPCHK(h, hipMemcpyAsync(S, cb.S, sizeof(double) * nseg * h->lay.L, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (M) return copy_M(h, cb, b->T[u], M);
  return SCRF_OK;
}

extern "C" int scrf_forward_backward(scrf_handle h, scrf_batch b, uint32_t u, uint32_t prec, double* alpha_dur,
                                     double* alpha, double* beta, double* zx) {
  RCCHK(check_u(h, b, u, "scrf_forward_backward"));
  if (prec != SCRF_PREC_EXACT) return fail(h, SCRF_ERR_INVALID, "scrf_forward_backward: the node-value hook runs at SCRF_PREC_EXACT only");
  HIPCHK(h, hipSetDevice(h->device));
  if (nstate(h) || stdseg(h)) {
    // n-state: alpha, beta [T][nLabs], alpha_dur is not written; STDSEG: alpha_dur and beta, the nodes' alpha / beta over full
    // labels [N_seg][nActualLabs], `alpha` is not written
    SmallBufs sm;
    RCCHK(hook_small_chunk(h, b, u, &sm));
    const uint64_t n = nstate(h) ? (uint64_t)b->T[u] * h->lay.L : (b->seg_off[u + 1] - b->seg_off[u]) * stdseg_La(h);
    double* a_out = nstate(h) ? alpha : alpha_dur;
    int st = 0;
    if (a_out) HIPCHK(h, hipMemcpyAsync(a_out, nstate(h) ? sm.ns.alpha : sm.sg.alpha, sizeof(double) * n, hipMemcpyDeviceToHost, h->stream));
    if (beta) HIPCHK(h, hipMemcpyAsync(beta, nstate(h) ? sm.ns.beta : sm.sg.beta, sizeof(double) * n, hipMemcpyDeviceToHost, h->stream));
    if (zx) HIPCHK(h, hipMemcpyAsync(zx, b->d_zx + u, sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(&st, b->d_status + u, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (st != SCRF_OK) return fail(h, st, "utterance %u: numeric failure in forward-backward", u);
    return SCRF_OK;
  }
  const ScrfLayout& l = h->lay;
  const uint64_t nseg = b->seg_off[u + 1] - b->seg_off[u];
  const uint32_t T = b->T[u];
  ChunkBufs cb;
  RCCHK(hook_fb(h, b, u, "scrf_forward_backward", &cb));
  if (alpha_dur) HIPCHK(h, hipMemcpyAsync(alpha_dur, cb.AD, sizeof(double) * nseg * l.L, hipMemcpyDeviceToHost, h->stream));
  if (alpha) HIPCHK(h, hipMemcpyAsync(alpha, cb.alpha, sizeof(double) * T * l.L, hipMemcpyDeviceToHost, h->stream));
  if (beta) HIPCHK(h, hipMemcpyAsync(beta, cb.beta, sizeof(double) * T * l.L, hipMemcpyDeviceToHost, h->stream));
  if (zx) HIPCHK(h, hipMemcpyAsync(zx, b->d_zx + u, sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return SCRF_OK;
}

extern "C" int scrf_seg_posteriors(scrf_handle h, scrf_batch b, uint32_t u, double* gamma) {
  RCCHK(check_u(h, b, u, "scrf_seg_posteriors"));
  if (!gamma) return SCRF_ERR_INVALID;
  RCCHK(model_ok(h, "scrf_seg_posteriors", "posterior output"));
  HIPCHK(h, hipSetDevice(h->device));
  const ScrfLayout& l = h->lay;
  const uint64_t nseg = b->seg_off[u + 1] - b->seg_off[u];
  ChunkBufs cb;
  RCCHK(hook_fb(h, b, u, "scrf_seg_posteriors", &cb));
  launch_gamma_log(h->stream, l, b->T[u], cb.AD, cb.beta, b->d_zx + u, cb.AD);
  HIPCHK(h, hipMemcpyAsync(gamma, cb.AD, sizeof(double) * nseg * l.L, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return SCRF_OK;
}


// ---------------------------------------------------------------------------------------------
// decode
// ---------------------------------------------------------------------------------------------
extern "C" int scrf_lattice_arcs(scrf_handle h, scrf_batch b, uint32_t u, int norm, scrf_arc* arcs, uint64_t* n_arcs,
                                 uint32_t* n_states, int32_t* final_state) {
  RCCHK(check_u(h, b, u, "scrf_lattice_arcs"));
  HIPCHK(h, hipSetDevice(h->device));
  if (nstate(h)) {   // decoders/CRF_LatticeBuilder.h nStateBuildLattice
    const uint32_t T = b->T[u], L = h->lay.L;
    const uint64_t na = b->arc_off[u + 1] - b->arc_off[u];
    if (n_arcs) *n_arcs = na;
    if (n_states) *n_states = L * T + 2;
    if (final_state) *final_state = (int32_t)(L * T + 1);
    if (!arcs) return SCRF_OK;
    SmallBufs sm;
    RCCHK(hook_small_chunk(h, b, u, &sm));
    const NstateBufs& nb = sm.ns;
    double Zx = 0.0;
    if (norm) RCCHK(read_zx(h, b, u, &Zx));
    const float final_w = norm ? (float)Zx : 0.0f;
    DevArray<scrf_arc> d_arcs;
    HIPCHK(h, d_arcs.reserve(na));
    launch_ns_arcs(h->stream, h->lay, T, nb.S, nb.TD, nb.TO, nb.TE, final_w, d_arcs);
    hipError_t e = hipMemcpyAsync(arcs, d_arcs, sizeof(scrf_arc) * na, hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) return fail(h, SCRF_ERR_HIP, "scrf_lattice_arcs: %s", hipGetErrorString(e));
    return SCRF_OK;
  }
  if (stdseg(h)) {   // decoders/CRF_LatticeBuilder_StdSeg.h: one state per (node, available full label)
    const uint32_t La = stdseg_La(h), T = b->T[u];
    const uint64_t ns = b->seg_off[u + 1] - b->seg_off[u], na = b->arc_off[u + 1] - b->arc_off[u];
    if (n_arcs) *n_arcs = na;
    if (n_states) *n_states = (uint32_t)(2 + ns * La);
    if (final_state) *final_state = (int32_t)(1 + ns * La);
    if (!arcs) return SCRF_OK;
    SmallBufs sm;
    RCCHK(hook_small_chunk(h, b, u, &sm));
    const StdsegBufs& sb = sm.sg;
    double Zx = 0.0;
    if (norm) RCCHK(read_zx(h, b, u, &Zx));
    const float final_w = norm ? (float)(-Zx) : -0.0f;
    std::vector<uint64_t> off;
    stdseg_row_arc_offsets(T, La, h->lay.D, &off);
    DevArray<uint64_t> d_off;
    DevArray<scrf_arc> d_arcs;
    hipError_t e = d_off.reserve(off.size());
    if (e == hipSuccess) e = d_arcs.reserve(na);
    if (e == hipSuccess) e = hipMemcpyAsync(d_off, off.data(), sizeof(uint64_t) * off.size(), hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) {
      launch_stdseg_arcs(h->stream, h->lay, La, T, ns, d_off, sb.S, sb.MX, final_w, d_arcs);
      e = hipMemcpyAsync(arcs, d_arcs, sizeof(scrf_arc) * na, hipMemcpyDeviceToHost, h->stream);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) return fail(h, SCRF_ERR_HIP, "scrf_lattice_arcs: %s", hipGetErrorString(e));
    return SCRF_OK;
  }
  const ScrfLayout& l = h->lay;
  const uint32_t T = b->T[u];
  const bool frame_model = h->cfg.model_type == SCRF_STDFRAME;
  const uint64_t na = b->arc_off[u + 1] - b->arc_off[u];
  if (n_arcs) *n_arcs = h->shadow ? shadow_num_arcs(h, T) : na;
  // STDSEG_NO_DUR: one state per (node, label) like the frame lattice (decoders/CRF_LatticeBuilder_StdSeg_WithoutDurLab.h)
  if (n_states) *n_states = (frame_model || segtrans(h)) ? l.L * T + 2 : (uint32_t)scrf_node_start_state(T, l.L) + 1;
  if (final_state) *final_state = (frame_model || segtrans(h)) ? (int32_t)(l.L * T + 1) : scrf_node_start_state(T, l.L);
  if (!arcs) return SCRF_OK;
  ChunkBufs cb;
  RCCHK(score_chunk(h, b, u, u + 1, Need::alpha_sum(norm != 0), &cb));
  float final_w = frame_model ? 0.0f : -0.0f;
  if (norm) {
    // Zx = -computeAlphaSum(): final arcs carry -Zx (segmental, :371,397) / Zx (frame, CRF_LatticeBuilder.h:191-198)
    HIPCHK(h, hipMemsetAsync(b->d_status, 0, sizeof(int) * b->U, h->stream));
    RCCHK(run_dp(h, b, u, u + 1, cb, DpOpts(), nullptr));
    double Zx = 0.0;
    RCCHK(read_zx(h, b, u, &Zx));
    final_w = frame_model ? (float)Zx : (float)(-Zx);
  }
  DevArray<scrf_arc> d_arcs;
  HIPCHK(h, d_arcs.reserve(na));
  if (segtrans(h)) launch_arcs_segtrans(h->stream, l, T, cb.S, cb.M, final_w, d_arcs);
  else launch_arcs(h->stream, l, T, arc_src(h, cb), final_w, d_arcs);
  std::vector<scrf_arc> dense;
  if (h->shadow) dense.resize(na);
  hipError_t e = hipMemcpyAsync(h->shadow ? dense.data() : arcs, d_arcs, sizeof(scrf_arc) * na, hipMemcpyDeviceToHost, h->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
  if (e != hipSuccess) return fail(h, SCRF_ERR_HIP, "scrf_lattice_arcs: %s", hipGetErrorString(e));
  if (h->shadow) {
    // nStateBuildLattice :563-597: of the L*L boundary arcs of a frame (state-major, previous label ascending) a
    // phone's start state keeps those from the end states, ascending, and then its own; any other state the one from
    // the state before it and then its own.  States, segment arcs and final arcs are the dense lattice's.
    const uint32_t L = l.L, K = h->xlay.K;
    const scrf_arc* in = dense.data();
    scrf_arc* out = arcs;
    for (uint32_t t = 0; t < T; t++) {
      if (t > 0) {
        for (uint32_t lab = 0; lab < L; lab++, in += L) {
          if (lab % K == 0) { for (uint32_t e2 = K - 1; e2 < L; e2 += K) *out++ = in[e2]; }
          else *out++ = in[lab - 1];
          *out++ = in[lab];
        }
      }
      const uint64_t nseg = (uint64_t)L * scrf_node_max_dur(t, l.D);
      memcpy(out, in, sizeof(scrf_arc) * nseg);
      out += nseg; in += nseg;
    }
    memcpy(out, in, sizeof(scrf_arc) * L);
    out += L; in += L;
    if ((uint64_t)(out - arcs) != shadow_num_arcs(h, T) || (uint64_t)(in - dense.data()) != na)
      return fail(h, SCRF_ERR_INVALID, "scrf_lattice_arcs: arc count mismatch (internal)");
  }
  return SCRF_OK;
}

// ---------------------------------------------------------------------------------------------
// beam-pruned lattices of a batch
// ---------------------------------------------------------------------------------------------
extern "C" int scrf_lattice_prune_batch(scrf_handle h, scrf_batch b, double beam, uint64_t* arc_off, double* best_cost) {
  if (!h || !b || !arc_off) return SCRF_ERR_INVALID;
  h->lp.batch = nullptr;   // whatever happens, the previous result is gone
  RCCHK(model_ok(h, "scrf_lattice_prune_batch", "the lattice beam"));
  if (!(beam > 0.0) || !std::isfinite(beam))
    return fail(h, SCRF_ERR_INVALID, "scrf_lattice_prune_batch: the beam must be finite and > 0 (got %g)", beam);
  const ScrfLayout& l = h->lay;
  if (lat_sweep_smem_bytes(dp_shape(l)) > SCRF_LDS_BYTES)
    return fail(h, SCRF_ERR_INVALID, "scrf_lattice_prune_batch: %u labels x maximum duration %u do not fit the sweep kernel's LDS window", l.L, l.D);
  HIPCHK(h, hipSetDevice(h->device));
  const uint32_t U = b->U;
  const size_t by_best = pad256(sizeof(double) * U), need_meta = by_best + pad256(sizeof(uint64_t) * (U + 1));
  RCCHK(reserve_drained(h, h->lp.meta, need_meta));
  double* d_best = (double*)h->lp.meta.get();
  uint64_t* d_uoff = (uint64_t*)(h->lp.meta + by_best);
  CallTimer call(h);
  h->lp.n_calls++;
  const Need nd = Need::lattice();
  ScrfBatchView bv = b->view();
  uint64_t total = 0;   // kept arcs of the chunks done
  for (uint32_t u0 = 0; u0 < U;) {
    const uint32_t u1 = plan_chunk(h, b, u0, nd);
    ChunkBufs cb;
    RCCHK(score_chunk(h, b, u0, u1, nd, &cb));
    h->lp.n_chunks++;
    const uint32_t nutt = u1 - u0;
    const uint64_t nfr = b->frame_off[u1] - b->frame_off[u0], n_nodes = nfr + nutt;
    const uint32_t t_max = longest_utt(b, u0, u1);
    cb.lat.best = d_best;
    const ScrfArcSrc src = arc_src(h, cb);
    KT_RUN("k_lat_sweep", cb.st, launch_lat_sweep(cb.st, l, bv, u0, nutt, src, cb.lat));
    KT_RUN("k_lat_count", cb.st, launch_lat_count(cb.st, l, bv, u0, nutt, t_max, src, cb.lat, beam, cb.lat_counts));
    KT_RUN("k_lat_scan", cb.st, launch_lat_scan(cb.st, bv, u0, nutt, cb.lat_counts, n_nodes, cb.lat_node_off, total, d_uoff));
    uint64_t kept = 0;   // the chunk's arcs must have room before they are written
    HIPCHK(h, hipMemcpyAsync(&kept, cb.lat_node_off + n_nodes, sizeof(uint64_t), hipMemcpyDeviceToHost, cb.st));
    HIPCHK(h, hipStreamSynchronize(cb.st));
    HIPCHK(h, h->lp.arcs.reserve_keep(total + kept, total, cb.st));   // the arcs of the chunks done move with it
    KT_RUN("k_lat_emit", cb.st, launch_lat_emit(cb.st, l, bv, u0, nutt, t_max, src, cb.lat, beam, cb.lat_node_off, total, h->lp.arcs.cap(),
                                                h->lp.arcs));
    HIPCHK(h, hipGetLastError());
    total += kept;
    u0 = u1;
  }
  h->lp.off.resize(U + 1);
  HIPCHK(h, hipMemcpyAsync(h->lp.off.data(), d_uoff, sizeof(uint64_t) * (U + 1), hipMemcpyDeviceToHost, h->stream));
  if (best_cost) HIPCHK(h, hipMemcpyAsync(best_cost, d_best, sizeof(double) * U, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  call.stop();
  if (h->lp.off[U] != total) return fail(h, SCRF_ERR_INVALID, "scrf_lattice_prune_batch: arc count mismatch (internal)");
  memcpy(arc_off, h->lp.off.data(), sizeof(uint64_t) * (U + 1));
  h->lp.batch = b;
  return SCRF_OK;
}

extern "C" int scrf_lattice_pruned_arcs(scrf_handle h, scrf_batch b, uint32_t u0, uint32_t n, scrf_arc* arcs, uint64_t cap) {
  if (!h || !b) return SCRF_ERR_INVALID;
  if (h->lp.batch != b)
    return fail(h, SCRF_ERR_INVALID, "scrf_lattice_pruned_arcs: no valid result for this batch (call scrf_lattice_prune_batch first; new weights, "
                "another prune call or destroying the batch drop it)");
  if ((uint64_t)u0 + n > b->U) return fail(h, SCRF_ERR_INVALID, "scrf_lattice_pruned_arcs: utterances %u .. %llu of a batch of %u", u0,
                                           (unsigned long long)u0 + n, b->U);
  const uint64_t a0 = h->lp.off[u0], na = h->lp.off[u0 + n] - a0;
  if (cap < na) return fail(h, SCRF_ERR_INVALID, "scrf_lattice_pruned_arcs: room for %llu arcs, %llu needed", (unsigned long long)cap, (unsigned long long)na);
  if (na == 0) return SCRF_OK;
  if (!arcs) return SCRF_ERR_INVALID;
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipMemcpyAsync(arcs, h->lp.arcs + a0, sizeof(scrf_arc) * na, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return SCRF_OK;
}

extern "C" int scrf_lattice_prune_stats(scrf_handle h, uint64_t* n_calls, uint64_t* n_chunks) {
  if (!h) return SCRF_ERR_INVALID;
  if (n_calls) *n_calls = h->lp.n_calls;
  if (n_chunks) *n_chunks = h->lp.n_chunks;
  return SCRF_OK;
}

// The chunk loop of the decode entry points of the one-state models (scrf_viterbi_batch, scrf_align_batch); only the search
// differs.  Fast decode: the fused score kernel writes the float arc weights (cb.Wn) and lists the entries whose
// rounding it cannot guarantee; those are recomputed in reference order.  A chunk whose list
// overflows (pathological cancellation) goes through the EXACT path (cb.S) instead.
// search(cb, u0, u1, fast) launches the search of chunk [u0, u1) on the engine stream.
template <class Search>
static int decode_chunks(scrf_handle h, scrf_batch b, const Need& nd, Search&& search) {
  const ScrfLayout& l = h->lay;
  const bool frame_model = h->cfg.model_type == SCRF_STDFRAME;
  Need ndf = nd;
  ndf.fused = ndf.vitfast = true;
  const bool fast = h->kn.fast_decode && b->fused_ok && !b->mixed && h->kn.fuse && !frame_model && l.L <= 0xffff;
  int rc = SCRF_OK;
  for (uint32_t u0 = 0; u0 < b->U && rc == SCRF_OK;) {
    uint32_t u_end = u0;
    if (fast) {
      const uint32_t u1 = plan_chunk(h, b, u0, ndf);
      ChunkBufs cb;
      ensure_m0(h, h->stream);
      rc = score_chunk(h, b, u0, u1, ndf, &cb);
      if (rc != SCRF_OK) break;
      uint32_t n_fix = 0;
      HIPCHK(h, hipMemcpyAsync(&n_fix, cb.fix_cnt, sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
      HIPCHK(h, hipStreamSynchronize(h->stream));
      h->dec.n_fix += n_fix;
      if (n_fix <= cb.fix_cap) {
        PhaseTimer tm(h, PH_VIT);
        launch_decode_fixup(h->stream, b->d_frames[0], b->recipe[0].in_width, b->view(), u0, u1, h->d_lambda, l, cb.fix_cnt,
                            cb.fix_list, std::min(n_fix, cb.fix_cap), cb.Wn);
        search(cb, u0, u1, true);
        tm.stop(2);
        u0 = u1;
        continue;
      }
      h->dec.n_fallback++;
      u_end = u1;  // this range again, through the EXACT path
    }
    do {
      const uint32_t u1 = std::min(fast ? u_end : b->U, plan_chunk(h, b, u0, nd));
      ChunkBufs cb;
      rc = score_chunk(h, b, u0, u1, nd, &cb);
      if (rc != SCRF_OK) break;
      PhaseTimer tm(h, PH_VIT);
      search(cb, u0, u1, false);
      tm.stop(1);
      u0 = u1;
    } while (fast && u0 < u_end && rc == SCRF_OK);
  }
  return rc;
}

// labels, counts and costs of the whole batch to the caller, through the pinned images; closes the timed region
static int decode_result_fetch(scrf_handle h, scrf_batch b, const char* fn, CallTimer& call, uint32_t* seg_labels, uint64_t max_labels,
                               uint64_t* lab_off, float* best_cost) {
  const uint64_t NF = b->frame_off[b->U];
  const uint32_t *lab = h->dec.hlab, *cnt = h->dec.hn;
  hipError_t e = hipMemcpyAsync(h->dec.hlab, h->dec.lab, sizeof(uint32_t) * NF, hipMemcpyDeviceToHost, h->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(h->dec.hn, h->dec.n, sizeof(uint32_t) * b->U, hipMemcpyDeviceToHost, h->stream);
  if (e == hipSuccess && best_cost) e = hipMemcpyAsync(h->dec.hcost, h->dec.cost, sizeof(float) * b->U, hipMemcpyDeviceToHost, h->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
  if (e != hipSuccess) return fail(h, SCRF_ERR_HIP, "%s: %s", fn, hipGetErrorString(e));
  if (best_cost) memcpy(best_cost, h->dec.hcost, sizeof(float) * b->U);
  call.stop();
  uint64_t pos = 0;
  for (uint32_t u = 0; u < b->U; u++) {
    lab_off[u] = pos;
    if (pos + cnt[u] > max_labels) return fail(h, SCRF_ERR_INVALID, "%s: seg_labels capacity %llu too small", fn, (unsigned long long)max_labels);
    memcpy(seg_labels + pos, &lab[b->frame_off[u]], sizeof(uint32_t) * cnt[u]);
    pos += cnt[u];
  }
  lab_off[b->U] = pos;
  return SCRF_OK;
}

extern "C" int scrf_viterbi_batch(scrf_handle h, scrf_batch b, uint32_t* seg_labels, uint64_t max_labels,
                                  uint64_t* lab_off, float* best_cost) {
  if (!h || !b || !seg_labels || !lab_off) return SCRF_ERR_INVALID;
  HIPCHK(h, hipSetDevice(h->device));
  const ScrfLayout& l = h->lay;
  CallTimer call(h);
  HIPCHK(h, h->dec.reserve(b->frame_off[b->U], b->U));
  int rc = SCRF_OK;
  uint32_t *d_lab = h->dec.lab, *d_n = h->dec.n;
  float* d_cost = h->dec.cost;
  if (nstate(h) || stdseg(h)) {
    // the chunk's scores in the scratch arena (chunks planned with the `post` sizing), path costs and back pointers per
    // (row, label) in buffers of their own
    const uint32_t n_lab = nstate(h) ? l.L : stdseg_La(h);
    HIPCHK(h, hipMemsetAsync(b->d_status, 0, sizeof(int) * b->U, h->stream));
    for (uint32_t u0 = 0; u0 < b->U;) {
      const uint32_t u1 = small_plan_chunk(h, b, u0, true);
      SmallBufs sm;
      rc = run_small_chunk(h, b, u0, u1, &sm);
      if (rc != SCRF_OK) break;
      const uint64_t rows = nstate(h) ? b->frame_off[u1] - b->frame_off[u0] : b->seg_off[u1] - b->seg_off[u0];
      DevArray<float> vc;
      DevArray<uint16_t> bp;
      hipError_t e = vc.reserve(rows * n_lab);
      if (e == hipSuccess) e = bp.reserve(rows * n_lab);
      if (e == hipSuccess) {
        if (nstate(h)) launch_ns_viterbi(h->stream, l, b->view(), u0, u1 - u0, sm.ns.S, sm.ns.TD, sm.ns.TO, sm.ns.TE, vc, bp, d_lab, d_n, d_cost);
        else launch_stdseg_viterbi(h->stream, l, n_lab, b->view(), u0, u1 - u0, sm.sg.S, sm.sg.MX, vc, bp, d_lab, d_n, d_cost);
        e = hipStreamSynchronize(h->stream);
      }
      if (e != hipSuccess) { rc = fail(h, SCRF_ERR_HIP, "scrf_viterbi_batch: %s", hipGetErrorString(e)); break; }
      u0 = u1;
    }
  }
  else
    rc = decode_chunks(h, b, Need::viterbi(), [&](const ChunkBufs& cb, uint32_t u0, uint32_t u1, bool fast) {
      if (fast && viterbi_fast_supported(dp_shape(l)))
        launch_viterbi_fast(h->stream, h->kn, l, b->view(), u0, u1 - u0, arc_src(h, cb, fast), cb.bp_b, cb.bp_e, d_lab, d_n, d_cost);
      else if (segtrans(h)) launch_viterbi_segtrans(h->stream, l, b->view(), u0, u1 - u0, cb.S, cb.M, cb.bp_b, cb.bp_e, d_lab, d_n, d_cost);
      else launch_viterbi(h->stream, l, b->view(), u0, u1 - u0, arc_src(h, cb, fast), cb.bp_b, cb.bp_e, d_lab, d_n, d_cost);
    });
  if (rc != SCRF_OK) return rc;
  return decode_result_fetch(h, b, "scrf_viterbi_batch", call, seg_labels, max_labels, lab_off, best_cost);
}

// the transcripts of a call and two offset arrays ([U + 1] each: phone_off | a second one, the cells before each utterance),
// uploaded once per call into buffers kept across calls (scrf_align_batch, scrf_transcript_batch)
static int upload_transcripts(scrf_handle h, uint32_t U, const uint32_t* phones, const uint64_t* phone_off, const uint64_t* cell_off) {
  const uint64_t NP = phone_off[U];
  RCCHK(reserve_drained(h, h->tx.ph, NP));
  RCCHK(reserve_drained(h, h->tx.off, 2 * ((size_t)U + 1)));   // two offset arrays
  if (NP) HIPCHK(h, hipMemcpyAsync(h->tx.ph, phones, sizeof(uint32_t) * NP, hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipMemcpyAsync(h->tx.off, phone_off, sizeof(uint64_t) * (U + 1), hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipMemcpyAsync(h->tx.off + (U + 1), cell_off, sizeof(uint64_t) * (U + 1), hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));   // the host arrays are the caller's (and pageable)
  return SCRF_OK;
}

// The checks of a call's transcripts, one pass in a fixed order (scrf_align_batch, scrf_transcript_batch), and cell_off [U + 1]:
// the T x K cells before each utterance, none for a transcript that no path realises (the chunk planner sizes a chunk with
// them).  no_repeats: with SCRF_ALIGN_RUNS equal neighbours are refused.  lds(K): the bytes of LDS the caller's workgroup
// kernel needs for a transcript of K phones, `cell_bytes` a cell, or 0 where another kernel serves it; a workgroup has
// SCRF_LDS_BYTES less `lds_less`.  An offset past phone_off[U] counts as a decrease: no phone is read outside the array.
template <class Lds>
static int check_transcripts(scrf_handle h, scrf_batch b, const char* fn, const uint32_t* phones, const uint64_t* phone_off, int mode,
                             bool no_repeats, int cell_bytes, int lds_less, Lds&& lds, std::vector<uint64_t>* cell_off) {
  const ScrfLayout& l = h->lay;
  const uint32_t U = b->U;
  const uint64_t NP = phone_off[U];
  if (phone_off[0] != 0 || (NP && !phones)) return fail(h, SCRF_ERR_INVALID, "%s: phone_off must start at 0 and phones must be given", fn);
  char less[24] = "";
  if (lds_less) snprintf(less, sizeof(less), " less %d", lds_less);
  cell_off->assign(U + 1, 0);
  for (uint32_t u = 0; u < U; u++) {
    if (phone_off[u + 1] < phone_off[u] || phone_off[u + 1] > NP) return fail(h, SCRF_ERR_INVALID, "%s: phone_off decreases at utterance %u", fn, u);
    const uint64_t K = phone_off[u + 1] - phone_off[u];
    const uint32_t* ph = phones + phone_off[u];
    for (uint64_t k = 0; k < K; k++) {
      if (ph[k] >= l.L)
        return fail(h, SCRF_ERR_INVALID, "%s: phone %u at position %llu of utterance %u's transcript (the model has %u)", fn, ph[k],
                    (unsigned long long)k, u, l.L);
      if (no_repeats && mode == SCRF_ALIGN_RUNS && k >= 1 && ph[k] == ph[k - 1])
        return fail(h, SCRF_ERR_INVALID, "%s: utterance %u's transcript repeats phone %u at position %llu; with SCRF_ALIGN_RUNS equal "
                    "neighbours make the sum count a path more than once: collapse them first", fn, u, ph[k], (unsigned long long)k);
    }
    const bool fits = scrf_align_feasible(b->T[u], K, l.D, mode);
    const size_t need = fits ? lds(K) : 0;
    if (need > (size_t)(SCRF_LDS_BYTES - lds_less))
      return fail(h, SCRF_ERR_INVALID, "%s: utterance %u's transcript of %llu phones needs (%u + 2) x %llu x %d = %zu bytes of LDS, "
                  "a workgroup has %d%s", fn, u, (unsigned long long)K, l.D, (unsigned long long)K, cell_bytes, need, SCRF_LDS_BYTES, less);
    (*cell_off)[u + 1] = (*cell_off)[u] + (fits ? (uint64_t)b->T[u] * K : 0);
  }
  return SCRF_OK;
}

// ---------------------------------------------------------------------------------------------
// batched forced alignment: scrf_viterbi_batch's chunk loop and score stage, a constrained search
// ---------------------------------------------------------------------------------------------
extern "C" int scrf_align_batch(scrf_handle h, scrf_batch b, const uint32_t* phones, const uint64_t* phone_off, int mode,
                                uint32_t* seg_labels, uint64_t max_labels, uint64_t* lab_off, float* cost) {
  if (!h || !b || !phone_off || !seg_labels || !lab_off) return SCRF_ERR_INVALID;
  RCCHK(model_ok(h, "scrf_align_batch", "forced alignment"));
  if (mode != SCRF_ALIGN_ONE && mode != SCRF_ALIGN_RUNS)
    return fail(h, SCRF_ERR_INVALID, "scrf_align_batch: unknown mode %d (SCRF_ALIGN_ONE = 0, SCRF_ALIGN_RUNS = 1)", mode);
  const ScrfLayout& l = h->lay;
  if (l.D > 0x7fff)
    return fail(h, SCRF_ERR_INVALID, "scrf_align_batch: maximum duration %u does not fit the 15 duration bits of a back pointer (at most %u)", l.D, 0x7fffu);
  const uint32_t U = b->U;
  // back-pointer cells before each utterance; the workgroup kernel takes the transcripts the wavefront kernel does not
  const bool wave_on = h->kn.align_wave && align_wave_supported(dp_shape(l));
  RCCHK(check_transcripts(h, b, "scrf_align_batch", phones, phone_off, mode, false, 4, 0,
                          [&](uint64_t K) { return (K > 64 || !wave_on) ? align_group_smem_bytes(dp_shape(l), K) : 0; }, &h->tx.bp_off));
  HIPCHK(h, hipSetDevice(h->device));
  CallTimer call(h);
  HIPCHK(h, h->dec.reserve(b->frame_off[b->U], b->U));
  RCCHK(upload_transcripts(h, U, phones, phone_off, h->tx.bp_off.data()));
  h->tx.n_al_calls++;
  RCCHK(decode_chunks(h, b, Need::alignment(), [&](const ChunkBufs& cb, uint32_t u0, uint32_t u1, bool fast) {
    const ScrfAlignArgs aa{h->tx.ph, h->tx.off, h->tx.off + (U + 1), cb.al_bp, mode};
    uint64_t k_max = 0;   // over the transcripts that fit
    for (uint32_t u = u0; u < u1; u++)
      if (h->tx.bp_off[u + 1] > h->tx.bp_off[u]) k_max = std::max(k_max, phone_off[u + 1] - phone_off[u]);
    const ScrfArcSrc src = arc_src(h, cb, fast);
    h->tx.n_al_chunks++;
    if (wave_on && k_max <= 64) {
      h->tx.n_al_wave++;
      KT_RUN("k_align_wave", h->stream, launch_align_wave(h->stream, l, b->view(), u0, u1 - u0, src, aa, h->dec.lab, h->dec.n, h->dec.cost));
    } else {
      h->tx.n_al_group++;
      KT_RUN("k_align_group", h->stream, launch_align_group(h->stream, l, b->view(), u0, u1 - u0, (uint32_t)k_max, src, aa, h->dec.lab, h->dec.n,
                                                            h->dec.cost));
    }
  }));
  return decode_result_fetch(h, b, "scrf_align_batch", call, seg_labels, max_labels, lab_off, cost);
}

// ---------------------------------------------------------------------------------------------
// batched N-best decoding: scrf_viterbi_batch's chunk loop and score stage, a search that keeps a list per
// state; the backtrace of a chunk runs before its scratch goes, into a result sized by what it found
// ---------------------------------------------------------------------------------------------
extern "C" int scrf_nbest_batch(scrf_handle h, scrf_batch b, uint32_t n_best, uint64_t* hyp_off, uint64_t* n_labels) {
  if (!h || !b || !hyp_off) return SCRF_ERR_INVALID;
  const char* fn = "scrf_nbest_batch";
  h->nb.batch = nullptr;   // whatever happens, the previous result is gone
  RCCHK(model_ok(h, fn, "N-best decoding"));
  const ScrfLayout& l = h->lay;
  if (l.D > 0x7fff) return fail(h, SCRF_ERR_INVALID, "%s: maximum duration %u does not fit the 15 duration bits of a back pointer (at most %u)", fn, l.D, 0x7fffu);
  if (l.L > 0xffff) return fail(h, SCRF_ERR_INVALID, "%s: %u labels do not fit the 16 label bits of a back pointer (at most %u)", fn, l.L, 0xffffu);
  if (n_best == 0 || n_best > 0xffff) return fail(h, SCRF_ERR_INVALID, "%s: n_best must be 1 .. 65535 (got %u)", fn, n_best);
  if (nbest_smem_bytes(dp_shape(l), n_best) > SCRF_LDS_BYTES)
    return fail(h, SCRF_ERR_INVALID, "%s: n_best %u with %u labels and maximum duration %u needs (%u + 2) x %u x %u x 4 + %zu = %zu bytes of LDS, "
                "a workgroup has %d", fn, n_best, l.L, l.D, l.D, l.L, n_best, nbest_smem_bytes(dp_shape(l), n_best) - sizeof(float) * ((size_t)l.D + 2) * l.L * n_best,
                nbest_smem_bytes(dp_shape(l), n_best), SCRF_LDS_BYTES);
  HIPCHK(h, hipSetDevice(h->device));
  const bool frame_model = h->cfg.model_type == SCRF_STDFRAME;
  const uint32_t U = b->U;
  RCCHK(reserve_drained(h, h->nb.hyp_off, (size_t)U + 1));
  CallTimer call(h);
  h->nb.n_calls++;
  ScrfBatchView bv = b->view();
  uint64_t n_lab = 0, n_hyp = 0;   // of the chunks done
  int rc2 = SCRF_OK;
  if (U == 0) HIPCHK(h, hipMemsetAsync(h->nb.hyp_off, 0, sizeof(uint64_t), h->stream));
  RCCHK(decode_chunks(h, b, Need::nbest_of(n_best), [&](const ChunkBufs& cb, uint32_t u0, uint32_t u1, bool fast) {
    if (rc2 != SCRF_OK) return;
    const uint32_t nutt = u1 - u0;
    h->nb.n_chunks++;
    if (fast) h->nb.n_fast_chunks++;
    KT_RUN("k_nbest", h->stream, launch_nbest(h->stream, l, bv, u0, nutt, arc_src(h, cb, fast), cb.nb));
    KT_RUN("k_nbest_count", h->stream, launch_nbest_count(h->stream, l, bv, u0, nutt, frame_model, cb.nb));
    KT_RUN("k_nbest_scan", h->stream, launch_nbest_scan(h->stream, cb.nb, u0, nutt, n_lab, n_hyp, h->nb.hyp_off));
    uint64_t tot[2] = {0, 0};   // the chunk's labels and hypotheses must have room before they are written
    hipError_t e = hipMemcpyAsync(tot, cb.nb.tot, sizeof(tot), hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    // what the chunks done wrote moves with a growing array
    if (e == hipSuccess) e = h->nb.lab.reserve_keep(n_lab + tot[0], n_lab, h->stream);
    if (e == hipSuccess) e = h->nb.cost.reserve_keep(n_hyp + tot[1], n_hyp, h->stream);
    if (e == hipSuccess) e = h->nb.lab_off.reserve_keep(n_hyp + tot[1] + 1, u0 ? n_hyp + 1 : 0, h->stream);   // (the first chunk finds nothing to keep)
    if (e != hipSuccess) { rc2 = fail(h, SCRF_ERR_HIP, "%s: %s", fn, hipGetErrorString(e)); return; }
    KT_RUN("k_nbest_trace", h->stream, launch_nbest_trace(h->stream, l, bv, u0, nutt, frame_model, cb.nb, h->nb.lab.cap(),
                                                          std::min(h->nb.cost.cap(), h->nb.lab_off.cap() - 1), h->nb.lab, h->nb.lab_off, h->nb.cost));
    n_lab += tot[0];
    n_hyp += tot[1];
  }));
  if (rc2 != SCRF_OK) return rc2;
  HIPCHK(h, hipGetLastError());
  h->nb.off.resize((size_t)U + 1);
  HIPCHK(h, hipMemcpyAsync(h->nb.off.data(), h->nb.hyp_off, sizeof(uint64_t) * ((size_t)U + 1), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  call.stop();
  if (h->nb.off[U] != n_hyp) return fail(h, SCRF_ERR_INVALID, "%s: hypothesis count mismatch (internal)", fn);
  memcpy(hyp_off, h->nb.off.data(), sizeof(uint64_t) * ((size_t)U + 1));
  if (n_labels) *n_labels = n_lab;
  h->nb.n_labels = n_lab;
  h->nb.batch = b;
  return SCRF_OK;
}

extern "C" int scrf_nbest_paths(scrf_handle h, scrf_batch b, uint32_t u0, uint32_t n, uint32_t* seg_labels, uint64_t max_labels,
                                uint64_t* lab_off, float* cost) {
  if (!h || !b) return SCRF_ERR_INVALID;
  const char* fn = "scrf_nbest_paths";
  if (h->nb.batch != b)
    return fail(h, SCRF_ERR_INVALID, "%s: no valid result for this batch (call scrf_nbest_batch first; new weights, another N-best call or "
                "destroying the batch drop it)", fn);
  if ((uint64_t)u0 + n > b->U) return fail(h, SCRF_ERR_INVALID, "%s: utterances %u .. %llu of a batch of %u", fn, u0, (unsigned long long)u0 + n, b->U);
  if (!lab_off) return SCRF_ERR_INVALID;
  const uint64_t h0 = h->nb.off[u0], nh = h->nb.off[u0 + n] - h0;
  if (nh == 0) { lab_off[0] = 0; return SCRF_OK; }
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipMemcpyAsync(lab_off, h->nb.lab_off + h0, sizeof(uint64_t) * (nh + 1), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  const uint64_t a0 = lab_off[0], na = lab_off[nh] - a0;
  for (uint64_t i = 0; i <= nh; i++) lab_off[i] -= a0;
  if (max_labels < na) return fail(h, SCRF_ERR_INVALID, "%s: room for %llu labels, %llu needed", fn, (unsigned long long)max_labels, (unsigned long long)na);
  if (na && !seg_labels) return SCRF_ERR_INVALID;
  if (na) HIPCHK(h, hipMemcpyAsync(seg_labels, h->nb.lab + a0, sizeof(uint32_t) * na, hipMemcpyDeviceToHost, h->stream));
  if (cost && nh) HIPCHK(h, hipMemcpyAsync(cost, h->nb.cost + h0, sizeof(float) * nh, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return SCRF_OK;
}

extern "C" int scrf_nbest_stats(scrf_handle h, uint64_t* n_calls, uint64_t* n_chunks, uint64_t* n_fast_chunks) {
  if (!h) return SCRF_ERR_INVALID;
  if (n_calls) *n_calls = h->nb.n_calls;
  if (n_chunks) *n_chunks = h->nb.n_chunks;
  if (n_fast_chunks) *n_fast_chunks = h->nb.n_fast_chunks;
  return SCRF_OK;
}

extern "C" int scrf_align_stats(scrf_handle h, uint64_t* n_calls, uint64_t* n_chunks, uint64_t* n_wave, uint64_t* n_group) {
  if (!h) return SCRF_ERR_INVALID;
  if (n_calls) *n_calls = h->tx.n_al_calls;
  if (n_chunks) *n_chunks = h->tx.n_al_chunks;
  if (n_wave) *n_wave = h->tx.n_al_wave;
  if (n_group) *n_group = h->tx.n_al_group;
  return SCRF_OK;
}

// ---------------------------------------------------------------------------------------------
// transcript scoring: label_free_run's chunk loop, score stage and free recursion (for Zx); the sums over the
// alignments of each transcript in place of the free occupancy walk
// ---------------------------------------------------------------------------------------------
struct TransOut : PostOut {
  double* log_num = nullptr;   // [U], always formed (the segment queries read it)
};

// The transcript kernels of a chunk, behind its recursion.  The free occupancy walk (k_post_occ*) does not run, so the
// per-frame state mass k_mass_check compares is not formed and that check is skipped here; the recursion's own checks (an
// emptied vector, a transition sum below DBL_MIN) still raise SCRF_ERR_NUMERIC, and so does a fitting transcript whose sum
// is not finite.
static int transcript_chunk(scrf_handle h, scrf_batch b, const uint64_t* phone_off, int mode, const TransOut& to, ChunkBufs& cb, uint32_t u0,
                            uint32_t u1, uint32_t* nl) {
  const ScrfLayout& l = h->lay;
  const uint32_t U = b->U;
  ScrfBatchView bv = b->view();
  uint64_t k_max = 0;   // over the transcripts that fit
  for (uint32_t u = u0; u < u1; u++)
    if (h->tx.cell_off[u + 1] > h->tx.cell_off[u]) k_max = std::max(k_max, phone_off[u + 1] - phone_off[u]);
  const ScrfTransArgs ta{h->tx.ph, h->tx.off, h->tx.off + (U + 1), h->tx.inv, h->tx.inv + phone_off[U], cb.tr_aB, cb.tr_bE,
                         mode, cb.lin ? 1 : 0, to.seg ? 1 : 0};
  h->tx.n_tr_chunks++;
  KT_RUN("k_transcript", cb.st, launch_transcript(cb.st, l, bv, u0, u1 - u0, k_max, cb.S, cb.smax, cb.M, cb.m_per_frame, ta, b->d_status,
                                                  to.log_num, to.occ, to.end));
  *nl += 1;
  if (to.seg) {
    const uint64_t q0 = to.lab_off[u0], nq = to.lab_off[u1] - q0;
    KT_RUN("k_transcript_seg", cb.st, launch_transcript_seg(cb.st, l, bv, u0, to.q_u, to.q_e, to.q_lab, q0, nq, cb.S, cb.smax, ta, to.log_num, to.seg));
    *nl += 1;
  }
  return SCRF_OK;
}

// The inverted lists of a call's (checked) transcripts into h->tx.inv_h, [inv_pos (sum K) | inv_off (U x (L + 1))]: per
// utterance its positions sorted by label (a counting sort: ascending inside a label).  Returns the number of entries.
static uint64_t inverted_lists(scrf_handle h, uint32_t U, const uint32_t* phones, const uint64_t* phone_off) {
  const ScrfLayout& l = h->lay;
  const uint64_t NP = phone_off[U], n_inv = NP + (uint64_t)U * (l.L + 1);
  h->tx.inv_h.assign(n_inv, 0);
  for (uint32_t u = 0; u < U; u++) {
    const uint64_t K = phone_off[u + 1] - phone_off[u];
    const uint32_t* ph = phones + phone_off[u];
    uint32_t* ioff = h->tx.inv_h.data() + NP + (uint64_t)u * (l.L + 1);
    uint32_t* ipos = h->tx.inv_h.data() + phone_off[u];
    for (uint64_t k = 0; k < K; k++) ioff[ph[k] + 1]++;
    for (uint32_t c = 0; c < l.L; c++) ioff[c + 1] += ioff[c];
    for (uint64_t k = 0; k < K; k++) ipos[ioff[ph[k]]++] = (uint32_t)k;   // ioff[c] now = the end of c's list = the start of c + 1's
    for (uint32_t c = l.L; c >= 1; c--) ioff[c] = ioff[c - 1];
    ioff[0] = 0;
  }
  return n_inv;
}

extern "C" int scrf_transcript_batch(scrf_handle h, scrf_batch b, const uint32_t* phones, const uint64_t* phone_off, int mode,
                                     double* log_num, double* zx, double* frame_post, double* end_post,
                                     const uint32_t* seg_labels, const uint64_t* lab_off, double* seg_post) {
  if (!h || !b || !phone_off) return SCRF_ERR_INVALID;
  const char* fn = "scrf_transcript_batch";
  RCCHK(model_ok(h, fn, "posterior output"));
  const ScrfLayout& l = h->lay;
  if (l.D > 0x7fff) return fail(h, SCRF_ERR_INVALID, "%s: maximum duration %u is not served (at most %u, as scrf_align_batch)", fn, l.D, 0x7fffu);
  if (mode != SCRF_ALIGN_ONE && mode != SCRF_ALIGN_RUNS)
    return fail(h, SCRF_ERR_INVALID, "%s: unknown mode %d (SCRF_ALIGN_ONE = 0, SCRF_ALIGN_RUNS = 1)", fn, mode);
  const uint32_t U = b->U;
  const uint64_t nF = b->frame_off[U];
  // the checks of every transcript and the cells before each utterance; 128 bytes of LDS go to the 16 per-wavefront parts of
  // end[t].  Then the inverted lists (inverted_lists)
  RCCHK(check_transcripts(h, b, fn, phones, phone_off, mode, true, 8, 128, [&](uint64_t K) { return transcript_smem_bytes(dp_shape(l), K); },
                          &h->tx.cell_off));
  std::vector<uint32_t> q;   // [3][nq]: utterance, end frame, label value
  uint64_t nq = 0;
  RCCHK(seg_queries(h, b, fn, seg_labels, lab_off, seg_post != nullptr, &q, &nq));
  const uint64_t n_inv = inverted_lists(h, U, phones, phone_off);
  HIPCHK(h, hipSetDevice(h->device));
  TransOut to;
  RCCHK(reserve_drained(h, h->tx.inv, n_inv));
  RCCHK(post_out_carve(h, b, frame_post, end_post, seg_post, q, nq, lab_off, U, &to, &to.log_num));
  if (n_inv) HIPCHK(h, hipMemcpyAsync(h->tx.inv, h->tx.inv_h.data(), sizeof(uint32_t) * n_inv, hipMemcpyHostToDevice, h->stream));
  RCCHK(upload_transcripts(h, U, phones, phone_off, h->tx.cell_off.data()));   // ends with a synchronize: q may go
  CallTimer call(h);
  h->tx.n_tr_calls++;
  const uint64_t fb0 = h->n_lin_fallback;
  int latch[2] = {0, 0};
  const int rc = run_with_redo(h, latch, [&] {
    return label_free_run(h, b, Need::transcript(prec_fast(h)), latch, [&](ChunkBufs& cb, uint32_t u0, uint32_t u1, uint32_t* nl) {
      return transcript_chunk(h, b, phone_off, mode, to, cb, u0, u1, nl);
    });
  });
  if (h->n_lin_fallback != fb0) h->tx.n_tr_redone++;
  if (rc != SCRF_OK) return rc;
  call.stop();
  if (latch[0] != 0) return fail(h, latch[0], "%s: utterance %d: %s", fn, latch[1], status_text(latch[0]));
  if (log_num) HIPCHK(h, hipMemcpyAsync(log_num, to.log_num, sizeof(double) * U, hipMemcpyDeviceToHost, h->stream));
  if (zx) HIPCHK(h, hipMemcpyAsync(zx, b->d_zx, sizeof(double) * U, hipMemcpyDeviceToHost, h->stream));
  if (frame_post) HIPCHK(h, hipMemcpyAsync(frame_post, to.occ, sizeof(double) * nF * l.L, hipMemcpyDeviceToHost, h->stream));
  if (end_post) HIPCHK(h, hipMemcpyAsync(end_post, to.end, sizeof(double) * nF, hipMemcpyDeviceToHost, h->stream));
  if (to.seg) HIPCHK(h, hipMemcpyAsync(seg_post, to.seg, sizeof(double) * nq, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return SCRF_OK;
}

extern "C" int scrf_transcript_stats(scrf_handle h, uint64_t* n_calls, uint64_t* n_chunks, uint64_t* n_redone) {
  if (!h) return SCRF_ERR_INVALID;
  if (n_calls) *n_calls = h->tx.n_tr_calls;
  if (n_chunks) *n_chunks = h->tx.n_tr_chunks;
  if (n_redone) *n_redone = h->tx.n_tr_redone;
  return SCRF_OK;
}

// ---------------------------------------------------------------------------------------------
// training from transcripts: the training pass over label arrays that are all SCRF_LAB_BAD, which leaves
// R = -gamma and XI = -xi (or the A^T B factors); the transcript sweep and the numerator kernels between the recursion and
// the posterior walk; R += G and the transition numerators behind it; then the count and reduce phases as they are.  One
// lane, no side route, no all-reduce overlap.
// ---------------------------------------------------------------------------------------------
// The batch reads as one whose every label is SCRF_LAB_BAD for the lifetime of this guard.  (k_xi_full and the posterior
// walks read next_lab where a label is present or not, so a null pointer will not do.)  The label pointers of the caller's
// batch are swapped and put back, because run_dp and the kernels' launchers take them from the batch (b->view(),
// b->d_next_lab) at a dozen places: like every call on a handle, the call is not to run beside another call on the same
// handle or batch (scrf_abi.h says so for this entry point).
struct AllBadLabels {
  scrf_batch b;
  uint32_t *lab, *next;
  AllBadLabels(scrf_batch b_, uint32_t* bad) : b(b_), lab(b_->d_labels), next(b_->d_next_lab) { b->d_labels = b->d_next_lab = bad; }
  ~AllBadLabels() { b->d_labels = lab; b->d_next_lab = next; }
  AllBadLabels(const AllBadLabels&) = delete;
  AllBadLabels& operator=(const AllBadLabels&) = delete;
};

static int soft_chunk(scrf_handle h, scrf_batch b, const uint64_t* phone_off, int mode, uint32_t u0, uint32_t u1, bool last, const Need& nd) {
  const ScrfLayout& l = h->lay;
  const uint32_t U = b->U, nutt = u1 - u0;
  const uint64_t nseg = b->seg_off[u1] - b->seg_off[u0];
  ChunkBufs cb;
  RCCHK(score_chunk(h, b, u0, u1, nd, &cb, SCORE_PASS));
  cb.grad = h->d_stage;
  cb.sums = h->d_sums_stage;
  FbRoute rt;
  rt.last = last;
  ScrfBatchView bv = b->view();
  uint64_t k_max = 0, cells_max = 0;
  for (uint32_t u = u0; u < u1; u++) {
    k_max = std::max(k_max, phone_off[u + 1] - phone_off[u]);
    cells_max = std::max(cells_max, h->tx.cell_off[u + 1] - h->tx.cell_off[u]);
  }
  const uint32_t t_max = longest_utt(b, u0, u1);
  const ScrfTransArgs ta{h->tx.ph, h->tx.off, h->tx.off + (U + 1), h->tx.inv, h->tx.inv + phone_off[U], cb.tr_aB, cb.tr_bE,
                         mode, cb.lin ? 1 : 0, 1};
  const ScrfSoftArgs sa{h->soft.log_num, b->d_status, cb.sn_aE, cb.sn_bB, cb.sn_G, cb.sn_adv, cb.sn_stay, cb.sn_tab};
  h->soft.n_chunks++;
  uint32_t nl = 0;
  // everything that reads the scores: the sweep (A, aB, bE), then G and the aE / bB cells
  auto numerators = [&]() -> int {
    KT_RUN("k_transcript", cb.st, launch_transcript(cb.st, l, bv, u0, nutt, k_max, cb.S, cb.smax, cb.M, cb.m_per_frame, ta, b->d_status,
                                                    h->soft.log_num, nullptr, nullptr));
    KT_RUN("k_soft_state", cb.st, launch_soft_state(cb.st, l, bv, u0, nutt, t_max, cb.S, cb.smax, ta, sa));
    KT_RUN("k_soft_trans", cb.st, launch_soft_trans(cb.st, l, bv, u0, nutt, cells_max, cb.S, cb.smax, ta, sa));
    nl += 3;
    HIPCHK(h, hipGetLastError());
    return SCRF_OK;
  };
  {
    PhaseTimer tm(h, PH_FB, cb.st);
    DpOpts o = DpOpts::training(rt);
    o.reads_scores = numerators;   // run_dp queues them while the scores exist (DpOpts)
    uint32_t nl_dp = 0;
    RCCHK(run_dp(h, b, u0, u1, cb, o, &nl_dp));
    KT_RUN("k_soft_add_r", cb.st, launch_soft_add_r(cb.st, cb.R, cb.sn_G, nseg * l.L));
    if (l.use_tf) KT_RUN("k_soft_add_xi", cb.st, launch_soft_add_xi(cb.st, l, bv, u0, nutt, t_max, cb.M, ta, sa, cb.XI));
    else KT_RUN("k_soft_trans_table", cb.st, launch_soft_trans_table(cb.st, l, bv, u0, nutt, k_max, cb.M, ta, sa, cb.grad));
    cb.z_ready = false;   // the fused form's Z was summed from R before the numerators went in: k_lin_z forms it again
    // the numerator of the batch sums (k_numer_reduce / k_fb left 0: no label was observed)
    HIPCHK(h, hipMemcpyAsync(b->d_numer + u0, h->soft.log_num.get() + u0, sizeof(double) * nutt, hipMemcpyDeviceToDevice, cb.st));
    tm.stop(nl + nl_dp + 2);
  }
  if (last) RCCHK(queue_status(h, b));
  ChunkCounts cc;
  RCCHK(fb_count(h, b, u0, u1, cb, rt, &cc));
  RCCHK(fb_reduce(h, b, u0, u1, cb, rt, cc));
  HIPCHK(h, hipGetLastError());
  return SCRF_OK;
}

static int soft_run(scrf_handle h, scrf_batch b, const uint64_t* phone_off, int mode, int latch[2]) {
  const ScrfLayout& l = h->lay;
  RCCHK(fb_begin(h, b));
  Need nd = Need::soft_training();
  set_batch_form(h, b, &nd);
  nd.la = false;   // the six-block Z of the linear-average form exists only inside k_post_z: SCRF_PREC_FASTLIN runs as FAST
  if (!l.use_tf) ensure_m0(h, h->stream);
  if (sparse(h)) relay_sparse_lambda(h, h->stream);
  for (uint32_t u0 = 0; u0 < b->U;) {
    const uint32_t u1 = plan_chunk(h, b, u0, nd);
    RCCHK(soft_chunk(h, b, phone_off, mode, u0, u1, u1 == b->U, nd));
    u0 = u1;
  }
  return fb_commit(h, latch);   // no observed transition counts to add (launch_add_trans_counts): there are no labels
}

extern "C" int scrf_fb_transcript_batch(scrf_handle h, scrf_batch b, const uint32_t* phones, const uint64_t* phone_off, int mode,
                                        double* log_num, double* zx) {
  if (!h || !b || !phone_off) return SCRF_ERR_INVALID;
  const char* fn = "scrf_fb_transcript_batch";
  RCCHK(model_ok(h, fn, "training from transcripts"));
  const ScrfLayout& l = h->lay;
  if (l.D > 0x7fff) return fail(h, SCRF_ERR_INVALID, "%s: maximum duration %u is not served (at most %u, as scrf_align_batch)", fn, l.D, 0x7fffu);
  if (mode != SCRF_ALIGN_ONE && mode != SCRF_ALIGN_RUNS)
    return fail(h, SCRF_ERR_INVALID, "%s: unknown mode %d (SCRF_ALIGN_ONE = 0, SCRF_ALIGN_RUNS = 1)", fn, mode);
  const uint32_t U = b->U;
  const uint64_t nF = b->frame_off[U];
  RCCHK(check_transcripts(h, b, fn, phones, phone_off, mode, true, 8, 128, [&](uint64_t K) { return transcript_smem_bytes(dp_shape(l), K); },
                          &h->tx.cell_off));
  // a transcript no path realises has no numerator: in training that is an error, not an empty sum
  for (uint32_t u = 0; u < U; u++)
    if (!scrf_align_feasible(b->T[u], phone_off[u + 1] - phone_off[u], l.D, mode))
      return fail(h, SCRF_ERR_INVALID, "%s: utterance %u's transcript of %llu phones does not fit its %u frames (%s, maximum duration %u)", fn, u,
                  (unsigned long long)(phone_off[u + 1] - phone_off[u]), b->T[u], mode == SCRF_ALIGN_ONE ? "SCRF_ALIGN_ONE" : "SCRF_ALIGN_RUNS", l.D);
  h->soft.ph_off.assign(phone_off, phone_off + U + 1);
  const uint64_t n_inv = inverted_lists(h, U, phones, phone_off);
  HIPCHK(h, hipSetDevice(h->device));
  RCCHK(reserve_drained(h, h->tx.inv, n_inv));
  RCCHK(reserve_drained(h, h->soft.log_num, U));
  if (nF > h->soft.bad.cap()) {
    RCCHK(reserve_drained(h, h->soft.bad, nF));
    HIPCHK(h, hipMemsetAsync(h->soft.bad, 0xff, sizeof(uint32_t) * h->soft.bad.cap(), h->stream));
  }
  if (n_inv) HIPCHK(h, hipMemcpyAsync(h->tx.inv, h->tx.inv_h.data(), sizeof(uint32_t) * n_inv, hipMemcpyHostToDevice, h->stream));
  RCCHK(upload_transcripts(h, U, phones, phone_off, h->tx.cell_off.data()));
  CallTimer call(h);
  h->soft.n_calls++;
  const uint64_t fb0 = h->n_lin_fallback;
  int latch[2] = {0, 0};
  int rc;
  {
    AllBadLabels unlabelled(b, h->soft.bad);
    rc = run_with_redo(h, latch, [&] { return soft_run(h, b, phone_off, mode, latch); });
  }
  if (h->n_lin_fallback != fb0) h->soft.n_redone++;
  if (rc != SCRF_OK) return rc;
  call.stop();
  if (latch[0] != 0) return fail(h, latch[0], "%s: utterance %d: %s", fn, latch[1], status_text(latch[0]));
  if (log_num || zx) {
    if (log_num) HIPCHK(h, hipMemcpyAsync(log_num, h->soft.log_num, sizeof(double) * U, hipMemcpyDeviceToHost, h->stream));
    if (zx) HIPCHK(h, hipMemcpyAsync(zx, b->d_zx, sizeof(double) * U, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
  }
  return SCRF_OK;
}

extern "C" int scrf_soft_stats(scrf_handle h, uint64_t* n_calls, uint64_t* n_chunks, uint64_t* n_redone) {
  if (!h) return SCRF_ERR_INVALID;
  if (n_calls) *n_calls = h->soft.n_calls;
  if (n_chunks) *n_chunks = h->soft.n_chunks;
  if (n_redone) *n_redone = h->soft.n_redone;
  return SCRF_OK;
}

extern "C" int scrf_batch_is_fused(scrf_handle h, scrf_batch b, int* fused) {
  if (!h || !b || !fused) return SCRF_ERR_INVALID;
  const BatchForm f = batch_form(h, b);
  // 1 for a fusable batch at every precision (decode fuses at SCRF_PREC_EXACT too); 3: hybrid; 2: training runs with the
  // linear window average
  *fused = f.fusable ? 1 : f.hybrid ? 3 : 0;
  if (*fused && f.la) *fused = 2;
  return SCRF_OK;
}

extern "C" int scrf_comm_stats(scrf_handle h, uint64_t* n_collectives, uint64_t* n_overlapped) {
  if (!h) return SCRF_ERR_INVALID;
  if (n_collectives) *n_collectives = h->n_collectives;
  if (n_overlapped) *n_overlapped = h->n_overlapped;
  return SCRF_OK;
}

extern "C" int scrf_set_frame_mass_check(scrf_handle h, int on) {
  if (!h) return SCRF_ERR_INVALID;
  h->frame_mass = on != 0;
  return SCRF_OK;
}

extern "C" int scrf_decode_stats(scrf_handle h, uint64_t* n_recomputed, uint64_t* n_fallback_chunks) {
  if (!h) return SCRF_ERR_INVALID;
  if (n_recomputed) *n_recomputed = h->dec.n_fix;
  if (n_fallback_chunks) *n_fallback_chunks = h->dec.n_fallback;
  return SCRF_OK;
}

// ---------------------------------------------------------------------------------------------
// minibatch reduce + optimizer
// ---------------------------------------------------------------------------------------------
extern "C" int scrf_comm_unique_id(void* id128) {
  std::string why;
  if (!id128) return SCRF_ERR_INVALID;
  if (!rccl_load(&why)) return fail(nullptr, SCRF_ERR_COMM, "%s", why.c_str());
  scrf_nccl_uid id;
  int r = g_rccl.GetUniqueId(&id);
  if (r != 0) return fail(nullptr, SCRF_ERR_COMM, "ncclGetUniqueId failed: %d", r);
  memcpy(id128, &id, 128);
  return SCRF_OK;
}

extern "C" int scrf_comm_init(scrf_handle h, const void* id128, int rank, int n_ranks) {
  if (!h || !id128 || n_ranks < 1 || rank < 0 || rank >= n_ranks) return SCRF_ERR_INVALID;
  std::string why;
  if (!rccl_load(&why)) return fail(h, SCRF_ERR_COMM, "%s", why.c_str());
  HIPCHK(h, hipSetDevice(h->device));
  scrf_nccl_uid id;
  memcpy(&id, id128, 128);
  int r = g_rccl.CommInitRank(&h->comm, n_ranks, id, rank);
  if (r != 0) return fail(h, SCRF_ERR_COMM, "ncclCommInitRank failed: %s", g_rccl.GetErrorString ? g_rccl.GetErrorString(r) : "?");
  h->rank = rank;
  h->nranks = n_ranks;
  return SCRF_OK;
}

__global__ void k_set_tail(double* sums8, int active, double e0, double e1, double e2, double e3) {
  sums8[3] = (double)active;
  sums8[4] = e0; sums8[5] = e1; sums8[6] = e2; sums8[7] = e3;
}
__global__ void k_div_by_active(double* __restrict__ g, uint32_t n, const double* __restrict__ sums4) {
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  double a = sums4[3];
  if (i < n && a > 0.0) g[i] = __ddiv_rn(g[i], a);  // grad[i] /= nStreams_active (:306-308)
}
__global__ void k_gauss_prior(double* __restrict__ g, uint32_t n, double inv) {
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) g[i] = __dsub_rn(g[i], __dmul_rn(g[i], inv));   // grad[i] -= grad[i] * invSquareVar
}

// ncclCommAbort: frees the communicator without waiting for outstanding collectives and makes the PEERS' pending
// operations fail (their watchdog below sees the asynchronous error) instead of leaving them in RCCL for ever.  The host
// calls it when a rank cannot enter or finish the per-step collective, then exits non-zero (a restart is a fresh process).
extern "C" int scrf_comm_abort(scrf_handle h) {
  if (!h) return SCRF_ERR_INVALID;
  if (h->comm) {
    if (g_rccl.CommAbort) g_rccl.CommAbort(h->comm);
    h->comm = nullptr;
  }
  return SCRF_OK;
}

// Bounded wait for the engine stream while a collective is on it: polls the stream and the communicator's asynchronous
// error state; after SCRF_COMM_TIMEOUT_S seconds (default 300) without completion, or on an asynchronous error (a peer
// aborted or died), the communicator is aborted and SCRF_ERR_COMM returned -- the caller ends the process.
static int wait_collective(scrf_handle h, const char* what) {
  const char* ts = getenv("SCRF_COMM_TIMEOUT_S");
  const double limit = ts && atof(ts) > 0 ? atof(ts) : 300.0;
  struct timespec t0, t1;
  clock_gettime(CLOCK_MONOTONIC, &t0);
  for (;;) {
    const hipError_t q = hipStreamQuery(h->stream);
    if (q == hipSuccess) return SCRF_OK;
    if (q != hipErrorNotReady) { scrf_comm_abort(h); return fail(h, SCRF_ERR_HIP, "%s: %s", what, hipGetErrorString(q)); }
    if (h->comm && g_rccl.CommGetAsyncError) {
      int ae = 0;
      if (g_rccl.CommGetAsyncError(h->comm, &ae) == 0 && ae != 0) {
        scrf_comm_abort(h);
        return fail(h, SCRF_ERR_COMM, "%s: rank %d: the communicator reports an asynchronous error (%s): a peer failed or aborted", what,
                    h->rank, g_rccl.GetErrorString ? g_rccl.GetErrorString(ae) : "?");
      }
    }
    clock_gettime(CLOCK_MONOTONIC, &t1);
    if ((double)(t1.tv_sec - t0.tv_sec) + 1e-9 * (double)(t1.tv_nsec - t0.tv_nsec) > limit) {
      scrf_comm_abort(h);
      return fail(h, SCRF_ERR_COMM, "%s: rank %d: the collective did not complete within %.0f s (SCRF_COMM_TIMEOUT_S): a peer died or never "
                  "joined; communicator aborted", what, h->rank, limit);
    }
    usleep(200);
  }
}

// ---- the per-step collective in two blocks (models with transition features, e.g. the TIMIT demo: 4.37 M weights) ----
// The weight vector interleaves, per label, [nsf state weights | L * ntf transition weights]; 98.7 % of the TIMIT-demo
// gradient are transition weights.  Block 1 = the transition weights of every label (L contiguous pieces, one RCCL
// group), block 0 = the state weights of every label packed with the 8 scalars into one small message.  Every rank
// issues block 1 then block 0, whatever it did before (active, exhausted or failed): the sequence is part of the protocol.
// Inside scrf_fb_batch_allreduce block 1 is issued early, on the second stream, under the state contraction.
__global__ void k_pack_state(const double* __restrict__ grad, const double* __restrict__ sums8, uint32_t L, uint32_t stride,
                             uint32_t nsf, double* __restrict__ pack) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < L * nsf) pack[i] = grad[(size_t)(i / nsf) * stride + i % nsf];
  else if (i < L * nsf + 8) pack[i] = sums8[i - L * nsf];
}
__global__ void k_unpack_state(const double* __restrict__ pack, uint32_t L, uint32_t stride, uint32_t nsf, double* __restrict__ grad,
                               double* __restrict__ sums8) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < L * nsf) grad[(size_t)(i / nsf) * stride + i % nsf] = pack[i];
  else if (i < L * nsf + 8) sums8[i - L * nsf] = pack[i];
}
static int allreduce_block(scrf_handle h, hipStream_t st, int part) {
  const ScrfLayout& l = h->lay;
  int r = 0;
  if (part == 1) {
    if (g_rccl.GroupStart && g_rccl.GroupEnd) r = g_rccl.GroupStart();
    for (uint32_t c = 0; c < l.L && r == 0; c++) {
      double* p = h->d_grad + (size_t)c * l.stride + l.nsf;
      r = g_rccl.AllReduce(p, p, (size_t)l.L * l.ntf, SCRF_NCCL_DOUBLE, SCRF_NCCL_SUM, h->comm, st);
    }
    if (g_rccl.GroupStart && g_rccl.GroupEnd) { const int r2 = g_rccl.GroupEnd(); if (r == 0) r = r2; }
  } else {
    const uint32_t n = l.L * l.nsf + 8;
    if (h->d_pack.reserve(n) != hipSuccess) { scrf_comm_abort(h); return fail(h, SCRF_ERR_HIP, "hipMalloc of the pack buffer failed"); }
    hipLaunchKernelGGL(k_pack_state, dim3((n + 255) / 256), dim3(256), 0, st, h->d_grad, h->d_sums, l.L, l.stride, l.nsf, h->d_pack);
    r = g_rccl.AllReduce(h->d_pack, h->d_pack, n, SCRF_NCCL_DOUBLE, SCRF_NCCL_SUM, h->comm, st);
    hipLaunchKernelGGL(k_unpack_state, dim3((n + 255) / 256), dim3(256), 0, st, h->d_pack, l.L, l.stride, l.nsf, h->d_grad, h->d_sums);
  }
  if (r != 0) {
    scrf_comm_abort(h);
    return fail(h, SCRF_ERR_COMM, "ncclAllReduce (block %d) failed: %s", part, g_rccl.GetErrorString ? g_rccl.GetErrorString(r) : "?");
  }
  return SCRF_OK;
}

extern "C" int scrf_allreduce_grad_ex(scrf_handle h, int active, const double* extra_in, uint32_t n_extra, double* sums4,
                                      double* extra_out) {
  if (!h || n_extra > 4 || (n_extra && !extra_in)) return SCRF_ERR_INVALID;
  // a rank that fails on its way into or out of the collective must not leave the others waiting in RCCL: every error
  // path below aborts the communicator first (the peers' wait_collective then ends with an error, not a hang)
#define ARCHK(call)                                                                                        \
  do {                                                                                                     \
    hipError_t e_ = (call);                                                                                \
    if (e_ != hipSuccess) { scrf_comm_abort(h); h->early_done = false; return fail(h, SCRF_ERR_HIP, "%s failed: %s", #call, hipGetErrorString(e_)); } \
  } while (0)
  ARCHK(hipSetDevice(h->device));
  const uint32_t n = h->lay.lambda_len;
  double e[4] = {0, 0, 0, 0};
  for (uint32_t i = 0; i < n_extra; i++) e[i] = extra_in[i];
  hipLaunchKernelGGL(k_set_tail, dim3(1), dim3(1), 0, h->stream, h->d_sums, active ? 1 : 0, e[0], e[1], e[2], e[3]);
  ARCHK(hipGetLastError());
  if (h->comm) {
    h->n_collectives++;
    if (two_block_reduce(h)) {
      const bool early = h->early_done;
      h->early_done = false;
      if (early) h->n_overlapped++;
      if (early) ARCHK(hipStreamWaitEvent(h->stream, h->ev_join, 0));   // block 1 went out on the second stream already
      else { const int rc = allreduce_block(h, h->stream, 1); if (rc != SCRF_OK) return rc; }
      const int rc = allreduce_block(h, h->stream, 0);
      if (rc != SCRF_OK) return rc;
    } else {
      int r = g_rccl.AllReduce(h->d_grad, h->d_grad, n, SCRF_NCCL_DOUBLE, SCRF_NCCL_SUM, h->comm, h->stream);
      if (r == 0) r = g_rccl.AllReduce(h->d_sums, h->d_sums, 8, SCRF_NCCL_DOUBLE, SCRF_NCCL_SUM, h->comm, h->stream);
      if (r != 0) {
        scrf_comm_abort(h);
        return fail(h, SCRF_ERR_COMM, "ncclAllReduce failed: %s", g_rccl.GetErrorString ? g_rccl.GetErrorString(r) : "?");
      }
    }
  }
  hipLaunchKernelGGL(k_div_by_active, dim3((n + 255) / 256), dim3(256), 0, h->stream, h->d_grad, n, h->d_sums);
  ARCHK(hipGetLastError());
  if (sums4 || extra_out || h->comm) {
    double s8[8];
    ARCHK(hipMemcpyAsync(s8, h->d_sums, sizeof(double) * 8, hipMemcpyDeviceToHost, h->stream));
    if (h->comm) {
      const int rc = wait_collective(h, "scrf_allreduce_grad");
      if (rc != SCRF_OK) return rc;
    } else ARCHK(hipStreamSynchronize(h->stream));
    if (sums4) memcpy(sums4, s8, sizeof(double) * 4);
    if (extra_out) memcpy(extra_out, s8 + 4, sizeof(double) * n_extra);
  }
#undef ARCHK
  return SCRF_OK;
}

// scrf_fb_batch + scrf_allreduce_grad_ex in one call, for a host whose rank runs exactly one batch per step (the
// distributed minibatch accumulator): the all-reduce of the transition block overlaps the state contraction (above).
// The batch's own failure is reported through *fb_status (and extra[fail_slot] is raised, `active` cleared) while the
// collective still runs -- the peers learn it from the summed flag; the return value is the collective's.
extern "C" int scrf_fb_batch_allreduce(scrf_handle h, scrf_batch b, int active, const double* extra_in, uint32_t n_extra,
                                       uint32_t fail_slot, double* sums4, double* extra_out, int* fb_status) {
  if (!h || !b || n_extra > 4 || (n_extra && !extra_in) || (n_extra && fail_slot >= n_extra)) return SCRF_ERR_INVALID;
  h->overlap_comm = true;
  h->early_done = false;
  const int frc = scrf_fb_batch(h, b, nullptr, nullptr);
  h->overlap_comm = false;
  if (fb_status) *fb_status = frc;
  if (frc == SCRF_ERR_HIP || frc == SCRF_ERR_COMM) {   // the device or the communicator is gone: no collective can follow
    scrf_comm_abort(h);
    h->early_done = false;
    return frc;
  }
  const std::string batch_err = h->err;
  double e[4] = {0, 0, 0, 0};
  for (uint32_t i = 0; i < n_extra; i++) e[i] = extra_in[i];
  if (frc != SCRF_OK && n_extra) e[fail_slot] = 1.0;
  const int rc = scrf_allreduce_grad_ex(h, frc == SCRF_OK ? active : 0, e, n_extra, sums4, extra_out);
  if (rc == SCRF_OK && frc != SCRF_OK) h->err = batch_err;   // scrf_last_error keeps the batch's message
  return rc;
}
extern "C" int scrf_allreduce_grad(scrf_handle h, int active, double* sums4) {
  return scrf_allreduce_grad_ex(h, active, nullptr, 0, sums4, nullptr);
}

extern "C" int scrf_gauss_prior(scrf_handle h, float inv_square_var) {
  if (!h) return SCRF_ERR_INVALID;
  HIPCHK(h, hipSetDevice(h->device));
  const uint32_t n = h->lay.lambda_len;
  hipLaunchKernelGGL(k_gauss_prior, dim3((n + 255) / 256), dim3(256), 0, h->stream, h->d_grad, n, (double)inv_square_var);
  HIPCHK(h, hipGetLastError());
  return SCRF_OK;
}

extern "C" int scrf_div_grad(scrf_handle h, double d) {
  if (!h || d == 0.0) return SCRF_ERR_INVALID;
  HIPCHK(h, hipSetDevice(h->device));
  launch_scale(h->stream, h->d_grad, h->lay.lambda_len, d, 1);
  HIPCHK(h, hipGetLastError());
  return SCRF_OK;
}

extern "C" int scrf_scale_grad(scrf_handle h, double s) {
  if (!h) return SCRF_ERR_INVALID;
  HIPCHK(h, hipSetDevice(h->device));
  launch_scale(h->stream, h->d_grad, h->lay.lambda_len, s, 0);
  HIPCHK(h, hipGetLastError());
  return SCRF_OK;
}

extern "C" int scrf_sgd_step(scrf_handle h, double lr_or_eta, int use_adagrad, double eps) {
  if (!h) return SCRF_ERR_INVALID;
  HIPCHK(h, hipSetDevice(h->device));
  launch_sgd_step(h->stream, h->d_lambda, h->d_lambda_acc, h->d_gsa, h->d_grad, h->lay.lambda_len, lr_or_eta,
                  use_adagrad, eps);
  HIPCHK(h, hipMemsetAsync(h->d_sums, 0, sizeof(double) * 4, h->stream));
  h->m0_valid = false;
  h->lp.batch = nullptr;
  h->nb.batch = nullptr;
  HIPCHK(h, hipGetLastError());
  return SCRF_OK;
}

// ---------------------------------------------------------------------------------------------
// measurement
// ---------------------------------------------------------------------------------------------
extern "C" int scrf_kernel_timing(scrf_handle h, char* buf, size_t cap) {
  if (!h || !buf || cap == 0) return SCRF_ERR_INVALID;
  std::string out;
  char line[256];
  for (const auto& k : h->tm.ktimes) {
    snprintf(line, sizeof line, "%s\t%.6f\t%u\n", k.name.c_str(), k.ms, k.n);
    out += line;
  }
  if (out.size() + 1 > cap) return fail(h, SCRF_ERR_INVALID, "scrf_kernel_timing: buffer of %zu bytes too small (%zu needed)", cap, out.size() + 1);
  memcpy(buf, out.c_str(), out.size() + 1);
  return SCRF_OK;
}
extern "C" int scrf_train_stats(scrf_handle h, uint64_t* n_lin_fallback) {
  if (!h) return SCRF_ERR_INVALID;
  if (n_lin_fallback) *n_lin_fallback = h->n_lin_fallback;
  return SCRF_OK;
}
extern "C" int scrf_posterior_stats(scrf_handle h, uint64_t* n_split, uint64_t* n_whole) {
  if (!h) return SCRF_ERR_INVALID;
  if (n_split) *n_split = h->n_post_split;
  if (n_whole) *n_whole = h->n_post_whole;
  return SCRF_OK;
}
extern "C" int scrf_enable_timing(scrf_handle h, int on) { if (!h) return SCRF_ERR_INVALID; h->tm.on = on != 0; return SCRF_OK; }
extern "C" int scrf_last_timing(scrf_handle h, float* ms, uint32_t* n_launch) {
  if (!h) return SCRF_ERR_INVALID;
  if (ms) memcpy(ms, h->tm.ms, sizeof(h->tm.ms));
  if (n_launch) memcpy(n_launch, h->tm.nlaunch, sizeof(h->tm.nlaunch));
  return SCRF_OK;
}
