// transcript_args_check.cpp -- TEST-ONLY stand-alone program over the host side of transcript scoring
// (asr-craft_amd/host/crf_transcript.cpp: crf_amd_transcript_scores), linked against the ABI stub (scrf_stub.cpp) plus the
// three entry points below that the stub does not have.  No GPU, no Python: tests/test_host_transcript_args.py compiles it
// with -fsanitize=address,undefined and runs it.  The stand-ins check what the host hands the ABI (transcripts read from
// the node labels, RUNS collapsing, offsets, capacities, which pointers are NULL) and write every output array to its full
// extent, so that a buffer the host sized wrongly is an AddressSanitizer report.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include <stdexcept>
#include <string>
#include <vector>

#include "crf_amd.h"

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "FAILED line %d: %s\n", __LINE__, #c); exit(1); } } while (0)

static const uint32_t L = 3, D = 3, W = 2;
static const uint32_t NONE = CRF_LAB_BAD;
// frame labels per utterance: runs; a run of 5 (two pieces of the label stream); phone-duration labels; nothing labelled
static const std::vector<std::vector<uint32_t> > HARD = {{0, 1, 1}, {2, 2, 2, 2, 2}, {1, 0, 0, 2, 2, 2, 4, 4}, {NONE, NONE, NONE, NONE}};

static std::vector<uint32_t> g_T;                 // utterance lengths of the batch the host built
static int g_mode = -1, g_calls[3] = {0, 0, 0};   // align, transcript, posteriors
static std::vector<uint32_t> g_phones;
static std::vector<uint64_t> g_poff;

static void check_transcripts(const uint32_t* phones, const uint64_t* phone_off, int mode) {
  const size_t U = g_T.size();
  CHECK(phone_off && phone_off[0] == 0);
  for (size_t u = 0; u < U; u++) {
    CHECK(phone_off[u + 1] >= phone_off[u]);
    for (uint64_t k = phone_off[u]; k < phone_off[u + 1]; k++) {
      CHECK(phones[k] < L);
      if (mode == SCRF_ALIGN_RUNS && k > phone_off[u]) CHECK(phones[k] != phones[k - 1]);   // the engine refuses these
    }
  }
  g_phones.assign(phones, phones + phone_off[U]);
  g_poff.assign(phone_off, phone_off + U + 1);
  g_mode = mode;
}

extern "C" {
// one segment per frame carrying the transcript's first phone; an empty transcript gets no labels and cost +inf
int scrf_align_batch(scrf_handle, scrf_batch, const uint32_t* phones, const uint64_t* phone_off, int mode, uint32_t* seg_labels,
                     uint64_t max_labels, uint64_t* lab_off, float* cost) {
  g_calls[0]++;
  check_transcripts(phones, phone_off, mode);
  uint64_t nf = 0;
  for (uint32_t t : g_T) nf += t;
  CHECK(seg_labels && lab_off && max_labels == nf);
  for (uint64_t i = 0; i < max_labels; i++) seg_labels[i] = 0xdeadbeefu;   // the whole capacity is the callee's
  uint64_t pos = 0;
  for (size_t u = 0; u < g_T.size(); u++) {
    lab_off[u] = pos;
    const bool fits = phone_off[u + 1] > phone_off[u];
    if (fits) for (uint32_t t = 0; t < g_T[u]; t++) seg_labels[pos++] = phones[phone_off[u]];
    if (cost) cost[u] = fits ? 1.5f * (float)u : INFINITY;
  }
  lab_off[g_T.size()] = pos;
  return SCRF_OK;
}
int scrf_transcript_batch(scrf_handle, scrf_batch, const uint32_t* phones, const uint64_t* phone_off, int mode, double* log_num, double* zx,
                          double* frame_post, double* end_post, const uint32_t* seg_labels, const uint64_t* lab_off, double* seg_post) {
  g_calls[1]++;
  const size_t U = g_T.size();
  if (g_calls[0]) {   // the alignment of the same call saw the same transcripts
    CHECK(mode == g_mode && g_poff == std::vector<uint64_t>(phone_off, phone_off + U + 1));
    CHECK(g_phones == std::vector<uint32_t>(phones, phones + phone_off[U]));
  }
  check_transcripts(phones, phone_off, mode);
  CHECK(!frame_post && !end_post);   // the host unit asks for neither
  for (size_t u = 0; u < U; u++) {
    const bool fits = phone_off[u + 1] > phone_off[u];
    if (log_num) log_num[u] = fits ? -10.0 - (double)u : -INFINITY;
    if (zx) zx[u] = 100.0 + (double)u;
  }
  if (seg_post) {
    CHECK(seg_labels && lab_off && lab_off[0] == 0);
    for (size_t u = 0; u < U; u++)
      for (uint64_t i = lab_off[u]; i < lab_off[u + 1]; i++) { CHECK(seg_labels[i] < L * D); seg_post[i] = 0.5 + 0.001 * (double)i; }
  } else {
    CHECK(!seg_labels && !lab_off);
  }
  return SCRF_OK;
}
int scrf_posteriors_batch(scrf_handle, scrf_batch, double* zx, double* frame_post, double* end_post, const uint32_t* seg_labels,
                          const uint64_t* lab_off, double* seg_post) {
  g_calls[2]++;
  CHECK(!zx && !frame_post && !end_post && seg_labels && lab_off && seg_post);
  for (uint64_t i = 0; i < lab_off[g_T.size()]; i++) seg_post[i] = 0.25 + 0.001 * (double)i;
  return SCRF_OK;
}
}

static CRF_FeatureMap_config g_cfg;   // outlives the model, which keeps a pointer to it

static void make_model(CRF_Model* crf) {
  const uint32_t F = 8 * W + D;
  CRF_FeatureMap_config& c = g_cfg;
  c.map_type = STDSTATE;
  c.numLabs = L; c.numFeas = F; c.numStates = 1;
  c.useStateFtrs = true; c.stateFidxStart = 0; c.stateFidxEnd = F - 1;
  c.useTransFtrs = false; c.transFidxStart = 0; c.transFidxEnd = F - 1;
  c.useStateBias = true; c.useTransBias = true; c.stateBiasVal = 1.0; c.transBiasVal = 1.0;
  c.maxDur = D; c.durFtrStart = 0; c.nActualLabs = L;
  crf->setLabMaxDur(D);
  crf->setNActualLabs(L);
  crf->setModelType(STDSEG_NO_DUR_NO_SEGTRANSFTR);
  crf->setFeatureMap(CRF_FeatureMap::createFeatureMap(&c));
}

static void fill(CRF_MemoryFeatureStream* strm, size_t n_utts, bool with_labels) {
  g_T.clear();
  for (size_t u = 0; u < n_utts; u++) {
    const size_t T = HARD[u].size();
    std::vector<std::vector<float> > fr(1, std::vector<float>(T * W));
    for (size_t i = 0; i < T * W; i++) fr[0][i] = 0.125f * (float)((i + 3 * u) % 7);
    strm->addUtterance(fr, with_labels ? HARD[u] : std::vector<uint32_t>());
    g_T.push_back((uint32_t)T);
  }
}

template <class F>
static std::string thrown(F f) {
  try { f(); } catch (std::exception& e) { return e.what(); }
  return "";
}

int main() {
  const std::vector<scrf_stream_recipe> rec = {scrf_stream_recipe{W, 0, 0, 1}};
  // 1. the whole call in both modes: transcripts, alignment, both kinds of segment posteriors
  for (int mode : {SCRF_ALIGN_RUNS, SCRF_ALIGN_ONE}) {
    CRF_Model crf(L);
    make_model(&crf);
    CRF_MemoryFeatureStream strm(rec, D, L);
    fill(&strm, HARD.size(), true);
    strm.rewind();
    CHECK(strm.nextseg() != QN_SEGID_BAD);
    g_calls[0] = g_calls[1] = g_calls[2] = 0;
    std::vector<double> ln, zx;
    std::vector<uint32_t> np;
    std::vector<std::vector<uint32_t> > labs;
    std::vector<float> costs;
    std::vector<std::vector<double> > given, free_;
    bool at_end = false;
    const size_t U = crf_amd_transcript_scores(&strm, &crf, 256, mode, &ln, &zx, &np, &labs, &costs, &given, &free_, &at_end);
    CHECK(U == HARD.size() && at_end && g_calls[0] == 1 && g_calls[1] == 1 && g_calls[2] == 1 && g_mode == mode);
    // label % L of every labelled node, equal neighbours collapsed (the run of 5 frames is two nodes of phone 2: one phone)
    const std::vector<uint32_t> want_runs = {0, 1, 2, 1, 0, 2, 1};
    if (mode == SCRF_ALIGN_RUNS) {
      CHECK(g_phones == want_runs && g_poff == (std::vector<uint64_t>{0, 2, 3, 7, 7}));
      CHECK(np == (std::vector<uint32_t>{2, 1, 4, 0}));
    } else {
      CHECK(np == (std::vector<uint32_t>{2, 2, 4, 0}));   // ONE keeps the two pieces of the long run
    }
    CHECK(ln.size() == U && zx.size() == U && np.size() == U && labs.size() == U && costs.size() == U && given.size() == U && free_.size() == U);
    for (size_t u = 0; u < U; u++) {
      const bool fits = np[u] > 0;
      CHECK(fits == (u != 3));
      CHECK(fits ? ln[u] == -10.0 - (double)u : (std::isinf(ln[u]) && ln[u] < 0));
      CHECK(zx[u] == 100.0 + (double)u);
      CHECK(labs[u].size() == (fits ? g_T[u] : 0) && given[u].size() == labs[u].size() && free_[u].size() == labs[u].size());
      CHECK(fits ? costs[u] == 1.5f * (float)u : std::isinf(costs[u]));
      for (size_t i = 0; i < labs[u].size(); i++) CHECK(given[u][i] >= 0.5 && free_[u][i] >= 0.25 && free_[u][i] < 0.5);
    }
  }
  // 2. scores only: no alignment, no queries; a bunch of 2 leaves the stream on the third utterance
  {
    CRF_Model crf(L);
    make_model(&crf);
    CRF_MemoryFeatureStream strm(rec, D, L);
    fill(&strm, 3, true);
    strm.rewind();
    CHECK(strm.nextseg() != QN_SEGID_BAD);
    g_calls[0] = g_calls[1] = g_calls[2] = 0;
    std::vector<double> ln;
    bool at_end = true;
    g_T.resize(2);
    CHECK(crf_amd_transcript_scores(&strm, &crf, 2, SCRF_ALIGN_RUNS, &ln, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &at_end) == 2);
    CHECK(!at_end && ln.size() == 2 && g_calls[0] == 0 && g_calls[1] == 1 && g_calls[2] == 0);
    g_T.assign(1, (uint32_t)HARD[2].size());
    CHECK(crf_amd_transcript_scores(&strm, &crf, 2, SCRF_ALIGN_RUNS, &ln, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &at_end) == 1);
    CHECK(at_end && ln.size() == 1 && g_calls[1] == 2);
  }
  // 3. the argument checks: results of the aligned paths without the paths; a stream without labels
  {
    CRF_Model crf(L);
    make_model(&crf);
    CRF_MemoryFeatureStream strm(rec, D, L);
    fill(&strm, 2, false);
    strm.rewind();
    CHECK(strm.nextseg() != QN_SEGID_BAD);
    std::vector<float> costs;
    std::vector<std::vector<double> > sp;
    std::string m = thrown([&] { crf_amd_transcript_scores(&strm, &crf, 2, SCRF_ALIGN_RUNS, nullptr, nullptr, nullptr, nullptr, &costs, nullptr, nullptr, nullptr); });
    CHECK(m.find("pass labels as well") != std::string::npos);
    m = thrown([&] { crf_amd_transcript_scores(&strm, &crf, 2, SCRF_ALIGN_RUNS, nullptr, nullptr, nullptr, nullptr, nullptr, &sp, nullptr, nullptr); });
    CHECK(m.find("pass labels as well") != std::string::npos);
    // (the refused calls did not advance the stream.)  Without labels every node is unlabelled: empty transcripts, -inf
    std::vector<double> ln;
    std::vector<uint32_t> np;
    g_calls[1] = 0;
    CHECK(crf_amd_transcript_scores(&strm, &crf, 2, SCRF_ALIGN_RUNS, &ln, nullptr, &np, nullptr, nullptr, nullptr, nullptr, nullptr) == 2);
    CHECK(g_calls[1] == 1 && np == (std::vector<uint32_t>{0, 0}) && std::isinf(ln[0]) && std::isinf(ln[1]));
  }
  printf("transcript_args_check OK\n");
  return 0;
}
