// nbest_args_check.cpp -- TEST-ONLY stand-alone program over the host side of N-best decoding
// (asr-craft_amd/host/crf_nbest.cpp: crf_amd_nbest), linked against the ABI stub (scrf_stub.cpp) plus the entry points below
// that the stub does not have.  No GPU, no Python: tests/test_host_nbest_args.py compiles it with
// -fsanitize=address,undefined and runs it.  The stand-ins serve a fixed N-best list, check what the host hands the ABI
// (counts, capacities, which pointers are NULL, the transcripts of every rescoring pass) and write every output array to its
// full extent, so that a buffer the host sized wrongly is an AddressSanitizer report.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include <stdexcept>
#include <string>
#include <vector>

#include "crf_amd.h"

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "FAILED line %d: %s\n", __LINE__, #c); exit(1); } } while (0)

static const uint32_t L = 3, D = 3, W = 2, NBEST = 4;
struct Hyp { std::vector<uint32_t> labels; float cost; };
// labels are phone + L * (duration - 1).  Utterance 0 (T = 3): phones [0], [0 0] (the same sequence once collapsed),
// [1 0 2], [1 2]; utterance 1 (T = 2): [1], [1 1]; utterance 2 (T = 1): one path only
static const std::vector<std::vector<Hyp> > HYPS = {
    {{{6}, 1.0f}, {{0, 3}, 2.0f}, {{1, 0, 2}, 3.0f}, {{4, 2}, 4.0f}},
    {{{4}, -1.5f}, {{1, 1}, -1.0f}},
    {{{2}, 0.25f}},
};
static const std::vector<std::vector<std::vector<uint32_t> > > SEQS = {{{0}, {1, 0, 2}, {1, 2}}, {{1}}, {{2}}};
static const std::vector<uint32_t> TS = {3, 2, 1};

static size_t g_U = 0;   // utterances of the batch the host built
static int g_calls[4] = {0, 0, 0, 0};   // nbest_batch, nbest_paths, transcript, posteriors
static uint64_t g_n_labels = 0;

extern "C" {
int scrf_nbest_batch(scrf_handle, scrf_batch, uint32_t n_best, uint64_t* hyp_off, uint64_t* n_labels) {
  g_calls[0]++;
  CHECK(n_best == NBEST && hyp_off && n_labels);
  g_n_labels = 0;
  hyp_off[0] = 0;
  for (size_t u = 0; u < g_U; u++) {
    hyp_off[u + 1] = hyp_off[u] + HYPS[u].size();
    for (const Hyp& h : HYPS[u]) g_n_labels += h.labels.size();
  }
  *n_labels = g_n_labels;
  return SCRF_OK;
}
int scrf_nbest_paths(scrf_handle, scrf_batch, uint32_t u0, uint32_t n, uint32_t* seg_labels, uint64_t max_labels, uint64_t* lab_off, float* cost) {
  g_calls[1]++;
  CHECK(g_calls[0] == g_calls[1]);   // after the search of the same call
  CHECK(u0 == 0 && n == g_U && seg_labels && lab_off && cost && max_labels == g_n_labels);
  for (uint64_t i = 0; i < max_labels; i++) seg_labels[i] = 0xdeadbeefu;   // the whole capacity is the callee's
  uint64_t pos = 0, hi = 0;
  for (size_t u = 0; u < g_U; u++)
    for (const Hyp& h : HYPS[u]) {
      lab_off[hi] = pos;
      cost[hi++] = h.cost;
      for (uint32_t l : h.labels) seg_labels[pos++] = l;
    }
  lab_off[hi] = pos;
  return SCRF_OK;
}
int scrf_nbest_stats(scrf_handle, uint64_t*, uint64_t*, uint64_t*) { CHECK(!"crf_amd_nbest does not ask for the counters"); return SCRF_OK; }
// pass r carries every utterance's r-th kept sequence; an utterance with fewer passes an empty transcript and gets -inf
int scrf_transcript_batch(scrf_handle, scrf_batch, const uint32_t* phones, const uint64_t* phone_off, int mode, double* log_num, double* zx,
                          double* frame_post, double* end_post, const uint32_t* seg_labels, const uint64_t* lab_off, double* seg_post) {
  const size_t r = (size_t)g_calls[2]++;
  CHECK(mode == SCRF_ALIGN_RUNS && phone_off && phone_off[0] == 0 && log_num && zx);
  CHECK(!frame_post && !end_post && !seg_labels && !lab_off && !seg_post);
  for (size_t u = 0; u < g_U; u++) {
    const std::vector<uint32_t> got(phones + phone_off[u], phones + phone_off[u + 1]);
    const bool has = r < SEQS[u].size();
    CHECK(got == (has ? SEQS[u][r] : std::vector<uint32_t>()));
    log_num[u] = has ? -1.0 - (double)r - 0.125 * (double)u : -INFINITY;
    zx[u] = 10.0 + (double)u;
  }
  return SCRF_OK;
}
int scrf_posteriors_batch(scrf_handle, scrf_batch, double* zx, double* frame_post, double* end_post, const uint32_t* seg_labels,
                          const uint64_t* lab_off, double* seg_post) {
  g_calls[3]++;
  CHECK(!zx && !frame_post && !end_post && seg_labels && lab_off && seg_post && lab_off[0] == 0);
  for (size_t u = 0; u < g_U; u++) {   // the queries are hypothesis 0 of every utterance
    CHECK(std::vector<uint32_t>(seg_labels + lab_off[u], seg_labels + lab_off[u + 1]) == HYPS[u][0].labels);
    for (uint64_t i = lab_off[u]; i < lab_off[u + 1]; i++) seg_post[i] = 0.5 + 0.001 * (double)i;
  }
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

static void fill(CRF_MemoryFeatureStream* strm, size_t n_utts) {
  for (size_t u = 0; u < n_utts; u++) {
    const size_t T = TS[u];
    std::vector<std::vector<float> > fr(1, std::vector<float>(T * W));
    for (size_t i = 0; i < T * W; i++) fr[0][i] = 0.125f * (float)((i + 3 * u) % 7);
    strm->addUtterance(fr, std::vector<uint32_t>());
  }
}

template <class F>
static std::string thrown(F f) {
  try { f(); } catch (std::exception& e) { return e.what(); }
  return "";
}

int main() {
  const std::vector<scrf_stream_recipe> rec = {scrf_stream_recipe{W, 0, 0, 1}};
  // 0. the collapse on its own
  CHECK(crf_amd_collapsed_phones({0, 3, 6, 1, 4, 0}, L) == (std::vector<uint32_t>{0, 1, 0}));
  CHECK(crf_amd_collapsed_phones({}, L).empty());
  // 1. every path; unique phone sequences; unique + rescoring with the best paths and their posteriors
  for (int variant = 0; variant < 3; variant++) {
    const bool unique = variant >= 1, rescore = variant == 2;
    CRF_Model crf(L);
    make_model(&crf);
    CRF_MemoryFeatureStream strm(rec, D, L);
    fill(&strm, TS.size());
    strm.rewind();
    CHECK(strm.nextseg() != QN_SEGID_BAD);
    g_calls[0] = g_calls[1] = g_calls[2] = g_calls[3] = 0;
    g_U = TS.size();
    std::vector<std::vector<CRF_NbestHyp> > hyps;
    std::vector<std::vector<uint32_t> > best;
    std::vector<std::vector<double> > sp;
    bool at_end = false;
    const size_t U = crf_amd_nbest(&strm, &crf, 256, NBEST, unique, rescore, &hyps, &at_end, rescore ? &best : nullptr, rescore ? &sp : nullptr);
    CHECK(U == TS.size() && at_end && hyps.size() == U && g_calls[0] == 1 && g_calls[1] == 1);
    CHECK(g_calls[2] == (rescore ? 3 : 0) && g_calls[3] == (rescore ? 1 : 0));   // one transcript pass per rank of the longest list
    for (size_t u = 0; u < U; u++) {
      if (!unique) {
        CHECK(hyps[u].size() == HYPS[u].size());
        for (size_t r = 0; r < hyps[u].size(); r++)
          CHECK(hyps[u][r].labels == HYPS[u][r].labels && hyps[u][r].cost == HYPS[u][r].cost && hyps[u][r].phones.empty() && std::isnan(hyps[u][r].logp));
        continue;
      }
      CHECK(hyps[u].size() == SEQS[u].size());
      for (size_t r = 0; r < hyps[u].size(); r++) {
        const CRF_NbestHyp& h = hyps[u][r];
        CHECK(h.phones == SEQS[u][r]);
        if (r > 0) CHECK(h.cost >= hyps[u][r - 1].cost);
        if (rescore) CHECK(h.logp == (-1.0 - (double)r - 0.125 * (double)u) - (10.0 + (double)u));
        else CHECK(std::isnan(h.logp));
      }
      // the first -- cheapest -- path of each sequence is the one kept
      CHECK(hyps[u][0].labels == HYPS[u][0].labels && hyps[u][0].cost == HYPS[u][0].cost);
      if (u == 0) CHECK(hyps[0][1].labels == HYPS[0][2].labels && hyps[0][2].labels == HYPS[0][3].labels && hyps[0][2].cost == 4.0f);
    }
    if (rescore) {
      CHECK(best.size() == U && sp.size() == U);
      for (size_t u = 0; u < U; u++) {
        CHECK(best[u] == HYPS[u][0].labels && sp[u].size() == best[u].size());
        for (double x : sp[u]) CHECK(x >= 0.5 && x < 0.6);
      }
    }
  }
  // 2. a bunch of 2 leaves the stream on the third utterance
  {
    CRF_Model crf(L);
    make_model(&crf);
    CRF_MemoryFeatureStream strm(rec, D, L);
    fill(&strm, 3);
    strm.rewind();
    CHECK(strm.nextseg() != QN_SEGID_BAD);
    g_calls[0] = g_calls[1] = g_calls[2] = g_calls[3] = 0;
    std::vector<std::vector<CRF_NbestHyp> > hyps;
    bool at_end = true;
    g_U = 2;
    CHECK(crf_amd_nbest(&strm, &crf, 2, NBEST, true, true, &hyps, &at_end) == 2);
    CHECK(!at_end && hyps.size() == 2 && hyps[0].size() == 3 && hyps[1].size() == 1 && g_calls[2] == 3 && g_calls[3] == 0);
  }
  // 3. the argument checks, all before the stream is advanced
  {
    CRF_Model crf(L);
    make_model(&crf);
    CRF_MemoryFeatureStream strm(rec, D, L);
    fill(&strm, 1);
    strm.rewind();
    CHECK(strm.nextseg() != QN_SEGID_BAD);
    g_calls[0] = g_calls[1] = 0;
    g_U = 1;
    std::vector<std::vector<CRF_NbestHyp> > hyps;
    std::vector<std::vector<double> > sp;
    std::string m = thrown([&] { crf_amd_nbest(&strm, &crf, 2, NBEST, false, true, &hyps, nullptr); });
    CHECK(m.find("needs unique_phones") != std::string::npos);
    m = thrown([&] { crf_amd_nbest(&strm, &crf, 2, 0, false, false, &hyps, nullptr); });
    CHECK(m.find("n_best must be at least 1") != std::string::npos);
    m = thrown([&] { crf_amd_nbest(&strm, &crf, 2, NBEST, false, false, nullptr, nullptr); });
    CHECK(m.find("hyps must be given") != std::string::npos);
    m = thrown([&] { crf_amd_nbest(&strm, &crf, 2, NBEST, false, false, &hyps, nullptr, nullptr, &sp); });
    CHECK(m.find("pass best_labels as well") != std::string::npos);
    CHECK(g_calls[0] == 0);
    CHECK(crf_amd_nbest(&strm, &crf, 2, NBEST, false, false, &hyps, nullptr) == 1 && hyps.size() == 1 && hyps[0].size() == 4);
  }
  printf("nbest_args_check OK\n");
  return 0;
}
