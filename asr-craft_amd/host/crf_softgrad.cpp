// crf_softgrad.cpp -- the soft objective above the C ABI (scrf_fb_transcript_batch; the reference's
// CRF_NewGradBuilderSoft, crf_objective_function=softexpf).  A translation unit of its own inside libcrf_amd_host.so:
// crf_amd.cpp stays linkable against an ABI without the entry point, and holds only the empty slot crf_amd_soft_fb that this
// unit fills from a static initialiser.
#include "crf_amd.h"

namespace {

// Each utterance's transcript from its label stream, as crf_amd_transcript_scores reads it: the phones (label % n_labs) of
// the labelled frames in order, durations dropped, equal neighbours collapsed under SCRF_ALIGN_RUNS; then the device pass.
int soft_fb(scrf_handle h, scrf_batch b, const uint32_t* const* labels, const uint32_t* T, uint32_t n_utts, uint32_t n_labs, int mode,
            double* log_num, double* zx) {
  std::vector<uint32_t> phones;
  std::vector<uint64_t> poff(n_utts + 1, 0);
  for (uint32_t u = 0; u < n_utts; u++) {
    if (!labels[u]) throw std::runtime_error("CRF_NewGradBuilderSoft: utterance without a label stream: the soft objective reads the transcript from the labels");
    for (uint32_t t = 0; t < T[u]; t++) {
      if (labels[u][t] == CRF_LAB_BAD) continue;
      const uint32_t p = labels[u][t] % n_labs;
      if (mode == SCRF_ALIGN_RUNS && phones.size() > poff[u] && phones.back() == p) continue;
      phones.push_back(p);
    }
    poff[u + 1] = phones.size();
  }
  return scrf_fb_transcript_batch(h, b, phones.data(), poff.data(), mode, log_num, zx);
}

struct Fill { Fill() { crf_amd_soft_fb = soft_fb; } } fill;

}  // namespace
