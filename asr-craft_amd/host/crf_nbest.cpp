// crf_nbest.cpp -- N-best lists above the C ABI (scrf_nbest_batch / scrf_nbest_paths).  A translation unit of
// its own inside libcrf_amd_host.so: crf_amd.cpp stays linkable against an ABI without the N-best entry points.
#include "crf_amd.h"

#include <math.h>

std::vector<uint32_t> crf_amd_collapsed_phones(const std::vector<uint32_t>& labels, uint32_t n_labs) {
  std::vector<uint32_t> ph;
  for (uint32_t l : labels) {
    const uint32_t p = l % n_labs;
    if (ph.empty() || ph.back() != p) ph.push_back(p);
  }
  return ph;
}

size_t crf_amd_nbest(CRF_FeatureStream* ftr_strm, CRF_Model* crf, size_t max_utts, uint32_t n_best, bool unique_phones, bool rescore,
                     std::vector<std::vector<CRF_NbestHyp> >* hyps, bool* at_end, std::vector<std::vector<uint32_t> >* best_labels,
                     std::vector<std::vector<double> >* best_seg_post) {
  if (best_seg_post && !best_labels) throw std::runtime_error("crf_amd_nbest: segment posteriors belong to the best paths: pass best_labels as well");
  if (!hyps) throw std::runtime_error("crf_amd_nbest: hyps must be given");
  if (n_best == 0) throw std::runtime_error("crf_amd_nbest: n_best must be at least 1");
  if (rescore && !unique_phones)
    throw std::runtime_error("crf_amd_nbest: rescoring scores phone sequences: it needs unique_phones (one hypothesis per collapsed sequence)");
  crf_amd::StreamBatch sb(ftr_strm, crf, max_utts);   // advances the stream, like crf_amd_best_paths
  if (at_end) *at_end = sb.at_end;
  const size_t U = sb.T.size();
  const uint32_t L = crf->getNActualLabs() ? crf->getNActualLabs() : crf->getNLabs();
  std::vector<uint64_t> hoff(U + 1, 0);
  uint64_t n_labels = 0;
  sb.e->check(scrf_nbest_batch(sb.e->h, sb.b, n_best, hoff.data(), &n_labels), "crf_amd_nbest");
  const uint64_t H = hoff[U];
  std::vector<uint32_t> labs(n_labels);
  std::vector<uint64_t> loff(H + 1, 0);
  std::vector<float> cost(H);
  sb.e->check(scrf_nbest_paths(sb.e->h, sb.b, 0, (uint32_t)U, labs.data(), labs.size(), loff.data(), cost.data()), "crf_amd_nbest");
  if (best_labels) {
    // hypothesis 0 of every utterance, back to back: the segment queries of the posterior call
    std::vector<uint32_t> q;
    std::vector<uint64_t> qoff(U + 1, 0);
    best_labels->assign(U, std::vector<uint32_t>());
    for (size_t u = 0; u < U; u++) {
      if (hoff[u + 1] > hoff[u]) (*best_labels)[u].assign(labs.begin() + loff[hoff[u]], labs.begin() + loff[hoff[u] + 1]);
      q.insert(q.end(), (*best_labels)[u].begin(), (*best_labels)[u].end());
      qoff[u + 1] = q.size();
    }
    if (best_seg_post) {
      std::vector<double> sp(q.size());
      if (!q.empty())
        sb.e->check(scrf_posteriors_batch(sb.e->h, sb.b, nullptr, nullptr, nullptr, q.data(), qoff.data(), sp.data()), "crf_amd_nbest");
      best_seg_post->assign(U, std::vector<double>());
      for (size_t u = 0; u < U; u++) (*best_seg_post)[u].assign(sp.begin() + qoff[u], sp.begin() + qoff[u + 1]);
    }
  }
  hyps->assign(U, std::vector<CRF_NbestHyp>());
  size_t n_ranks = 0;   // the longest list kept
  for (size_t u = 0; u < U; u++) {
    std::vector<CRF_NbestHyp>& out = (*hyps)[u];
    for (uint64_t i = hoff[u]; i < hoff[u + 1]; i++) {
      CRF_NbestHyp hy;
      hy.labels.assign(labs.begin() + loff[i], labs.begin() + loff[i + 1]);
      hy.cost = cost[i];
      hy.logp = NAN;
      if (unique_phones) {   // ascending by cost: the first of a sequence is its cheapest
        hy.phones = crf_amd_collapsed_phones(hy.labels, L);
        bool seen = false;
        for (const CRF_NbestHyp& k : out) seen = seen || k.phones == hy.phones;
        if (seen) continue;
      }
      out.push_back(std::move(hy));
    }
    n_ranks = std::max(n_ranks, out.size());
  }
  if (!rescore) return U;
  // one transcript pass per rank over the whole batch, with every utterance's r-th kept sequence; an utterance with fewer
  // gives an empty transcript, which the ABI answers with -inf
  std::vector<uint32_t> phones;
  std::vector<uint64_t> poff(U + 1, 0);
  std::vector<double> ln(U), zx(U);
  for (size_t r = 0; r < n_ranks; r++) {
    phones.clear();
    for (size_t u = 0; u < U; u++) {
      if (r < (*hyps)[u].size()) phones.insert(phones.end(), (*hyps)[u][r].phones.begin(), (*hyps)[u][r].phones.end());
      poff[u + 1] = phones.size();
    }
    sb.e->check(scrf_transcript_batch(sb.e->h, sb.b, phones.data(), poff.data(), SCRF_ALIGN_RUNS, ln.data(), zx.data(), nullptr, nullptr,
                                      nullptr, nullptr, nullptr), "crf_amd_nbest");
    for (size_t u = 0; u < U; u++)
      if (r < (*hyps)[u].size()) (*hyps)[u][r].logp = ln[u] - zx[u];
  }
  return U;
}
