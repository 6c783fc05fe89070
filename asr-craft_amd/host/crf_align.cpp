// crf_align.cpp -- batched forced alignment on phones above the C ABI (scrf_align_batch).  A translation
// unit of its own inside libcrf_amd_host.so: crf_amd.cpp stays linkable against an ABI without the alignment entry points.
#include "crf_amd.h"

size_t crf_amd_alignments(CRF_FeatureStream* ftr_strm, CRF_Model* crf, size_t max_utts, int mode,
                          std::vector<std::vector<uint32_t> >* labels, std::vector<float>* costs,
                          std::vector<std::vector<double> >* seg_post, bool* at_end) {
  crf_amd::StreamBatch sb(ftr_strm, crf, max_utts);   // advances the stream, like crf_amd_best_paths
  if (at_end) *at_end = sb.at_end;
  const size_t U = sb.T.size();
  const uint32_t L = crf->getNActualLabs() ? crf->getNActualLabs() : crf->getNLabs();
  // the transcripts: the phones of the labelled nodes in order, runs collapsed where a phone may repeat over segments anyway
  std::vector<uint32_t> phones;
  std::vector<uint64_t> poff;
  crf_amd::node_label_transcripts(sb, L, mode, "crf_amd_alignments", &phones, &poff);
  std::vector<uint32_t> labs(sb.frames);
  std::vector<uint64_t> off(U + 1, 0);
  std::vector<float> cst(U, 0.0f);
  sb.e->check(scrf_align_batch(sb.e->h, sb.b, phones.data(), poff.data(), mode, labs.data(), labs.size(), off.data(), cst.data()),
              "crf_amd_alignments");
  std::vector<double> sp(seg_post ? off[U] : 0);
  if (seg_post && off[U])
    sb.e->check(scrf_posteriors_batch(sb.e->h, sb.b, nullptr, nullptr, nullptr, labs.data(), off.data(), sp.data()), "crf_amd_alignments");
  if (costs) *costs = cst;
  if (labels) labels->resize(U);
  if (seg_post) seg_post->resize(U);
  for (size_t u = 0; u < U; u++) {
    if (labels) (*labels)[u].assign(labs.begin() + off[u], labs.begin() + off[u + 1]);
    if (seg_post) (*seg_post)[u].assign(sp.begin() + off[u], sp.begin() + off[u + 1]);
  }
  return U;
}
