// crf_transcript.cpp -- transcript scoring above the C ABI (scrf_transcript_batch).  A translation unit of
// its own inside libcrf_amd_host.so: crf_amd.cpp stays linkable against an ABI without the transcript entry points.
#include "crf_amd.h"

size_t crf_amd_transcript_scores(CRF_FeatureStream* ftr_strm, CRF_Model* crf, size_t max_utts, int mode,
                                 std::vector<double>* log_num, std::vector<double>* zx, std::vector<uint32_t>* n_phones,
                                 std::vector<std::vector<uint32_t> >* labels, std::vector<float>* costs,
                                 std::vector<std::vector<double> >* seg_post_given,
                                 std::vector<std::vector<double> >* seg_post_free, bool* at_end) {
  if ((costs || seg_post_given || seg_post_free) && !labels)
    throw std::runtime_error("crf_amd_transcript_scores: costs and segment posteriors belong to the aligned paths: pass labels as well");
  crf_amd::StreamBatch sb(ftr_strm, crf, max_utts);   // advances the stream, like crf_amd_alignments
  if (at_end) *at_end = sb.at_end;
  const size_t U = sb.T.size();
  const uint32_t L = crf->getNActualLabs() ? crf->getNActualLabs() : crf->getNLabs();
  std::vector<uint32_t> phones;
  std::vector<uint64_t> poff;
  crf_amd::node_label_transcripts(sb, L, mode, "crf_amd_transcript_scores", &phones, &poff);
  // the aligned paths first: they are the segment queries of the scoring call
  std::vector<uint32_t> labs(labels ? sb.frames : 0);
  std::vector<uint64_t> off(U + 1, 0);
  std::vector<float> cst(U, 0.0f);
  if (labels)
    sb.e->check(scrf_align_batch(sb.e->h, sb.b, phones.data(), poff.data(), mode, labs.data(), labs.size(), off.data(), cst.data()),
                "crf_amd_transcript_scores");
  const bool given = seg_post_given && off[U];
  std::vector<double> ln(U), z(U), spg(given ? off[U] : 0), spf(seg_post_free ? off[U] : 0);
  sb.e->check(scrf_transcript_batch(sb.e->h, sb.b, phones.data(), poff.data(), mode, ln.data(), z.data(), nullptr, nullptr,
                                    given ? labs.data() : nullptr, given ? off.data() : nullptr, given ? spg.data() : nullptr),
              "crf_amd_transcript_scores");
  if (seg_post_free && off[U])
    sb.e->check(scrf_posteriors_batch(sb.e->h, sb.b, nullptr, nullptr, nullptr, labs.data(), off.data(), spf.data()), "crf_amd_transcript_scores");
  if (log_num) *log_num = ln;
  if (zx) *zx = z;
  if (n_phones) {
    n_phones->resize(U);
    for (size_t u = 0; u < U; u++) (*n_phones)[u] = (uint32_t)(poff[u + 1] - poff[u]);
  }
  if (costs) *costs = cst;
  if (labels) labels->resize(U);
  if (seg_post_given) seg_post_given->resize(U);
  if (seg_post_free) seg_post_free->resize(U);
  for (size_t u = 0; u < U; u++) {
    if (labels) (*labels)[u].assign(labs.begin() + off[u], labs.begin() + off[u + 1]);
    if (seg_post_given) (*seg_post_given)[u].assign(spg.begin() + off[u], spg.begin() + off[u + 1]);
    if (seg_post_free) (*seg_post_free)[u].assign(spf.begin() + off[u], spf.begin() + off[u + 1]);
  }
  return U;
}
