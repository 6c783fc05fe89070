// crf_posteriors.cpp -- posterior output above the C ABI (scrf_posteriors_batch): the reference's
// CRF_NewLocalPosteriorBuilder (decoders/CRF_NewLocalPosteriorBuilder.{h,cpp}) and its batched form.  A translation unit
// of its own inside libcrf_amd_host.so: crf_amd.cpp stays linkable against an ABI without the posterior entry point.
#include "crf_amd.h"

#include <math.h>

#include <iostream>

using std::runtime_error;

CRF_NewLocalPosteriorBuilder::CRF_NewLocalPosteriorBuilder(CRF_Model* crf_in, bool norm) : crf(crf_in), normalize(norm) {}
CRF_NewLocalPosteriorBuilder::~CRF_NewLocalPosteriorBuilder() { delete nodeList; }

CRF_StateVector* CRF_NewLocalPosteriorBuilder::buildFtrSeq(CRF_FeatureStream* ftr_strm) {
  crf_amd::StreamBatch sb(ftr_strm, crf, 1, false);
  const uint32_t T = sb.T[0];
  const uint32_t L = crf->getNActualLabs() ? crf->getNActualLabs() : crf->getNLabs();
  delete nodeList;
  nodeList = new CRF_StateVector();
  CRF_StateVector& v = *nodeList;
  v.AB.assign((size_t)T * L, 0.0);
  sb.e->check(scrf_posteriors_batch(sb.e->h, sb.b, &v.zx, v.AB.data(), nullptr, nullptr, nullptr, nullptr),
              "CRF_LocalPosteriorBuilder::buildFtrSeq");
  v.nodes.resize(T);
  const double norm_const = normalize ? 0.0 : v.zx;
  for (uint32_t t = 0; t < T; t++) {
    double* row = v.AB.data() + (size_t)t * L;
    double tot = 0.0;
    for (uint32_t l = 0; l < L; l++) tot += row[l];
    // decoders/CRF_NewLocalPosteriorBuilder.cpp:171-181
    if (tot > 1.1) {
      std::cout << "Total: " << tot << std::endl;
      throw runtime_error("CRF_LocalPosteriorBuilder::buildFtrSeq: Probability sums greater than 1.0");
    }
    if (!(tot >= 0.9)) throw runtime_error("CRF_LocalPosteriorBuilder::buildFtrSeq: Probability sums less than 1.0");
    for (uint32_t l = 0; l < L; l++) row[l] = log(row[l]) + norm_const;
    CRF_StateNode& n = v.nodes[t];
    n.alpha_beta = row;
    n.nLabs = L;
    n.nodeMaxDur = t + 1 < crf->getLabMaxDur() ? t + 1 : crf->getLabMaxDur();
    n.zx = v.zx;
    n.last = t + 1 == T;
  }
  return nodeList;
}

size_t crf_amd_posteriors(CRF_FeatureStream* ftr_strm, CRF_Model* crf, size_t max_utts,
                          std::vector<std::vector<double> >* frame_post, std::vector<std::vector<double> >* end_post,
                          std::vector<double>* zx, std::vector<std::vector<uint32_t> >* labels, std::vector<float>* costs,
                          std::vector<std::vector<double> >* seg_post, bool* at_end) {
  crf_amd::StreamBatch sb(ftr_strm, crf, max_utts);   // advances the stream, like crf_amd_best_paths
  if (at_end) *at_end = sb.at_end;
  const size_t U = sb.T.size();
  const uint32_t L = crf->getNActualLabs() ? crf->getNActualLabs() : crf->getNLabs();
  std::vector<uint32_t> labs;
  std::vector<uint64_t> off(U + 1, 0);
  std::vector<float> cst(U, 0.0f);
  const bool paths = labels || seg_post;
  if (paths) {
    labs.resize(sb.frames);
    sb.e->check(scrf_viterbi_batch(sb.e->h, sb.b, labs.data(), labs.size(), off.data(), cst.data()), "ShortestPath");
  }
  std::vector<double> fp(frame_post ? sb.frames * L : 0), ep(end_post ? sb.frames : 0), z(U), sp(seg_post ? off[U] : 0);
  sb.e->check(scrf_posteriors_batch(sb.e->h, sb.b, z.data(), frame_post ? fp.data() : nullptr, end_post ? ep.data() : nullptr,
                                    seg_post ? labs.data() : nullptr, seg_post ? off.data() : nullptr, seg_post ? sp.data() : nullptr),
              "crf_amd_posteriors");
  if (zx) *zx = z;
  if (costs) *costs = cst;
  if (frame_post) frame_post->resize(U);
  if (end_post) end_post->resize(U);
  if (labels) labels->resize(U);
  if (seg_post) seg_post->resize(U);
  size_t f0 = 0;
  for (size_t u = 0; u < U; u++) {
    if (frame_post) (*frame_post)[u].assign(fp.begin() + f0 * L, fp.begin() + (f0 + sb.T[u]) * L);
    if (end_post) (*end_post)[u].assign(ep.begin() + f0, ep.begin() + f0 + sb.T[u]);
    if (labels) (*labels)[u].assign(labs.begin() + off[u], labs.begin() + off[u + 1]);
    if (seg_post) (*seg_post)[u].assign(sp.begin() + off[u], sp.begin() + off[u + 1]);
    f0 += sb.T[u];
  }
  return U;
}
