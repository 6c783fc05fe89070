// Compile-time check (g++ -fsyntax-only) that CRF_NewLocalPosteriorBuilder of asr-craft_amd/host/crf_amd.h keeps the
// shape of the reference's class (decoders/CRF_NewLocalPosteriorBuilder.h:38-53): constructor (CRF_Model*, bool norm =
// true), virtual CRF_StateVector* buildFtrSeq(CRF_FeatureStream*), nodes with getAlphaBeta().
#include <type_traits>

#include "crf_amd.h"

static_assert(std::is_constructible<CRF_NewLocalPosteriorBuilder, CRF_Model*, bool>::value, "constructor (CRF_Model*, bool)");
static_assert(std::is_constructible<CRF_NewLocalPosteriorBuilder, CRF_Model*>::value, "norm defaults (to true)");
static_assert(std::is_same<decltype(&CRF_NewLocalPosteriorBuilder::buildFtrSeq),
                           CRF_StateVector* (CRF_NewLocalPosteriorBuilder::*)(CRF_FeatureStream*)>::value,
              "CRF_StateVector* buildFtrSeq(CRF_FeatureStream*)");
static_assert(std::has_virtual_destructor<CRF_NewLocalPosteriorBuilder>::value, "virtual destructor");
static_assert(std::is_polymorphic<CRF_NewLocalPosteriorBuilder>::value, "buildFtrSeq is virtual");
static_assert(std::is_same<decltype(&CRF_StateNode::getAlphaBeta), double* (CRF_StateNode::*)()>::value, "double* getAlphaBeta()");
static_assert(std::is_same<decltype(&crf_amd_posteriors),
                           size_t (*)(CRF_FeatureStream*, CRF_Model*, size_t, std::vector<std::vector<double> >*,
                                      std::vector<std::vector<double> >*, std::vector<double>*, std::vector<std::vector<uint32_t> >*,
                                      std::vector<float>*, std::vector<std::vector<double> >*, bool*)>::value,
              "crf_amd_posteriors");

// what a caller writes (never run here)
double first_log_posterior(CRF_Model* crf, CRF_FeatureStream* strm) {
  CRF_NewLocalPosteriorBuilder lpb(crf);
  CRF_StateVector* nodes = lpb.buildFtrSeq(strm);
  return nodes->getNodeCount() ? nodes->at(0)->getAlphaBeta()[0] : 0.0;
}

#ifdef POSTERIOR_CONFORMANCE_MAIN
// posterior_conformance weights.txt frames.txt L D W norm [precision]: a segmental model (stdseg_no_dur_no_segtransftr,
// stdstate) over one segment-recipe stream of W-wide frames; frames.txt holds per utterance a line `T` and T lines of W
// values.  Prints `u t v_0 .. v_{L-1}` (getAlphaBeta of every node, 17 significant digits) and `zx u value`.
#include <stdlib.h>

#include <fstream>
#include <iostream>

int main(int argc, char** argv) {
  if (argc < 7) return 2;
  const QNUInt32 L = (QNUInt32)atoi(argv[3]), D = (QNUInt32)atoi(argv[4]), W = (QNUInt32)atoi(argv[5]);
  const bool norm = atoi(argv[6]) != 0;
  try {
    CRF_FeatureMap_config cnf;
    cnf.map_type = STDSTATE;
    cnf.numLabs = L; cnf.nActualLabs = L; cnf.maxDur = D;
    cnf.numFeas = D == 1 ? W : 8 * W + D;
    cnf.stateFidxStart = 0; cnf.stateFidxEnd = cnf.numFeas - 1;
    CRF_Model crf(L);
    crf.setLabMaxDur(D);
    crf.setNActualLabs(L);
    crf.setModelType(D == 1 ? STDFRAME : STDSEG_NO_DUR_NO_SEGTRANSFTR);
    if (argc > 7) crf.setTrainPrecision((uint32_t)atoi(argv[7]));
    crf.setFeatureMap(CRF_FeatureMap::createFeatureMap(&cnf));
    if (!crf.readFromFile(argv[1])) { std::cerr << "cannot read " << argv[1] << std::endl; return 1; }
    std::vector<scrf_stream_recipe> rec(1);
    rec[0].in_width = W; rec[0].left_ctx = 0; rec[0].right_ctx = 0; rec[0].extract_seg_ftr = 1;
    CRF_MemoryFeatureStream strm(rec, D, L);
    std::ifstream f(argv[2]);
    size_t T;
    while (f >> T) {
      std::vector<std::vector<float> > fr(1, std::vector<float>(T * W));
      for (float& x : fr[0]) f >> x;
      strm.addUtterance(fr, std::vector<uint32_t>());
    }
    strm.rewind();
    CRF_NewLocalPosteriorBuilder lpb(&crf, norm);
    std::cout.precision(17);
    for (size_t u = 0; strm.nextseg() != QN_SEGID_BAD; u++) {
      CRF_StateVector* nodes = lpb.buildFtrSeq(&strm);
      for (size_t t = 0; t < nodes->getNodeCount(); t++) {
        std::cout << u << " " << t;
        for (QNUInt32 l = 0; l < L; l++) std::cout << " " << nodes->at(t)->getAlphaBeta()[l];
        std::cout << "\n";
      }
      std::cout << "zx " << u << " " << nodes->getZx() << "\n";
    }
  } catch (std::exception& e) {
    std::cerr << "Exception: " << e.what() << std::endl;
    return 1;
  }
  return 0;
}
#endif
