// scrf_softnum.h -- the numerator of the soft-alignment gradient (scrf_fb_transcript_batch): launchers of
// scrf_softnum.hip.
#ifndef SCRF_SOFTNUM_H_
#define SCRF_SOFTNUM_H_

#include "scrf_kernels.h"

// What the numerator kernels of a chunk read and write beside the transcript sweep's own arguments (ScrfTransArgs: the
// transcripts, the inverted lists, the aB / bE cells k_transcript left).  Every array is the chunk's; utterance u's cells
// start at cell_off[u] - cell_off[u0], its positions at phone_off[u] - phone_off[u0].
struct ScrfSoftArgs {
  const double* log_num;   // [U] A of every utterance of the batch (k_transcript)
  const int* status;       // [U] an utterance whose status is set has no numerator: its sweep may have stopped half way
  double* aE;              // [T][K] cells: the forward sum at the END of a segment of position k at frame t
  double* bB;              // [T][K] cells: the backward sum at the START of a segment of position k at frame t (t >= 1)
  double* G;               // [nseg][L] state numerators, the rows of R
  double* adv;             // [sum K] bias-only transitions: per position the sum over t of xa(t, k) ...
  double* stay;            // ... and of xs(t, k)
  double* tab;             // [n_utts][L * L] bias-only transitions: per utterance the transition numerators summed over (t, k)
};

void launch_soft_state(hipStream_t st, const ScrfLayout& lay, ScrfBatchView bv, uint32_t u0, uint32_t n_utts, uint32_t t_max,
                       const double* S, const double* smax, const ScrfTransArgs& ta, const ScrfSoftArgs& sa);
void launch_soft_trans(hipStream_t st, const ScrfLayout& lay, ScrfBatchView bv, uint32_t u0, uint32_t n_utts, uint64_t cells_max,
                       const double* S, const double* smax, const ScrfTransArgs& ta, const ScrfSoftArgs& sa);
void launch_soft_add_r(hipStream_t st, double* R, const double* G, uint64_t n);
void launch_soft_add_xi(hipStream_t st, const ScrfLayout& lay, ScrfBatchView bv, uint32_t u0, uint32_t n_utts, uint32_t t_max,
                        const double* M, const ScrfTransArgs& ta, const ScrfSoftArgs& sa, double* XI);
void launch_soft_trans_table(hipStream_t st, const ScrfLayout& lay, ScrfBatchView bv, uint32_t u0, uint32_t n_utts, uint64_t k_max,
                             const double* M, const ScrfTransArgs& ta, const ScrfSoftArgs& sa, double* grad);

#endif  // SCRF_SOFTNUM_H_
