// crf_lattice_prune.cpp -- beam-pruned lattices above the C ABI (scrf_lattice_prune_batch): the batched
// fetch and the host-side compaction of a pruned arc list into a machine of its own.  A translation unit of its own inside
// libcrf_amd_host.so: crf_amd.cpp stays linkable against an ABI without the lattice-beam entry points.
#include "crf_amd.h"

namespace crf_amd {

void compactLattice(const scrf_arc* arcs, size_t n, int32_t final_state, ArcListFst* out) {
  *out = ArcListFst();
  if (n == 0) return;   // an empty machine: no states, no start
  int32_t top = final_state;
  for (size_t i = 0; i < n; i++) top = std::max(top, std::max(arcs[i].src, arcs[i].dst));
  std::vector<int32_t> id((size_t)top + 1, -1);
  for (size_t i = 0; i < n; i++) { id[arcs[i].src] = 0; id[arcs[i].dst] = 0; }
  int32_t next = 0;
  for (int32_t s = 0; s <= top; s++)   // ascending old id: the start (0) stays 0, a topological order stays one
    if (id[s] == 0) id[s] = next++;
  out->n_states = next;
  out->start = 0;
  out->arcs.reserve(n);
  for (size_t i = 0; i < n; i++) out->arcs.push_back(scrf_arc{id[arcs[i].src], arcs[i].ilabel, arcs[i].olabel, arcs[i].w, id[arcs[i].dst]});
  if (final_state >= 0 && id[final_state] >= 0) out->SetFinal(id[final_state], 0.0f);
}

}  // namespace crf_amd

size_t crf_amd_pruned_lattices(CRF_FeatureStream* ftr_strm, CRF_Model* crf, size_t max_utts, double beam,
                               std::vector<crf_amd::ArcListFst>* lats, std::vector<double>* best, uint64_t* n_full_arcs,
                               bool* at_end) {
  crf_amd::StreamBatch sb(ftr_strm, crf, max_utts);   // advances the stream, like crf_amd_best_paths
  if (at_end) *at_end = sb.at_end;
  const size_t U = sb.T.size();
  std::vector<uint64_t> off(U + 1, 0);
  std::vector<double> bc(U, 0.0);
  sb.e->check(scrf_lattice_prune_batch(sb.e->h, sb.b, beam, off.data(), bc.data()), "crf_amd_pruned_lattices");
  std::vector<scrf_arc> arcs(off[U]);
  sb.e->check(scrf_lattice_pruned_arcs(sb.e->h, sb.b, 0, (uint32_t)U, arcs.data(), arcs.size()), "crf_amd_pruned_lattices");
  if (n_full_arcs) {
    uint32_t nu = 0;
    uint64_t nf = 0, ns = 0, na = 0;
    sb.e->check(scrf_batch_info(sb.e->h, sb.b, &nu, &nf, &ns, &na), "crf_amd_pruned_lattices");
    *n_full_arcs = na;
  }
  if (best) *best = bc;
  if (lats) {
    lats->resize(U);
    for (size_t u = 0; u < U; u++) {
      int32_t fin = -1;
      sb.e->check(scrf_lattice_arcs(sb.e->h, sb.b, (uint32_t)u, 0, nullptr, nullptr, nullptr, &fin), "crf_amd_pruned_lattices");
      crf_amd::compactLattice(arcs.data() + off[u], (size_t)(off[u + 1] - off[u]), fin, &(*lats)[u]);
    }
  }
  return U;
}
