// compact_lattice.cpp -- crf_amd::compactLattice on a hand-written pruned arc list whose state ids have gaps: renumbering in
// ascending old id, arc order, start and final state, and the empty case.
#include "crf_amd.h"

#include <stdio.h>
#include <stdlib.h>

#define CHECK(c) do { if (!(c)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

int main() {
  // old states touched: 0 3 4 9 10 17 22 (final 22); 1, 2, 5..8, 11..16, 18..21 are gone
  const scrf_arc in[9] = {
      {0, 5, 5, 1.5f, 3},  {0, 7, 7, 2.5f, 4},   {3, 0, 0, 0.25f, 9},   {4, 0, 0, 0.5f, 9},   {4, 0, 0, 0.75f, 10},
      {9, 2, 2, -1.0f, 17}, {10, 3, 3, -2.0f, 17}, {17, 0, 0, -0.0f, 22}, {0, 11, 11, 4.0f, 17},
  };
  const int old_id[7] = {0, 3, 4, 9, 10, 17, 22};
  crf_amd::ArcListFst f;
  f.n_states = 99; f.arcs.push_back(in[0]);   // whatever the machine held is replaced
  crf_amd::compactLattice(in, 9, 22, &f);
  CHECK(f.n_states == 7);
  CHECK(f.start == 0);
  CHECK(f.final_state == 6 && f.final_weight == 0.0f);
  CHECK(f.finals.size() == 1 && f.finals[0].first == 6 && f.finals[0].second == 0.0f);
  CHECK(f.arcs.size() == 9);
  for (int i = 0; i < 9; i++) {
    const scrf_arc& a = f.arcs[i];
    CHECK(a.src >= 0 && a.src < 7 && a.dst >= 0 && a.dst < 7);
    CHECK(old_id[a.src] == in[i].src && old_id[a.dst] == in[i].dst);   // same arcs in the same order, ids ascending with the old ones
    CHECK(a.ilabel == in[i].ilabel && a.olabel == in[i].olabel);
    CHECK(a.w == in[i].w);
    CHECK(a.src < a.dst);   // the topological order survives
  }
  // nothing kept: an empty machine
  crf_amd::compactLattice(in, 0, 22, &f);
  CHECK(f.n_states == 0 && f.arcs.empty() && f.finals.empty() && f.start == -1 && f.final_state == -1);
  crf_amd::compactLattice(nullptr, 0, -1, &f);
  CHECK(f.n_states == 0 && f.arcs.empty());
  // no gaps: the identity
  const scrf_arc dense[2] = {{0, 1, 1, 1.0f, 1}, {1, 0, 0, 0.0f, 2}};
  crf_amd::compactLattice(dense, 2, 2, &f);
  CHECK(f.n_states == 3 && f.final_state == 2 && f.arcs[0].dst == 1 && f.arcs[1].src == 1 && f.arcs[1].dst == 2);
  printf("compact_lattice OK\n");
  return 0;
}
