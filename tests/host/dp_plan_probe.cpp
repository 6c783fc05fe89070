// dp_plan_probe SECTION ARGS... [NAME=VALUE ...] -- the launches scrf_dp_plan.h plans, one line each, under knobs read from the
// arguments alone (as knobs_probe).  tests/test_dp_plan.py
//   exp_m L N_MAT                          dp_wave L D MPF N_UTTS            dp_lin L D MPF N_UTTS N_CU
//   atb L N_CHUNKS                         fb L D                            viterbi L D
//   viterbi_fast L D USE_TF N_UTTS         fb_segtrans L D N_UTTS            post_occ L D SPLIT_OK N_UTTS T_MAX
//   align_wave D N_UTTS                    sl_fb L D LA N_UTTS                sl_atb L D LA N_CHUNKS
//   support L D USE_TF USE_TB              what the predicates and the LDS-size functions say about a layout
//   sweep SECTION                          every call of one section over the shapes below
// A line: the section, the call's arguments by name, then kernel=NAME<template arguments> grid=x/y/z threads=N lds=BYTES and
// what else the plan carries.  ok=1: the predicate (or the engine's LDS check) that guards the launch admits the shape.
// post_occ folds N_UTTS x T_MAX into one line: walk=gx/nz/seg_len per call, and stops if they move anything else.
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "scrf_dp_plan.h"

static int g_argc;
static char** g_argv;
static const char* get(const char* name) {
  const size_t n = strlen(name);
  for (int i = 1; i < g_argc; i++)
    if (!strncmp(g_argv[i], name, n) && g_argv[i][n] == '=') return g_argv[i] + n + 1;
  return nullptr;
}

static const uint32_t LS[] = {1, 3, 4, 16, 32, 33, 47, 48, 49, 52, 63, 64, 65, 96, 128, 129, 192, 193, 200, 208, 209, 256, 257, 512, 1024};
static const uint32_t N_UTTS[] = {1, 11, 12, 13, 95, 96, 97, 128, 129, 256, 257, 383, 384, 385, 1024, 3072, 3073, 8192, 65535};
static const int N_CUS[] = {256, 64};
static const uint32_t LAS[] = {1, 16, 17, 48, 64, 65};
static const uint32_t D_MAX = 41;
static const size_t LDS_BYTES = 160 * 1024;   // SCRF_LDS_BYTES, what the engine's checks compare with
#define N_OF(a) (sizeof(a) / sizeof((a)[0]))
static std::vector<uint32_t> t_maxes(uint32_t D) { return {1, 2 * D - 1, 2 * D, 4 * D - 1, 4 * D, 1000}; }

static std::string fmt(const char* f, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, f);
  vsnprintf(buf, sizeof(buf), f, ap);
  va_end(ap);
  return buf;
}
static ScrfDpShape shape(uint32_t L, uint32_t D, int tf = 0, int tb = 1) { return ScrfDpShape{L, D, tf, tb}; }

// ---- what a call launches
struct Launch {
  std::string kernel;
  uint32_t gx = 1, gy = 1, gz = 1, threads = 0;
  size_t lds = 0;
  std::string text() const { return fmt("kernel=%s grid=%u/%u/%u threads=%u lds=%zu", kernel.c_str(), gx, gy, gz, threads, lds); }
};

static Launch exp_m(const ScrfKnobs& kn, uint32_t L, uint64_t n_mat) {
  const ScrfExpMPlan p = exp_m_plan(kn, L, n_mat);
  return {p.ne ? fmt("k_exp_m_tile<%d>", p.ne) : "k_exp_m", p.gx, 1, 1, p.threads, 0};
}
static Launch dp_wave(uint32_t L, uint32_t D, int mpf, uint32_t n_utts) {
  const ScrfDpWavePlan p = dp_wave_plan(shape(L, D), n_utts, mpf);
  return {fmt("k_dp_wave<%d,%d>", p.dmax, p.mpf), p.blocks, 1, 1, p.threads, p.lds};
}
static Launch dp_lin(const ScrfKnobs& kn, uint32_t L, uint32_t D, int mpf, uint32_t n_utts, int n_cu) {
  const ScrfDpLinPlan p = dp_lin_plan(kn, shape(L, D), n_utts, mpf, n_cu);
  const std::string k = p.kernel == SCRF_DK_LIN      ? fmt("k_dp_lin<%d,%d,%d>", p.dmax, p.mpf, p.lc)
                        : p.kernel == SCRF_DK_LIN_MV ? fmt("k_dp_lin_mv<%d,%d>", p.dmax, p.mpf)
                                                     : fmt("k_dp_lin_mw<%d,%d,%d,%d>", p.dmax, p.mpf, p.lr, p.tail);
  if (k.compare(0, k.find('<'), scrf_dp_lin_kernel_name(p.kernel)) || p.threads != 64 * p.wpb) { fprintf(stderr, "dp_lin: the plan disagrees with itself\n"); exit(3); }
  return {k, p.blocks, 1, 1, p.threads, p.lds};
}
static Launch atb(uint32_t L, uint32_t n_chunks) {
  const ScrfAtbPlan p = atb_plan(shape(L, 1), n_chunks);
  return {fmt("k_atb<%d>", p.lt), p.gx, p.gy, 1, p.threads, 0};
}
static Launch fb(uint32_t L, uint32_t D) {
  const ScrfGroupPlan p = fb_plan(shape(L, D));
  return {"k_fb", 1, 1, 1, p.threads, p.lds};
}
static Launch viterbi(uint32_t L, uint32_t D) {
  const ScrfGroupPlan p = viterbi_plan(shape(L, D));
  return {"k_viterbi", 1, 1, 1, p.threads, p.lds};
}
static Launch viterbi_fast(const ScrfKnobs& kn, uint32_t L, uint32_t D, int tf, uint32_t n_utts) {
  const ScrfViterbiFastPlan p = viterbi_fast_plan(kn, shape(L, D, tf), n_utts);
  return {fmt("k_viterbi_fast<%d,%d>", p.dmax, p.lv), p.gx, 1, 1, p.threads, p.lds};
}
static Launch fb_segtrans(const ScrfKnobs& kn, uint32_t L, uint32_t D, uint32_t n_utts) {
  const ScrfFbSegtransPlan p = fb_segtrans_plan(kn, shape(L, D), n_utts);
  return {p.wave ? "k_fb_segtrans_w" : "k_fb_segtrans", n_utts, 1, 1, p.threads, p.lds};
}
// seg_len and whether k_sum_groups follows, beside the launch
static Launch post_occ(uint32_t L, uint32_t D, int split_ok, uint32_t n_utts, uint32_t t_max, int* seg_len, int* sum_groups) {
  const ScrfPostOccPlan p = post_occ_plan(shape(L, D), n_utts, t_max, split_ok);
  *seg_len = p.seg_len;
  *sum_groups = p.sum_groups;
  return {fmt("k_post_occ<%d,%d>", p.dmax, p.rw), p.gx, p.gy, p.nz, 64, 0};
}
static Launch align_wave(uint32_t D, uint32_t n_utts) {
  const ScrfAlignWavePlan p = align_wave_plan(shape(1, D), n_utts);
  return {fmt("k_align_wave<%d>", p.dmax), p.gx, 1, 1, p.threads, p.lds};
}
static Launch sl_fb(uint32_t L, uint32_t D, uint32_t n_utts) {
  const ScrfSlFbPlan p = sl_fb_plan(shape(L, D), n_utts);
  return {"k_sl_fb", p.gx, 1, 1, p.threads, p.lds};
}
static Launch sl_atb(uint32_t L, uint32_t D, uint32_t La, uint32_t n_chunks) {
  const ScrfSlAtbPlan p = sl_atb_plan(shape(L, D), La, n_chunks);
  return {fmt("k_sl_atb<%d>", p.nt), p.gx, 1, 1, p.threads, 0};
}
static std::string support(uint32_t L, uint32_t D, int tf, int tb) {
  const ScrfDpShape s = shape(L, D, tf, tb);
  std::string t = fmt("dp_wave=%d dplin=%d dplin_mw=%d atb=%d viterbi_fast=%d align_wave=%d fb_threads=%d fb_smem=%zu fb_segtrans_smem=%zu",
                      dp_wave_supported(s), dplin_supported(s), dplin_mw_supported(s), atb_supported(s), viterbi_fast_supported(s),
                      align_wave_supported(s), fb_block_threads(s), fb_smem_bytes(s, fb_block_threads(s)),
                      fb_segtrans_smem_bytes(s, fb_block_threads(s)));
  t += fmt(" lat_sweep_smem=%zu post_occ_groups=%u align_group_smem=%zu/%zu transcript_smem=%zu/%zu nbest_smem=%zu/%zu stdseg_lin=", lat_sweep_smem_bytes(s),
           post_occ_groups(s), align_group_smem_bytes(s, 65), align_group_smem_bytes(s, 1000), transcript_smem_bytes(s, 1), transcript_smem_bytes(s, 128),
           nbest_smem_bytes(s, 1), nbest_smem_bytes(s, 10));
  for (size_t i = 0; i < N_OF(LAS); i++) t += fmt("%s%d", i ? "/" : "", stdseg_lin_supported(s, LAS[i]));
  return t;
}
// ---- the lines

static void line_exp_m(const ScrfKnobs& kn, uint32_t L, uint64_t n) { printf("exp_m L=%u n_mat=%llu %s\n", L, (unsigned long long)n, exp_m(kn, L, n).text().c_str()); }
static void line_dp_wave(uint32_t L, uint32_t D, int mpf, uint32_t n) {
  printf("dp_wave L=%u D=%u mpf=%d n_utts=%u ok=%d %s\n", L, D, mpf, n, dp_wave_supported(shape(L, D)), dp_wave(L, D, mpf, n).text().c_str());
}
static void line_dp_lin(const ScrfKnobs& kn, uint32_t L, uint32_t D, int mpf, uint32_t n, int cu) {
  printf("dp_lin L=%u D=%u mpf=%d n_utts=%u n_cu=%d ok=%d %s\n", L, D, mpf, n, cu, dplin_supported(shape(L, D)) || dplin_mw_supported(shape(L, D)),
         dp_lin(kn, L, D, mpf, n, cu).text().c_str());
}
static void line_atb(uint32_t L, uint32_t n) { printf("atb L=%u n_chunks=%u ok=%d %s\n", L, n, atb_supported(shape(L, 1)), atb(L, n).text().c_str()); }
// (the engine refuses a layout whose k_fb / k_fb_segtrans workgroup passes the LDS; launch_viterbi has no such check)
static void line_fb(uint32_t L, uint32_t D) {
  const Launch l = fb(L, D);
  printf("fb L=%u D=%u ok=%d %s\n", L, D, l.lds <= LDS_BYTES, l.text().c_str());
}
static void line_viterbi(uint32_t L, uint32_t D) { printf("viterbi L=%u D=%u ok=0 %s\n", L, D, viterbi(L, D).text().c_str()); }
static void line_viterbi_fast(const ScrfKnobs& kn, uint32_t L, uint32_t D, int tf, uint32_t n) {
  printf("viterbi_fast L=%u D=%u use_tf=%d n_utts=%u ok=%d %s\n", L, D, tf, n, viterbi_fast_supported(shape(L, D, tf)), viterbi_fast(kn, L, D, tf, n).text().c_str());
}
static void line_fb_segtrans(const ScrfKnobs& kn, uint32_t L, uint32_t D, uint32_t n) {
  const Launch l = fb_segtrans(kn, L, D, n);
  printf("fb_segtrans L=%u D=%u n_utts=%u ok=%d %s\n", L, D, n, l.lds <= LDS_BYTES, l.text().c_str());
}
static void line_post_occ(uint32_t L, uint32_t D, int split_ok, const std::vector<uint32_t>& utts, const std::vector<uint32_t>& tms) {
  std::string form, walk;
  for (uint32_t n : utts)
    for (uint32_t tm : tms) {
      int seg_len, sum_groups;
      const Launch l = post_occ(L, D, split_ok, n, tm, &seg_len, &sum_groups);
      const std::string f = fmt("kernel=%s gy=%u threads=%u lds=%zu sum_groups=%d", l.kernel.c_str(), l.gy, l.threads, l.lds, sum_groups);
      if (form.empty()) form = f;
      else if (f != form) { fprintf(stderr, "post_occ: a folded axis moves the form: \"%s\" / \"%s\"\n", form.c_str(), f.c_str()); exit(3); }
      walk += fmt("%s%u/%u/%d", walk.empty() ? "" : ",", l.gx, l.gz, seg_len);
    }
  printf("post_occ L=%u D=%u split_ok=%d ok=%d %s walk=%s\n", L, D, split_ok, dplin_supported(shape(L, D)) || dplin_mw_supported(shape(L, D)), form.c_str(), walk.c_str());
}
static void line_align_wave(uint32_t D, uint32_t n) { printf("align_wave D=%u n_utts=%u ok=%d %s\n", D, n, align_wave_supported(shape(1, D)), align_wave(D, n).text().c_str()); }
// (use_tf / use_tb move stdseg_lin_supported alone: the support section has them)
static void line_sl_fb(uint32_t L, uint32_t D, uint32_t La, uint32_t n) {
  printf("sl_fb L=%u D=%u La=%u n_utts=%u ok=%d %s\n", L, D, La, n, stdseg_lin_supported(shape(L, D), La), sl_fb(L, D, n).text().c_str());
}
static void line_sl_atb(uint32_t L, uint32_t D, uint32_t La, uint32_t n) {
  printf("sl_atb L=%u D=%u La=%u n_chunks=%u ok=%d %s\n", L, D, La, n, stdseg_lin_supported(shape(L, D), La), sl_atb(L, D, La, n).text().c_str());
}
static void line_support(uint32_t L, uint32_t D, int tf, int tb) { printf("support L=%u D=%u use_tf=%d use_tb=%d %s\n", L, D, tf, tb, support(L, D, tf, tb).c_str()); }

// ---- the sweep
#define FOR_L for (uint32_t L : LS)
#define FOR_D for (uint32_t D = 1; D <= D_MAX; D++)
#define FOR_N for (uint32_t n : N_UTTS)
#define FOR_01(v) for (int v = 0; v < 2; v++)
static int sweep(const ScrfKnobs& kn, const char* s) {
  if (!strcmp(s, "exp_m")) { FOR_L FOR_N line_exp_m(kn, L, n); }
  else if (!strcmp(s, "dp_wave")) { FOR_L FOR_D FOR_01(mpf) FOR_N line_dp_wave(L, D, mpf, n); }
  else if (!strcmp(s, "dp_lin")) { FOR_L FOR_D FOR_01(mpf) FOR_N for (int cu : N_CUS) line_dp_lin(kn, L, D, mpf, n, cu); }
  else if (!strcmp(s, "atb")) { FOR_L FOR_N line_atb(L, n); }
  else if (!strcmp(s, "fb")) { FOR_L FOR_D line_fb(L, D); }
  else if (!strcmp(s, "viterbi")) { FOR_L FOR_D line_viterbi(L, D); }
  else if (!strcmp(s, "viterbi_fast")) { FOR_L FOR_D FOR_01(tf) FOR_N line_viterbi_fast(kn, L, D, tf, n); }
  else if (!strcmp(s, "fb_segtrans")) { FOR_L FOR_D FOR_N line_fb_segtrans(kn, L, D, n); }
  else if (!strcmp(s, "post_occ")) { FOR_L FOR_D FOR_01(ok) line_post_occ(L, D, ok, std::vector<uint32_t>(N_UTTS, N_UTTS + N_OF(N_UTTS)), t_maxes(D)); }
  else if (!strcmp(s, "align_wave")) { FOR_D FOR_N line_align_wave(D, n); }
  else if (!strcmp(s, "sl_fb")) { FOR_L FOR_D for (uint32_t La : LAS) for (uint32_t n : {1u, 65535u}) line_sl_fb(L, D, La, n); }
  else if (!strcmp(s, "sl_atb")) { FOR_L FOR_D for (uint32_t La : LAS) for (uint32_t n : {1u, 13u, 1024u}) line_sl_atb(L, D, La, n); }
  else if (!strcmp(s, "support")) { FOR_L FOR_D FOR_01(tf) FOR_01(tb) line_support(L, D, tf, tb); }
  else return 2;
  return 0;
}

int main(int argc, char** argv) {
  g_argc = argc;
  g_argv = argv;
  const ScrfKnobs kn = scrf_knobs_read(get);
  std::vector<unsigned long> v;   // the positional arguments: everything after the section that is not NAME=VALUE
  for (int i = 2; i < argc; i++)
    if (!strchr(argv[i], '=')) v.push_back(strtoul(argv[i], nullptr, 10));
  const char* s = argc > 1 ? argv[1] : "";
  const size_t n = v.size();
  if (!strcmp(s, "sweep") && argc > 2) return sweep(kn, argv[2]);
  if (!strcmp(s, "exp_m") && n == 2) line_exp_m(kn, v[0], v[1]);
  else if (!strcmp(s, "dp_wave") && n == 4) line_dp_wave(v[0], v[1], (int)v[2], v[3]);
  else if (!strcmp(s, "dp_lin") && n == 5) line_dp_lin(kn, v[0], v[1], (int)v[2], v[3], (int)v[4]);
  else if (!strcmp(s, "atb") && n == 2) line_atb(v[0], v[1]);
  else if (!strcmp(s, "fb") && n == 2) line_fb(v[0], v[1]);
  else if (!strcmp(s, "viterbi") && n == 2) line_viterbi(v[0], v[1]);
  else if (!strcmp(s, "viterbi_fast") && n == 4) line_viterbi_fast(kn, v[0], v[1], (int)v[2], v[3]);
  else if (!strcmp(s, "fb_segtrans") && n == 3) line_fb_segtrans(kn, v[0], v[1], v[2]);
  else if (!strcmp(s, "post_occ") && n == 5) line_post_occ(v[0], v[1], (int)v[2], {(uint32_t)v[3]}, {(uint32_t)v[4]});
  else if (!strcmp(s, "align_wave") && n == 2) line_align_wave(v[0], v[1]);
  else if (!strcmp(s, "sl_fb") && n == 4) line_sl_fb(v[0], v[1], v[2], v[3]);
  else if (!strcmp(s, "sl_atb") && n == 4) line_sl_atb(v[0], v[1], v[2], v[3]);
  else if (!strcmp(s, "support") && n == 4) line_support(v[0], v[1], (int)v[2], (int)v[3]);
  else {
    fprintf(stderr, "usage: dp_plan_probe SECTION ARGS... | sweep SECTION  [NAME=VALUE ...]  (the sections and their arguments: the head of dp_plan_probe.cpp)\n");
    return 2;
  }
  return 0;
}
