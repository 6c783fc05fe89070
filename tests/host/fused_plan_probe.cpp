// fused_plan_probe KIND ARGS... [NAME=VALUE ...] -- the launches scrf_fused_plan.h plans, one line each, under knobs read from
// the arguments alone (as knobs_probe).  tests/test_fused_plan.py
//   scores L D W MODE                            one call of launch_scores_fused (MODE 0 fp64, 1 f32, 2 la) / _decode (3)
//   counts L D USE_SB W F32 LA ALIGNED N_TILES    one call of launch_expf_fused
//   sweep SECTION                                 every call of one launcher over the shapes below; SECTION is one of
//                                                 support scores counts post_z lin_z lin_z5 pframe ztf
// A line: the section, the call's arguments by name, then the plan's fields by name.  W=lo..hi is a run of frame widths
// whose calls plan the same launch field for field (the sweep prints a run once; a single call has lo = hi).  The axes
// that move nothing but the grid are folded into the line: such a field is a comma list with one entry per value of the
// axis (N_TILES, N_UTTS x T_MAX, ... in the order below; "/" separates the fields of an entry).  The sweep still plans
// every call of the cross product, and stops with an error if a folded axis moves any other field, so nothing of the
// sweep is left out.
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "scrf_fused_plan.h"

static int g_argc;
static char** g_argv;
static const char* get(const char* name) {
  const size_t n = strlen(name);
  for (int i = 1; i < g_argc; i++)
    if (!strncmp(g_argv[i], name, n) && g_argv[i][n] == '=') return g_argv[i] + n + 1;
  return nullptr;
}

static const uint32_t LS[] = {1, 6, 7, 47, 48, 49, 63, 64, 65, 96, 200, 256};
static const uint64_t N_TILES[] = {0, 1, 3, 255, 256, 257, 511, 512, 513, 100000};
static const uint32_t N_UTTS[] = {1, 8, 64, 256, 512, 513, 2048};
static const uint32_t D_MAX = 41, W_MAX = 210;
#define N_OF(a) (sizeof(a) / sizeof((a)[0]))
// t_max of the walks, by D
static std::vector<uint32_t> t_maxes(uint32_t D) { return {1, 2 * D - 1, 2 * D, 4 * D - 1, 4 * D, 1000}; }

static std::string fmt(const char* f, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, f);
  vsnprintf(buf, sizeof(buf), f, ap);
  va_end(ap);
  return buf;
}
[[noreturn]] static void folded_axis_moved(const char* section, const std::string& a, const std::string& b) {
  fprintf(stderr, "%s: a folded axis moves the form: \"%s\" / \"%s\"\n", section, a.c_str(), b.c_str());
  exit(3);
}

// ---- what a call plans, as text: `form` (everything the folded axes must leave alone) and the grid entry
struct Planned { std::string form, grid; };

static ScrfFusedShape shape(uint32_t L, uint32_t D, int sb) { return ScrfFusedShape{L, D, sb}; }

static std::string support(const ScrfKnobs& kn, uint32_t L, uint32_t D, int sb, uint32_t W, int f32) {
  return fmt("fused=%d la=%d", fused_supported(kn, shape(L, D, sb), W, f32), f32 ? 0 : fused_la_supported(kn, shape(L, D, sb), W));
}
// the launch tables as the engine has them: the duration table under SCRF_DTAB, the tile tables under SCRF_RTAB beside it
// (L moves the grid's gy and smax, nothing else)
static Planned scores(const ScrfKnobs& kn, uint32_t L, uint32_t D, uint32_t W, int mode) {
  const ScrfFusedScoresPlan p = fused_scores_plan(kn, shape(L, D, 0), W, mode == 1, mode == 3, mode == 2, kn.dtab, kn.dtab && kn.rtab);
  if (!p.tb) return {"kernel=none", "0/0"};
  return {fmt("kernel=k_scores_fused dmax=%d f32=%d dec=%d la=%d dma=%d tb=%u threads=%u lds=%zu", p.dmax, p.f32, p.dec, p.la, p.dma, p.tb, p.threads, p.lds),
          fmt("%u/%d", p.gy, p.smax)};
}
// (the form as numbers: the sweep compares it across 240 calls per width and prints it once)
static const char* const COUNT_FIELDS[] = {"ws", "g0", "ncol", "ndur", "rows", "frames", "tile_list", "nz", "nt", "dmax", "nks", "f32", "n_ct", "xs", "nfmax", "threads", "lds"};
struct Counts {
  int kernel;   // ScrfFusedExpfKernel
  long form[N_OF(COUNT_FIELDS)];
  uint32_t gy; int dma; uint32_t gx;
  bool same_form(const Counts& o) const { return kernel == o.kernel && !memcmp(form, o.form, sizeof(form)); }
  std::string text() const {
    std::string t = fmt("kernel=%s", scrf_fused_expf_kernel_name(kernel));
    for (size_t i = 0; i < N_OF(COUNT_FIELDS) && kernel != SCRF_FK_NONE; i++) t += fmt(" %s=%ld", COUNT_FIELDS[i], form[i]);
    return t;
  }
};
static Counts counts(const ScrfKnobs& kn, uint32_t L, uint32_t D, int sb, uint32_t W, int f32, int la, int aligned, uint64_t n_tiles) {
  const ScrfFusedExpfPlan p = fused_expf_plan(kn, shape(L, D, sb), W, f32, la, aligned);
  Counts c = {p.kernel, {p.ws, p.g0, (long)p.ncol, (long)p.ndur, (long)p.rows, (long)p.frames, p.tile_list, (long)p.nz, p.nt, p.dmax, p.nks, p.f32,
                         (long)p.n_ct, (long)p.xs, (long)p.nfmax, (long)p.threads, (long)p.lds},
              p.gy, p.dma, fused_expf_blocks(p, n_tiles)};
  return c;
}
static Planned post_z(const ScrfKnobs& kn, uint32_t L, uint32_t D, int la, uint32_t n_utts, uint32_t t_max) {
  const ScrfFusedWalkPlan p = fused_post_z_plan(kn, shape(L, D, 0), n_utts, la, t_max);
  return {fmt("kernel=k_post_z dmax=%d la=%d rw=%d gy=%u", p.dmax, p.la, p.rw, p.gy), fmt("%u/%u/%d/%d/%d", p.gx, p.nz, p.split, p.seg_len, p.clear_z)};
}
static Planned lin_z(uint32_t L, uint32_t D, uint32_t n_utts) {
  const ScrfFusedWalkPlan p = fused_lin_z_plan(shape(L, D, 0), n_utts);
  return {fmt("kernel=k_lin_z dmax=%d gy=%u", p.dmax, p.gy), fmt("%u", p.gx)};
}
static Planned lin_z5(uint32_t L, uint32_t D, uint32_t n_utts, uint32_t t_max) {
  const ScrfFusedWalkPlan p = fused_lin_z5_plan(shape(L, D, 0), n_utts, t_max);
  return {fmt("kernel=k_lin_z5 dmax=%d gy=%u", p.dmax, p.gy), fmt("%u/%u/%d/%d", p.gx, p.nz, p.seg_len, p.clear_z)};
}
static Planned pframe(uint32_t W, uint64_t n_frames, uint32_t n_out) {
  const ScrfPframePlan p = fused_pframe_plan(W, n_frames, n_out);
  return {fmt("kernel=k_pframe ks=%d gy=%u", p.ks, p.gy), fmt("%u/%llu", p.gx, (unsigned long long)p.fpw)};
}
static Planned ztf(uint32_t W, uint32_t n_out, uint32_t n_chunks, int narrow) {
  const ScrfZtfPlan p = fused_ztf_plan(W, n_out, n_chunks, narrow);
  return {fmt("kernel=k_ztf nt=%d mt=%d gy=%u", p.nt, p.mt, p.gy), fmt("%u", p.gx)};
}

// ---- the sweep
// the lines of one key over W = 1..w_max, each run of equal lines once
struct Runs {
  std::string key, cur;
  uint32_t lo = 1, last = 0;
  explicit Runs(const std::string& k) : key(k) {}
  void add(uint32_t W, const std::string& line) {
    if (last && line != cur) flush();
    if (!last || line != cur) { cur = line; lo = W; }
    last = W;
  }
  void flush() {
    if (last) printf("%s W=%u..%u %s\n", key.c_str(), lo, last, cur.c_str());
  }
};
// folds the grid entries of the calls f(i), i < n, into one list; the forms must agree
template <class F>
static std::string fold(const char* section, size_t n, F f) {
  std::string form, list;
  for (size_t i = 0; i < n; i++) {
    const Planned p = f(i);
    if (i == 0) form = p.form;
    else if (p.form != form) folded_axis_moved(section, form, p.form);
    list += (i ? "," : "") + p.grid;
  }
  return form + " grid=" + list;
}

static void sweep_support(const ScrfKnobs& kn) {
  for (uint32_t L : LS)
    for (uint32_t D = 1; D <= D_MAX; D++)
      for (int sb = 0; sb < 2; sb++)
        for (int f32 = 0; f32 < 2; f32++) {
          Runs r(fmt("support L=%u D=%u use_sb=%d f32=%d", L, D, sb, f32));
          for (uint32_t W = 1; W <= W_MAX; W++) r.add(W, support(kn, L, D, sb, W, f32));
          r.flush();
        }
}
static void sweep_scores(const ScrfKnobs& kn) {
  for (uint32_t D = 1; D <= D_MAX; D++)
    for (int mode = 0; mode < 4; mode++) {
      Runs r(fmt("scores D=%u mode=%d", D, mode));
      for (uint32_t W = 1; W <= W_MAX; W++) r.add(W, fold("scores", N_OF(LS), [&](size_t i) { return scores(kn, LS[i], D, W, mode); }));
      r.flush();
    }
}
// L moves gy and, by its parity, dma; the alignment of R moves dma; n_tiles moves gx: three lists (gy by L, dma by L and
// alignment, gx by n_tiles), each checked against every call of the cross product
static void sweep_counts(const ScrfKnobs& kn) {
  for (uint32_t D = 1; D <= D_MAX; D++)
    for (int sb = 0; sb < 2; sb++)
      for (int f32 = 0; f32 < 2; f32++)
        for (int la = 0; la < 2; la++) {
          Runs r(fmt("counts D=%u use_sb=%d f32=%d la=%d", D, sb, f32, la));
          for (uint32_t W = 1; W <= W_MAX; W++) {
            const Counts c0 = counts(kn, LS[0], D, sb, W, f32, la, 0, N_TILES[0]);
            std::string gy, dma, gx;
            uint32_t gx_of[N_OF(N_TILES)];
            for (size_t ti = 0; ti < N_OF(N_TILES); ti++) {
              gx_of[ti] = counts(kn, LS[0], D, sb, W, f32, la, 0, N_TILES[ti]).gx;
              gx += fmt("%s%u", ti ? "," : "", gx_of[ti]);
            }
            for (size_t li = 0; li < N_OF(LS); li++)
              for (int al = 0; al < 2; al++) {
                const Counts ca = counts(kn, LS[li], D, sb, W, f32, la, al, N_TILES[0]);
                if (al == 0) gy += fmt("%s%u", li ? "," : "", ca.gy);
                dma += fmt("%s%d", (li || al) ? "," : "", ca.dma);
                for (size_t ti = 0; ti < N_OF(N_TILES); ti++) {
                  const Counts c = counts(kn, LS[li], D, sb, W, f32, la, al, N_TILES[ti]);
                  if (!c.same_form(c0)) folded_axis_moved("counts", c0.text(), c.text());
                  if (c.gy != ca.gy || c.dma != ca.dma || c.gx != gx_of[ti])
                    folded_axis_moved("counts (grid)", c0.text(), c.text());
                }
              }
            r.add(W, c0.kernel == SCRF_FK_NONE ? c0.text() : c0.text() + " gy=" + gy + " dma=" + dma + " gx=" + gx);
          }
          r.flush();
        }
}
static void sweep_walks(const ScrfKnobs& kn, int which) {   // 0 k_post_z, 1 k_lin_z, 2 k_lin_z5
  for (uint32_t L : LS)
    for (uint32_t D = 1; D <= D_MAX; D++) {
      const std::vector<uint32_t> tm = t_maxes(D);
      const size_t nu = N_OF(N_UTTS), nt = tm.size();
      if (which == 0) {
        for (int la = 0; la < 2; la++)
          printf("post_z L=%u D=%u la=%d %s\n", L, D, la,
                 fold("post_z", nu * nt, [&](size_t i) { return post_z(kn, L, D, la, N_UTTS[i / nt], tm[i % nt]); }).c_str());
      } else if (which == 1) {
        printf("lin_z L=%u D=%u %s\n", L, D, fold("lin_z", nu, [&](size_t i) { return lin_z(L, D, N_UTTS[i]); }).c_str());
      } else {
        printf("lin_z5 L=%u D=%u %s\n", L, D, fold("lin_z5", nu * nt, [&](size_t i) { return lin_z5(L, D, N_UTTS[i / nt], tm[i % nt]); }).c_str());
      }
    }
}
// the per-frame contractions where pframe_supported says they run: outputs = 5 L (la: 6 L); frames / row chunks from N_TILES
static void sweep_frames(int ztf_section) {
  for (uint32_t L : LS)
    for (int la = 0; la < 2; la++)
      for (int narrow = 0; narrow < (ztf_section ? 2 : 1); narrow++) {
        Runs r(ztf_section ? fmt("ztf L=%u la=%d narrow=%d", L, la, narrow) : fmt("pframe L=%u la=%d", L, la));
        const uint32_t n_out = (la ? 6 : 5) * L;
        for (uint32_t W = 1; W <= W_MAX; W++) {
          if (!pframe_supported(W)) { r.add(W, "kernel=none"); continue; }
          r.add(W, fold(ztf_section ? "ztf" : "pframe", N_OF(N_TILES) - 1, [&](size_t i) {
                  return ztf_section ? ztf(W, n_out, (uint32_t)N_TILES[i + 1], narrow) : pframe(W, N_TILES[i + 1], n_out);
                }));
        }
        r.flush();
      }
}

static int usage() {
  fprintf(stderr, "usage: fused_plan_probe scores L D W MODE | counts L D USE_SB W F32 LA ALIGNED N_TILES | sweep SECTION  [NAME=VALUE ...]\n");
  return 2;
}

int main(int argc, char** argv) {
  g_argc = argc;
  g_argv = argv;
  const ScrfKnobs kn = scrf_knobs_read(get);
  std::vector<const char*> pos;   // the positional arguments: everything after the kind that is not NAME=VALUE
  for (int i = 2; i < argc; i++)
    if (!strchr(argv[i], '=')) pos.push_back(argv[i]);
  std::vector<unsigned long> v;
  for (const char* s : pos) v.push_back(strtoul(s, nullptr, 10));
  if (argc < 2) return usage();
  if (!strcmp(argv[1], "scores") && v.size() == 4) {
    const Planned p = scores(kn, v[0], v[1], v[2], (int)v[3]);
    printf("scores D=%lu mode=%lu W=%lu..%lu %s grid=%s\n", v[1], v[3], v[2], v[2], p.form.c_str(), p.grid.c_str());
  } else if (!strcmp(argv[1], "counts") && v.size() == 8) {
    const Counts c = counts(kn, v[0], v[1], (int)v[2], v[3], (int)v[4], (int)v[5], (int)v[6], v[7]);
    printf("counts D=%lu use_sb=%lu f32=%lu la=%lu W=%lu..%lu %s gy=%u dma=%d gx=%u\n", v[1], v[2], v[4], v[5], v[3], v[3], c.text().c_str(), c.gy, c.dma, c.gx);
  } else if (!strcmp(argv[1], "sweep") && pos.size() == 1) {
    const char* s = pos[0];
    if (!strcmp(s, "support")) sweep_support(kn);
    else if (!strcmp(s, "scores")) sweep_scores(kn);
    else if (!strcmp(s, "counts")) sweep_counts(kn);
    else if (!strcmp(s, "post_z")) sweep_walks(kn, 0);
    else if (!strcmp(s, "lin_z")) sweep_walks(kn, 1);
    else if (!strcmp(s, "lin_z5")) sweep_walks(kn, 2);
    else if (!strcmp(s, "pframe")) sweep_frames(0);
    else if (!strcmp(s, "ztf")) sweep_frames(1);
    else return usage();
  } else {
    return usage();
  }
  return 0;
}
