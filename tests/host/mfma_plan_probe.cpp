// mfma_plan_probe KIND SHAPE... [NAME=VALUE ...] -- the launches scrf_mfma_plan.h plans, one line each, under knobs read from
// the arguments alone (as knobs_probe).  tests/test_mfma_plan.py, tests/test_mfma_forms.py
//   scores N_OUT NFE F32              one call of launch_scores_mfma
//   counts N_OUT NFUN F32 HAS_XROW    one call of launch_expf_mfma
//   sweep  N_OUT_MAX NF_MAX           every call of both over n_out 1..N_OUT_MAX, nfe / nfun 1..NF_MAX, f32 and has_xrow 0 / 1
// A launch line: the call ("scores n_out nfe_lo nfe_hi f32" / "counts n_out nfun_lo nfun_hi f32 has_xrow"), then "kernel=..."
// and the fields of ScrfMfmaLaunch by name; "wide_tiles=" closes a counts line (expf_mfma_wide_tiles of the call).  lo..hi
// is a run of feature counts whose calls plan the same launches field for field (the sweep prints a run once; a single call
// has lo = hi), so nothing of the sweep is left out.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "scrf_mfma_plan.h"

static int g_argc;
static char** g_argv;
static const char* get(const char* name) {
  const size_t n = strlen(name);
  for (int i = 1; i < g_argc; i++)
    if (!strncmp(g_argv[i], name, n) && g_argv[i][n] == '=') return g_argv[i] + n + 1;
  return nullptr;
}

struct Plan {
  int n = 0;
  ScrfMfmaLaunch l[SCRF_MFMA_MAX_LAUNCHES];
  uint32_t wide = 0;
};

static bool same(const ScrfMfmaLaunch& a, const ScrfMfmaLaunch& b) {
  return a.kernel == b.kernel && a.f32 == b.f32 && a.nt == b.nt && a.mw == b.mw && a.ntw == b.ntw && a.has_xrow == b.has_xrow && a.nw == b.nw &&
         a.kc == b.kc && a.mt == b.mt && a.mtw == b.mtw && a.db == b.db && a.o_base == b.o_base && a.gy == b.gy && a.o_step == b.o_step &&
         a.gx == b.gx && a.lds == b.lds;
}
static bool same(const Plan& a, const Plan& b) {
  if (a.n != b.n || a.wide != b.wide) return false;
  for (int i = 0; i < a.n; i++)
    if (!same(a.l[i], b.l[i])) return false;
  return true;
}

static Plan scores(const ScrfKnobs& kn, uint32_t n_out, uint32_t nfe, int f32) {
  Plan p;
  p.n = scrf_scores_mfma_plan(kn, n_out, nfe, f32, p.l);
  return p;
}
static Plan counts(const ScrfKnobs& kn, uint32_t n_out, uint32_t nfun, int f32, int has_xrow) {
  Plan p;
  p.n = scrf_expf_mfma_plan(kn, n_out, nfun, f32, has_xrow, p.l);
  p.wide = expf_mfma_wide_tiles(n_out, nfun, f32);
  return p;
}

// has_xrow < 0: a score call
static void print_plan(const Plan& pl, uint32_t n_out, uint32_t lo, uint32_t hi, int f32, int has_xrow) {
  for (int i = 0; i < pl.n; i++) {
    const ScrfMfmaLaunch& p = pl.l[i];
    if (has_xrow < 0) printf("scores %u %u %u %d", n_out, lo, hi, f32);
    else printf("counts %u %u %u %d %d", n_out, lo, hi, f32, has_xrow);
    printf(" kernel=%s f32=%d nt=%d mw=%d ntw=%d has_xrow=%d nw=%d kc=%d mt=%d mtw=%d db=%d o_base=%u gy=%u o_step=%u gx=%u lds=%zu",
           scrf_mfma_kernel_name(p.kernel), p.f32, p.nt, p.mw, p.ntw, p.has_xrow, p.nw, p.kc, p.mt, p.mtw, p.db, p.o_base, p.gy, p.o_step, p.gx, p.lds);
    if (has_xrow < 0) printf("\n");
    else printf(" wide_tiles=%u\n", pl.wide);
  }
}

// the calls of one (n_out, f32, has_xrow) over nf = 1..nf_max, each run of equal plans once
static void sweep_nf(const ScrfKnobs& kn, uint32_t n_out, uint32_t nf_max, int f32, int has_xrow) {
  Plan run;
  uint32_t lo = 1;
  for (uint32_t nf = 1; nf <= nf_max; nf++) {
    const Plan p = has_xrow < 0 ? scores(kn, n_out, nf, f32) : counts(kn, n_out, nf, f32, has_xrow);
    if (nf == 1) run = p;
    if (!same(p, run)) {
      print_plan(run, n_out, lo, nf - 1, f32, has_xrow);
      run = p;
      lo = nf;
    }
  }
  if (nf_max) print_plan(run, n_out, lo, nf_max, f32, has_xrow);
}

static int usage() {
  fprintf(stderr, "usage: mfma_plan_probe scores N_OUT NFE F32 | counts N_OUT NFUN F32 HAS_XROW | sweep N_OUT_MAX NF_MAX  [NAME=VALUE ...]\n");
  return 2;
}

int main(int argc, char** argv) {
  g_argc = argc;
  g_argv = argv;
  const ScrfKnobs kn = scrf_knobs_read(get);
  // the positional arguments: everything after the kind that is not NAME=VALUE
  unsigned long v[4] = {0, 0, 0, 0};
  int nv = 0;
  for (int i = 2; i < argc; i++) {
    if (strchr(argv[i], '=')) continue;
    if (nv == 4) return usage();
    v[nv++] = strtoul(argv[i], nullptr, 10);
  }
  if (argc < 2) return usage();
  if (!strcmp(argv[1], "scores") && nv == 3) {
    print_plan(scores(kn, (uint32_t)v[0], (uint32_t)v[1], v[2] != 0), (uint32_t)v[0], (uint32_t)v[1], (uint32_t)v[1], v[2] != 0, -1);
  } else if (!strcmp(argv[1], "counts") && nv == 4) {
    print_plan(counts(kn, (uint32_t)v[0], (uint32_t)v[1], v[2] != 0, v[3] != 0), (uint32_t)v[0], (uint32_t)v[1], (uint32_t)v[1], v[2] != 0, v[3] != 0);
  } else if (!strcmp(argv[1], "sweep") && nv == 2) {
    for (uint32_t n_out = 1; n_out <= v[0]; n_out++)
      for (int f32 = 0; f32 < 2; f32++) {
        sweep_nf(kn, n_out, (uint32_t)v[1], f32, -1);
        for (int x = 0; x < 2; x++) sweep_nf(kn, n_out, (uint32_t)v[1], f32, x);
      }
  } else {
    return usage();
  }
  return 0;
}
