// knobs_probe NAME=VALUE ... -- scrf_knobs_read over an environment made of the arguments alone; prints every field
// ("field value") and every name of the table ("name SCRF_X").  tests/test_knobs.py
#include <stdio.h>
#include <string.h>

#include "scrf_knobs.h"

static int g_argc;
static char** g_argv;
static const char* get(const char* name) {
  const size_t n = strlen(name);
  for (int i = 1; i < g_argc; i++)
    if (!strncmp(g_argv[i], name, n) && g_argv[i][n] == '=') return g_argv[i] + n + 1;
  return nullptr;
}

int main(int argc, char** argv) {
  g_argc = argc;
  g_argv = argv;
  const ScrfKnobs k = scrf_knobs_read(get);
#define X(T, f, d, name, parse, doc) printf("%s %.17g\n", #f, (double)k.f);
  SCRF_KNOBS(X)
#undef X
  printf("pool_on %d\npool_up %d\nhybrid_on %d\nhybrid_first %d\n", k.pool_on(), k.pool_up(), k.hybrid_on(), k.hybrid_first());
  for (const ScrfKnobDoc& d : scrf_knob_docs) printf("name %s\n", d.name);
  return 0;
}
