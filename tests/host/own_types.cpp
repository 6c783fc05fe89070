// The engine's owning types (asr-craft_amd/csrc/scrf_own.h) on the CPU, against tests/host/fakehip: whatever is done with
// them -- reserve, reserve_keep, move, a failure at every creating call, destruction -- nothing stays live, nothing borrowed is
// released, and a failed reserve leaves an empty array.  The last part is scrf_create's allocation sequence in miniature,
// leaving through scrf_destroy's path when a call fails.
//   own_types              all checks; exit status 0 and "own_types OK"
//   own_types delete-only  the miniature leaves through `delete` alone, as scrf_create did on raw pointers: the same check
//                          must fail (exit status 1), which shows that it can
// Built with -fsanitize=address,undefined by tests/test_host_own.py.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <utility>
#include <vector>

#include "scrf_own.h"
using namespace scrf_eng;

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); exit(1); } } while (0)

static void fill(uint32_t* p, size_t n, uint32_t seed) { for (size_t i = 0; i < n; i++) p[i] = seed + (uint32_t)i * 2654435761u; }
static bool filled(const uint32_t* p, size_t n, uint32_t seed) {
  for (size_t i = 0; i < n; i++) if (p[i] != seed + (uint32_t)i * 2654435761u) return false;
  return true;
}

// one walk through everything an array, an event and a stream can do; any creating call may fail
static void exercise() {
  hipStream_t st = nullptr;
  {
    DevArray<uint32_t> a;
    CHECK(a.get() == nullptr && a.cap() == 0 && a.owned());
    if (a.reserve(100) != hipSuccess) CHECK(a.cap() == 0 && a.get() == nullptr);
    else CHECK(a.cap() == 100);
    uint32_t* before = a.get();
    if (before) CHECK(a.reserve(40) == hipSuccess && a.get() == before);   // enough room: nothing happens
    if (a.reserve(1000) != hipSuccess) CHECK(a.cap() == 0 && a.get() == nullptr);   // a failed reserve: empty, not dangling
    else CHECK(a.cap() == 1000);
    DevArray<uint32_t> b(std::move(a));
    CHECK(a.get() == nullptr && a.cap() == 0);
    DevArray<uint32_t> c;
    c.reserve(7);
    c = std::move(b);   // what c held is released
    CHECK(b.get() == nullptr && b.cap() == 0);
    DevArray<uint32_t>& same = c;
    c = std::move(same);   // self-assignment keeps it
    CHECK(c.cap() == 0 || c.cap() == 1000);
    // reserve_keep: the growth rule max(n_new, 2 cap, 65536), the first n_live elements survive
    DevArray<uint32_t> g;
    if (g.reserve_keep(10, 0, st) == hipSuccess) {
      CHECK(g.cap() == 65536);
      fill(g.get(), 65536, 17);
      CHECK(g.reserve_keep(65536, 65536, st) == hipSuccess && g.cap() == 65536);
      const size_t cap0 = g.cap();
      uint32_t* p0 = g.get();
      const hipError_t e = g.reserve_keep(65537, 60000, st);
      if (e == hipSuccess) {
        CHECK(g.cap() == 2 * 65536 && filled(g.get(), 60000, 17));
        fill(g.get(), g.cap(), 23);
        if (g.reserve_keep(1000000, g.cap(), st) == hipSuccess) CHECK(g.cap() == 1000000 && filled(g.get(), 2 * 65536, 23));
      } else {
        CHECK(g.cap() == cap0 && g.get() == p0 && filled(g.get(), 65536, 17));   // a failed reserve_keep: as it was
      }
    }
    PinnedArray<double> h;
    if (h.reserve(4) != hipSuccess) CHECK(h.cap() == 0 && h.get() == nullptr);
    else { h[0] = 1.5; CHECK(h.cap() == 4); }
    if (h.reserve(9) != hipSuccess) CHECK(h.cap() == 0 && h.get() == nullptr);
    PinnedArray<double> h2(std::move(h));
    CHECK(h.get() == nullptr);
    h = std::move(h2);
    Event ev, ev2;
    if (ev.create(hipEventDisableTiming) != hipSuccess) CHECK((hipEvent_t)ev == nullptr);
    if (ev.create() != hipSuccess) CHECK((hipEvent_t)ev == nullptr);   // the first one is destroyed
    ev2 = std::move(ev);
    CHECK((hipEvent_t)ev == nullptr);
    Stream s, s2;
    if (s.create(hipStreamNonBlocking) != hipSuccess) CHECK(s.get() == nullptr);
    s2 = std::move(s);
    CHECK(s.get() == nullptr && s.owned());
    if (s2.create(hipStreamNonBlocking) != hipSuccess) CHECK(s2.get() == nullptr);
  }
  CHECK(fakehip::live() == 0);
}

// borrowed memory and streams are the caller's: forgotten, never released (fakehip aborts on a release of what it did not
// hand out, and these it did not)
static void borrowed() {
  std::vector<double> mine(32, 2.0);
  fakehip_stream my_stream{7};
  {
    DevArray<double> a;
    CHECK(a.reserve(8) == hipSuccess);
    a.borrow(mine.data(), mine.size());   // the own block goes
    CHECK(fakehip::live() == 0 && !a.owned() && a.get() == mine.data() && a.cap() == 32);
    DevArray<double> b(std::move(a));     // borrowed state moves along
    CHECK(!b.owned() && a.owned() && a.get() == nullptr);
    b.reset();
    CHECK(b.owned() && b.get() == nullptr);
    CHECK(b.reserve(8) == hipSuccess && b.owned());
    b.borrow(mine.data(), mine.size());
    DevArray<double> c;
    c = std::move(b);   // destroyed while borrowed
    Stream s;
    CHECK(s.create(hipStreamNonBlocking) == hipSuccess && s.owned());
    s.borrow(&my_stream);                 // the own stream is destroyed
    CHECK(fakehip::live() == 0 && !s.owned() && s.get() == &my_stream);
    Stream t(std::move(s));
    CHECK(!t.owned() && t.get() == &my_stream);
    CHECK(t.create(hipStreamNonBlocking) == hipSuccess && t.owned());   // back to an own one
    t.borrow(&my_stream);                 // destroyed while borrowed
  }
  CHECK(fakehip::live() == 0 && mine[31] == 2.0 && my_stream.tag == 7);
}

// scrf_create in miniature: a handle of a dozen owning members made in sequence; a failing call leaves through the path of
// scrf_destroy (drain the streams, delete)
// One list of what the miniature makes, in order, for both variants below: S a stream, D a device array (type, name,
// elements), P a pinned array, E an event without timing, T a timing event.
#define MINI_SEQUENCE(S, D, P, E, T)                                                                                       \
  S(stream) D(double, d_lambda, 100) D(double, d_grad, 100) D(double, d_stage, 100) D(double, d_sums, 8) D(int, d_latch, 2) \
  P(int, h_latch, 2) P(double, h_sums, 4) E(ev_sums) E(ev_status) S(stream2) S(up_stream) E(ev_fork)                       \
  T(ev0a) T(ev0b) T(ev1a) T(ev1b) T(ev2a) T(ev2b)

struct MiniEngine {
#define S(n) Stream n;
#define D(t, n, c) DevArray<t> n;
#define P(t, n, c) PinnedArray<t> n;
#define E(n) Event n;
  MINI_SEQUENCE(S, D, P, E, E)
#undef S
#undef D
#undef P
#undef E
};
static void mini_destroy(MiniEngine* h) {
  for (hipStream_t s : {h->stream.get(), h->stream2.get(), h->up_stream.get()})
    if (s) hipStreamSynchronize(s);
  delete h;
}
static bool mini_create(MiniEngine** out) {
  MiniEngine* h = new MiniEngine();
#define CRCHK(call) if ((call) != hipSuccess) { mini_destroy(h); return false; }
#define S(n) CRCHK(h->n.create(hipStreamNonBlocking))
#define D(t, n, c) CRCHK(h->n.reserve(c))
#define E(n) CRCHK(h->n.create(hipEventDisableTiming))
#define T(n) CRCHK(h->n.create())
  MINI_SEQUENCE(S, D, D, E, T)
#undef CRCHK
#undef S
#undef D
#undef E
#undef T
  *out = h;
  return true;
}

// the same sequence on raw pointers, left through `delete` alone when a call fails: what scrf_create did before
struct RawEngine {
#define S(n) hipStream_t n = nullptr;
#define D(t, n, c) t* n = nullptr;
#define E(n) hipEvent_t n = nullptr;
  MINI_SEQUENCE(S, D, D, E, E)
#undef S
#undef D
#undef E
};
static bool raw_create(RawEngine** out) {
  RawEngine* h = new RawEngine();
#define CRCHK(call) if ((call) != hipSuccess) { delete h; return false; }
#define S(n) CRCHK(hipStreamCreateWithFlags(&h->n, hipStreamNonBlocking))
#define D(t, n, c) CRCHK(hipMalloc((void**)&h->n, sizeof(t) * c))
#define P(t, n, c) CRCHK(hipHostMalloc((void**)&h->n, sizeof(t) * c, hipHostMallocDefault))
#define E(n) CRCHK(hipEventCreateWithFlags(&h->n, hipEventDisableTiming))
#define T(n) CRCHK(hipEventCreate(&h->n))
  MINI_SEQUENCE(S, D, P, E, T)
#undef CRCHK
#undef S
#undef D
#undef P
#undef E
#undef T
  *out = h;
  return true;
}

int main(int argc, char** argv) {
  if (argc > 1 && strcmp(argv[1], "delete-only") == 0) {
    // the check of the miniature below, on the delete-only path: the last creating call fails, the 18 before it stay live
    fakehip::arm(19);
    RawEngine* h = nullptr;
    CHECK(!raw_create(&h));
    const size_t left = fakehip::sweep();
    printf("delete-only: %zu live after a failed create\n", left);
    CHECK(left == 0);
    return 0;
  }
  fakehip::arm(0);
  exercise();
  borrowed();
  // a failure at every creating call of the walk: it has fewer than 40
  for (long k = 1; k <= 40; k++) {
    fakehip::arm(k);
    exercise();
  }
  CHECK(fakehip::st().n_created < 40);
  // the miniature: clean, then failing at every one of its creating calls
  fakehip::arm(0);
  MiniEngine* h = nullptr;
  CHECK(mini_create(&h) && fakehip::live() == 19);
  const long n_calls = fakehip::st().n_created;
  CHECK(n_calls == 19);
  mini_destroy(h);
  CHECK(fakehip::live() == 0 && fakehip::st().n_synced >= 3);
  for (long k = 1; k <= n_calls; k++) {
    fakehip::arm(k);
    h = nullptr;
    CHECK(!mini_create(&h) && h == nullptr);
    CHECK(fakehip::st().blocks.empty() && fakehip::st().pinned.empty() && fakehip::st().streams.empty() && fakehip::st().events.empty());
  }
  printf("own_types OK\n");
  return 0;
}
