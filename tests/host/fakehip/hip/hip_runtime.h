// A stand-in for <hip/hip_runtime.h> on the CPU: exactly what asr-craft_amd/csrc/scrf_own.h uses of it, on top of malloc.
// It counts what is live (blocks, streams, events), refuses to release what it did not hand out, and can make the k-th
// creating call fail.  tests/host/own_types.cpp is its one user.
#pragma once
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <set>

enum hipError_t { hipSuccess = 0, hipErrorOutOfMemory = 2 };
enum hipMemcpyKind { hipMemcpyHostToDevice = 1, hipMemcpyDeviceToHost = 2, hipMemcpyDeviceToDevice = 3 };
struct fakehip_stream { int tag; };
struct fakehip_event { int tag; };
typedef fakehip_stream* hipStream_t;
typedef fakehip_event* hipEvent_t;
enum { hipHostMallocDefault = 0, hipStreamNonBlocking = 1, hipEventDisableTiming = 2 };

namespace fakehip {
struct State {
  std::set<void*> blocks, pinned, streams, events;
  long n_created = 0;   // creating calls so far (device and pinned blocks, streams, events)
  long fail_at = 0;     // the creating call of this number fails (1-based; 0: none)
  long n_copied = 0, n_synced = 0;
};
inline State& st() { static State s; return s; }
inline size_t live() { return st().blocks.size() + st().pinned.size() + st().streams.size() + st().events.size(); }
inline bool refuse() { return ++st().n_created == st().fail_at; }
inline void arm(long k) { st().n_created = 0; st().fail_at = k; }
inline void die(const char* what) { fprintf(stderr, "fakehip: %s\n", what); abort(); }
template <class Set> inline void release(Set& s, void* p, const char* what) { if (!s.erase(p)) die(what); }
// gives back what a leaking caller left behind (so that the leak can be counted without the sanitizer reporting it too)
inline size_t sweep() {
  const size_t n = live();
  for (void* p : st().blocks) free(p);
  for (void* p : st().pinned) free(p);
  for (void* p : st().streams) delete (fakehip_stream*)p;
  for (void* p : st().events) delete (fakehip_event*)p;
  st().blocks.clear(); st().pinned.clear(); st().streams.clear(); st().events.clear();
  return n;
}
}  // namespace fakehip

inline hipError_t hipMalloc(void** p, size_t bytes) {
  *p = nullptr;
  if (fakehip::refuse()) return hipErrorOutOfMemory;
  *p = malloc(bytes ? bytes : 1);
  fakehip::st().blocks.insert(*p);
  return hipSuccess;
}
inline hipError_t hipFree(void* p) {
  if (p) { fakehip::release(fakehip::st().blocks, p, "hipFree of a block that is not live"); free(p); }
  return hipSuccess;
}
inline hipError_t hipHostMalloc(void** p, size_t bytes, unsigned) {
  *p = nullptr;
  if (fakehip::refuse()) return hipErrorOutOfMemory;
  *p = malloc(bytes ? bytes : 1);
  fakehip::st().pinned.insert(*p);
  return hipSuccess;
}
inline hipError_t hipHostFree(void* p) {
  if (p) { fakehip::release(fakehip::st().pinned, p, "hipHostFree of a block that is not live"); free(p); }
  return hipSuccess;
}
inline hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned) {
  *s = nullptr;
  if (fakehip::refuse()) return hipErrorOutOfMemory;
  *s = new fakehip_stream{0};
  fakehip::st().streams.insert(*s);
  return hipSuccess;
}
inline hipError_t hipStreamDestroy(hipStream_t s) {
  fakehip::release(fakehip::st().streams, s, "hipStreamDestroy of a stream that is not live");
  delete s;
  return hipSuccess;
}
inline hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned) {
  *e = nullptr;
  if (fakehip::refuse()) return hipErrorOutOfMemory;
  *e = new fakehip_event{0};
  fakehip::st().events.insert(*e);
  return hipSuccess;
}
inline hipError_t hipEventCreate(hipEvent_t* e) { return hipEventCreateWithFlags(e, 0); }
inline hipError_t hipEventDestroy(hipEvent_t e) {
  fakehip::release(fakehip::st().events, e, "hipEventDestroy of an event that is not live");
  delete e;
  return hipSuccess;
}
inline hipError_t hipMemcpyAsync(void* dst, const void* src, size_t bytes, hipMemcpyKind, hipStream_t) {
  memcpy(dst, src, bytes);
  fakehip::st().n_copied++;
  return hipSuccess;
}
inline hipError_t hipStreamSynchronize(hipStream_t) { fakehip::st().n_synced++; return hipSuccess; }
