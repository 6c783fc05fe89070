// scrf_own.h -- the owning types of the engine: what the handle and a scope hold of the device is one of these, and is given
// back by its destructor.  All are move-only.  None synchronises anything before it releases a buffer: what has to finish
// before a buffer may go is the caller's decision (scrf_engine.cpp, above the handle).
// The header uses hip/hip_runtime.h alone, and of it only hipMalloc / hipFree, hipHostMalloc / hipHostFree, the event and
// stream create / destroy calls, hipMemcpyAsync and hipStreamSynchronize: tests/host/own_types.cpp compiles it on the CPU
// against a counting stand-in (tests/host/fakehip).
#pragma once
#include <hip/hip_runtime.h>

#include <stddef.h>

#include <algorithm>
#include <utility>

namespace scrf_eng {   // the one namespace of the engine's internal types

// A device array with a capacity in elements.  Borrowed (scrf_set_grad_buffer): the caller's memory, never freed here.
template <class T>
class DevArray {
  T* p_ = nullptr;
  size_t cap_ = 0;
  bool own_ = true;
 public:
  DevArray() = default;
  DevArray(DevArray&& o) noexcept : p_(o.p_), cap_(o.cap_), own_(o.own_) { o.p_ = nullptr; o.cap_ = 0; o.own_ = true; }
  DevArray& operator=(DevArray&& o) noexcept {
    if (this != &o) { reset(); p_ = o.p_; cap_ = o.cap_; own_ = o.own_; o.p_ = nullptr; o.cap_ = 0; o.own_ = true; }
    return *this;
  }
  ~DevArray() { reset(); }
  void reset() { if (own_ && p_) hipFree(p_); p_ = nullptr; cap_ = 0; own_ = true; }
  void borrow(T* p, size_t n) { reset(); p_ = p; cap_ = n; own_ = false; }
  bool owned() const { return own_; }
  // room for n elements; a larger request drops the contents.  On failure the array is empty (cap() == 0).
  hipError_t reserve(size_t n) {
    if (n <= cap_) return hipSuccess;
    reset();
    const hipError_t e = hipMalloc((void**)&p_, sizeof(T) * n);
    if (e != hipSuccess) p_ = nullptr; else cap_ = n;
    return e;
  }
  // room for n_new elements, growing to max(n_new, 2 cap, 65536); the first n_live survive, copied on `st`, which is drained
  // before the old block goes.  On failure the array is as it was.
  hipError_t reserve_keep(size_t n_new, size_t n_live, hipStream_t st) {
    if (n_new <= cap_) return hipSuccess;
    DevArray g;
    hipError_t e = g.reserve(std::max(std::max(n_new, 2 * cap_), (size_t)1 << 16));
    if (e == hipSuccess && n_live) e = hipMemcpyAsync(g.p_, p_, sizeof(T) * n_live, hipMemcpyDeviceToDevice, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e == hipSuccess) *this = std::move(g);
    return e;
  }
  operator T*() const { return p_; }
  T* get() const { return p_; }
  size_t cap() const { return cap_; }
};

// The same in pinned host memory (hipHostMalloc).
template <class T>
class PinnedArray {
  T* p_ = nullptr;
  size_t cap_ = 0;
 public:
  PinnedArray() = default;
  PinnedArray(PinnedArray&& o) noexcept : p_(o.p_), cap_(o.cap_) { o.p_ = nullptr; o.cap_ = 0; }
  PinnedArray& operator=(PinnedArray&& o) noexcept {
    if (this != &o) { reset(); p_ = o.p_; cap_ = o.cap_; o.p_ = nullptr; o.cap_ = 0; }
    return *this;
  }
  ~PinnedArray() { reset(); }
  void reset() { if (p_) hipHostFree(p_); p_ = nullptr; cap_ = 0; }
  hipError_t reserve(size_t n) {
    if (n <= cap_) return hipSuccess;
    reset();
    const hipError_t e = hipHostMalloc((void**)&p_, sizeof(T) * n, hipHostMallocDefault);
    if (e != hipSuccess) p_ = nullptr; else cap_ = n;
    return e;
  }
  operator T*() const { return p_; }
  T* get() const { return p_; }
  size_t cap() const { return cap_; }
};

class Event {
  hipEvent_t e_ = nullptr;
 public:
  Event() = default;
  Event(Event&& o) noexcept : e_(o.e_) { o.e_ = nullptr; }
  Event& operator=(Event&& o) noexcept { if (this != &o) { reset(); e_ = o.e_; o.e_ = nullptr; } return *this; }
  ~Event() { reset(); }
  void reset() { if (e_) hipEventDestroy(e_); e_ = nullptr; }
  hipError_t create() { reset(); return hipEventCreate(&e_); }                                       // a timing event
  hipError_t create(unsigned flags) { reset(); return hipEventCreateWithFlags(&e_, flags); }
  operator hipEvent_t() const { return e_; }
};

// A stream of the engine's own, or the caller's (scrf_set_stream): a borrowed stream is never destroyed here.
class Stream {
  hipStream_t s_ = nullptr;
  bool own_ = true;
 public:
  Stream() = default;
  Stream(Stream&& o) noexcept : s_(o.s_), own_(o.own_) { o.s_ = nullptr; o.own_ = true; }
  Stream& operator=(Stream&& o) noexcept {
    if (this != &o) { reset(); s_ = o.s_; own_ = o.own_; o.s_ = nullptr; o.own_ = true; }
    return *this;
  }
  ~Stream() { reset(); }
  void reset() { if (own_ && s_) hipStreamDestroy(s_); s_ = nullptr; own_ = true; }
  void borrow(hipStream_t s) { reset(); s_ = s; own_ = false; }
  hipError_t create(unsigned flags) {
    reset();
    const hipError_t e = hipStreamCreateWithFlags(&s_, flags);
    if (e != hipSuccess) s_ = nullptr;
    return e;
  }
  bool owned() const { return own_; }
  operator hipStream_t() const { return s_; }
  hipStream_t get() const { return s_; }
};

}  // namespace scrf_eng
