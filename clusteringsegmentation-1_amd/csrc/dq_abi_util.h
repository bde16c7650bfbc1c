// dq_abi_util.h -- what the files of the exported surface share (dq_abi.cpp,
// dq_abi_regions.cpp): the device and stream an entry point runs on, and the
// device memory of one call.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <initializer_list>
#include <mutex>
#include <vector>

#include "dq_engine.h"

namespace dq {

inline int current_device() {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n == 0)
    die("no HIP device", __FILE__, __LINE__, "libdivquant_hip has no CPU fallback; run on an MI355X (gfx950)");
  int d = 0;
  DQ_HIP(hipGetDevice(&d));
  return d;
}

// Events for one-shot cross-stream joins (a call's "inputs ready" mark, a
// NULL-stream call's completion), one per use: concurrent calls never share
// one (an event re-recorded by another call before a stream waited on it
// would order the wait after the wrong work).  A stream wait captures the
// event's state when it is enqueued, so the event returns to the pool as
// soon as every wait on it has been enqueued.
class EventPool {
 public:
  hipEvent_t get() {
    {
      std::lock_guard<std::mutex> g(mu_);
      if (!free_.empty()) {
        hipEvent_t e = free_.back();
        free_.pop_back();
        return e;
      }
    }
    hipEvent_t e = nullptr;
    DQ_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    return e;
  }
  void put(hipEvent_t e) {
    std::lock_guard<std::mutex> g(mu_);
    free_.push_back(e);
  }

 private:
  std::mutex mu_;
  std::vector<hipEvent_t> free_;
};

inline EventPool& events() {
  static EventPool* p = new EventPool();   // (never destroyed, like the engines)
  return *p;
}

// The stream a device-pointer entry runs on: the caller's, or (NULL) the
// engine's non-blocking stream made to wait for the legacy default stream
// first -- the caller's inputs may still be in flight there (a torch
// host-to-device copy on the default stream, say).
inline hipStream_t dev_stream(Engine& e, void* stream) {
  if (stream) return (hipStream_t)stream;
  hipEvent_t ev = events().get();
  DQ_HIP(hipEventRecord(ev, nullptr));
  DQ_HIP(hipStreamWaitEvent(e.stream(), ev, 0));
  events().put(ev);
  return e.stream();
}

inline hipStream_t engine_stream(int device, void* stream) {
  Engine& e = engine_for(device);
  DQ_HIP(hipSetDevice(device));
  return dev_stream(e, stream);
}

// An asynchronous entry called with stream NULL ran on the engine's stream:
// order the legacy default stream after it, so work the caller queues there
// next (a framework's copy of the outputs) sees the results.
inline void join_default_stream(void* stream, hipStream_t used) {
  if (stream) return;
  hipEvent_t ev = events().get();
  DQ_HIP(hipEventRecord(ev, used));
  DQ_HIP(hipStreamWaitEvent(nullptr, ev, 0));
  events().put(ev);
}

// The device memory of one call, allocated and released in stream order on the
// call's stream.  What the call still holds when it ends is released then.
class Staging {
 public:
  explicit Staging(hipStream_t st) : st_(st) {}
  Staging(const Staging&) = delete;
  Staging& operator=(const Staging&) = delete;
  ~Staging() { release(); }
  hipStream_t stream() const { return st_; }

  template <class T = void>
  T* alloc_bytes(size_t bytes) {
    void* p = nullptr;
    DQ_HIP(hipMallocAsync(&p, bytes, st_));
    held_.push_back(p);
    return static_cast<T*>(p);
  }
  template <class T>
  T* alloc(size_t count) { return alloc_bytes<T>(count * sizeof(T)); }
  // The device copy of a host input (NULL: none).
  template <class T>
  T* upload(const T* host, size_t count) {
    if (!host) return nullptr;
    T* d = alloc<T>(count);
    DQ_HIP(hipMemcpyAsync(d, host, count * sizeof(T), hipMemcpyHostToDevice, st_));
    return d;
  }
  // The device twin of an optional host output (NULL or no entry: none).
  template <class T>
  T* twin(const T* host, size_t count) { return host && count ? alloc<T>(count) : nullptr; }
  // `count` entries of a twin back to the host array, when both exist.
  template <class T>
  void download(T* host, const T* d, size_t count) {
    if (host && d && count) DQ_HIP(hipMemcpyAsync(host, d, count * sizeof(T), hipMemcpyDeviceToHost, st_));
  }
  // One allocation before the call ends (scratch a later part no longer needs); NULL: nothing.
  void release(void* p) {
    if (!p) return;
    held_.erase(std::find(held_.begin(), held_.end(), p));
    DQ_HIP(hipFreeAsync(p, st_));
  }
  void release() {
    for (void* p : held_) DQ_HIP(hipFreeAsync(p, st_));
    held_.clear();
  }
  void sync() { DQ_HIP(hipStreamSynchronize(st_)); }
  // The end of a part that returns to a caller which allocates more: all released, then the wait.
  void finish() {
    release();
    sync();
  }

  // The status of the launches so far, then `count` words of device memory on their way to the host.
  void fetch(uint32_t* to, const uint32_t* from, size_t count = 1) {
    DQ_HIP(hipGetLastError());
    DQ_HIP(hipMemcpyAsync(to, from, count * 4, hipMemcpyDeviceToHost, st_));
  }
  // A small read-back: one word, or words that lie apart (a copy each; NULL: that word stays as it
  // is), under one synchronisation.
  uint32_t read_word(const uint32_t* from) {
    uint32_t w = 0;
    read_words({from}, &w);
    return w;
  }
  void read_words(std::initializer_list<const uint32_t*> from, uint32_t* to) {
    for (const uint32_t* p : from) {
      if (p) fetch(to, p);
      ++to;
    }
    sync();
  }

 private:
  hipStream_t st_;
  std::vector<void*> held_;
};

}  // namespace dq
