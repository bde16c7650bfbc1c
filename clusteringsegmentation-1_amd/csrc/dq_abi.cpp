// dq_abi.cpp -- the exported surface of libdivquant_hip.so:
//   * the C ABI of include/dq_hip.h (device- and host-pointer entry points);
//   * the reference signatures of include/DivQuantHeader.h and
//     include/quant_util.h, implemented on top of it.
// The product path has no CPU fallback: without a HIP device every compute
// entry point aborts with a message.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <atomic>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <thread>
#include <unordered_map>
#include <vector>

#include "../../include/DivQuantHeader.h"
#include "../../include/dq_hip.h"
#include "../../include/quant_util.h"
#include "dq_engine.h"
#include "dq_adjacency.h"
#include "dq_contain.h"
#include "dq_merge.h"
#include "dq_pixels.h"
#include "dq_regions.h"
#include "dq_weighted.h"
#include "dq_windows.h"
#include "dq_wtags.h"

#include <rccl/rccl.h>
#include <map>
#include <tuple>

using dq::Engine;
using dq::engine_for;

namespace {

int current_device() {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n == 0)
    dq::die("no HIP device", __FILE__, __LINE__,
            "libdivquant_hip has no CPU fallback; run on an MI355X (gfx950)");
  int d = 0;
  DQ_HIP(hipGetDevice(&d));
  return d;
}

bool quiet() {
  const char* q = std::getenv("DQ_HIP_QUIET");
  return q && *q && *q != '0';
}

void report_empty(int num_empty) {
  if (num_empty) std::fprintf(stderr, "# empty clusters: %d\n", num_empty);   // :1067-1069
}

// Persistent host threads for the batch lanes 1..L-1 (a std::thread per lane
// per call cost tens of microseconds of every call's host time).  run()
// hands job(i) to worker i, runs job(0) on the caller and returns when all
// are done.  A worker reads the generation, the job and the lane count
// together under mu_ (run() publishes them together under mu_), so it runs
// each generation's job at most once; a thread starts with `seen` = the
// generation current when it was created.  Workers spin briefly on the
// generation word before sleeping on the condition variable.
class LaneWorkers {
 public:
  void run(int n, const std::function<void(int)>& job) {
    std::lock_guard<std::mutex> call(call_mu_);
    while ((int)threads_.size() < n - 1) {
      const int id = (int)threads_.size() + 1;
      const uint64_t g0 = gen_.load(std::memory_order_acquire);   // (no publish in flight: call_mu_)
      threads_.emplace_back([this, id, g0] { loop(id, g0); });
      threads_.back().detach();
    }
    {
      std::lock_guard<std::mutex> g(mu_);
      job_ = &job;
      nact_ = n;
      pending_.store(n - 1, std::memory_order_relaxed);
      gen_.fetch_add(1, std::memory_order_release);
    }
    cv_.notify_all();
    job(0);
    for (uint64_t spin = 0; pending_.load(std::memory_order_acquire) != 0; ++spin) {
      if (spin < (1u << 16)) {
        __builtin_ia32_pause();
      } else {
        std::unique_lock<std::mutex> g(mu_);
        done_cv_.wait(g, [this] { return pending_.load(std::memory_order_acquire) == 0; });
      }
    }
  }

 private:
  void loop(int id, uint64_t seen) {
    for (;;) {
      for (uint32_t spin = 0; gen_.load(std::memory_order_acquire) == seen && spin < (1u << 14); ++spin)
        __builtin_ia32_pause();
      const std::function<void(int)>* job;
      int n;
      {
        std::unique_lock<std::mutex> l(mu_);
        cv_.wait(l, [&] { return gen_.load(std::memory_order_relaxed) != seen; });
        seen = gen_.load(std::memory_order_relaxed);   // the generation job_ / nact_ belong to
        job = job_;
        n = nact_;
      }
      if (id < n) {
        (*job)(id);
        if (pending_.fetch_sub(1, std::memory_order_acq_rel) == 1) {
          std::lock_guard<std::mutex> l(mu_);
          done_cv_.notify_all();
        }
      }
    }
  }
  std::mutex call_mu_, mu_;
  std::condition_variable cv_, done_cv_;
  std::atomic<uint64_t> gen_{0};
  std::atomic<int> pending_{0};
  const std::function<void(int)>* job_ = nullptr;
  int nact_ = 0;
  std::vector<std::thread> threads_;
};

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

EventPool& events() {
  static EventPool* p = new EventPool();   // (never destroyed, like the engines)
  return *p;
}

// The stream a device-pointer entry runs on: the caller's, or (NULL) the
// engine's non-blocking stream made to wait for the legacy default stream
// first -- the caller's inputs may still be in flight there (a torch
// host-to-device copy on the default stream, say).
hipStream_t dev_stream(Engine& e, void* stream) {
  if (stream) return (hipStream_t)stream;
  hipEvent_t ev = events().get();
  DQ_HIP(hipEventRecord(ev, nullptr));
  DQ_HIP(hipStreamWaitEvent(e.stream(), ev, 0));
  events().put(ev);
  return e.stream();
}

// An asynchronous entry called with stream NULL ran on the engine's stream:
// order the legacy default stream after it, so work the caller queues there
// next (a framework's copy of the outputs) sees the results.
void join_default_stream(void* stream, hipStream_t used) {
  if (stream) return;
  hipEvent_t ev = events().get();
  DQ_HIP(hipEventRecord(ev, used));
  DQ_HIP(hipStreamWaitEvent(nullptr, ev, 0));
  events().put(ev);
}

LaneWorkers& lane_workers() {
  static LaneWorkers* w = new LaneWorkers();   // (never destroyed: its threads are detached)
  return *w;
}

}  // namespace

// =========================================================================
// C ABI (include/dq_hip.h)
// =========================================================================
extern "C" {

int dq_hip_abi_version(void) { return DQ_HIP_ABI_VERSION; }

int dq_hip_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int dq_hip_cluster_dev(int device, const uint32_t* d_in, uint32_t n, uint32_t* k,
                       uint32_t* ct, int max_iters, void* stream) {
  if (!d_in || !k || !ct || n == 0 || *k == 0 || max_iters < 1) return -1;
  Engine& e = engine_for(device);
  std::lock_guard<std::mutex> g(e.mutex());
  dq::FrameJob j;
  j.d_in = d_in;
  j.n = n;
  j.k = (int)*k;
  j.ct = ct;
  e.run(&j, 1, max_iters, false, dev_stream(e, stream));
  *k = (uint32_t)j.k_out;
  return j.num_empty;
}

int dq_hip_quant_weighted_dev(int device, const uint32_t* d_in, uint32_t n, uint32_t* d_out,
                              uint32_t* k, uint32_t* ct, int max_iters, void* stream) {
  if (!d_in || !k || !ct || n == 0 || *k == 0 || max_iters < 1) return -1;
  Engine& e = engine_for(device);
  std::lock_guard<std::mutex> g(e.mutex());
  dq::FrameJob j;
  j.d_in = d_in;
  j.n = n;
  j.d_out = d_out;
  j.k = (int)*k;
  j.ct = ct;
  e.run_weighted(j, max_iters, d_out != nullptr, dev_stream(e, stream));
  *k = (uint32_t)j.k_out;
  return j.num_empty;
}

// Many weighted quant_recurse calls (the app's per-superpixel-region calls,
// ClusteringSegmentation.cpp:1779-1803) in one: region i = d_ins[i][0..ns[i])
// -> d_outs[i], K = ks[i], colortable at cts + i * ct_stride, its size at
// k_outs[i].  Returns the total of empty clusters, or < 0.
int dq_hip_quant_weighted_regions_dev(int device, int nregions, const uint32_t* const* d_ins, const uint32_t* ns,
                                      uint32_t* const* d_outs, const uint32_t* ks, uint32_t* cts,
                                      uint32_t ct_stride, uint32_t* k_outs, int max_iters, void* stream) {
  if (nregions < 0 || (nregions > 0 && (!d_ins || !ns || !ks || !cts || !k_outs)) || max_iters < 1) return -1;
  std::vector<dq::FrameJob> jobs((size_t)nregions);
  for (int i = 0; i < nregions; ++i) {
    if (!d_ins[i] || ns[i] == 0 || ks[i] == 0 || ks[i] > ct_stride) return -1;
    jobs[i].d_in = d_ins[i];
    jobs[i].n = ns[i];
    jobs[i].d_out = d_outs ? d_outs[i] : nullptr;
    jobs[i].k = (int)ks[i];
    jobs[i].ct = cts + (size_t)i * ct_stride;
  }
  Engine& e = engine_for(device);
  std::lock_guard<std::mutex> g(e.mutex());
  e.run_weighted_regions(jobs.data(), nregions, max_iters, dev_stream(e, stream));
  int empty = 0;
  for (int i = 0; i < nregions; ++i) {
    k_outs[i] = (uint32_t)jobs[i].k_out;
    empty += jobs[i].num_empty;
  }
  return empty;
}

static hipStream_t engine_stream(int device, void* stream);

int dq_hip_varpart_dev(int device, const uint32_t* d_in, uint32_t n, uint32_t rows, uint32_t cols,
                       uint32_t* k, uint32_t* ct, int num_bits, int dec_factor, int max_iters,
                       int uniq, void* stream) {
  if (!d_in || !k || !ct || n == 0 || *k == 0 || max_iters < 1 || num_bits < 1 || num_bits > 8 ||
      dec_factor < 1 || rows == 0 || cols == 0)
    return -1;
  // the reference's index ic + ir*numRows must stay inside the input (:124)
  const uint64_t nr = (rows + (uint64_t)dec_factor - 1) / dec_factor;
  const uint64_t nc = (cols + (uint64_t)dec_factor - 1) / dec_factor;
  if ((nc - 1) * dec_factor + (nr - 1) * dec_factor * (uint64_t)rows >= n) return -2;
  Engine& e = engine_for(device);
  std::lock_guard<std::mutex> g(e.mutex());
  dq::FrameJob j;
  j.d_in = d_in;
  j.n = n;
  j.k = (int)*k;
  j.ct = ct;
  j.num_bits = num_bits;
  j.dec = dec_factor;
  j.rows = rows;
  j.cols = cols;
  if (uniq && num_bits == 8 && dec_factor == 1) e.run(&j, 1, max_iters, false, dev_stream(e, stream));
  else e.run_weighted(j, max_iters, false, dev_stream(e, stream));
  *k = (uint32_t)j.k_out;
  return j.num_empty;
}

int dq_hip_cut_bits_dev(int device, const uint32_t* d_in, uint32_t n, uint32_t* d_out, int nbr,
                        int nbg, int nbb, void* stream) {
  if (!d_in || !d_out || nbr < 1 || nbr > 8 || nbg < 1 || nbg > 8 || nbb < 1 || nbb > 8) return -1;
  if (n == 0) return 0;
  hipStream_t st = engine_stream(device, stream);
  dq::launch_cut_gather(d_in, d_out, 1, n, 1, 1, (uint32_t)(8 - nbr), (uint32_t)(8 - nbg),
                        (uint32_t)(8 - nbb), st);
  join_default_stream(stream, st);
  return 0;
}

int dq_hip_map_dev(int device, const uint32_t* d_in, uint32_t n, uint32_t* d_out,
                   const uint32_t* ct, int k, void* stream) {
  if (!d_in || !d_out || !ct || k <= 0) return -1;
  if (n == 0) return 0;
  Engine& e = engine_for(device);
  std::lock_guard<std::mutex> g(e.mutex());
  e.map(d_in, n, d_out, ct, k, dev_stream(e, stream));
  return 0;
}

static bool block_hist_shape_ok(uint32_t w, uint32_t h, uint32_t dim, uint32_t bw, uint32_t bh) {
  // every block must hold a pixel (the reference asserts it, :468)
  return w > 0 && h > 0 && dim >= 1 && dim <= 4 && bw > 0 && bh > 0 &&
         (uint64_t)(bw - 1) * dim < w && (uint64_t)(bh - 1) * dim < h &&
         (uint64_t)w * h <= 0xFFFFFFFFull && (uint64_t)bw * bh < 0xFFFFFF00ull;
}

int dq_hip_block_hist_dev(int device, const uint32_t* d_in, uint32_t width, uint32_t height,
                          const uint32_t* palette, int npal, uint32_t dim, uint32_t block_w,
                          uint32_t block_h, uint32_t* d_quant, uint32_t* d_mode,
                          uint32_t* d_ndistinct, uint32_t* d_keys, uint32_t* d_counts,
                          void* stream) {
  if (!d_in || !palette || npal <= 0 || !d_quant || !d_mode || (!d_keys) != (!d_counts) ||
      !block_hist_shape_ok(width, height, dim, block_w, block_h))
    return -1;
  Engine& e = engine_for(device);
  std::lock_guard<std::mutex> g(e.mutex());
  hipStream_t st = dev_stream(e, stream);
  e.map(d_in, width * height, d_quant, palette, npal, st);
  // the tie queues are private to this call (stream-ordered allocation): the
  // kernels are still running when the call returns, and another call may
  // run on another stream meanwhile
  uint32_t* work = nullptr;
  DQ_HIP(hipMallocAsync((void**)&work, dq::block_hist_scratch_words(block_w, block_h) * 4, st));
  dq::BlockHistArgs a{d_quant, width, height, block_w, block_h, d_mode, d_ndistinct, d_keys, d_counts,
                      work, nullptr, 0};
  const int rc = dq::launch_block_hist(a, (int)dim, st);
  DQ_HIP(hipFreeAsync(work, st));
  join_default_stream(stream, st);
  return rc;
}

static bool bgr24_shape_ok(uint32_t width, uint32_t height, uint32_t stride) {
  return width > 0 && height > 0 && width <= 0xFFFFFFFFu / 3u && stride >= 3u * width &&
         (uint64_t)width * height <= 0xFFFFFFFFull;
}

static hipStream_t engine_stream(int device, void* stream) {
  Engine& e = engine_for(device);
  DQ_HIP(hipSetDevice(device));
  return dev_stream(e, stream);
}

int dq_hip_pack_bgr24_dev(int device, const uint8_t* d_bgr, uint32_t width, uint32_t height,
                          uint32_t stride, uint32_t* d_out, void* stream) {
  if (!d_bgr || !d_out || !bgr24_shape_ok(width, height, stride)) return -1;
  hipStream_t st = engine_stream(device, stream);
  dq::launch_bgr24_pack(d_bgr, width, height, stride, d_out, st);
  join_default_stream(stream, st);
  DQ_HIP(hipGetLastError());
  return 0;
}

int dq_hip_unpack_bgr24_dev(int device, const uint32_t* d_in, uint32_t width, uint32_t height,
                            uint32_t stride, uint8_t* d_bgr, void* stream) {
  if (!d_in || !d_bgr || !bgr24_shape_ok(width, height, stride)) return -1;
  hipStream_t st = engine_stream(device, stream);
  dq::launch_bgr24_unpack(d_in, width, height, stride, d_bgr, st);
  join_default_stream(stream, st);
  DQ_HIP(hipGetLastError());
  return 0;
}

int dq_hip_gather_bgr24_dev(int device, const uint8_t* d_bgr, uint32_t stride,
                            const uint32_t* d_coords, uint32_t n, uint32_t* d_out, void* stream) {
  if (!d_bgr || !d_coords || !d_out || stride < 3u) return -1;
  if (n == 0) return 0;
  hipStream_t st = engine_stream(device, stream);
  dq::launch_bgr24_gather(d_bgr, stride, d_coords, n, d_out, st);
  join_default_stream(stream, st);
  DQ_HIP(hipGetLastError());
  return 0;
}

// The uniform-weight batch over the engine lanes (frames split over the
// lanes' engines and streams).
static int quant_batch(int device, std::vector<dq::FrameJob>& jobs, int max_iters, void* stream) {
  const int nframes = (int)jobs.size();
  const int lanes = std::min(nframes, dq::batch_lanes());
  Engine& e0 = engine_for(device);
  if (lanes <= 1) {
    std::lock_guard<std::mutex> g(e0.mutex());
    e0.run(jobs.data(), nframes, max_iters, true, dev_stream(e0, stream));
  } else {
    // frames [f0(l), f0(l+1)) on lane l; every lane first waits for the
    // caller's stream (the frames may have been produced there)
    DQ_HIP(hipSetDevice(device));
    hipEvent_t ready = events().get();   // this call's own (concurrent calls: one each)
    DQ_HIP(hipEventRecord(ready, (hipStream_t)stream));
    for (int l = 1; l < lanes; ++l) {   // lanes inherit lane 0's switches
      Engine& e = engine_for(device, l);
      e.set_fixed_point(e0.fixed_point());
      e.set_plan(e0.plan());
      e.set_timing(e0.timing());
    }
    const std::function<void(int)> work = [&](int l) {
      const int f0 = nframes * l / lanes, f1 = nframes * (l + 1) / lanes;
      Engine& e = engine_for(device, l);
      DQ_HIP(hipSetDevice(device));
      std::lock_guard<std::mutex> g(e.mutex());
      DQ_HIP(hipStreamWaitEvent(e.stream(), ready, 0));
      e.run(jobs.data() + f0, f1 - f0, max_iters, true, e.stream());
    };
    lane_workers().run(lanes, work);
    events().put(ready);   // (every lane's wait on it is enqueued)
    // lane 0 reports for the batch: the last frame's diagnostics, summed counters
    Engine& el = engine_for(device, lanes - 1);
    std::lock_guard<std::mutex> g(e0.mutex());
    uint64_t swept = 0, full = 0, fixes = 0;
    int rounds = 0;
    for (int l = 0; l < lanes; ++l) {
      Engine& e = engine_for(device, l);
      swept += e.last_points_swept;
      full += e.last_points_full;
      fixes += e.last_cursor_fixes;
      rounds = std::max(rounds, e.last_rounds);
      if (l > 0) e0.absorb_stats(e);
    }
    e0.last_means = el.last_means;
    e0.last_sizes = el.last_sizes;
    e0.last_trace = el.last_trace;
    e0.last_rounds = rounds;
    e0.last_points_swept = swept;
    e0.last_points_full = full;
    e0.last_cursor_fixes = fixes;
  }
  int empty = 0;
  for (int i = 0; i < nframes; ++i) empty += jobs[i].num_empty;
  return empty;
}

int dq_hip_quant_batch_dev(int device, int nframes, const uint32_t* const* d_in,
                           const uint32_t* n, uint32_t* const* d_out, uint32_t k,
                           uint32_t* ct, uint32_t* k_out, int max_iters, void* stream) {
  if (nframes <= 0 || !d_in || !n || !d_out || !ct || !k_out || k == 0 || max_iters < 1)
    return -1;
  for (int i = 0; i < nframes; ++i)
    if (!d_in[i] || !d_out[i] || n[i] == 0) return -1;
  std::vector<dq::FrameJob> jobs(nframes);
  for (int i = 0; i < nframes; ++i) {
    jobs[i].d_in = d_in[i];
    jobs[i].n = n[i];
    jobs[i].d_out = d_out[i];
    jobs[i].k = (int)k;
    jobs[i].ct = ct + (size_t)i * k;
  }
  const int empty = quant_batch(device, jobs, max_iters, stream);
  for (int i = 0; i < nframes; ++i) k_out[i] = (uint32_t)jobs[i].k_out;
  return empty;
}

int dq_hip_quant_bgr24_batch_dev(int device, int nframes, const uint8_t* const* d_bgr, uint32_t width,
                                 uint32_t height, uint32_t stride, uint32_t* const* d_out, uint32_t k,
                                 uint32_t* ct, uint32_t* k_out, int uniq, int max_iters, void* stream) {
  if (nframes <= 0 || !d_bgr || !d_out || !ct || !k_out || k == 0 || max_iters < 1 ||
      !bgr24_shape_ok(width, height, stride))
    return -1;
  for (int i = 0; i < nframes; ++i)
    if (!d_bgr[i] || !d_out[i]) return -1;
  const uint32_t n = width * height;
  if (!uniq || stride != 3 * width) {
    // the weighted path's colour table (and padded rows) take packed pixels:
    // Vec3BToUID on the GPU into a scratch frame, then the packed entries
    int empty = 0;
    for (int i = 0; i < nframes; ++i) {
      uint32_t* px = nullptr;
      hipStream_t st = engine_stream(device, stream);
      DQ_HIP(hipMallocAsync((void**)&px, (size_t)n * 4 + 16, st));
      dq::launch_bgr24_pack(d_bgr[i], width, height, stride, px, st);
      uint32_t kk = k;
      int r;
      if (uniq) {
        const uint32_t* pin = px;
        r = dq_hip_quant_batch_dev(device, 1, &pin, &n, &d_out[i], k, ct + (size_t)i * k, &kk, max_iters, stream);
      } else {
        r = dq_hip_quant_weighted_dev(device, px, n, d_out[i], &kk, ct + (size_t)i * k, max_iters, stream);
      }
      DQ_HIP(hipFreeAsync(px, st));
      if (r < 0) return r;
      k_out[i] = kk;
      empty += r;
    }
    return empty;
  }
  std::vector<dq::FrameJob> jobs(nframes);
  for (int i = 0; i < nframes; ++i) {
    jobs[i].d_in = reinterpret_cast<const uint32_t*>(d_bgr[i]);
    jobs[i].bgr = true;
    jobs[i].n = n;
    jobs[i].d_out = d_out[i];
    jobs[i].k = (int)k;
    jobs[i].ct = ct + (size_t)i * k;
  }
  const int empty = quant_batch(device, jobs, max_iters, stream);
  for (int i = 0; i < nframes; ++i) k_out[i] = (uint32_t)jobs[i].k_out;
  return empty;
}

int dq_hip_quant_bgr24_dev(int device, const uint8_t* d_bgr, uint32_t width, uint32_t height,
                           uint32_t stride, uint32_t* d_out, uint32_t* k, uint32_t* ct, int uniq,
                           int max_iters, void* stream) {
  if (!k || *k == 0) return -1;
  uint32_t kk = 0;
  const int r = dq_hip_quant_bgr24_batch_dev(device, 1, &d_bgr, width, height, stride, &d_out, *k, ct, &kk,
                                             uniq, max_iters, stream);
  if (r >= 0) *k = kk;
  return r;
}

int dq_hip_map_bgr24_dev(int device, const uint8_t* d_bgr, uint32_t width, uint32_t height,
                         uint32_t stride, uint32_t* d_out, const uint32_t* ct, int k, void* stream) {
  if (!d_bgr || !d_out || !ct || k <= 0 || !bgr24_shape_ok(width, height, stride)) return -1;
  Engine& e = engine_for(device);
  std::lock_guard<std::mutex> g(e.mutex());
  hipStream_t st = dev_stream(e, stream);
  if (stride != 3 * width) {   // padded rows: packed first
    uint32_t* px = nullptr;
    const uint32_t n = width * height;
    DQ_HIP(hipMallocAsync((void**)&px, (size_t)n * 4 + 16, st));
    dq::launch_bgr24_pack(d_bgr, width, height, stride, px, st);
    e.map(px, n, d_out, ct, k, st);
    DQ_HIP(hipFreeAsync(px, st));
    return 0;
  }
  Engine::MapJob j{reinterpret_cast<const uint32_t*>(d_bgr), width * height, d_out, ct, k, true};
  e.map_many(&j, 1, st);
  return 0;
}

int dq_hip_quant_rows_dev(int device, int nframes, const uint32_t* const* d_in,
                          const uint32_t* n, const uint32_t* width, const uint64_t* n_global,
                          int nshard, uint32_t* const* d_out, uint32_t k, uint32_t* ct,
                          uint32_t* k_out, int max_iters, void* stream) {
  if (nframes <= 0 || !d_in || !n || !ct || !k_out || k == 0 || max_iters < 1) return -1;
  if (nshard < 1 || nshard > dq::kMaxShard) return -1;
  Engine& e = engine_for(device);
  for (int i = 0; i < nframes; ++i) {
    if (!d_in[i] || n[i] == 0) return -1;
    const uint64_t ng = n_global ? n_global[i] : 0;
    if (ng != 0 && ng < n[i]) return -1;
    if (ng > n[i] && e.comm_ranks() < 2) return -2;   // other rows live in other processes
  }
  std::lock_guard<std::mutex> g(e.mutex());
  std::vector<dq::FrameJob> jobs(nframes);
  for (int i = 0; i < nframes; ++i) {
    jobs[i].d_in = d_in[i];
    jobs[i].n = n[i];
    jobs[i].d_out = d_out ? d_out[i] : nullptr;
    jobs[i].k = (int)k;
    jobs[i].ct = ct + (size_t)i * k;
    jobs[i].nshard = nshard;
    jobs[i].width = width ? width[i] : 0;
    jobs[i].n_global = n_global ? n_global[i] : 0;
  }
  e.run(jobs.data(), nframes, max_iters, true, dev_stream(e, stream));
  int empty = 0;
  for (int i = 0; i < nframes; ++i) {
    k_out[i] = (uint32_t)jobs[i].k_out;
    empty += jobs[i].num_empty;
  }
  return empty;
}

// Test-only (dq_hip.h): row-tile sharding over nranks in-process ranks of
// one device, joined by the loopback collective (dq_engine.h Loopback).
// Rank r holds rows [r*H/N, (r+1)*H/N) of every frame (bench.py row_range),
// runs them on its own engine, stream and host thread with n_global = W*H,
// and maps them into its rows of d_out.
int dq_hip_loopback_rows_dev(int device, int nranks, int nframes, const uint32_t* const* d_in,
                             uint32_t width, uint32_t height, uint32_t* const* d_out, uint32_t k,
                             uint32_t* ct, uint32_t* k_out, int max_iters, uint64_t* coll_log,
                             int log_cap, int* log_len) {
  if (nranks < 1 || nranks > dq::kMaxShard || nframes <= 0 || !d_in || !d_out || !ct || !k_out || k == 0 ||
      max_iters < 1 || width == 0 || height < (uint32_t)nranks || (uint64_t)width * height >= (1ull << 32))
    return -1;
  for (int i = 0; i < nframes; ++i)
    if (!d_in[i] || !d_out[i]) return -1;
  // (rank engines are shared by every rank count: rank r of any group reuses
  // the same engine -- kMaxShard per device at most, not one per (N, r))
  static std::mutex mu;
  static std::map<std::pair<int, int>, Engine*> engines;
  static std::map<std::pair<int, int>, dq::Loopback*> groups;
  std::lock_guard<std::mutex> call(mu);
  DQ_HIP(hipSetDevice(device));
  dq::Loopback*& grp = groups[{device, nranks}];
  if (!grp) grp = new dq::Loopback(nranks, device);
  grp->reset_log();
  std::vector<Engine*> es(nranks);
  for (int r = 0; r < nranks; ++r) {
    Engine*& e = engines[std::make_pair(device, r)];
    if (!e) e = new Engine(device);
    es[r] = e;
  }
  // inputs may still be in flight on the legacy default stream
  hipEvent_t ready = events().get();
  DQ_HIP(hipEventRecord(ready, nullptr));
  for (Engine* e : es) DQ_HIP(hipStreamWaitEvent(e->stream(), ready, 0));
  events().put(ready);
  const uint64_t ng = (uint64_t)width * height;
  std::vector<int> empty(nranks, 0);
  auto work = [&](int r) {
    Engine& e = *es[r];
    DQ_HIP(hipSetDevice(device));
    std::lock_guard<std::mutex> g(e.mutex());
    const uint32_t r0 = (uint32_t)((uint64_t)height * r / nranks), r1 = (uint32_t)((uint64_t)height * (r + 1) / nranks);
    std::vector<dq::FrameJob> jobs(nframes);
    for (int i = 0; i < nframes; ++i) {
      jobs[i].d_in = d_in[i] + (size_t)r0 * width;
      jobs[i].n = (r1 - r0) * width;
      jobs[i].d_out = d_out[i] + (size_t)r0 * width;
      jobs[i].k = (int)k;
      jobs[i].ct = ct + ((size_t)r * nframes + i) * k;
      jobs[i].width = width;
      jobs[i].n_global = ng;
    }
    e.set_loopback(grp, r);
    e.run(jobs.data(), nframes, max_iters, true, e.stream());
    e.set_loopback(nullptr, 0);
    for (int i = 0; i < nframes; ++i) {
      k_out[(size_t)r * nframes + i] = (uint32_t)jobs[i].k_out;
      empty[r] += jobs[i].num_empty;
    }
  };
  std::vector<std::thread> th;
  for (int r = 1; r < nranks; ++r) th.emplace_back(work, r);
  work(0);
  for (auto& t : th) t.join();
  for (int r = 0; r < nranks; ++r) {
    if (log_len) log_len[r] = (int)grp->log[r].size();
    if (coll_log)
      for (int c = 0; c < log_cap && c < (int)grp->log[r].size(); ++c) coll_log[(size_t)r * log_cap + c] = grp->log[r][c];
  }
  {   // rank 0's diagnostics of its last frame on the device's lane-0 engine (dq_hip_last_*)
    Engine& e0 = engine_for(device);
    std::lock_guard<std::mutex> g(e0.mutex());
    e0.last_means = es[0]->last_means;
    e0.last_sizes = es[0]->last_sizes;
    e0.last_trace = es[0]->last_trace;
    e0.last_rounds = es[0]->last_rounds;
  }
  return empty[0];
}

int dq_hip_comm_unique_id(void* id128) {
  if (!id128) return -1;
  Engine::comm_unique_id(static_cast<char*>(id128));
  return 0;
}

int dq_hip_comm_init(int device, int nranks, int rank, const void* id128) {
  if (!id128 || nranks < 1 || rank < 0 || rank >= nranks) return -1;
  Engine& e = engine_for(device);
  std::lock_guard<std::mutex> g(e.mutex());
  e.comm_init(nranks, rank, static_cast<const char*>(id128));
  return 0;
}

int dq_hip_comm_size(int device) { return engine_for(device).comm_ranks(); }

int dq_hip_comm_destroy(int device) {
  Engine& e = engine_for(device);
  std::lock_guard<std::mutex> g(e.mutex());
  e.comm_destroy();
  return 0;
}

int dq_hip_quant_dev(int device, const uint32_t* d_in, uint32_t n, uint32_t* d_out,
                     uint32_t* k, uint32_t* ct, int max_iters, void* stream) {
  if (!d_in || !d_out || !k || !ct || n == 0 || *k == 0 || max_iters < 1) return -1;
  uint32_t kk = 0;
  const int r = dq_hip_quant_batch_dev(device, 1, &d_in, &n, &d_out, *k, ct, &kk, max_iters, stream);
  if (r >= 0) *k = kk;
  return r;
}

// dq_hip_quant over ngpus devices of this process: the frame's pixels split
// into ngpus row ranges (4-point multiples), one per device, every pass's node
// totals allreduced over an in-process RCCL communicator set
// (ncclCommInitAll, created once per device count); each device maps its own
// range.  Uniform-weight path only (the weighted path's folds are sequential).
static int quant_multi_gpu(const uint32_t* in, uint32_t n, uint32_t* out, uint32_t* k, uint32_t* ct,
                           int G) {
  static std::mutex mu;
  static std::map<int, std::vector<ncclComm_t>> sets;
  std::vector<ncclComm_t>* comms;
  {
    std::lock_guard<std::mutex> g(mu);
    auto it = sets.find(G);
    if (it == sets.end()) {
      std::vector<ncclComm_t> c(G);
      std::vector<int> devs(G);
      for (int d = 0; d < G; ++d) devs[d] = d;
      const ncclResult_t r = ncclCommInitAll(c.data(), G, devs.data());
      if (r != ncclSuccess) dq::die("ncclCommInitAll", __FILE__, __LINE__, ncclGetErrorString(r));
      it = sets.emplace(G, std::move(c)).first;
    }
    comms = &it->second;
  }
  std::vector<uint32_t> first(G + 1);
  for (int g = 0; g <= G; ++g) first[g] = g == G ? n : (uint32_t)(((uint64_t)n * g / G) & ~(uint64_t)3);
  std::vector<std::vector<uint32_t>> cts(G, std::vector<uint32_t>(*k));
  std::vector<int> kout(G, 0), empty(G, 0);
  auto work = [&](int g) {
    Engine& e = engine_for(g);
    std::lock_guard<std::mutex> lk(e.mutex());
    DQ_HIP(hipSetDevice(g));
    hipStream_t st = e.stream();
    const uint32_t len = first[g + 1] - first[g];
    const Engine::CommState prev = e.swap_comm({(*comms)[g], G, g});
    dq::FrameJob j;
    if (len > 0) {
      e.stage_in(in + first[g], len, st);
      j.d_in = e.staged_in();
      j.d_out = e.staged_out();
    } else {   // (n < 4 G: an empty range still takes part in every allreduce)
      e.stage_in(in, 1, st);
      j.d_in = e.staged_in();
    }
    j.n = len > 0 ? len : 1;
    j.n_global = n;
    j.k = (int)*k;
    j.ct = cts[g].data();
    e.run(&j, 1, 10, true, st);
    if (len > 0)
      DQ_HIP(hipMemcpyAsync(out + first[g], e.staged_out(), (size_t)len * 4, hipMemcpyDeviceToHost, st));
    DQ_HIP(hipStreamSynchronize(st));
    e.swap_comm(prev);
    kout[g] = j.k_out;
    empty[g] = j.num_empty;
  };
  std::vector<std::thread> th;
  for (int g = 1; g < G; ++g) th.emplace_back(work, g);
  work(0);
  for (auto& t : th) t.join();
  for (int g = 1; g < G; ++g)   // every device ran the identical FP64 updates on identical totals
    if (kout[g] != kout[0] || cts[g] != cts[0]) dq::die("dq_hip_quant", __FILE__, __LINE__, "devices disagree");
  std::memcpy(ct, cts[0].data(), (size_t)kout[0] * 4);
  *k = (uint32_t)kout[0];
  return empty[0];
}

int dq_hip_quant(const uint32_t* in, uint32_t n, uint32_t* out, uint32_t* k,
                 uint32_t* ct, int uniq, int ngpus) {
  if (!in || !out || !k || !ct || n == 0 || *k == 0) return -1;
  const int G = std::min(std::max(ngpus, 1), dq_hip_device_count());
  // (DQ_HIP_MULTI_1=1: the in-process communicator path even on one device -- tests)
  const char* m1 = std::getenv("DQ_HIP_MULTI_1");
  const bool force = m1 && m1[0] == '1' && ngpus >= 1;
  if ((G > 1 || force) && uniq && n >= 4u * (uint32_t)G) return quant_multi_gpu(in, n, out, k, ct, G);
  Engine& e = engine_for(current_device());
  std::lock_guard<std::mutex> g(e.mutex());
  hipStream_t st = e.stream();
  e.stage_in(in, n, st);
  dq::FrameJob j;
  j.d_in = e.staged_in();
  j.n = n;
  j.d_out = e.staged_out();
  j.k = (int)*k;
  j.ct = ct;
  if (uniq) e.run(&j, 1, 10, true, st);
  else e.run_weighted(j, 10, true, st);
  DQ_HIP(hipMemcpyAsync(out, e.staged_out(), (size_t)n * 4, hipMemcpyDeviceToHost, st));
  DQ_HIP(hipStreamSynchronize(st));
  *k = (uint32_t)j.k_out;
  return j.num_empty;
}

int dq_hip_map(const uint32_t* in, uint32_t n, uint32_t* out, const uint32_t* ct, int k) {
  if (!in || !out || !ct || k <= 0) return -1;
  if (n == 0) return 0;
  Engine& e = engine_for(current_device());
  std::lock_guard<std::mutex> g(e.mutex());
  hipStream_t st = e.stream();
  e.stage_in(in, n, st);
  e.map(e.staged_in(), n, e.staged_out(), ct, k, st);
  DQ_HIP(hipMemcpyAsync(out, e.staged_out(), (size_t)n * 4, hipMemcpyDeviceToHost, st));
  DQ_HIP(hipStreamSynchronize(st));
  return 0;
}

// Cluster labels (u8 / u16 / u32 label maps).  A width that cannot hold index
// k - 1 is a bad argument: checked, like everything else, before any HIP call.
static bool label_width_ok(int label_bytes, uint64_t k) {
  if (label_bytes != 1 && label_bytes != 2 && label_bytes != 4) return false;
  return k >= 1 && k - 1 <= (label_bytes == 4 ? 0xFFFFFFFFull : (1ull << (8 * label_bytes)) - 1);
}

int dq_hip_map_labels_dev(int device, const uint32_t* d_in, uint32_t n, void* d_labels,
                          int label_bytes, const uint32_t* ct, int k, void* stream) {
  if (!d_in || !d_labels || !ct || k <= 0 || !label_width_ok(label_bytes, (uint64_t)k)) return -1;
  if (((uintptr_t)d_labels & (uintptr_t)(label_bytes - 1)) != 0) return -1;
  if (n == 0) return 0;
  Engine& e = engine_for(device);
  std::lock_guard<std::mutex> g(e.mutex());
  e.map_labels(d_in, n, d_labels, label_bytes, ct, k, dev_stream(e, stream));
  return 0;
}

int dq_hip_quant_labels_batch_dev(int device, int nframes, const uint32_t* const* d_in,
                                  const uint32_t* n, void* const* d_labels, int label_bytes,
                                  uint32_t k, uint32_t* ct, uint32_t* k_out, int uniq,
                                  int max_iters, void* stream) {
  if (nframes <= 0 || !d_in || !n || !d_labels || !ct || !k_out || k == 0 || max_iters < 1 ||
      !label_width_ok(label_bytes, k))
    return -1;
  for (int i = 0; i < nframes; ++i)
    if (!d_in[i] || !d_labels[i] || n[i] == 0 || ((uintptr_t)d_labels[i] & (uintptr_t)(label_bytes - 1)) != 0)
      return -1;
  std::vector<dq::FrameJob> jobs(nframes);
  for (int i = 0; i < nframes; ++i) {
    jobs[i].d_in = d_in[i];
    jobs[i].n = n[i];
    jobs[i].d_labels = d_labels[i];
    jobs[i].label_bytes = label_bytes;
    jobs[i].k = (int)k;
    jobs[i].ct = ct + (size_t)i * k;
  }
  int empty = 0;
  if (uniq) {
    empty = quant_batch(device, jobs, max_iters, stream);
  } else {   // the weighted path, one frame after the other (as dq_hip_quant_weighted_dev)
    Engine& e = engine_for(device);
    std::lock_guard<std::mutex> g(e.mutex());
    for (int i = 0; i < nframes; ++i) {
      e.run_weighted(jobs[i], max_iters, true, dev_stream(e, stream));
      empty += jobs[i].num_empty;
    }
  }
  for (int i = 0; i < nframes; ++i) k_out[i] = (uint32_t)jobs[i].k_out;
  return empty;
}

int dq_hip_quant_labels(const uint32_t* in, uint32_t n, void* labels, int label_bytes,
                        uint32_t* k, uint32_t* ct, int uniq) {
  if (!in || !labels || !k || !ct || n == 0 || *k == 0 || !label_width_ok(label_bytes, *k)) return -1;
  Engine& e = engine_for(current_device());
  std::lock_guard<std::mutex> g(e.mutex());
  hipStream_t st = e.stream();
  e.stage_in(in, n, st);
  dq::FrameJob j;
  j.d_in = e.staged_in();
  j.n = n;
  j.d_labels = e.staged_out();   // (n words: room for n labels of any width)
  j.label_bytes = label_bytes;
  j.k = (int)*k;
  j.ct = ct;
  if (uniq) e.run(&j, 1, 10, true, st);
  else e.run_weighted(j, 10, true, st);
  DQ_HIP(hipMemcpyAsync(labels, e.staged_out(), (size_t)n * (size_t)label_bytes, hipMemcpyDeviceToHost, st));
  DQ_HIP(hipStreamSynchronize(st));
  *k = (uint32_t)j.k_out;
  return j.num_empty;
}

// Connected regions of a label map (dq_regions.hip).  Every argument check
// comes before the first HIP call.
static bool regions_args_ok(const void* labels, int label_bytes, uint32_t width, uint32_t height,
                            int connectivity, const uint32_t* regions, uint32_t stats_cap,
                            const uint32_t* area, const uint32_t* bbox, const uint32_t* first,
                            const uint32_t* label, const uint32_t* pixels, const uint64_t* sums) {
  if (label_bytes != 1 && label_bytes != 2 && label_bytes != 4) return false;
  if (connectivity != 4 && connectivity != 8) return false;
  if (width == 0 || height == 0 || width > 65535u || height > 65535u ||
      (uint64_t)width * height > 0x7FFFFFFFull)
    return false;
  if (!labels || !regions) return false;
  if (((uintptr_t)labels & (uintptr_t)(label_bytes - 1)) != 0) return false;
  for (const void* p : {(const void*)regions, (const void*)area, (const void*)bbox, (const void*)first,
                        (const void*)label, (const void*)pixels})
    if (((uintptr_t)p & 3u) != 0) return false;
  if (((uintptr_t)sums & 7u) != 0) return false;
  if (sums && !pixels) return false;
  if (stats_cap > 0 && !area && !bbox && !first && !label && !sums) return false;
  return true;
}

// Enqueues the passes on st with scratch owned by the call, waits, returns R.
static int64_t label_regions_on(hipStream_t st, const void* d_labels, int label_bytes, uint32_t width,
                                uint32_t height, int connectivity, uint32_t* d_regions, uint32_t stats_cap,
                                uint32_t* d_area, uint32_t* d_bbox, uint32_t* d_first, uint32_t* d_label,
                                const uint32_t* d_pixels, uint64_t* d_sums) {
  uint32_t* scratch = nullptr;
  DQ_HIP(hipMallocAsync((void**)&scratch, dq::region_scratch_words(width, height) * 4, st));
  dq::RegionArgs a{d_labels, label_bytes, width,   height,   connectivity, d_regions, stats_cap,
                   d_area,   d_bbox,      d_first, d_label, d_pixels,     (unsigned long long*)d_sums, scratch};
  dq::launch_label_regions(a, st);
  DQ_HIP(hipGetLastError());
  uint32_t count = 0;
  DQ_HIP(hipMemcpyAsync(&count, dq::region_count_word(a), 4, hipMemcpyDeviceToHost, st));
  DQ_HIP(hipFreeAsync(scratch, st));
  DQ_HIP(hipStreamSynchronize(st));
  return (int64_t)count;
}

int64_t dq_hip_label_regions_dev(int device, const void* d_labels, int label_bytes, uint32_t width,
                                 uint32_t height, int connectivity, uint32_t* d_regions, uint32_t stats_cap,
                                 uint32_t* d_area, uint32_t* d_bbox, uint32_t* d_first, uint32_t* d_label,
                                 const uint32_t* d_pixels, uint64_t* d_sums, void* stream) {
  if (!regions_args_ok(d_labels, label_bytes, width, height, connectivity, d_regions, stats_cap, d_area,
                       d_bbox, d_first, d_label, d_pixels, d_sums))
    return -1;
  // (no engine state is touched: calls on two streams may overlap)
  hipStream_t st = engine_stream(device, stream);
  return label_regions_on(st, d_labels, label_bytes, width, height, connectivity, d_regions, stats_cap, d_area,
                          d_bbox, d_first, d_label, d_pixels, d_sums);
}

int64_t dq_hip_label_regions(const void* labels, int label_bytes, uint32_t width, uint32_t height,
                             int connectivity, uint32_t* regions, uint32_t stats_cap, uint32_t* area,
                             uint32_t* bbox, uint32_t* first, uint32_t* label, const uint32_t* pixels,
                             uint64_t* sums) {
  if (!regions_args_ok(labels, label_bytes, width, height, connectivity, regions, stats_cap, area, bbox, first,
                       label, pixels, sums))
    return -1;
  Engine& e = engine_for(current_device());
  hipStream_t st = e.stream();
  const size_t n = (size_t)width * height, cap = stats_cap;
  void* d_labels = nullptr;
  uint32_t *d_regions = nullptr, *d_area = nullptr, *d_bbox = nullptr, *d_first = nullptr, *d_label = nullptr,
           *d_pixels = nullptr;
  uint64_t* d_sums = nullptr;
  DQ_HIP(hipMallocAsync(&d_labels, n * (size_t)label_bytes, st));
  DQ_HIP(hipMallocAsync((void**)&d_regions, n * 4, st));
  if (cap && area) DQ_HIP(hipMallocAsync((void**)&d_area, cap * 4, st));
  if (cap && bbox) DQ_HIP(hipMallocAsync((void**)&d_bbox, cap * 16, st));
  if (cap && first) DQ_HIP(hipMallocAsync((void**)&d_first, cap * 4, st));
  if (cap && label) DQ_HIP(hipMallocAsync((void**)&d_label, cap * 4, st));
  if (cap && sums) DQ_HIP(hipMallocAsync((void**)&d_sums, cap * 24, st));
  if (cap && sums) {
    DQ_HIP(hipMallocAsync((void**)&d_pixels, n * 4, st));
    DQ_HIP(hipMemcpyAsync(d_pixels, pixels, n * 4, hipMemcpyHostToDevice, st));
  }
  DQ_HIP(hipMemcpyAsync(d_labels, labels, n * (size_t)label_bytes, hipMemcpyHostToDevice, st));
  const int64_t count = label_regions_on(st, d_labels, label_bytes, width, height, connectivity, d_regions,
                                         stats_cap, d_area, d_bbox, d_first, d_label, d_pixels, d_sums);
  // nothing behind entry min(R, stats_cap) is written
  const size_t m = std::min((size_t)count, cap);
  DQ_HIP(hipMemcpyAsync(regions, d_regions, n * 4, hipMemcpyDeviceToHost, st));
  if (d_area && m) DQ_HIP(hipMemcpyAsync(area, d_area, m * 4, hipMemcpyDeviceToHost, st));
  if (d_bbox && m) DQ_HIP(hipMemcpyAsync(bbox, d_bbox, m * 16, hipMemcpyDeviceToHost, st));
  if (d_first && m) DQ_HIP(hipMemcpyAsync(first, d_first, m * 4, hipMemcpyDeviceToHost, st));
  if (d_label && m) DQ_HIP(hipMemcpyAsync(label, d_label, m * 4, hipMemcpyDeviceToHost, st));
  if (d_sums && m) DQ_HIP(hipMemcpyAsync(sums, d_sums, m * 24, hipMemcpyDeviceToHost, st));
  DQ_HIP(hipStreamSynchronize(st));
  for (void* p : {d_labels, (void*)d_regions, (void*)d_area, (void*)d_bbox, (void*)d_first, (void*)d_label,
                  (void*)d_pixels, (void*)d_sums})
    if (p) DQ_HIP(hipFreeAsync(p, st));
  return count;
}

// Region adjacency graph of a region map (dq_adjacency.hip).  Every argument
// check comes before the first HIP call.
static bool adjacency_args_ok(const uint32_t* regions, uint32_t width, uint32_t height, int connectivity,
                              uint32_t edge_cap, const uint32_t* edges, const uint32_t* border,
                              const uint32_t* contact, const uint32_t* pixels, const uint64_t* step,
                              uint32_t nregions, const uint32_t* degree) {
  if (connectivity != 4 && connectivity != 8) return false;
  // n <= 2^30: a contact is the one word 4 * p + dir, and E < 4 n fits uint32
  if (width == 0 || height == 0 || width > 65535u || height > 65535u ||
      (uint64_t)width * height > DQ_HIP_ADJACENCY_MAX_PIXELS)
    return false;
  if (!regions) return false;
  for (const void* p : {(const void*)regions, (const void*)edges, (const void*)border, (const void*)contact,
                        (const void*)pixels, (const void*)degree})
    if (((uintptr_t)p & 3u) != 0) return false;
  if (((uintptr_t)step & 7u) != 0) return false;
  if (step && !pixels) return false;
  if (edge_cap > 0 && !edges && !border && !contact && !step) return false;
  if (degree && nregions == 0) return false;
  return true;
}

// Enqueues both halves on st with scratch owned by the call, waits, returns E.
// One small read-back sits between the halves: the table is sized from the
// heads the first half counted.
static int64_t region_adjacency_on(hipStream_t st, const uint32_t* d_regions, uint32_t width, uint32_t height,
                                   int connectivity, uint32_t edge_cap, uint32_t* d_edges, uint32_t* d_border,
                                   uint32_t* d_contact, const uint32_t* d_pixels, uint64_t* d_step,
                                   uint32_t nregions, uint32_t* d_degree) {
  uint32_t* counts = nullptr;
  DQ_HIP(hipMallocAsync((void**)&counts, dq::adjacency_count_words(width, height) * 4, st));
  dq::AdjacencyArgs a{d_regions, width,    height,   connectivity,
                      edge_cap,  d_edges,  d_border, d_contact,
                      d_pixels,  (unsigned long long*)d_step, d_degree, counts, nullptr};
  if (d_degree) DQ_HIP(hipMemsetAsync(d_degree, 0, (size_t)nregions * 4, st));
  dq::launch_adjacency_count(a, st);
  DQ_HIP(hipGetLastError());
  uint32_t heads = 0, count = 0;
  DQ_HIP(hipMemcpyAsync(&heads, dq::adjacency_heads_word(a), 4, hipMemcpyDeviceToHost, st));
  DQ_HIP(hipStreamSynchronize(st));
  if (heads != 0) {   // (no head: no contact, no edge)
    DQ_HIP(hipMallocAsync(&a.table, dq::adjacency_scratch_bytes(heads, d_step != nullptr), st));
    dq::launch_adjacency_build(a, heads, st);
    DQ_HIP(hipGetLastError());
    DQ_HIP(hipMemcpyAsync(&count, dq::adjacency_edges_word(a), 4, hipMemcpyDeviceToHost, st));
    DQ_HIP(hipFreeAsync(a.table, st));
  }
  DQ_HIP(hipFreeAsync(counts, st));
  DQ_HIP(hipStreamSynchronize(st));
  return (int64_t)count;
}

int64_t dq_hip_region_adjacency_dev(int device, const uint32_t* d_regions, uint32_t width, uint32_t height,
                                    int connectivity, uint32_t edge_cap, uint32_t* d_edges, uint32_t* d_border,
                                    uint32_t* d_contact, const uint32_t* d_pixels, uint64_t* d_step,
                                    uint32_t nregions, uint32_t* d_degree, void* stream) {
  if (!adjacency_args_ok(d_regions, width, height, connectivity, edge_cap, d_edges, d_border, d_contact, d_pixels,
                         d_step, nregions, d_degree))
    return -1;
  // (no engine state is touched: calls on two streams may overlap)
  hipStream_t st = engine_stream(device, stream);
  return region_adjacency_on(st, d_regions, width, height, connectivity, edge_cap, d_edges, d_border, d_contact,
                             d_pixels, d_step, nregions, d_degree);
}

int64_t dq_hip_region_adjacency(const uint32_t* regions, uint32_t width, uint32_t height, int connectivity,
                                uint32_t edge_cap, uint32_t* edges, uint32_t* border, uint32_t* contact,
                                const uint32_t* pixels, uint64_t* step, uint32_t nregions, uint32_t* degree) {
  if (!adjacency_args_ok(regions, width, height, connectivity, edge_cap, edges, border, contact, pixels, step,
                         nregions, degree))
    return -1;
  Engine& e = engine_for(current_device());
  hipStream_t st = e.stream();
  const size_t n = (size_t)width * height, cap = edge_cap;
  uint32_t *d_regions = nullptr, *d_edges = nullptr, *d_border = nullptr, *d_contact = nullptr, *d_pixels = nullptr,
           *d_degree = nullptr;
  uint64_t* d_step = nullptr;
  DQ_HIP(hipMallocAsync((void**)&d_regions, n * 4, st));
  if (cap && edges) DQ_HIP(hipMallocAsync((void**)&d_edges, cap * 8, st));
  if (cap && border) DQ_HIP(hipMallocAsync((void**)&d_border, cap * 4, st));
  if (cap && contact) DQ_HIP(hipMallocAsync((void**)&d_contact, cap * 8, st));
  if (cap && step) {
    DQ_HIP(hipMallocAsync((void**)&d_step, cap * 8, st));
    DQ_HIP(hipMallocAsync((void**)&d_pixels, n * 4, st));
    DQ_HIP(hipMemcpyAsync(d_pixels, pixels, n * 4, hipMemcpyHostToDevice, st));
  }
  if (degree) DQ_HIP(hipMallocAsync((void**)&d_degree, (size_t)nregions * 4, st));
  DQ_HIP(hipMemcpyAsync(d_regions, regions, n * 4, hipMemcpyHostToDevice, st));
  const int64_t count = region_adjacency_on(st, d_regions, width, height, connectivity, edge_cap, d_edges, d_border,
                                            d_contact, d_pixels, d_step, nregions, d_degree);
  // nothing behind entry min(E, edge_cap) is written
  const size_t m = std::min((size_t)count, cap);
  if (d_edges && m) DQ_HIP(hipMemcpyAsync(edges, d_edges, m * 8, hipMemcpyDeviceToHost, st));
  if (d_border && m) DQ_HIP(hipMemcpyAsync(border, d_border, m * 4, hipMemcpyDeviceToHost, st));
  if (d_contact && m) DQ_HIP(hipMemcpyAsync(contact, d_contact, m * 8, hipMemcpyDeviceToHost, st));
  if (d_step && m) DQ_HIP(hipMemcpyAsync(step, d_step, m * 8, hipMemcpyDeviceToHost, st));
  if (d_degree) DQ_HIP(hipMemcpyAsync(degree, d_degree, (size_t)nregions * 4, hipMemcpyDeviceToHost, st));
  DQ_HIP(hipStreamSynchronize(st));
  for (void* p : {(void*)d_regions, (void*)d_edges, (void*)d_border, (void*)d_contact, (void*)d_pixels,
                  (void*)d_step, (void*)d_degree})
    if (p) DQ_HIP(hipFreeAsync(p, st));
  return count;
}

// Region merge over the adjacency graph (dq_merge.hip).  Every argument check
// comes before the first HIP call.
static bool merge_args_ok(const uint32_t* regions, uint32_t n, uint32_t nregions, const uint32_t* area,
                          const uint32_t* first, const uint64_t* sums, const uint32_t* bbox, uint32_t nedges,
                          const uint32_t* edges, const uint32_t* out_regions, const uint32_t* remap,
                          uint32_t stats_cap, const uint32_t* out_area, const uint32_t* out_bbox,
                          const uint32_t* out_first, const uint64_t* out_sums) {
  if (!regions || !area || !first || !sums || !out_regions) return false;
  if (n == 0 || n > 0x7FFFFFFFu) return false;
  if (nregions == 0 || nregions > n) return false;
  if (nedges > 0 && !edges) return false;
  for (const void* p : {(const void*)regions, (const void*)area, (const void*)first, (const void*)bbox,
                        (const void*)edges, (const void*)out_regions, (const void*)remap, (const void*)out_area,
                        (const void*)out_bbox, (const void*)out_first})
    if (((uintptr_t)p & 3u) != 0) return false;
  if (((uintptr_t)sums & 7u) != 0 || ((uintptr_t)out_sums & 7u) != 0) return false;
  if (out_bbox && !bbox) return false;
  if (stats_cap > 0 && !out_area && !out_bbox && !out_first && !out_sums) return false;
  return true;
}

// Enqueues the rounds on st with scratch owned by the call, waits, returns R'.
// The host reads the links of a round back (4 bytes) and stops at 0.
static int64_t merge_regions_on(hipStream_t st, dq::MergeArgs a, uint32_t max_rounds, uint32_t* rounds) {
  DQ_HIP(hipMallocAsync(&a.scratch, dq::merge_scratch_bytes(a.n, a.nregions, a.bbox != nullptr, a.remap != nullptr),
                        st));
  dq::launch_merge_init(a, st);
  uint32_t done = 0;
  // Every counted round makes a link, i.e. removes at least one component: fewer than nregions rounds,
  // so the loop ends by itself.  (Without a distance limit the restless components at least halve per
  // round; with one, a component may get its first offer only after a neighbour's mean has moved, and
  // a star of such leaves takes a round per leaf.)
  while (a.nedges != 0 && a.min_area != 0 && (max_rounds == 0 || done < max_rounds)) {
    dq::launch_merge_choose(a, st);
    DQ_HIP(hipGetLastError());
    uint32_t links = 0;
    DQ_HIP(hipMemcpyAsync(&links, dq::merge_links_word(a), 4, hipMemcpyDeviceToHost, st));
    DQ_HIP(hipStreamSynchronize(st));
    if (links == 0) break;
    dq::launch_merge_fold(a, st);
    ++done;
  }
  DQ_HIP(dq::launch_merge_finish(a, st));
  DQ_HIP(hipGetLastError());
  uint32_t count = 0;
  DQ_HIP(hipMemcpyAsync(&count, dq::merge_count_word(a), 4, hipMemcpyDeviceToHost, st));
  DQ_HIP(hipFreeAsync(a.scratch, st));
  DQ_HIP(hipStreamSynchronize(st));
  if (rounds) *rounds = done;
  return (int64_t)count;
}

int64_t dq_hip_merge_regions_dev(int device, const uint32_t* d_regions, uint32_t n, uint32_t nregions,
                                 const uint32_t* d_area, const uint32_t* d_first, const uint64_t* d_sums,
                                 const uint32_t* d_bbox, uint32_t nedges, const uint32_t* d_edges, uint32_t min_area,
                                 uint32_t max_dist, uint32_t max_rounds, uint32_t* d_out_regions, uint32_t* d_remap,
                                 uint32_t stats_cap, uint32_t* d_out_area, uint32_t* d_out_bbox,
                                 uint32_t* d_out_first, uint64_t* d_out_sums, uint32_t* rounds, void* stream) {
  if (!merge_args_ok(d_regions, n, nregions, d_area, d_first, d_sums, d_bbox, nedges, d_edges, d_out_regions, d_remap,
                     stats_cap, d_out_area, d_out_bbox, d_out_first, d_out_sums))
    return -1;
  // (no engine state is touched: calls on two streams may overlap)
  hipStream_t st = engine_stream(device, stream);
  dq::MergeArgs a{d_regions, n,        nregions,      d_area,  d_first,   (const unsigned long long*)d_sums,
                  d_bbox,    nedges,   d_edges,       min_area, max_dist, d_out_regions,
                  d_remap,   stats_cap, d_out_area,   d_out_bbox, d_out_first, (unsigned long long*)d_out_sums,
                  nullptr};
  return merge_regions_on(st, a, max_rounds, rounds);
}

int64_t dq_hip_segment_labels(const void* labels, int label_bytes, uint32_t width, uint32_t height, int connectivity,
                              const uint32_t* pixels, uint32_t min_area, uint32_t max_dist, uint32_t max_rounds,
                              uint32_t* regions, uint32_t stats_cap, uint32_t* area, uint32_t* bbox, uint32_t* first,
                              uint64_t* sums, uint32_t* rounds) {
  if (!pixels ||
      !regions_args_ok(labels, label_bytes, width, height, connectivity, regions, stats_cap, area, bbox, first,
                       nullptr, pixels, sums) ||
      !adjacency_args_ok(regions, width, height, connectivity, 0, nullptr, nullptr, nullptr, pixels, nullptr, 0,
                         nullptr))
    return -1;
  Engine& e = engine_for(current_device());
  hipStream_t st = e.stream();
  const size_t n = (size_t)width * height;
  void* d_labels = nullptr;
  uint32_t *d_pixels = nullptr, *d_regions = nullptr, *d_area = nullptr, *d_first = nullptr, *d_bbox = nullptr,
           *d_edges = nullptr, *o_area = nullptr, *o_bbox = nullptr, *o_first = nullptr;
  uint64_t *d_sums = nullptr, *o_sums = nullptr;
  DQ_HIP(hipMallocAsync(&d_labels, n * (size_t)label_bytes, st));
  DQ_HIP(hipMallocAsync((void**)&d_pixels, n * 4, st));
  DQ_HIP(hipMallocAsync((void**)&d_regions, n * 4, st));
  DQ_HIP(hipMemcpyAsync(d_labels, labels, n * (size_t)label_bytes, hipMemcpyHostToDevice, st));
  DQ_HIP(hipMemcpyAsync(d_pixels, pixels, n * 4, hipMemcpyHostToDevice, st));
  // R and E are known only after their stages ran: count-only, then with exact capacity
  const int64_t R = label_regions_on(st, d_labels, label_bytes, width, height, connectivity, d_regions, 0, nullptr,
                                     nullptr, nullptr, nullptr, nullptr, nullptr);
  DQ_HIP(hipMallocAsync((void**)&d_area, (size_t)R * 4, st));
  DQ_HIP(hipMallocAsync((void**)&d_first, (size_t)R * 4, st));
  DQ_HIP(hipMallocAsync((void**)&d_sums, (size_t)R * 24, st));
  if (stats_cap && bbox) DQ_HIP(hipMallocAsync((void**)&d_bbox, (size_t)R * 16, st));
  label_regions_on(st, d_labels, label_bytes, width, height, connectivity, d_regions, (uint32_t)R, d_area, d_bbox,
                   d_first, nullptr, d_pixels, d_sums);
  const int64_t E = region_adjacency_on(st, d_regions, width, height, connectivity, 0, nullptr, nullptr, nullptr,
                                        nullptr, nullptr, 0, nullptr);
  if (E > 0) {
    DQ_HIP(hipMallocAsync((void**)&d_edges, (size_t)E * 8, st));
    region_adjacency_on(st, d_regions, width, height, connectivity, (uint32_t)E, d_edges, nullptr, nullptr, nullptr,
                        nullptr, 0, nullptr);
  }
  const size_t cap = std::min((size_t)stats_cap, (size_t)R);   // (R' <= R)
  if (cap && area) DQ_HIP(hipMallocAsync((void**)&o_area, cap * 4, st));
  if (cap && bbox) DQ_HIP(hipMallocAsync((void**)&o_bbox, cap * 16, st));
  if (cap && first) DQ_HIP(hipMallocAsync((void**)&o_first, cap * 4, st));
  if (cap && sums) DQ_HIP(hipMallocAsync((void**)&o_sums, cap * 24, st));
  dq::MergeArgs a{d_regions, (uint32_t)n,   (uint32_t)R, d_area,   d_first,  (const unsigned long long*)d_sums,
                  d_bbox,    (uint32_t)E,   d_edges,     min_area, max_dist, d_regions,
                  nullptr,   (uint32_t)cap, o_area,      o_bbox,   o_first,  (unsigned long long*)o_sums,
                  nullptr};
  const int64_t count = merge_regions_on(st, a, max_rounds, rounds);
  // nothing behind entry min(R', stats_cap) is written
  const size_t m = std::min((size_t)count, cap);
  DQ_HIP(hipMemcpyAsync(regions, d_regions, n * 4, hipMemcpyDeviceToHost, st));
  if (o_area && m) DQ_HIP(hipMemcpyAsync(area, o_area, m * 4, hipMemcpyDeviceToHost, st));
  if (o_bbox && m) DQ_HIP(hipMemcpyAsync(bbox, o_bbox, m * 16, hipMemcpyDeviceToHost, st));
  if (o_first && m) DQ_HIP(hipMemcpyAsync(first, o_first, m * 4, hipMemcpyDeviceToHost, st));
  if (o_sums && m) DQ_HIP(hipMemcpyAsync(sums, o_sums, m * 24, hipMemcpyDeviceToHost, st));
  DQ_HIP(hipStreamSynchronize(st));
  for (void* p : {d_labels, (void*)d_pixels, (void*)d_regions, (void*)d_area, (void*)d_first, (void*)d_bbox,
                  (void*)d_edges, (void*)d_sums, (void*)o_area, (void*)o_bbox, (void*)o_first, (void*)o_sums})
    if (p) DQ_HIP(hipFreeAsync(p, st));
  return count;
}

// Containment tree of a region map (dq_contain.hip).  Every argument check
// comes before the first HIP call.
static bool containment_args_ok(const uint32_t* regions, uint32_t width, uint32_t height, uint32_t nregions,
                                const uint32_t* area, uint32_t nedges, const uint32_t* edges, const uint32_t* depth,
                                const uint32_t* parent, const uint32_t* roots, const uint32_t* child_offsets,
                                const uint32_t* children, const uint32_t* subtree, const uint64_t* enclosed,
                                const uint32_t* order, const uint32_t* pos) {
  if (!regions || !area) return false;
  if (nedges > 0 && !edges) return false;
  if (width == 0 || height == 0 || width > 65535u || height > 65535u) return false;
  if (nregions == 0 || nregions > (uint64_t)width * height) return false;
  for (const void* p : {(const void*)regions, (const void*)area, (const void*)edges, (const void*)depth,
                        (const void*)parent, (const void*)roots, (const void*)child_offsets, (const void*)children,
                        (const void*)subtree, (const void*)order, (const void*)pos})
    if (((uintptr_t)p & 3u) != 0) return false;
  if (((uintptr_t)enclosed & 7u) != 0) return false;
  if (children && !child_offsets) return false;
  return true;
}

struct ContainOut {
  uint32_t *depth, *parent, *roots, *child_offsets, *children, *subtree;
  uint64_t* enclosed;
  uint32_t *order, *pos;
};

// Enqueues the stages on st with scratch owned by the call, copies what is
// wanted to `to` (device or host arrays: `kind`), waits, returns nroots.  The
// host reads the regions reached back once per level (8 bytes) and stops at a
// level that reached nobody.
static int64_t region_containment_on(hipStream_t st, dq::ContainArgs a, const ContainOut& to, hipMemcpyKind kind,
                                     uint32_t* levels, uint32_t* reached) {
  DQ_HIP(hipMallocAsync(&a.scratch, dq::contain_scratch_bytes(a.nregions), st));
  dq::launch_contain_roots(a, st);
  DQ_HIP(hipGetLastError());
  uint32_t words[2] = {0, 0};   // reached so far, the OR of the areas
  DQ_HIP(hipMemcpyAsync(words, dq::contain_counters(a), 8, hipMemcpyDeviceToHost, st));
  DQ_HIP(hipStreamSynchronize(st));
  const uint32_t nroots = words[0], area_bits = dq::sort_key_bits(words[1]);
  // Every level but the last reaches at least one region: at most nregions levels, the loop ends by itself.
  uint32_t nlevels = 1, have = nroots;
  while (a.nedges != 0 && have < a.nregions) {
    dq::launch_contain_level(a, nlevels, st);
    DQ_HIP(hipGetLastError());
    DQ_HIP(hipMemcpyAsync(words, dq::contain_counters(a), 8, hipMemcpyDeviceToHost, st));
    DQ_HIP(hipStreamSynchronize(st));
    if (words[0] == have) break;
    have = words[0];
    ++nlevels;
  }
  dq::launch_contain_tree(a, nlevels, nroots, have, area_bits, st);
  DQ_HIP(hipGetLastError());
  const dq::ContainResults r = dq::contain_results(a);
  const size_t R = a.nregions, nchildren = have - nroots;
  // nothing behind the entries in use is written
  if (to.depth) DQ_HIP(hipMemcpyAsync(to.depth, r.depth, R * 4, kind, st));
  if (to.parent) DQ_HIP(hipMemcpyAsync(to.parent, r.parent, R * 4, kind, st));
  if (to.roots && nroots) DQ_HIP(hipMemcpyAsync(to.roots, r.sequence, (size_t)nroots * 4, kind, st));
  if (to.child_offsets) DQ_HIP(hipMemcpyAsync(to.child_offsets, r.child_offsets, (R + 1) * 4, kind, st));
  if (to.children && nchildren) DQ_HIP(hipMemcpyAsync(to.children, r.sequence + nroots, nchildren * 4, kind, st));
  if (to.subtree) DQ_HIP(hipMemcpyAsync(to.subtree, r.subtree, R * 4, kind, st));
  if (to.enclosed) DQ_HIP(hipMemcpyAsync(to.enclosed, r.enclosed, R * 8, kind, st));
  if (to.order && have) DQ_HIP(hipMemcpyAsync(to.order, r.order, (size_t)have * 4, kind, st));
  if (to.pos) DQ_HIP(hipMemcpyAsync(to.pos, r.pos, R * 4, kind, st));
  DQ_HIP(hipFreeAsync(a.scratch, st));
  DQ_HIP(hipStreamSynchronize(st));
  if (levels) *levels = nlevels;
  if (reached) *reached = have;
  return (int64_t)nroots;
}

int64_t dq_hip_region_containment_dev(int device, const uint32_t* d_regions, uint32_t width, uint32_t height,
                                      uint32_t nregions, const uint32_t* d_area, uint32_t nedges,
                                      const uint32_t* d_edges, uint32_t* d_depth, uint32_t* d_parent,
                                      uint32_t* d_roots, uint32_t* d_child_offsets, uint32_t* d_children,
                                      uint32_t* d_subtree, uint64_t* d_enclosed, uint32_t* d_order, uint32_t* d_pos,
                                      uint32_t* levels, uint32_t* reached, void* stream) {
  if (!containment_args_ok(d_regions, width, height, nregions, d_area, nedges, d_edges, d_depth, d_parent, d_roots,
                           d_child_offsets, d_children, d_subtree, d_enclosed, d_order, d_pos))
    return -1;
  // (no engine state is touched: calls on two streams may overlap)
  hipStream_t st = engine_stream(device, stream);
  dq::ContainArgs a{d_regions, width, height, nregions, d_area, nedges, d_edges, nullptr};
  const ContainOut to{d_depth, d_parent, d_roots, d_child_offsets, d_children, d_subtree, d_enclosed, d_order, d_pos};
  return region_containment_on(st, a, to, hipMemcpyDeviceToDevice, levels, reached);
}

int64_t dq_hip_region_containment(const uint32_t* regions, uint32_t width, uint32_t height, uint32_t nregions,
                                  const uint32_t* area, uint32_t nedges, const uint32_t* edges, uint32_t* depth,
                                  uint32_t* parent, uint32_t* roots, uint32_t* child_offsets, uint32_t* children,
                                  uint32_t* subtree, uint64_t* enclosed, uint32_t* order, uint32_t* pos,
                                  uint32_t* levels, uint32_t* reached) {
  if (!containment_args_ok(regions, width, height, nregions, area, nedges, edges, depth, parent, roots, child_offsets,
                           children, subtree, enclosed, order, pos))
    return -1;
  Engine& e = engine_for(current_device());
  hipStream_t st = e.stream();
  const size_t n = (size_t)width * height;
  uint32_t *d_regions = nullptr, *d_area = nullptr, *d_edges = nullptr;
  DQ_HIP(hipMallocAsync((void**)&d_regions, n * 4, st));
  DQ_HIP(hipMallocAsync((void**)&d_area, (size_t)nregions * 4, st));
  if (nedges) DQ_HIP(hipMallocAsync((void**)&d_edges, (size_t)nedges * 8, st));
  DQ_HIP(hipMemcpyAsync(d_regions, regions, n * 4, hipMemcpyHostToDevice, st));
  DQ_HIP(hipMemcpyAsync(d_area, area, (size_t)nregions * 4, hipMemcpyHostToDevice, st));
  if (nedges) DQ_HIP(hipMemcpyAsync(d_edges, edges, (size_t)nedges * 8, hipMemcpyHostToDevice, st));
  dq::ContainArgs a{d_regions, width, height, nregions, d_area, nedges, d_edges, nullptr};
  const ContainOut to{depth, parent, roots, child_offsets, children, subtree, enclosed, order, pos};
  const int64_t nroots = region_containment_on(st, a, to, hipMemcpyDeviceToHost, levels, reached);
  for (void* p : {(void*)d_regions, (void*)d_area, (void*)d_edges})
    if (p) DQ_HIP(hipFreeAsync(p, st));
  return nroots;
}

int dq_hip_regions_by_size_dev(int device, uint32_t nregions, const uint32_t* d_area, uint32_t* d_order,
                               uint32_t* d_rank, void* stream) {
  if (!d_area || nregions == 0 || (!d_order && !d_rank)) return -1;
  for (const void* p : {(const void*)d_area, (const void*)d_order, (const void*)d_rank})
    if (((uintptr_t)p & 3u) != 0) return -1;
  // (no engine state is touched: calls on two streams may overlap)
  hipStream_t st = engine_stream(device, stream);
  void* scratch = nullptr;
  DQ_HIP(hipMallocAsync(&scratch, dq::size_scratch_bytes(nregions), st));
  dq::launch_size_bits(nregions, d_area, scratch, st);
  DQ_HIP(hipGetLastError());
  uint32_t bits = 0;   // the OR of the areas: the sort runs over the key bits in use
  DQ_HIP(hipMemcpyAsync(&bits, dq::size_bits_word(scratch), 4, hipMemcpyDeviceToHost, st));
  DQ_HIP(hipStreamSynchronize(st));
  dq::launch_size_order(nregions, d_area, dq::sort_key_bits(bits), d_order, d_rank, scratch, st);
  DQ_HIP(hipGetLastError());
  DQ_HIP(hipFreeAsync(scratch, st));
  DQ_HIP(hipStreamSynchronize(st));
  return 0;
}

// Pixel lists of a region map (dq_pixels.hip).  Every argument check comes
// before the first HIP call.
static bool pixels_args_ok(const uint32_t* regions, uint32_t width, uint32_t height, uint32_t nregions,
                           const uint32_t* offsets, const uint32_t* coords, const uint32_t* index,
                           const uint32_t* pixels, const uint32_t* colors) {
  if (!regions || !offsets) return false;
  if (width == 0 || height == 0 || width > 65535u || height > 65535u || (uint64_t)width * height > 0x7FFFFFFFull)
    return false;
  if (nregions == 0 || nregions > 0x7FFFFFFFu) return false;
  for (const void* p : {(const void*)regions, (const void*)offsets, (const void*)coords, (const void*)index,
                        (const void*)pixels, (const void*)colors})
    if (((uintptr_t)p & 3u) != 0) return false;
  if (colors && !pixels) return false;
  return true;
}

// Enqueues both halves on st with scratch owned by the call and waits.  One
// small read-back sits between the halves: the table is sized from T, and a
// map with T > n is refused there, before any output array is written.
static int64_t region_pixels_on(hipStream_t st, const uint32_t* d_regions, uint32_t width, uint32_t height,
                                uint32_t nregions, uint32_t* d_offsets, uint32_t* d_coords, uint32_t* d_index,
                                const uint32_t* d_pixels, uint32_t* d_colors) {
  dq::PixelsArgs a{d_regions, width, height, nregions, d_offsets, d_coords, d_index, d_pixels, d_colors, nullptr, nullptr};
  DQ_HIP(hipMallocAsync((void**)&a.rows, dq::pixels_rows_bytes(nregions), st));
  dq::launch_pixels_rows(a, st);
  DQ_HIP(hipGetLastError());
  uint32_t total = 0;
  DQ_HIP(hipMemcpyAsync(&total, dq::pixels_total_word(a), 4, hipMemcpyDeviceToHost, st));
  DQ_HIP(hipStreamSynchronize(st));
  const bool fits = total <= width * height;
  if (fits) {
    DQ_HIP(hipMallocAsync((void**)&a.table, dq::pixels_table_bytes(total), st));
    dq::launch_pixels_lists(a, total, st);
    DQ_HIP(hipGetLastError());
    DQ_HIP(hipFreeAsync(a.table, st));
  }
  DQ_HIP(hipFreeAsync(a.rows, st));
  DQ_HIP(hipStreamSynchronize(st));
  return fits ? 0 : -2;
}

int64_t dq_hip_region_pixels_dev(int device, const uint32_t* d_regions, uint32_t width, uint32_t height,
                                 uint32_t nregions, uint32_t* d_offsets, uint32_t* d_coords, uint32_t* d_index,
                                 const uint32_t* d_pixels, uint32_t* d_colors, void* stream) {
  if (!pixels_args_ok(d_regions, width, height, nregions, d_offsets, d_coords, d_index, d_pixels, d_colors)) return -1;
  // (no engine state is touched: calls on two streams may overlap)
  hipStream_t st = engine_stream(device, stream);
  return region_pixels_on(st, d_regions, width, height, nregions, d_offsets, d_coords, d_index, d_pixels, d_colors);
}

int64_t dq_hip_region_pixels(const uint32_t* regions, uint32_t width, uint32_t height, uint32_t nregions,
                             uint32_t* offsets, uint32_t* coords, uint32_t* index, const uint32_t* pixels,
                             uint32_t* colors) {
  if (!pixels_args_ok(regions, width, height, nregions, offsets, coords, index, pixels, colors)) return -1;
  Engine& e = engine_for(current_device());
  hipStream_t st = e.stream();
  const size_t n = (size_t)width * height, no = (size_t)nregions + 1;
  uint32_t *d_regions = nullptr, *d_offsets = nullptr, *d_coords = nullptr, *d_index = nullptr, *d_pixels = nullptr,
           *d_colors = nullptr;
  DQ_HIP(hipMallocAsync((void**)&d_regions, n * 4, st));
  DQ_HIP(hipMallocAsync((void**)&d_offsets, no * 4, st));
  if (coords) DQ_HIP(hipMallocAsync((void**)&d_coords, n * 4, st));
  if (index) DQ_HIP(hipMallocAsync((void**)&d_index, n * 4, st));
  if (colors) {
    DQ_HIP(hipMallocAsync((void**)&d_colors, n * 4, st));
    DQ_HIP(hipMallocAsync((void**)&d_pixels, n * 4, st));
    DQ_HIP(hipMemcpyAsync(d_pixels, pixels, n * 4, hipMemcpyHostToDevice, st));
  }
  DQ_HIP(hipMemcpyAsync(d_regions, regions, n * 4, hipMemcpyHostToDevice, st));
  const int64_t rc = region_pixels_on(st, d_regions, width, height, nregions, d_offsets, d_coords, d_index, d_pixels,
                                      d_colors);
  if (rc == 0) {   // (a refused map leaves the host arrays as they were)
    DQ_HIP(hipMemcpyAsync(offsets, d_offsets, no * 4, hipMemcpyDeviceToHost, st));
    if (coords) DQ_HIP(hipMemcpyAsync(coords, d_coords, n * 4, hipMemcpyDeviceToHost, st));
    if (index) DQ_HIP(hipMemcpyAsync(index, d_index, n * 4, hipMemcpyDeviceToHost, st));
    if (colors) DQ_HIP(hipMemcpyAsync(colors, d_colors, n * 4, hipMemcpyDeviceToHost, st));
    DQ_HIP(hipStreamSynchronize(st));
  }
  for (void* p : {(void*)d_regions, (void*)d_offsets, (void*)d_coords, (void*)d_index, (void*)d_pixels,
                  (void*)d_colors})
    if (p) DQ_HIP(hipFreeAsync(p, st));
  return rc;
}

int dq_hip_scatter_coords_dev(int device, const uint32_t* d_values, const uint32_t* d_coords, uint32_t n,
                              uint32_t width, uint32_t* d_frame, void* stream) {
  if (!d_values || !d_coords || !d_frame || width == 0) return -1;
  for (const void* p : {(const void*)d_values, (const void*)d_coords, (const void*)d_frame})
    if (((uintptr_t)p & 3u) != 0) return -1;
  if (n == 0) return 0;
  hipStream_t st = engine_stream(device, stream);
  dq::launch_scatter_coords(d_values, d_coords, n, width, d_frame, st);
  join_default_stream(stream, st);
  DQ_HIP(hipGetLastError());
  return 0;
}

// Region map -> pixel lists -> one weighted quant per region -> painted frame.
// The regions path keeps one pinned argument and one pinned result record per
// job of a call (about 4.5 KB): the jobs go to it kRegionMapJobs at a time.
static constexpr size_t kRegionMapJobs = 8192;

static bool region_map_args_ok(const uint32_t* regions, uint32_t width, uint32_t height, uint32_t nregions,
                               const uint32_t* pixels, uint32_t k, const uint32_t* out, const uint32_t* cts,
                               const uint32_t* k_outs, int max_iters) {
  if (!pixels || !cts || !k_outs || k == 0 || k > 0x7FFFFFFFu || max_iters < 1) return false;
  if (((uintptr_t)out & 3u) != 0) return false;
  // (the offsets and lists are the call's own: any aligned non-NULL pointer stands in for them)
  return pixels_args_ok(regions, width, height, nregions, regions, nullptr, nullptr, pixels, nullptr);
}

// One weighted-regions call over the ranges [off[r], off[r + 1]) of d_colors, region r's K = k: its
// colortable to cts + r * k, its count to k_outs[r] (0 for an empty range, the row untouched), its
// mapped colours to the same range of d_mapped when given.  Returns the total of empty clusters.
static int64_t quant_ranges_on(int device, hipStream_t st, const std::vector<uint32_t>& off, uint32_t nregions,
                               const uint32_t* d_colors, uint32_t* d_mapped, uint32_t k, uint32_t* cts,
                               uint32_t* k_outs, int max_iters) {
  int64_t empty = 0;
  Engine& e = engine_for(device);
  std::vector<dq::FrameJob> jobs;
  std::vector<uint32_t> ids;
  jobs.reserve(std::min<size_t>(nregions, kRegionMapJobs));
  ids.reserve(jobs.capacity());
  auto flush = [&] {
    if (jobs.empty()) return;
    {
      std::lock_guard<std::mutex> g(e.mutex());
      e.run_weighted_regions(jobs.data(), (int)jobs.size(), max_iters, st);
    }
    for (size_t i = 0; i < jobs.size(); ++i) {
      k_outs[ids[i]] = (uint32_t)jobs[i].k_out;
      empty += jobs[i].num_empty;
    }
    jobs.clear();
    ids.clear();
  };
  for (uint32_t r = 0; r < nregions; ++r) {
    const uint32_t len = off[r + 1] - off[r];
    if (len == 0) {   // an empty list: no call, its colortable row stays as it is
      k_outs[r] = 0;
      continue;
    }
    dq::FrameJob j;
    j.d_in = d_colors + off[r];
    j.n = len;
    j.d_out = d_mapped ? d_mapped + off[r] : nullptr;
    j.k = (int)k;
    j.ct = cts + (size_t)r * k;
    jobs.push_back(j);
    ids.push_back(r);
    if (jobs.size() == kRegionMapJobs) flush();
  }
  flush();
  return empty;
}

static int64_t quant_region_map_on(int device, hipStream_t st, const uint32_t* d_regions, uint32_t width,
                                   uint32_t height, uint32_t nregions, const uint32_t* d_pixels, uint32_t k,
                                   uint32_t* d_out, uint32_t* cts, uint32_t* k_outs, int max_iters) {
  const size_t n = (size_t)width * height, no = (size_t)nregions + 1;
  uint32_t *d_offsets = nullptr, *d_colors = nullptr, *d_coords = nullptr, *d_mapped = nullptr;
  DQ_HIP(hipMallocAsync((void**)&d_offsets, no * 4, st));
  DQ_HIP(hipMallocAsync((void**)&d_colors, n * 4, st));
  if (d_out) {
    DQ_HIP(hipMallocAsync((void**)&d_coords, n * 4, st));
    DQ_HIP(hipMallocAsync((void**)&d_mapped, n * 4, st));
    // (an id >= nregions leaves its pixel out of the lists: the scatter below then reads Coord 0, not garbage)
    DQ_HIP(hipMemsetAsync(d_coords, 0, n * 4, st));
  }
  int64_t rc = region_pixels_on(st, d_regions, width, height, nregions, d_offsets, d_coords, nullptr, d_pixels, d_colors);
  if (rc == 0) {
    std::vector<uint32_t> off(no);
    DQ_HIP(hipMemcpyAsync(off.data(), d_offsets, no * 4, hipMemcpyDeviceToHost, st));
    DQ_HIP(hipStreamSynchronize(st));
    rc = quant_ranges_on(device, st, off, nregions, d_colors, d_mapped, k, cts, k_outs, max_iters);
    if (d_out) {
      dq::launch_scatter_coords(d_mapped, d_coords, (uint32_t)n, width, d_out, st);
      DQ_HIP(hipGetLastError());
    }
  }
  for (void* p : {(void*)d_offsets, (void*)d_colors, (void*)d_coords, (void*)d_mapped})
    if (p) DQ_HIP(hipFreeAsync(p, st));
  DQ_HIP(hipStreamSynchronize(st));
  return rc;
}

int64_t dq_hip_quant_region_map_dev(int device, const uint32_t* d_regions, uint32_t width, uint32_t height,
                                    uint32_t nregions, const uint32_t* d_pixels, uint32_t k, uint32_t* d_out,
                                    uint32_t* cts, uint32_t* k_outs, int max_iters, void* stream) {
  if (!region_map_args_ok(d_regions, width, height, nregions, d_pixels, k, d_out, cts, k_outs, max_iters)) return -1;
  hipStream_t st = engine_stream(device, stream);
  return quant_region_map_on(device, st, d_regions, width, height, nregions, d_pixels, k, d_out, cts, k_outs,
                             max_iters);
}

int64_t dq_hip_quant_region_map(const uint32_t* regions, uint32_t width, uint32_t height, uint32_t nregions,
                                const uint32_t* pixels, uint32_t k, uint32_t* out, uint32_t* cts, uint32_t* k_outs,
                                int max_iters) {
  if (!region_map_args_ok(regions, width, height, nregions, pixels, k, out, cts, k_outs, max_iters)) return -1;
  const int device = current_device();
  hipStream_t st = engine_for(device).stream();
  const size_t n = (size_t)width * height;
  uint32_t *d_regions = nullptr, *d_pixels = nullptr, *d_out = nullptr;
  DQ_HIP(hipMallocAsync((void**)&d_regions, n * 4, st));
  DQ_HIP(hipMallocAsync((void**)&d_pixels, n * 4, st));
  if (out) DQ_HIP(hipMallocAsync((void**)&d_out, n * 4, st));
  DQ_HIP(hipMemcpyAsync(d_regions, regions, n * 4, hipMemcpyHostToDevice, st));
  DQ_HIP(hipMemcpyAsync(d_pixels, pixels, n * 4, hipMemcpyHostToDevice, st));
  const int64_t rc = quant_region_map_on(device, st, d_regions, width, height, nregions, d_pixels, k, d_out, cts,
                                         k_outs, max_iters);
  if (rc >= 0 && out) {
    DQ_HIP(hipMemcpyAsync(out, d_out, n * 4, hipMemcpyDeviceToHost, st));
    DQ_HIP(hipStreamSynchronize(st));
  }
  for (void* p : {(void*)d_regions, (void*)d_pixels, (void*)d_out})
    if (p) DQ_HIP(hipFreeAsync(p, st));
  return rc;
}

// Capture windows of a region map (dq_windows.hip).  Every argument check comes
// before the first HIP call.
static bool windows_args_ok(const uint32_t* regions, uint32_t width, uint32_t height, uint32_t nregions, uint32_t block,
                            uint32_t expand, const uint32_t* area, const uint32_t* offsets, uint32_t cap,
                            const uint32_t* coords, const uint32_t* index, const uint32_t* pixels,
                            const uint32_t* colors) {
  if (!pixels_args_ok(regions, width, height, nregions, offsets, coords, index, pixels, colors)) return false;
  if (block < 1 || block > 8 || expand > 3) return false;
  if (((uintptr_t)area & 3u) != 0) return false;
  if (cap > 0 && !coords && !index && !colors) return false;
  return true;
}

// Enqueues the parts on st with scratch owned by the call and waits.  Two small
// read-backs sit between them: P and T size the pairs and the table (a map with
// T > P is refused there), and M decides -3 and whether the lists fit, before
// any output array is written.
static int64_t region_windows_on(hipStream_t st, const uint32_t* d_regions, uint32_t width, uint32_t height,
                                 uint32_t nregions, uint32_t block, uint32_t expand, const uint8_t* d_mask,
                                 const uint32_t* d_area, uint32_t min_area, uint32_t* d_offsets, uint32_t cap,
                                 uint32_t* d_coords, uint32_t* d_index, const uint32_t* d_pixels, uint32_t* d_colors) {
  dq::WindowsArgs a{d_regions, width,    height,  nregions, block,    expand,   d_mask, d_area,
                    min_area,  d_offsets, d_coords, d_index, d_pixels, d_colors, nullptr, nullptr};
  DQ_HIP(hipMallocAsync((void**)&a.blocks, dq::windows_blocks_bytes(width, height, block, nregions), st));
  dq::launch_windows_blocks(a, st);
  DQ_HIP(hipGetLastError());
  uint32_t npairs = 0, nrows = 0, total = 0;
  DQ_HIP(hipMemcpyAsync(&npairs, dq::windows_pairs_word(a), 4, hipMemcpyDeviceToHost, st));
  DQ_HIP(hipMemcpyAsync(&nrows, dq::windows_rows_word(a), 4, hipMemcpyDeviceToHost, st));
  DQ_HIP(hipStreamSynchronize(st));
  int64_t rc;
  if (npairs == 0xFFFFFFFFu) {
    rc = -3;   // (the pairs are indexed by words)
  } else if (nrows > npairs) {
    rc = -2;
  } else {
    DQ_HIP(hipMallocAsync((void**)&a.pairs, dq::windows_pairs_bytes(npairs, nrows), st));
    if (npairs != 0 && nrows != 0) {
      dq::launch_windows_count(a, npairs, nrows, st);
      DQ_HIP(hipGetLastError());
      DQ_HIP(hipMemcpyAsync(&total, dq::windows_total_word(a, npairs, nrows), 4, hipMemcpyDeviceToHost, st));
      DQ_HIP(hipStreamSynchronize(st));
    }
    if (total == 0xFFFFFFFFu) {
      rc = -3;
    } else {
      rc = total;
      dq::launch_windows_offsets(a, npairs, nrows, total, st);
      if (total <= cap) dq::launch_windows_lists(a, npairs, nrows, total, st);
      DQ_HIP(hipGetLastError());
    }
    DQ_HIP(hipFreeAsync(a.pairs, st));
  }
  DQ_HIP(hipFreeAsync(a.blocks, st));
  DQ_HIP(hipStreamSynchronize(st));
  return rc;
}

int64_t dq_hip_region_windows_dev(int device, const uint32_t* d_regions, uint32_t width, uint32_t height,
                                  uint32_t nregions, uint32_t block, uint32_t expand, const uint8_t* d_mask,
                                  const uint32_t* d_area, uint32_t min_area, uint32_t* d_offsets, uint32_t cap,
                                  uint32_t* d_coords, uint32_t* d_index, const uint32_t* d_pixels, uint32_t* d_colors,
                                  void* stream) {
  if (!windows_args_ok(d_regions, width, height, nregions, block, expand, d_area, d_offsets, cap, d_coords, d_index,
                       d_pixels, d_colors))
    return -1;
  // (no engine state is touched: calls on two streams may overlap)
  hipStream_t st = engine_stream(device, stream);
  return region_windows_on(st, d_regions, width, height, nregions, block, expand, d_mask, d_area, min_area, d_offsets,
                           cap, d_coords, d_index, d_pixels, d_colors);
}

// The device copies of a host windows call's inputs.
struct WindowsInputs {
  uint32_t *regions = nullptr, *area = nullptr, *pixels = nullptr;
  uint8_t* mask = nullptr;
  void upload(hipStream_t st, size_t n, uint32_t nregions, const uint32_t* h_regions, const uint8_t* h_mask,
              const uint32_t* h_area, const uint32_t* h_pixels) {
    DQ_HIP(hipMallocAsync((void**)&regions, n * 4, st));
    DQ_HIP(hipMemcpyAsync(regions, h_regions, n * 4, hipMemcpyHostToDevice, st));
    if (h_mask) {
      DQ_HIP(hipMallocAsync((void**)&mask, n, st));
      DQ_HIP(hipMemcpyAsync(mask, h_mask, n, hipMemcpyHostToDevice, st));
    }
    if (h_area) {
      DQ_HIP(hipMallocAsync((void**)&area, (size_t)nregions * 4, st));
      DQ_HIP(hipMemcpyAsync(area, h_area, (size_t)nregions * 4, hipMemcpyHostToDevice, st));
    }
    if (h_pixels) {
      DQ_HIP(hipMallocAsync((void**)&pixels, n * 4, st));
      DQ_HIP(hipMemcpyAsync(pixels, h_pixels, n * 4, hipMemcpyHostToDevice, st));
    }
  }
  void release(hipStream_t st) {
    for (void* p : {(void*)regions, (void*)area, (void*)pixels, (void*)mask})
      if (p) DQ_HIP(hipFreeAsync(p, st));
  }
};

int64_t dq_hip_region_windows(const uint32_t* regions, uint32_t width, uint32_t height, uint32_t nregions,
                              uint32_t block, uint32_t expand, const uint8_t* mask, const uint32_t* area,
                              uint32_t min_area, uint32_t* offsets, uint32_t cap, uint32_t* coords, uint32_t* index,
                              const uint32_t* pixels, uint32_t* colors) {
  if (!windows_args_ok(regions, width, height, nregions, block, expand, area, offsets, cap, coords, index, pixels,
                       colors))
    return -1;
  Engine& e = engine_for(current_device());
  hipStream_t st = e.stream();
  const size_t n = (size_t)width * height, no = (size_t)nregions + 1;
  WindowsInputs in;
  in.upload(st, n, nregions, regions, mask, area, colors ? pixels : nullptr);
  uint32_t *d_offsets = nullptr, *d_coords = nullptr, *d_index = nullptr, *d_colors = nullptr;
  DQ_HIP(hipMallocAsync((void**)&d_offsets, no * 4, st));
  if (cap && coords) DQ_HIP(hipMallocAsync((void**)&d_coords, (size_t)cap * 4, st));
  if (cap && index) DQ_HIP(hipMallocAsync((void**)&d_index, (size_t)cap * 4, st));
  if (cap && colors) DQ_HIP(hipMallocAsync((void**)&d_colors, (size_t)cap * 4, st));
  const int64_t rc = region_windows_on(st, in.regions, width, height, nregions, block, expand, in.mask, in.area,
                                       min_area, d_offsets, cap, d_coords, d_index, in.pixels, d_colors);
  if (rc >= 0) {   // (a refused map leaves the host arrays as they were)
    DQ_HIP(hipMemcpyAsync(offsets, d_offsets, no * 4, hipMemcpyDeviceToHost, st));
    if (rc > 0 && rc <= (int64_t)cap) {
      if (d_coords) DQ_HIP(hipMemcpyAsync(coords, d_coords, (size_t)rc * 4, hipMemcpyDeviceToHost, st));
      if (d_index) DQ_HIP(hipMemcpyAsync(index, d_index, (size_t)rc * 4, hipMemcpyDeviceToHost, st));
      if (d_colors) DQ_HIP(hipMemcpyAsync(colors, d_colors, (size_t)rc * 4, hipMemcpyDeviceToHost, st));
    }
    DQ_HIP(hipStreamSynchronize(st));
  }
  in.release(st);
  for (void* p : {(void*)d_offsets, (void*)d_coords, (void*)d_index, (void*)d_colors})
    if (p) DQ_HIP(hipFreeAsync(p, st));
  return rc;
}

// Region map -> capture windows -> one weighted quant per window.
static bool quant_windows_args_ok(const uint32_t* regions, uint32_t width, uint32_t height, uint32_t nregions,
                                  uint32_t block, uint32_t expand, const uint32_t* area, const uint32_t* offsets,
                                  uint32_t cap, const uint32_t* coords, const uint32_t* index, const uint32_t* pixels,
                                  const uint32_t* colors, uint32_t k, const uint32_t* out, const uint32_t* cts,
                                  const uint32_t* k_outs, int max_iters) {
  if (!pixels || !cts || !k_outs || k == 0 || k > 0x7FFFFFFFu || max_iters < 1) return false;
  if (((uintptr_t)out & 3u) != 0) return false;
  if (cap > 0 && !coords && !index && !colors && out) coords = out;   // (d_out alone is a list array of cap words)
  return windows_args_ok(regions, width, height, nregions, block, expand, area, offsets, cap, coords, index, pixels,
                         colors);
}

static int64_t quant_region_windows_on(int device, hipStream_t st, const uint32_t* d_regions, uint32_t width,
                                       uint32_t height, uint32_t nregions, uint32_t block, uint32_t expand,
                                       const uint8_t* d_mask, const uint32_t* d_area, uint32_t min_area,
                                       uint32_t* d_offsets, uint32_t cap, uint32_t* d_coords, uint32_t* d_index,
                                       const uint32_t* d_pixels, uint32_t* d_colors, uint32_t k, uint32_t* d_out,
                                       uint32_t* cts, uint32_t* k_outs, int max_iters) {
  const size_t no = (size_t)nregions + 1;
  const bool lists = d_coords || d_index || d_colors;
  int64_t rc = region_windows_on(st, d_regions, width, height, nregions, block, expand, d_mask, d_area, min_area,
                                 d_offsets, lists ? cap : 0u, d_coords, d_index, d_pixels, d_colors);
  if (rc < 0) return rc;
  const int64_t total = rc;
  if (d_out && total > (int64_t)cap) return -4;
  // the colours in list order: the caller's when they were written, else the call's own
  uint32_t *own_offsets = nullptr, *own_colors = nullptr;
  const uint32_t* colors = d_colors;
  if (!(d_colors && total <= (int64_t)cap) && total > 0) {
    DQ_HIP(hipMallocAsync((void**)&own_offsets, no * 4, st));
    DQ_HIP(hipMallocAsync((void**)&own_colors, (size_t)total * 4, st));
    rc = region_windows_on(st, d_regions, width, height, nregions, block, expand, d_mask, d_area, min_area,
                           own_offsets, (uint32_t)total, nullptr, nullptr, d_pixels, own_colors);
    colors = own_colors;
  }
  if (rc >= 0) {
    std::vector<uint32_t> off(no);
    DQ_HIP(hipMemcpyAsync(off.data(), d_offsets, no * 4, hipMemcpyDeviceToHost, st));
    DQ_HIP(hipStreamSynchronize(st));
    rc = quant_ranges_on(device, st, off, nregions, colors, d_out, k, cts, k_outs, max_iters);
  }
  for (void* p : {(void*)own_offsets, (void*)own_colors})
    if (p) DQ_HIP(hipFreeAsync(p, st));
  DQ_HIP(hipStreamSynchronize(st));
  return rc;
}

int64_t dq_hip_quant_region_windows_dev(int device, const uint32_t* d_regions, uint32_t width, uint32_t height,
                                        uint32_t nregions, uint32_t block, uint32_t expand, const uint8_t* d_mask,
                                        const uint32_t* d_area, uint32_t min_area, uint32_t* d_offsets, uint32_t cap,
                                        uint32_t* d_coords, uint32_t* d_index, const uint32_t* d_pixels,
                                        uint32_t* d_colors, uint32_t k, uint32_t* d_out, uint32_t* cts,
                                        uint32_t* k_outs, int max_iters, void* stream) {
  if (!quant_windows_args_ok(d_regions, width, height, nregions, block, expand, d_area, d_offsets, cap, d_coords,
                             d_index, d_pixels, d_colors, k, d_out, cts, k_outs, max_iters))
    return -1;
  hipStream_t st = engine_stream(device, stream);
  return quant_region_windows_on(device, st, d_regions, width, height, nregions, block, expand, d_mask, d_area,
                                 min_area, d_offsets, cap, d_coords, d_index, d_pixels, d_colors, k, d_out, cts, k_outs,
                                 max_iters);
}

int64_t dq_hip_quant_region_windows(const uint32_t* regions, uint32_t width, uint32_t height, uint32_t nregions,
                                    uint32_t block, uint32_t expand, const uint8_t* mask, const uint32_t* area,
                                    uint32_t min_area, uint32_t* offsets, uint32_t cap, uint32_t* coords,
                                    uint32_t* index, const uint32_t* pixels, uint32_t* colors, uint32_t k,
                                    uint32_t* out, uint32_t* cts, uint32_t* k_outs, int max_iters) {
  if (!quant_windows_args_ok(regions, width, height, nregions, block, expand, area, offsets, cap, coords, index,
                             pixels, colors, k, out, cts, k_outs, max_iters))
    return -1;
  const int device = current_device();
  hipStream_t st = engine_for(device).stream();
  const size_t n = (size_t)width * height, no = (size_t)nregions + 1;
  WindowsInputs in;
  in.upload(st, n, nregions, regions, mask, area, pixels);
  uint32_t *d_offsets = nullptr, *d_coords = nullptr, *d_index = nullptr, *d_colors = nullptr, *d_out = nullptr;
  DQ_HIP(hipMallocAsync((void**)&d_offsets, no * 4, st));
  if (cap && coords) DQ_HIP(hipMallocAsync((void**)&d_coords, (size_t)cap * 4, st));
  if (cap && index) DQ_HIP(hipMallocAsync((void**)&d_index, (size_t)cap * 4, st));
  if (cap && colors) DQ_HIP(hipMallocAsync((void**)&d_colors, (size_t)cap * 4, st));
  if (out) DQ_HIP(hipMallocAsync((void**)&d_out, (size_t)std::max<uint32_t>(cap, 1u) * 4, st));
  uint32_t total = 0;
  const int64_t rc = quant_region_windows_on(device, st, in.regions, width, height, nregions, block, expand, in.mask,
                                             in.area, min_area, d_offsets, cap, d_coords, d_index, in.pixels, d_colors,
                                             k, d_out, cts, k_outs, max_iters);
  if (rc >= 0) {   // (a refused call leaves the host arrays as they were)
    DQ_HIP(hipMemcpyAsync(offsets, d_offsets, no * 4, hipMemcpyDeviceToHost, st));
    DQ_HIP(hipMemcpyAsync(&total, d_offsets + nregions, 4, hipMemcpyDeviceToHost, st));
    DQ_HIP(hipStreamSynchronize(st));
    if (total > 0 && total <= cap) {
      if (d_coords) DQ_HIP(hipMemcpyAsync(coords, d_coords, (size_t)total * 4, hipMemcpyDeviceToHost, st));
      if (d_index) DQ_HIP(hipMemcpyAsync(index, d_index, (size_t)total * 4, hipMemcpyDeviceToHost, st));
      if (d_colors) DQ_HIP(hipMemcpyAsync(colors, d_colors, (size_t)total * 4, hipMemcpyDeviceToHost, st));
      if (d_out) DQ_HIP(hipMemcpyAsync(out, d_out, (size_t)total * 4, hipMemcpyDeviceToHost, st));
      DQ_HIP(hipStreamSynchronize(st));
    }
  }
  in.release(st);
  for (void* p : {(void*)d_offsets, (void*)d_coords, (void*)d_index, (void*)d_colors, (void*)d_out})
    if (p) DQ_HIP(hipFreeAsync(p, st));
  return rc;
}

// Window tags (dq_wtags.hip): the windows stage up to the pair positions, then
// the tag histogram of every window from its pairs.  Every argument check comes
// before the first HIP call.
static bool wtags_args_ok(const uint32_t* regions, uint32_t width, uint32_t height, uint32_t nregions, uint32_t block,
                          uint32_t expand, const uint32_t* area, const uint32_t* rows, uint32_t cap,
                          const uint32_t* ids, const uint32_t* counts, const uint32_t* first, const uint32_t* inside,
                          const uint32_t* best, const uint32_t* best_count, const uint32_t* offsets) {
  // (rows stands where the windows call has its offsets: required; the entry arrays are its list arrays)
  if (!windows_args_ok(regions, width, height, nregions, block, expand, area, rows, 0, ids, counts, nullptr, nullptr))
    return false;
  if (cap > 0 && !ids && !counts && !first) return false;
  for (const void* p : {(const void*)first, (const void*)inside, (const void*)best, (const void*)best_count,
                        (const void*)offsets})
    if (((uintptr_t)p & 3u) != 0) return false;
  return true;
}

// Three read-backs with a synchronisation each: P, T and Q (Q sizes the table;
// a map with T > P is refused and -3 is decided there), M (-3; sizes the bitmap)
// and E (do the entries fit), all before any output array is written.
static int64_t window_tags_on(hipStream_t st, const uint32_t* d_regions, uint32_t width, uint32_t height,
                              uint32_t nregions, uint32_t block, uint32_t expand, const uint8_t* d_mask,
                              const uint32_t* d_area, uint32_t min_area, uint32_t* d_rows, uint32_t cap,
                              uint32_t* d_ids, uint32_t* d_counts, uint32_t* d_first, uint32_t* d_inside,
                              uint32_t* d_best, uint32_t* d_best_count, uint32_t* d_offsets) {
  const size_t no = (size_t)nregions + 1;
  uint32_t *own_offsets = nullptr, *pair_ids = nullptr;
  dq::WindowsArgs a{d_regions, width,   height,  nregions, block,   expand,  d_mask,  d_area,
                    min_area,  nullptr, nullptr, nullptr,  nullptr, nullptr, nullptr, nullptr};
  DQ_HIP(hipMallocAsync((void**)&a.blocks, dq::windows_blocks_bytes(width, height, block, nregions), st));
  dq::WindowsView v = dq::windows_view(a, 0);   // (what the first part leaves: the pairs come later)
  dq::WtagsArgs t{};
  t.regions = d_regions, t.width = width, t.height = height, t.nregions = nregions, t.block = block;
  t.mask = d_mask, t.nblocks = v.nblocks, t.pairbase = v.pairbase;
  t.rows = d_rows, t.ids = d_ids, t.counts = d_counts, t.first = d_first;
  t.inside = d_inside, t.best = d_best, t.best_count = d_best_count;
  DQ_HIP(hipMallocAsync((void**)&t.live, dq::wtags_live_bytes(v.nblocks), st));
  dq::launch_windows_blocks(a, st);
  dq::launch_wtags_count(t, st);   // (the members of every block are counted by then: Q needs no pair)
  DQ_HIP(hipGetLastError());
  uint32_t npairs = 0, nrows = 0, total = 0, ncontribs = 0, nentries = 0;
  DQ_HIP(hipMemcpyAsync(&npairs, dq::windows_pairs_word(a), 4, hipMemcpyDeviceToHost, st));
  DQ_HIP(hipMemcpyAsync(&nrows, dq::windows_rows_word(a), 4, hipMemcpyDeviceToHost, st));
  DQ_HIP(hipMemcpyAsync(&ncontribs, dq::wtags_contribs_word(t), 4, hipMemcpyDeviceToHost, st));
  DQ_HIP(hipStreamSynchronize(st));
  int64_t rc;
  if (npairs == 0xFFFFFFFFu || ncontribs == 0xFFFFFFFFu) {
    rc = -3;
  } else if (nrows > npairs) {
    rc = -2;
  } else {
    DQ_HIP(hipMallocAsync((void**)&a.pairs, dq::windows_pairs_bytes(npairs, nrows), st));
    if (npairs != 0 && nrows != 0) {
      dq::launch_windows_count(a, npairs, nrows, st);
      DQ_HIP(hipGetLastError());
      DQ_HIP(hipMemcpyAsync(&total, dq::windows_total_word(a, npairs, nrows), 4, hipMemcpyDeviceToHost, st));
      DQ_HIP(hipStreamSynchronize(st));
    } else {
      ncontribs = 0;   // (no pair, no contribution)
    }
    if (total == 0xFFFFFFFFu) {
      rc = -3;
    } else {
      v = dq::windows_view(a, npairs);
      if (ncontribs != 0) {
        // the member ids of the pairs: the walk below turns the windows stage's into positions
        DQ_HIP(hipMallocAsync((void**)&pair_ids, (size_t)npairs * 4, st));
        DQ_HIP(hipMemcpyAsync(pair_ids, v.pair_word, (size_t)npairs * 4, hipMemcpyDeviceToDevice, st));
      }
      t.pair_id = pair_ids, t.pair_pos = v.pair_word, t.npairs = npairs, t.total = total;
      a.offsets = d_offsets;
      if (!a.offsets) {
        DQ_HIP(hipMallocAsync((void**)&own_offsets, no * 4, st));
        a.offsets = own_offsets;
      }
      t.offsets = a.offsets;
      dq::launch_windows_offsets(a, npairs, nrows, total, st);
      if (ncontribs != 0) dq::launch_windows_walk(a, npairs, nrows, st);
      DQ_HIP(hipMallocAsync((void**)&t.table, dq::wtags_table_bytes(ncontribs, total, nregions), st));
      dq::launch_wtags_fill(t, ncontribs, st);
      DQ_HIP(hipGetLastError());
      DQ_HIP(hipMemcpyAsync(&nentries, dq::wtags_entries_word(t, ncontribs), 4, hipMemcpyDeviceToHost, st));
      DQ_HIP(hipStreamSynchronize(st));
      rc = nentries;
      dq::launch_wtags_rows(t, ncontribs, st);
      if (nentries <= cap) dq::launch_wtags_entries(t, ncontribs, nentries, st);
      DQ_HIP(hipGetLastError());
      DQ_HIP(hipFreeAsync(t.table, st));
    }
    for (void* p : {(void*)pair_ids, (void*)own_offsets, (void*)a.pairs})
      if (p) DQ_HIP(hipFreeAsync(p, st));
  }
  DQ_HIP(hipFreeAsync(t.live, st));
  DQ_HIP(hipFreeAsync(a.blocks, st));
  DQ_HIP(hipStreamSynchronize(st));
  return rc;
}

int64_t dq_hip_window_tags_dev(int device, const uint32_t* d_regions, uint32_t width, uint32_t height,
                               uint32_t nregions, uint32_t block, uint32_t expand, const uint8_t* d_mask,
                               const uint32_t* d_area, uint32_t min_area, uint32_t* d_rows, uint32_t cap,
                               uint32_t* d_ids, uint32_t* d_counts, uint32_t* d_first, uint32_t* d_inside,
                               uint32_t* d_best, uint32_t* d_best_count, uint32_t* d_offsets, void* stream) {
  if (!wtags_args_ok(d_regions, width, height, nregions, block, expand, d_area, d_rows, cap, d_ids, d_counts, d_first,
                     d_inside, d_best, d_best_count, d_offsets))
    return -1;
  // (no engine state is touched: calls on two streams may overlap)
  hipStream_t st = engine_stream(device, stream);
  return window_tags_on(st, d_regions, width, height, nregions, block, expand, d_mask, d_area, min_area, d_rows, cap,
                        d_ids, d_counts, d_first, d_inside, d_best, d_best_count, d_offsets);
}

int64_t dq_hip_window_tags(const uint32_t* regions, uint32_t width, uint32_t height, uint32_t nregions, uint32_t block,
                           uint32_t expand, const uint8_t* mask, const uint32_t* area, uint32_t min_area,
                           uint32_t* rows, uint32_t cap, uint32_t* ids, uint32_t* counts, uint32_t* first,
                           uint32_t* inside, uint32_t* best, uint32_t* best_count, uint32_t* offsets) {
  if (!wtags_args_ok(regions, width, height, nregions, block, expand, area, rows, cap, ids, counts, first, inside, best,
                     best_count, offsets))
    return -1;
  Engine& e = engine_for(current_device());
  hipStream_t st = e.stream();
  const size_t n = (size_t)width * height, no = (size_t)nregions + 1;
  WindowsInputs in;
  in.upload(st, n, nregions, regions, mask, area, nullptr);
  // the device twins of the host arrays given: rows | offsets, the three entry arrays, the three per region
  uint32_t* const host[8] = {rows, offsets, ids, counts, first, inside, best, best_count};
  const size_t words[8] = {no, no, cap, cap, cap, nregions, nregions, nregions};
  uint32_t* dev[8] = {};
  for (int i = 0; i < 8; ++i)
    if (host[i] && words[i]) DQ_HIP(hipMallocAsync((void**)&dev[i], words[i] * 4, st));
  const int64_t rc = window_tags_on(st, in.regions, width, height, nregions, block, expand, in.mask, in.area, min_area,
                                    dev[0], cap, dev[2], dev[3], dev[4], dev[5], dev[6], dev[7], dev[1]);
  if (rc >= 0) {   // (a refused map leaves the host arrays as they were)
    for (int i = 0; i < 8; ++i) {
      const bool entries = i >= 2 && i <= 4;
      if (!dev[i] || (entries && (rc == 0 || rc > (int64_t)cap))) continue;
      DQ_HIP(hipMemcpyAsync(host[i], dev[i], (entries ? (size_t)rc : words[i]) * 4, hipMemcpyDeviceToHost, st));
    }
    DQ_HIP(hipStreamSynchronize(st));
  }
  in.release(st);
  for (uint32_t* p : dev)
    if (p) DQ_HIP(hipFreeAsync(p, st));
  return rc;
}

// Window votes (dq_wtags.hip).  There is no host-pointer twin: the call consumes
// device arrays that only the device pipeline produces.
int64_t dq_hip_window_votes_dev(int device, const uint32_t* d_regions, uint32_t n, uint32_t nregions,
                                const uint32_t* d_offsets, const uint32_t* d_index, uint32_t total,
                                const uint32_t* d_mapped, const uint32_t* cts, const uint32_t* k_outs, uint32_t k,
                                uint32_t* d_votes, uint32_t* d_best, void* stream) {
  if (!d_regions || !d_offsets || !cts || !k_outs || !d_votes || !d_best) return -1;
  if (total > 0 && (!d_index || !d_mapped)) return -1;
  if (n == 0 || n > 0x7FFFFFFFu || nregions == 0 || nregions > 0x7FFFFFFFu || k < 1 || k > dq::kVotesMaxK) return -1;
  if (total == 0xFFFFFFFFu) return -1;   // (the windows call gives such an M up)
  for (const void* p : {(const void*)d_regions, (const void*)d_offsets, (const void*)d_index, (const void*)d_mapped,
                        (const void*)cts, (const void*)k_outs, (const void*)d_votes, (const void*)d_best})
    if (((uintptr_t)p & 3u) != 0) return -1;
  hipStream_t st = engine_stream(device, stream);
  const size_t table = (size_t)nregions * k;
  uint32_t *d_cts = nullptr, *d_kouts = nullptr;
  dq::WvotesArgs a{d_regions, n, nregions, d_offsets, d_index, d_mapped, total, k, nullptr, nullptr, nullptr, d_votes,
                   d_best};
  DQ_HIP(hipMallocAsync((void**)&d_cts, table * 4, st));
  DQ_HIP(hipMallocAsync((void**)&d_kouts, (size_t)nregions * 4, st));
  DQ_HIP(hipMallocAsync((void**)&a.jobs, dq::wvotes_jobs_bytes(nregions), st));
  DQ_HIP(hipMemcpyAsync(d_cts, cts, table * 4, hipMemcpyHostToDevice, st));
  DQ_HIP(hipMemcpyAsync(d_kouts, k_outs, (size_t)nregions * 4, hipMemcpyHostToDevice, st));
  a.cts = d_cts, a.k_outs = d_kouts;
  dq::launch_wvotes(a, st);
  DQ_HIP(hipGetLastError());
  unsigned long long misses = 0;
  DQ_HIP(hipMemcpyAsync(&misses, dq::wvotes_misses_word(a), 8, hipMemcpyDeviceToHost, st));
  for (void* p : {(void*)d_cts, (void*)d_kouts, (void*)a.jobs})
    DQ_HIP(hipFreeAsync(p, st));
  DQ_HIP(hipStreamSynchronize(st));
  return (int64_t)misses;
}

// Synthetic frames of the benchmark configs (SURVEY 8c/8d generator) and the
// output checksum the golden fixtures are keyed by.
void dq_synth_xorshift(uint32_t* out, uint64_t n, uint64_t seed) {
  uint64_t s = seed;
  for (uint64_t i = 0; i < n; ++i) {
    s ^= s << 13;
    s ^= s >> 7;
    s ^= s << 17;
    out[i] = (uint32_t)(s & 0xFFFFFFu);
  }
}

uint64_t dq_fnv1a64(const uint32_t* w, uint64_t n) {
  uint64_t h = 0xcbf29ce484222325ull;
  for (uint64_t i = 0; i < n; ++i) {
    h ^= w[i];
    h *= 0x100000001b3ull;
  }
  return h;
}

void dq_subdivided_colors(uint32_t* out125) {
  static const uint32_t v[5] = {0, 63, 127, 191, 255};
  for (int i = 0; i < 125; ++i)   // R outermost, B innermost, alpha 0xFF (:874-888)
    out125[i] = 0xFF000000u | (v[i / 25] << 16) | (v[i / 5 % 5] << 8) | v[i % 5];
}

int dq_hip_block_hist(const uint32_t* in, uint32_t width, uint32_t height, const uint32_t* palette,
                      int npal, uint32_t dim, uint32_t block_w, uint32_t block_h, uint32_t* quant,
                      uint32_t* mode, uint32_t* ndistinct, uint32_t* keys, uint32_t* counts) {
  if (!in || !palette || npal <= 0 || !mode || (!keys) != (!counts) ||
      !block_hist_shape_ok(width, height, dim, block_w, block_h))
    return -1;
  const int dev = current_device();
  Engine& e = engine_for(dev);
  hipStream_t st = e.stream();
  const size_t n = (size_t)width * height, nb = (size_t)block_w * block_h, cap = (size_t)dim * dim;
  uint32_t *d_mode = nullptr, *d_nd = nullptr, *d_keys = nullptr, *d_counts = nullptr;
  DQ_HIP(hipMallocAsync((void**)&d_mode, nb * 4, st));
  if (ndistinct) DQ_HIP(hipMallocAsync((void**)&d_nd, nb * 4, st));
  if (keys) {
    DQ_HIP(hipMallocAsync((void**)&d_keys, nb * cap * 4, st));
    DQ_HIP(hipMallocAsync((void**)&d_counts, nb * cap * 4, st));
    DQ_HIP(hipMemsetAsync(d_keys, 0, nb * cap * 4, st));
    DQ_HIP(hipMemsetAsync(d_counts, 0, nb * cap * 4, st));
  }
  int rc;
  {
    std::lock_guard<std::mutex> g(e.mutex());
    e.stage_in(in, (uint32_t)n, st);
    e.map(e.staged_in(), (uint32_t)n, e.staged_out(), palette, npal, st);
    uint32_t* work = nullptr;
    DQ_HIP(hipMallocAsync((void**)&work, dq::block_hist_scratch_words(block_w, block_h) * 4, st));
    dq::BlockHistArgs a{e.staged_out(), width, height, block_w, block_h, d_mode, d_nd, d_keys, d_counts,
                        work, nullptr, 0};
    rc = dq::launch_block_hist(a, (int)dim, st);
    DQ_HIP(hipFreeAsync(work, st));
    if (quant) DQ_HIP(hipMemcpyAsync(quant, e.staged_out(), n * 4, hipMemcpyDeviceToHost, st));
    DQ_HIP(hipMemcpyAsync(mode, d_mode, nb * 4, hipMemcpyDeviceToHost, st));
    if (ndistinct) DQ_HIP(hipMemcpyAsync(ndistinct, d_nd, nb * 4, hipMemcpyDeviceToHost, st));
    if (keys) {
      DQ_HIP(hipMemcpyAsync(keys, d_keys, nb * cap * 4, hipMemcpyDeviceToHost, st));
      DQ_HIP(hipMemcpyAsync(counts, d_counts, nb * cap * 4, hipMemcpyDeviceToHost, st));
    }
    DQ_HIP(hipStreamSynchronize(st));
  }
  for (uint32_t* p : {d_mode, d_nd, d_keys, d_counts})
    if (p) DQ_HIP(hipFreeAsync(p, st));
  return rc;
}

int dq_hip_last_centroids(int device, double* means, int64_t* sizes, int k) {
  Engine& e = engine_for(device);
  std::lock_guard<std::mutex> g(e.mutex());
  if ((size_t)k != e.last_sizes.size()) return -1;
  if (means) std::memcpy(means, e.last_means.data(), sizeof(double) * 3 * k);
  if (sizes) std::memcpy(sizes, e.last_sizes.data(), sizeof(int64_t) * k);
  return 0;
}

int dq_hip_last_trace(int device, int64_t* trace, int k) {
  Engine& e = engine_for(device);
  std::lock_guard<std::mutex> g(e.mutex());
  if (k < 1 || (size_t)(k - 1) * 4 != e.last_trace.size()) return -1;
  if (trace && k > 1) std::memcpy(trace, e.last_trace.data(), sizeof(int64_t) * 4 * (k - 1));
  return 0;
}

int dq_hip_last_rounds(int device) { return engine_for(device).last_rounds; }

uint64_t dq_hip_last_points_swept(int device) { return engine_for(device).last_points_swept; }
uint64_t dq_hip_last_points_full(int device) { return engine_for(device).last_points_full; }
uint64_t dq_hip_last_seq_tiles(int device) { return engine_for(device).last_seq_tiles; }
uint64_t dq_hip_last_cursor_fixes(int device) { return engine_for(device).last_cursor_fixes; }

int dq_hip_last_wsmall_profile(int device, uint64_t* out, int nout) {
  const std::vector<uint64_t>& p = engine_for(device).last_wsmall_prof;
  const int n = std::min<int>(nout, (int)p.size());
  for (int i = 0; i < n; ++i) out[i] = p[i];
  return n;
}
void dq_hip_set_fixed_point(int device, int on) { engine_for(device).set_fixed_point(on != 0); }
void dq_hip_set_planned_rounds(int device, int on) {
  for (int l = 0; l < dq::kMaxLanes; ++l) engine_for(device, l).set_plan(on != 0);
}
int dq_hip_last_planned_rounds(int device) { return engine_for(device).last_planned; }

void dq_hip_set_loop_max(int device, uint32_t max_points) {
  for (int l = 0; l < dq::kMaxLanes; ++l) engine_for(device, l).set_loop_max(max_points);
}

int dq_hip_last_loop_rounds(int device) { return engine_for(device).last_loop_rounds; }

void dq_hip_set_persist(int device, int on) {
  for (int l = 0; l < dq::kMaxLanes; ++l) engine_for(device, l).set_persist(on != 0);
}

int dq_hip_last_persist_rounds(int device) { return engine_for(device).last_persist_rounds; }

void dq_hip_set_wsmall(int device, int on) {
  for (int l = 0; l < dq::kMaxLanes; ++l) engine_for(device, l).set_wsmall(on != 0);
}

void dq_hip_set_lds_map(int device, int on) {
  for (int l = 0; l < dq::kMaxLanes; ++l) engine_for(device, l).set_lds_map(on != 0);
}

void dq_hip_set_timing(int device, int on) { engine_for(device).set_timing(on != 0); }

void dq_hip_set_debug(int device, int flags) {
  (void)device;   // (process-wide: every engine reads it when a run starts)
  dq::set_debug_flags(flags);
}

void dq_hip_set_lanes(int lanes) { dq::set_batch_lanes(lanes); }
int dq_hip_get_lanes(void) { return dq::batch_lanes(); }

void dq_hip_reset_stats(int device) { engine_for(device).reset_stats(); }

int dq_hip_get_stat(int device, int kind, uint64_t* launches, double* ms, double* bytes) {
  if (kind < 0 || kind >= dq::ST_COUNT) return -1;
  const dq::KernelStat& s = engine_for(device).stats[kind];
  if (launches) *launches = s.launches;
  if (ms) *ms = s.ms;
  if (bytes) *bytes = s.bytes;
  return 0;
}

int dq_hip_get_stat_units(int device, int kind, double* units) {
  if (kind < 0 || kind >= dq::ST_COUNT) return -1;
  if (units) *units = engine_for(device).stats[kind].units;
  return 0;
}

const char* dq_hip_stat_name(int kind) {
  static const char* names[] = {"pass_init", "pass_split", "pass_kmeans", "pass_klast",
                                "epilogue", "partition", "map_cells", "map", "plan", "kloop"};
  if (kind < 0 || kind >= dq::ST_COUNT) return "";
  return names[kind];
}

// =========================================================================
// Reference signatures (include/quant_util.h, include/DivQuantHeader.h)
// =========================================================================

// quant_util.cpp:20-158.
void quant_recurse(uint32_t numPixels, const uint32_t* inPixelsPtr, uint32_t* outPixelsPtr,
                   uint32_t* numClustersPtr, uint32_t* outColortablePtr, int allPixelsUnique) {
  if (numPixels == 0 || *numClustersPtr == 0)
    dq::die("quant_recurse", __FILE__, __LINE__, "numPixels and *numClustersPtr must be > 0");
  Engine& e = engine_for(current_device());
  std::lock_guard<std::mutex> g(e.mutex());
  hipStream_t st = e.stream();
  // the reference's timing lines (quant_util.cpp:48-66, 141-145): clock()
  // CPU time of this process from t1, the map line cumulative from t1 too
  const clock_t t1 = clock();
  e.stage_in(inPixelsPtr, numPixels, st);
  dq::FrameJob j;
  j.d_in = e.staged_in();
  j.n = numPixels;
  j.k = (int)*numClustersPtr;
  j.ct = outColortablePtr;
  if (allPixelsUnique) e.run(&j, 1, 10, false, st);   // uniform weights (:1130-1132)
  else e.run_weighted(j, 10, false, st);               // calc_color_table + weighted (:1133-1138)
  report_empty(j.num_empty);
  uint32_t k = (uint32_t)j.k_out;
  *numClustersPtr = k;
  clock_t t2 = clock();
  if (!quiet()) {
    const long el = timediff(t1, t2);
    std::printf("quant_varpart_fast() elapsed: %ld ms aka %0.2f s\n", el, el / 1000.0f);
  }
  std::vector<uint32_t> scratch;
  k = (uint32_t)dq::dedup_colortable(outColortablePtr, (int)k, scratch);
  *numClustersPtr = k;
  e.map(e.staged_in(), numPixels, e.staged_out(), outColortablePtr, (int)k, st);
  DQ_HIP(hipMemcpyAsync(outPixelsPtr, e.staged_out(), (size_t)numPixels * 4,
                        hipMemcpyDeviceToHost, st));
  DQ_HIP(hipStreamSynchronize(st));
  t2 = clock();
  if (!quiet()) {
    const long el = timediff(t1, t2);
    std::printf("map_colors_mps() elapsed: %ld ms aka %0.2f s\n", el, el / 1000.0f);
  }
}

}  // extern "C"

// DivQuantMapColors.cpp:243-539.
void map_colors_mps(const uint32_t* inPixelsPtr, uint32_t numPixels, uint32_t* outPixelsPtr,
                    uint32_t* outColortablePtr, int colormapSize) {
  if (colormapSize <= 0)
    dq::die("map_colors_mps", __FILE__, __LINE__, "colormapSize must be > 0");
  dq_hip_map(inPixelsPtr, numPixels, outPixelsPtr, outColortablePtr, colormapSize);
}

// DivQuantCluster.cpp:1099-1179.
void quant_varpart_fast(const uint32_t numPixels, const uint32_t* inPixels, uint32_t* tmpPixels,
                        const uint32_t numRows, const uint32_t numCols, uint32_t* numClustersPtr,
                        uint32_t* colortablePtr, const int num_bits, const int dec_factor,
                        const int max_iters, const int allPixelsUnique) {
  (void)tmpPixels;
  if (!validate_num_bits((uchar)num_bits))   // (:1115-1118 asserts)
    dq::die("quant_varpart_fast", __FILE__, __LINE__, "invalid num_bits");
  if (dec_factor <= 0)   // calc_color_table's message (:103-108); the reference then runs on garbage
    dq::die("quant_varpart_fast", __FILE__, __LINE__, "Decimation factor should be positive");
  if (max_iters < 1)
    dq::die("quant_varpart_fast", __FILE__, __LINE__, "max_iters < 1 is not supported");
  Engine& e = engine_for(current_device());
  std::lock_guard<std::mutex> g(e.mutex());
  hipStream_t st = e.stream();
  e.stage_in(inPixels, numPixels, st);
  dq::FrameJob j;
  j.d_in = e.staged_in();
  j.n = numPixels;
  j.k = (int)*numClustersPtr;
  j.ct = colortablePtr;
  j.num_bits = num_bits;
  j.dec = dec_factor;
  j.rows = numRows;
  j.cols = numCols;
  // uniform weights only for unique 8-bit undecimated input (:1130-1132);
  // else calc_color_table (after cut_bits unless !unique && 8 bits, :1133-1146)
  if (allPixelsUnique && num_bits == 8 && dec_factor == 1) {
    e.run(&j, 1, max_iters, false, st);
  } else {
    if (numRows == 0 || numCols == 0)   // calc_color_table visits no pixel; DivQuantCluster asserts (:211)
      dq::die("quant_varpart_fast", __FILE__, __LINE__, "numRows and numCols must be > 0 for calc_color_table");
    e.run_weighted(j, max_iters, false, st);
  }
  report_empty(j.num_empty);
  const int k = j.k_out;
  *numClustersPtr = (uint32_t)k;
}

// DivQuantMapColors.cpp:205-220.
double get_double_scale(const uint32_t* inPixels, const uint32_t numPixels) {
  (void)inPixels;
  const int numRows = 1, dec = 1;
  const int numCols = (int)numPixels;
  return 1.0 / (ceil(numRows / (double)dec) * ceil(numCols / (double)dec));
}

// DivQuantMapColors.cpp:43-51.
void check_mem(const int x) {
  if (x != 0) {
    std::fprintf(stderr, "Insufficient memory !\n");
    std::abort();
  }
}

// DivQuantMisc.cpp:18-46.
clock_t start_timer(void) { return clock(); }
double stop_timer(const clock_t start_time) {
  return ((double)(clock() - start_time)) / CLOCKS_PER_SEC;
}
long timediff(clock_t t1, clock_t t2) {
  return (long)(((double)t2 - t1) / CLOCKS_PER_SEC * 1000);
}
int validate_num_bits(const uchar num_bits) {
  if (!(0 < num_bits && num_bits <= 8)) {
    std::fprintf(stderr, "Number of bits per channel ( %d ) must be in [1,8] !\n", num_bits);
    return 0;
  }
  return 1;
}

// DivQuantUni.cpp:28-100: drop the low (8 - num_bits) bits of each channel
// and shift the rest down (in place allowed).
void cut_bits(const uint32_t* inPixels, const uint32_t numPixels, uint32_t* outPixels,
              const uchar num_bits_red, const uchar num_bits_green, const uchar num_bits_blue) {
  if (!validate_num_bits(num_bits_red) || !validate_num_bits(num_bits_green) ||
      !validate_num_bits(num_bits_blue))
    return;
  const uint32_t sr = 8 - num_bits_red, sg = 8 - num_bits_green, sb = 8 - num_bits_blue;
  for (uint32_t i = 0; i < numPixels; ++i) {
    const uint32_t p = inPixels[i];
    const uint32_t R = ((p >> 16) & 0xFF) >> sr;
    const uint32_t G = ((p >> 8) & 0xFF) >> sg;
    const uint32_t B = (p & 0xFF) >> sb;
    outPixels[i] = (R << 16) | (G << 8) | B;
  }
}

// DivQuantMapColors.cpp:82-203 on the device (dq_weighted.hip's colour
// table, the weighted path's own): unique colours with weights count*norm in
// the reference's output order -- hash buckets ascending (HASH(R,G,B) =
// (R*33023 + G*30013 + B*27011) & 0x7fffffff) % 20023), and inside a bucket
// the most recently first-seen colour first (the chains are prepended).  The
// pixel index quirk inPixels[ic + ir*numRows] is kept (:124); numPixels is
// not read, as in the reference.
double* calc_color_table(const uint32_t* inPixels, const uint32_t numPixels, uint32_t* outPixels,
                         const uint32_t numRows, const uint32_t numCols, const int dec_factor,
                         int* num_colors) {
  (void)numPixels;
  if (dec_factor <= 0) {
    std::fprintf(stderr, "Decimation factor ( %d ) should be positive !\n", dec_factor);
    return NULL;
  }
  const uint64_t nr = (numRows + (uint64_t)dec_factor - 1) / dec_factor;
  const uint64_t nc = (numCols + (uint64_t)dec_factor - 1) / dec_factor;
  double* weights = new double[std::max<uint64_t>(1, nr * nc)];
  Engine& e = engine_for(current_device());
  std::lock_guard<std::mutex> g(e.mutex());
  *num_colors = (int)e.color_table(inPixels, numRows, numCols, (uint32_t)dec_factor, outPixels, weights, e.stream());
  return weights;
}
