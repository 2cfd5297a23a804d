// nlsolver_amd/csrc/nlsg_engine.h — the host skeleton every engine file (nlsg_*.hip) shares: who owns
// the device blocks, streams and events of an engine or of one call, the fields and calls every
// `struct nlsg_X` has in common, the event-timed repeat loop and the create clock. Host only: no
// kernel header includes it and the run-time compiler never sees it. (Which kernel instantiation a
// launch site picks from run-time values: nlsg_dispatch.h, and `routed` below.)
#pragma once
#ifndef __HIPCC_RTC__
#include <new>
#include <vector>

#include "nlsg_common.h"
#include "nlsg_dispatch.h"

// (host plumbing of the translation units, not part of what libnlsolver_hip.so exports)
#pragma GCC visibility push(hidden)
namespace nlsg {

// Owner of pool blocks, pooled streams and events on one device. Setup calls chain on the sticky
// `err`: once it is set, alloc / zeroed / event / stream do nothing, and an engine's own setup steps
// join the chain as `if (he == hipSuccess) he = ...` on a reference to it. release() hands everything
// back in the order every destroy needs: the streams drained first (pool_free does not synchronise the
// way hipFree does: nothing may be in flight), then the blocks, the events, the pooled streams.
class DeviceOwner {
 public:
  int device = 0;
  hipError_t err = hipSuccess;

  DeviceOwner() = default;
  explicit DeviceOwner(int dev) : device(dev) {}
  DeviceOwner(const DeviceOwner &) = delete;
  DeviceOwner &operator=(const DeviceOwner &) = delete;
  ~DeviceOwner() { release(); }

  bool ok() const { return err == hipSuccess; }

  // pool_malloc outside the chain (a block an entry point adds later); the owner frees it all the same
  template <typename T>
  hipError_t take(T **ptr, size_t bytes) {
    void *p = nullptr;
    const hipError_t he = pool_malloc(&p, bytes);
    if (p) {  // (a block whose poison fill failed is the pool's all the same)
      *ptr = static_cast<T *>(p);
      blocks_.push_back(p);
    }
    return he;
  }
  template <typename T>
  void alloc(T **ptr, size_t bytes) {
    if (ok()) err = take(ptr, bytes);
  }
  template <typename T>
  void zeroed(T **ptr, size_t bytes) {
    alloc(ptr, bytes);
    if (ok()) err = hipMemset(*ptr, 0, bytes);
  }
  void event(hipEvent_t *ev, unsigned flags = hipEventDefault) {
    if (!ok()) return;
    err = hipEventCreateWithFlags(ev, flags);
    if (ok()) events_.push_back(*ev);
  }
  // a non-blocking stream from the pool, returned to it at release
  void stream(hipStream_t *s) {
    if (!ok()) return;
    err = pool_stream_get(s);
    if (ok()) pooled_.push_back(*s);
  }
  // somebody else's stream that work on the owner's blocks is queued on (the null stream included):
  // drained at release, not returned
  void watch(hipStream_t s) { watched_.push_back(s); }
  void reserve(size_t blocks) { blocks_.reserve(blocks); }
  // every stream the owner knows about is idle afterwards
  void drain() {
    hipSetDevice(device);
    for (hipStream_t s : pooled_) hipStreamSynchronize(s);
    for (hipStream_t s : watched_) hipStreamSynchronize(s);
  }
  void release() {
    if (blocks_.empty() && events_.empty() && pooled_.empty()) return;
    drain();
    give_back();
  }
  // release() for a caller that has just drained the streams itself and queued nothing since
  void give_back() {
    for (void *p : blocks_) pool_free(p);
    for (hipEvent_t ev : events_) hipEventDestroy(ev);
    for (hipStream_t s : pooled_) pool_stream_put(device, s);
    blocks_.clear();
    events_.clear();
    pooled_.clear();
    watched_.clear();
  }

 private:
  std::vector<void *> blocks_;
  std::vector<hipEvent_t> events_;
  std::vector<hipStream_t> pooled_, watched_;
};

// What every `struct nlsg_X` starts from. Create: open_engine(), the engine's blocks through `own`,
// setup_status(). Destroy lists only what is engine-specific (a run-time compiled module, a
// communicator) between drain() and close(); everything `own` handed out goes back in close().
// close() does not drain again: nothing is queued between the two.
struct EngineBase {
  DeviceOwner own;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;  // the pair around a timed interval (time_repeats)
  int32_t n_params = 0;          // the objective's run-time doubles per problem (0: none)
  double *params_dev = nullptr;  // [batch][n_params]
  bool params_set = false;

  // is `device` a gfx950 this process can see? then the caller's stream, or one from the pool
  int open(int device, void *stream_handle) {
    if (const int rc = check_device(device)) return rc;
    NLSG_HIP(hipSetDevice(device));
    own.device = device;
    own.reserve(24);  // (most engines take a dozen blocks or two: one host allocation for the list)
    if (stream_handle) {
      stream = borrowed_stream(stream_handle);
      own.watch(stream);
      return NLSG_OK;
    }
    own.stream(&stream);
    if (!own.ok()) return fail(NLSG_ERR_HIP, "hipStreamCreate failed: %s", hipGetErrorString(own.err));
    own_stream = true;
    return NLSG_OK;
  }
  // the timing pair, last in every engine's chain of blocks
  void timing_events() {
    own.event(&ev0);
    own.event(&ev1);
  }
  int setup_status(const char *format = "device setup failed: %s") const {
    if (own.ok()) return NLSG_OK;
    return fail(own.err == hipErrorOutOfMemory ? NLSG_ERR_OOM : NLSG_ERR_HIP, format, hipGetErrorString(own.err));
  }
  void alloc_params(uint64_t batch, int32_t n) {
    n_params = n;
    if (n) own.alloc(&params_dev, batch * static_cast<uint64_t>(n) * 8);
  }
  int set_params(uint64_t batch, const double *params_host, const char *no_params_message) {
    if (n_params <= 0) return fail(NLSG_ERR_INVALID_ARG, "%s", no_params_message);
    NLSG_HIP(hipSetDevice(own.device));
    NLSG_HIP(hipMemcpyAsync(params_dev, params_host, batch * static_cast<uint64_t>(n_params) * 8,
                            hipMemcpyHostToDevice, stream));
    NLSG_HIP(hipStreamSynchronize(stream));  // the host buffer is borrowed for this call only
    params_set = true;
    return NLSG_OK;
  }
  // a parametrised engine launches nothing before its first rows; `message_format` takes n_params (%d)
  int params_ready(const char *message_format) const {
    if (n_params > 0 && !params_set) return fail(NLSG_ERR_STATE, message_format, n_params);
    return NLSG_OK;
  }
  void drain() { own.drain(); }
  void close() { own.give_back(); }
};

// What a launch site does with the answer of its with_*(...) selection (nlsg_dispatch.h): a value no
// list holds launched nothing, and the entry point's launches_status() reports hipErrorInvalidValue.
inline void routed(bool matched) {
  if (!matched && module_launch_error() == hipSuccess) module_launch_error() = hipErrorInvalidValue;
}

// `new` and open() for an engine struct; nothing to clean up when it fails
template <typename E>
int open_engine(int device, void *stream_handle, E **out) {
  E *e = new (std::nothrow) E();
  if (!e) return fail(NLSG_ERR_OOM, "host allocation failed");
  if (const int rc = e->open(device, stream_handle)) {
    delete e;
    return rc;
  }
  *out = e;
  return NLSG_OK;
}

// `repeats` intervals, each bracketed by ev0 / ev1 on `stream` and added up in milliseconds.
// per_repeat() is what is timed; before() runs ahead of each interval, outside it (re-uploading a
// start point). Both return an NLSG_* code, which ends the measurement.
template <typename Run, typename Before>
int time_repeats(hipStream_t stream, hipEvent_t ev0, hipEvent_t ev1, uint32_t repeats, float *ms_total,
                 Run per_repeat, Before before) {
  float total = 0.f;
  for (uint32_t r = 0; r < repeats; r++) {
    if (const int rc = before()) return rc;
    NLSG_HIP(hipEventRecord(ev0, stream));
    if (const int rc = per_repeat()) return rc;
    NLSG_HIP(hipEventRecord(ev1, stream));
    NLSG_HIP(hipEventSynchronize(ev1));
    NLSG_HIP(launches_status());
    float ms = 0.f;
    NLSG_HIP(hipEventElapsedTime(&ms, ev0, ev1));
    total += ms;
  }
  *ms_total = total;
  return NLSG_OK;
}
template <typename Run>
int time_repeats(hipStream_t stream, hipEvent_t ev0, hipEvent_t ev1, uint32_t repeats, float *ms_total,
                 Run per_repeat) {
  return time_repeats(stream, ev0, ev1, repeats, ms_total, per_repeat, [] { return NLSG_OK; });
}

// nlsg_call_timing's create_ms around an engine's create
template <typename Create>
int timed_create(Create create) {
  PhaseClock clk;
  const int rc = create();
  call_timing().create_ms = clk.lap();
  return rc;
}

}  // namespace nlsg
#pragma GCC visibility pop
#endif  // !__HIPCC_RTC__
