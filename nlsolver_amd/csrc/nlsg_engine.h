// nlsolver_amd/csrc/nlsg_engine.h — the host skeleton every engine file (nlsg_*.hip) shares: who owns
// the device blocks, streams and events of an engine or of one call, the fields and calls every
// `struct nlsg_X` has in common, the front doors of a create, its guard and the destroy, the status
// rows, the one-launch solve, the event-timed repeat loop and the create clock. Host only: no
// kernel header includes it and the run-time compiler never sees it. (Which kernel instantiation a
// launch site picks from run-time values: nlsg_dispatch.h, and `routed` below.)
#pragma once
#ifndef __HIPCC_RTC__
#include <new>
#include <vector>

#include "nlsg_common.h"
#include "nlsg_dispatch.h"
#include "nlsg_rtc.h"

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

// What every `struct nlsg_X` starts from. Create: its front door, open_engine() under a CreateGuard, the
// engine's blocks through `own`, setup_status(). Destroy is destroy_engine(): drain(), what only that
// engine has (a communicator), the run-time compiled module, close(); everything `own` handed out goes
// back in close(). close() does not drain again: nothing is queued between the two.
struct EngineBase {
  const char *api = "";  // "nlsg_nm", "nlsg_de_batch": the prefix of the engine's entry points, in its errors
  DeviceOwner own;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;  // the pair around a timed interval (time_repeats)
  int32_t n_params = 0;          // the objective's run-time doubles per problem (0: none)
  uint64_t params_rows = 0;      // problems: a row of n_params each
  double *params_dev = nullptr;  // [params_rows][n_params]
  bool params_set = false;
  // what the two calls below say; both take `api` (the resident pair words them its own way: nlsg_resident.h)
  const char *params_first = "the objective has %d parameters: call %s_set_params first";
  const char *no_params = "the engine's objective declares no parameters (%s_create_params)";

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
    params_rows = batch;
    if (n) own.alloc(&params_dev, batch * static_cast<uint64_t>(n) * 8);
  }
  int set_params(const double *params_host) {
    if (n_params <= 0) return fail(NLSG_ERR_INVALID_ARG, no_params, api);
    NLSG_HIP(hipSetDevice(own.device));
    NLSG_HIP(hipMemcpyAsync(params_dev, params_host, params_rows * static_cast<uint64_t>(n_params) * 8,
                            hipMemcpyHostToDevice, stream));
    NLSG_HIP(hipStreamSynchronize(stream));  // the host buffer is borrowed for this call only
    params_set = true;
    return NLSG_OK;
  }
  // a parametrised engine launches nothing before its first rows
  int params_ready() const {
    if (n_params > 0 && !params_set) return fail(NLSG_ERR_STATE, params_first, n_params, api);
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

// ---- the front doors of a create: what nlsg_X_create* checks before the engine's own create ----
// (the objective id comes before the config's size, which is the create's to report: the order the C-ABI
// header documents for its creators; `objective` sits at one offset in every config)

// A built-in door refuses an objective kind that a run-time door makes: "<api>_create_<door>"
template <typename Cfg>
int builtin_door(const Cfg *cfg, const char *api, int32_t kind = NLSG_OBJ_CUSTOM,
                 const char *kind_name = "NLSG_OBJ_CUSTOM", const char *door = "custom") {
  if (cfg && cfg->objective == kind)
    return fail(NLSG_ERR_INVALID_ARG, "%s engines are made by %s_create_%s", kind_name, api, door);
  return NLSG_OK;
}
// A run-time door (`body`: the source it compiles) makes one objective kind only
template <typename Cfg>
int runtime_door(const Cfg *cfg, const void *body, const void *out, int32_t kind = NLSG_OBJ_CUSTOM,
                 const char *kind_name = "NLSG_OBJ_CUSTOM") {
  if (!cfg || !body || !out) return fail(NLSG_ERR_INVALID_ARG, "null argument");
  if (cfg->objective != kind) return fail(NLSG_ERR_INVALID_ARG, "cfg.objective must be %s", kind_name);
  return NLSG_OK;
}
// nlsg_X_create_custom of an engine whose objective parameters have a door of their own, or none
template <typename Cfg>
int custom_door(const Cfg *cfg, const nlsg_custom_objective *obj, const void *out) {
  if (const int rc = runtime_door(cfg, obj, out)) return rc;
  return reject_custom_params(obj);
}

// `new` and open() for an engine struct; nothing to clean up when it fails
template <typename E>
int open_engine(int device, void *stream_handle, const char *api, E **out) {
  E *e = new (std::nothrow) E();
  if (!e) return fail(NLSG_ERR_OOM, "host allocation failed");
  e->api = api;
  if (const int rc = e->open(device, stream_handle)) {
    delete e;
    return rc;
  }
  *out = e;
  return NLSG_OK;
}

// The engine of a create between open_engine() and `*out = guard.release()`: every return in between
// hands it to the engine's own nlsg_X_destroy.
template <typename E>
class CreateGuard {
 public:
  CreateGuard(E *e, int (*destroy)(E *)) : e_(e), destroy_(destroy) {}
  CreateGuard(const CreateGuard &) = delete;
  CreateGuard &operator=(const CreateGuard &) = delete;
  ~CreateGuard() {
    if (e_) destroy_(e_);
  }
  E *release() {
    E *e = e_;
    e_ = nullptr;
    return e;
  }

 private:
  E *e_;
  int (*destroy_)(E *);
};

// nlsg_X_destroy: nothing in flight, then `between()` (what only DE and PSO have: their communicator),
// the run-time compiled module while the device is still the engine's, the blocks, the engine
struct NothingBetween {
  void operator()() const {}
};
template <typename E, typename Between = NothingBetween>
int destroy_engine(E *e, Between between = {}) {
  if (!e) return NLSG_OK;
  e->drain();
  between();
  rtc_release(&e->rtc);
  e->close();
  delete e;
  return NLSG_OK;
}
// the same for the engines that report nlsg_call_timing's destroy_ms
template <typename E, typename Between = NothingBetween>
int timed_destroy(E *e, Between between = {}) {
  if (!e) return NLSG_OK;
  PhaseClock clk;
  destroy_engine(e, between);
  call_timing().destroy_ms = clk.lap();
  return NLSG_OK;
}

// nlsg_X_set_params
template <typename E>
int set_params_entry(E *e, const double *params_host) {
  if (!e || !params_host) return fail(NLSG_ERR_INVALID_ARG, "null argument");
  return e->set_params(params_host);
}

// The dynamic-LDS limit of a run-time module's kernel: the module API's counterpart of the attribute a
// built-in kernel gets on its symbol. `past_64k_only`: a launch may take 64 KiB without it, and the caller
// asks only beyond. `fail_format` takes the HIP error's text (%s).
inline int module_kernel_lds(hipFunction_t fn, size_t bytes, const char *fail_format, bool past_64k_only = false) {
  if (past_64k_only && bytes <= 64 * 1024) return NLSG_OK;
  const hipError_t he = hipFuncSetAttribute(reinterpret_cast<const void *>(fn),
                                            hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(bytes));
  return he == hipSuccess ? NLSG_OK : fail(NLSG_ERR_HIP, fail_format, hipGetErrorString(he));
}

// ---- status rows (the row itself: status_row, nlsg_common.h) ----

// The per-problem rows of a finished solve, downloaded (the stream is idle), and from each: a status through
// row(problem, b) when the caller wants statuses, and extra(problem, b) — an output next to the status
template <typename Problem, typename Row, typename Extra>
int download_rows(const Problem *prob_dev, uint64_t batch, nlsg_status *status_host, Row row, Extra extra) {
  std::vector<Problem> pr(batch);
  NLSG_HIP(hipMemcpy(pr.data(), prob_dev, batch * sizeof(Problem), hipMemcpyDeviceToHost));
  for (uint64_t b = 0; b < batch; b++) {
    if (status_host) status_host[b] = row(pr[b], b);
    extra(pr[b], b);
  }
  return NLSG_OK;
}
// statuses only: nothing to read when nobody asks
template <typename Problem, typename Row>
int download_rows(const Problem *prob_dev, uint64_t batch, nlsg_status *status_host, Row row) {
  if (!status_host) return NLSG_OK;
  return download_rows(prob_dev, batch, status_host, row, [](const Problem &, uint64_t) {});
}

// "count on the device, read one word": launch() queues a kernel that adds into *count_dev
template <typename Launch>
int device_count(hipStream_t stream, unsigned long long *count_dev, uint64_t *count, Launch launch) {
  NLSG_HIP(hipMemsetAsync(count_dev, 0, 8, stream));
  launch();
  unsigned long long c = 0;
  NLSG_HIP(hipMemcpyAsync(&c, count_dev, 8, hipMemcpyDeviceToHost, stream));
  NLSG_HIP(hipStreamSynchronize(stream));
  *count = c;
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

// ---- the one-launch solve (NM, the NM/PSO hybrid, SANN): the whole solve of every start is launch() ----
// Behind the engine's argument checks, params_ready(), hipSetDevice and bounds: the starts (`count` doubles at
// x_dev) in, launch(), the results out, then rows() — the engine's download_rows
template <typename E, typename Launch, typename Rows>
int one_launch_minimize(E *e, double *x_dev, uint64_t count, double *x_inout_host, Launch launch, Rows rows) {
  NLSG_HIP(hipMemcpy(x_dev, x_inout_host, count * 8, hipMemcpyHostToDevice));
  launch();
  NLSG_HIP(launches_status());
  NLSG_HIP(hipStreamSynchronize(e->stream));
  NLSG_HIP(hipMemcpy(x_inout_host, x_dev, count * 8, hipMemcpyDeviceToHost));
  return rows();
}
// nlsg_X_time_solve behind the same checks: the start points again ahead of each repeat, outside the interval
template <typename E, typename Launch>
int one_launch_time_solve(E *e, double *x_dev, uint64_t count, const double *x0_host, uint32_t repeats,
                          float *ms_total, Launch launch) {
  return time_repeats(
      e->stream, e->ev0, e->ev1, repeats, ms_total,
      [&]() -> int {
        launch();
        return NLSG_OK;
      },
      [&]() -> int {
        NLSG_HIP(hipMemcpy(x_dev, x0_host, count * 8, hipMemcpyHostToDevice));
        return NLSG_OK;
      });
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
