// nlsolver_amd/csrc/nlsg_resident.h — the host side the resident batch engines share (nlsg_de_batch.hip,
// nlsg_pso_batch.hip): `batch` keyed solves of one shape, one workgroup each, an init kernel and a kernel
// that runs the turns, built in or of the engine's own run-time module. An engine file keeps its config
// checks, its blocks and parameter struct (`p`, which both kernels take by value), pick_kernels, its input
// upload, download and upload; what it has in common with the other is here, on EngineBase. A solve's
// state becomes a status through fill_status(const State &, nlsg_status *) of nlsg_de_state.h / nlsg_pso_state.h.
// Host only, as nlsg_engine.h.
#pragma once
#ifndef __HIPCC_RTC__
#include <algorithm>
#include <cstdio>
#include <vector>

#include "nlsg_engine.h"

#pragma GCC visibility push(hidden)
namespace nlsg {

// No launch runs unbounded: step / minimize are cut into launches of at most this many turns
// (turns_per_launch = 0 in the engine's config)
constexpr uint64_t kResidentTurnsPerLaunch = 1024;

struct ResidentEngine : EngineBase {  // (n_params: a row per solve, nlsg_X_batch_set_params)
  ResidentEngine() {  // (this pair's own words for the two parameter errors)
    params_first = "the objective has %d parameters: %s_set_params has not been called";
    no_params = "the engine's objective declares no parameters (n_params == 0)";
  }
  const char *name = "";         // "DE", "PSO": who speaks in an error
  size_t lds = 0;                // dynamic LDS of a turn workgroup
  int group = 0;                 // lanes per row: 4 / 8 / 16 / 32, or 64 = one wave per row
  const void *init_fn = nullptr, *turn_fn = nullptr;  // built-in objectives
  ResidentRtcKernels rtc;        // objective == NLSG_OBJ_CUSTOM
  uint64_t turns_per_launch = 0;
  uint64_t batch = 0, dim = 0;
  uint32_t init_blocks_per = 0;  // workgroups of the init kernel per solve: a wave per row
  uint32_t *n_done = nullptr;    // solves whose stop test has fired since the last init
  double *best_x = nullptr;      // [batch][dim], written by a turn's head
  uint64_t *seeds_dev = nullptr;
  bool initialised = false;

  int ready() const {
    return initialised ? NLSG_OK : fail(NLSG_ERR_STATE, "%s_init has not been called", api);
  }
};

// `params`: the engine's parameter struct, the first argument of both kernels
inline void launch_init(ResidentEngine *e, void *params) {
  uint32_t per = e->init_blocks_per;
  const unsigned grid = static_cast<unsigned>(e->batch * per);
  void *args[] = {params, &per};
  if (e->rtc.mod) {
    launch_module_kernel(e->rtc.init, grid, 256, 0, e->stream, args);
    return;
  }
  (void)hipLaunchKernel(e->init_fn, dim3(grid), dim3(256), args, 0, e->stream);
}

inline void launch_turns(ResidentEngine *e, void *params, uint64_t turns) {
  const unsigned grid = static_cast<unsigned>(e->batch);
  void *args[] = {params, &turns};
  if (e->rtc.mod) {
    launch_module_kernel(e->rtc.turns, grid, 256, static_cast<unsigned>(e->lds), e->stream, args);
    return;
  }
  (void)hipLaunchKernel(e->turn_fn, dim3(grid), dim3(256), args, e->lds, e->stream);
}

// the state reset ahead of an init launch. Asynchronous.
inline int reset_state(ResidentEngine *e) {
  NLSG_HIP(hipMemsetAsync(e->n_done, 0, sizeof(uint32_t), e->stream));
  // no head has run yet: best() before the first step gives zeros, not an earlier solve's rows
  NLSG_HIP(hipMemsetAsync(e->best_x, 0, e->batch * e->dim * 8, e->stream));
  return NLSG_OK;
}

// generation 0 seeded and scored, behind the inputs and reset_state. Asynchronous.
inline int begin(ResidentEngine *e, void *params) {
  launch_init(e, params);
  NLSG_HIP(launches_status());
  e->initialised = true;
  return NLSG_OK;
}

// launches of at most turns_per_launch turns until every solve is done; one word read per launch
inline int run_to_done(ResidentEngine *e, void *params, uint64_t max_iter) {
  const uint64_t B = e->batch, tpl = e->turns_per_launch;
  // the head after max_iter turns stops at iter >= max_iter: max_iter + 1 turns end every solve
  const uint64_t bound = max_iter / tpl + 2;
  for (uint64_t launched = 1;; launched++) {
    launch_turns(e, params, tpl);
    NLSG_HIP(launches_status());
    uint32_t done = 0;
    NLSG_HIP(hipMemcpyAsync(&done, e->n_done, sizeof done, hipMemcpyDeviceToHost, e->stream));
    NLSG_HIP(hipStreamSynchronize(e->stream));
    if (done >= B) return NLSG_OK;
    if (launched > bound)
      return fail(NLSG_ERR_STATE, "resident %s: %llu of %llu solves unfinished after %llu launches", e->name,
                  (unsigned long long)(B - done), (unsigned long long)B, (unsigned long long)launched);
  }
}

// nlsg_X_batch_step
template <typename E>
int resident_step(E *e, uint64_t turns) {
  if (!e) return fail(NLSG_ERR_INVALID_ARG, "null engine");
  if (const int rc = e->ready()) return rc;
  NLSG_HIP(hipSetDevice(e->cfg.device));
  while (turns) {
    const uint64_t t = std::min(turns, e->turns_per_launch);
    launch_turns(e, &e->p, t);
    turns -= t;
  }
  NLSG_HIP(launches_status());
  return NLSG_OK;
}

template <typename State>
int read_states(ResidentEngine *e, const State *states_dev, std::vector<State> &host) {
  host.resize(e->batch);
  NLSG_HIP(hipMemcpyAsync(host.data(), states_dev, e->batch * sizeof(State), hipMemcpyDeviceToHost, e->stream));
  NLSG_HIP(hipStreamSynchronize(e->stream));
  NLSG_HIP(launches_status());
  return NLSG_OK;
}

// a status per solve
template <typename State>
int read_statuses(ResidentEngine *e, const State *states_dev, nlsg_status *out) {
  std::vector<State> s;
  if (const int rc = read_states(e, states_dev, s)) return rc;
  for (uint64_t b = 0; b < e->batch; b++) fill_status(s[b], out + b);
  return NLSG_OK;
}

// nlsg_X_batch_status
template <typename E, typename State>
int resident_status(E *e, const State *states_dev, nlsg_status *out) {
  if (!e || !out) return fail(NLSG_ERR_INVALID_ARG, "null argument");
  if (const int rc = e->ready()) return rc;
  NLSG_HIP(hipSetDevice(e->cfg.device));
  return read_statuses(e, states_dev, out);
}

// nlsg_X_batch_best: every output may be null
template <typename E, typename State>
int resident_best(E *e, const State *states_dev, double *x_host, double *f, uint64_t *index) {
  if (!e) return fail(NLSG_ERR_INVALID_ARG, "null engine");
  if (const int rc = e->ready()) return rc;
  NLSG_HIP(hipSetDevice(e->cfg.device));
  std::vector<State> s;
  if (const int rc = read_states(e, states_dev, s)) return rc;
  if (x_host) NLSG_HIP(hipMemcpy(x_host, e->best_x, e->batch * e->dim * 8, hipMemcpyDeviceToHost));
  for (uint64_t b = 0; b < e->batch; b++) {
    nlsg_status st;
    fill_status(s[b], &st);
    if (f) f[b] = st.f_value;
    if (index) index[b] = st.best_index;
  }
  return NLSG_OK;
}

// nlsg_X_batch_minimize behind its argument checks: start() takes the inputs up and ends in begin()
template <typename E, typename Start, typename State>
int resident_minimize(E *e, Start start, double *x_host, const State *states_dev, nlsg_status *status_host) {
  PhaseClock clk;
  int rc = start();
  if (rc) return rc;
  call_timing().init_ms = clk.lap();
  rc = run_to_done(e, &e->p, e->cfg.max_iter);
  if (rc) return rc;
  call_timing().iterate_ms = clk.lap();
  // x = the best row (nlsolver.h:2444, :2601)
  NLSG_HIP(hipMemcpyAsync(x_host, e->best_x, e->batch * e->dim * 8, hipMemcpyDeviceToHost, e->stream));
  if (status_host) {
    rc = read_statuses(e, states_dev, status_host);
    if (rc) return rc;
  } else {
    NLSG_HIP(hipStreamSynchronize(e->stream));
  }
  call_timing().readback_ms = clk.lap();
  return NLSG_OK;
}

// nlsg_X_batch_time_solve once the inputs are on the device: init launch to the last solve's end, per repeat
template <typename E>
int resident_time_solve(E *e, uint32_t repeats, float *ms_total) {
  return time_repeats(
      e->stream, e->ev0, e->ev1, repeats, ms_total,
      [&]() -> int {
        launch_init(e, &e->p);
        e->initialised = true;
        return run_to_done(e, &e->p, e->cfg.max_iter);
      },
      [&]() -> int { return reset_state(e); });  // outside the interval
}

// The checks of a create that both engines make alike, in their order: the objective's parameter count,
// the LDS of a workgroup (`lds` for the shape, the parameter row static in front of it), the batch size,
// the built-in objective. `shape_format` takes rows and dim (%llu each) and ends in the verb:
// "pop %llu x dim %llu needs".
template <typename Cfg>
int resident_checks(const Cfg *cfg, const nlsg_custom_objective *custom, const char *name,
                    const char *shape_format, uint64_t rows, uint64_t lds, uint64_t budget) {
  const int32_t n_params = custom ? custom->n_params : 0;
  if (n_params < 0) return fail(NLSG_ERR_INVALID_ARG, "n_params must be >= 0, not %d", n_params);
  if (n_params > NLSG_CUSTOM_MAX_PARAMS)
    return fail(NLSG_ERR_UNSUPPORTED, "a custom objective takes at most %d parameters, not %d",
                NLSG_CUSTOM_MAX_PARAMS, n_params);
  const uint64_t params_lds = custom_params_lds_bytes(n_params);
  if (lds + params_lds > budget) {
    char shape[96];
    std::snprintf(shape, sizeof shape, shape_format, (unsigned long long)rows, (unsigned long long)cfg->dim);
    if (params_lds)
      return fail(NLSG_ERR_UNSUPPORTED,
                  "resident %s: %s %llu bytes of LDS and %d parameters %llu more, a workgroup has %llu", name,
                  shape, (unsigned long long)lds, n_params, (unsigned long long)params_lds,
                  (unsigned long long)budget);
    return fail(NLSG_ERR_UNSUPPORTED, "resident %s: %s %llu bytes of LDS, a workgroup has %llu", name, shape,
                (unsigned long long)lds, (unsigned long long)budget);
  }
  if (cfg->batch >= (1ull << 23)) return fail(NLSG_ERR_UNSUPPORTED, "batch must be < 2^23 solves");
  if (!custom && (cfg->objective < 0 || cfg->objective > NLSG_OBJ_RASTRIGIN))
    return fail(NLSG_ERR_INVALID_ARG, "unknown objective %d", cfg->objective);
  return NLSG_OK;
}

// what a fresh engine knows before its blocks: its name, the config, the shape's launch geometry
template <typename E, typename Cfg>
void resident_shape(E *e, const Cfg *cfg, const char *name, uint64_t rows, uint64_t lds) {
  e->name = name;
  e->cfg = *cfg;
  e->lds = lds;
  e->batch = cfg->batch;
  e->dim = cfg->dim;
  e->init_blocks_per = static_cast<uint32_t>((rows + 3) / 4);
  e->group = lane_group_of(cfg->dim, true);  // the turn engine's mappings
  e->turns_per_launch = cfg->turns_per_launch ? cfg->turns_per_launch : kResidentTurnsPerLaunch;
}

// The last step of a create, behind the blocks: the two kernels and the turn kernel's LDS opt-in.
// The > 64 KiB dynamic-LDS opt-in belongs to the kernel instantiation, which every live engine of that
// class shares: for a built-in objective it is set to the budget, never to one engine's size — a later,
// smaller engine must not lower it under a kept larger one (as nlsg_nm.hip does). A run-time module is the
// engine's own; its static LDS (the parameter row) comes off the budget.
// pick_kernels(e): init_fn and turn_fn of a built-in objective, false for a value outside the lists.
// build_module(&e->rtc): the engine's rtc_build_*.
template <typename E, typename Pick, typename Build>
int resident_kernels(E *e, bool custom, uint64_t budget, Pick pick_kernels, Build build_module) {
  hipError_t &he = e->own.err;
  if (he == hipSuccess && !custom) {
    he = pick_kernels(e) ? hipFuncSetAttribute(e->turn_fn, hipFuncAttributeMaxDynamicSharedMemorySize,
                                               static_cast<int>(budget))
                         : hipErrorInvalidValue;
  }
  if (he == hipSuccess && custom) {
    if (const int rc = build_module(&e->rtc)) return rc;
    if (const int rc = module_kernel_lds(e->rtc.turns, budget - custom_params_lds_bytes(e->n_params),
                                         "device setup failed: %s"))
      return rc;
  }
  return e->setup_status();
}

}  // namespace nlsg
#pragma GCC visibility pop
#endif  // !__HIPCC_RTC__
