// nlsolver_amd/csrc/nlsg_de_batch.hip — host side of the resident batch DE engine + its C-ABI
// (include/nlsg_c_api.h, nlsg_de_batch_*): `batch` keyed solves of one shape, one workgroup each,
// the turn loop inside de_batch_kernel (nlsg_de_batch_kernels.h). Solve b equals the turn engine
// (nlsg_de_*) with seed seeds[b] bit for bit. No global-memory fallback: a shape whose population
// does not fit a workgroup's LDS is NLSG_ERR_UNSUPPORTED.
#include <algorithm>
#include <vector>

#include "nlsg_de_batch_kernels.h"
#include "nlsg_engine.h"
#include "nlsg_rtc.h"

using namespace nlsg;

struct nlsg_de_batch : EngineBase {  // (n_params: a row per solve, nlsg_de_batch_set_params)
  nlsg_de_batch_config cfg;
  DeBatchParams p;
  size_t lds = 0;
  int group = 0;                 // lanes per agent: 4 / 8 / 16 / 32, or 64 = one wave per agent
  const void *init_fn = nullptr, *turn_fn = nullptr;  // built-in objectives
  DeBatchRtcKernels rtc;         // objective == NLSG_OBJ_CUSTOM
  uint64_t turns_per_launch = 0;
  uint64_t *seeds_dev = nullptr;
  double *x0_dev = nullptr;
  bool initialised = false;
};

namespace {

// No launch runs unbounded: step / minimize are cut into launches of at most this many turns
// (nlsg_de_batch_config.turns_per_launch = 0)
constexpr uint64_t kDeBatchTurnsPerLaunch = 1024;

// the two kernels of a built-in objective; false (and nothing picked) for a value outside the lists
bool pick_kernels(nlsg_de_batch *e) {
  return with_objective(e->cfg.objective, [&](auto O) {
    e->init_fn = reinterpret_cast<const void *>(de_batch_init_kernel<O>);
    return with_batch_groups(e->group, [&](auto G) {
      e->turn_fn = reinterpret_cast<const void *>(de_batch_kernel<O, G>);
    });
  });
}

uint32_t init_blocks_per(const nlsg_de_batch *e) { return static_cast<uint32_t>((e->p.pop + 3) / 4); }

void launch_init(nlsg_de_batch *e) {
  uint32_t per = init_blocks_per(e);
  const unsigned grid = static_cast<unsigned>(e->p.batch * per);
  void *args[] = {&e->p, &per};
  if (e->cfg.objective == NLSG_OBJ_CUSTOM) {
    launch_module_kernel(e->rtc.init, grid, 256, 0, e->stream, args);
    return;
  }
  (void)hipLaunchKernel(e->init_fn, dim3(grid), dim3(256), args, 0, e->stream);
}

void launch_turns(nlsg_de_batch *e, uint64_t turns) {
  const unsigned grid = static_cast<unsigned>(e->p.batch);
  void *args[] = {&e->p, &turns};
  if (e->cfg.objective == NLSG_OBJ_CUSTOM) {
    launch_module_kernel(e->rtc.turns, grid, 256, static_cast<unsigned>(e->lds), e->stream, args);
    return;
  }
  (void)hipLaunchKernel(e->turn_fn, dim3(grid), dim3(256), args, e->lds, e->stream);
}

int params_ready(const nlsg_de_batch *e) {
  return e->params_ready("the objective has %d parameters: nlsg_de_batch_set_params has not been called");
}

// x0 and the seeds in, state reset, generation 0 scored. Asynchronous after the copies.
int start(nlsg_de_batch *e, const double *x0_host, const uint64_t *seeds_host) {
  const uint64_t B = e->p.batch, D = e->p.D;
  NLSG_HIP(hipMemcpyAsync(e->x0_dev, x0_host, B * D * 8, hipMemcpyHostToDevice, e->stream));
  NLSG_HIP(hipMemcpyAsync(e->seeds_dev, seeds_host, B * 8, hipMemcpyHostToDevice, e->stream));
  NLSG_HIP(hipMemsetAsync(e->p.n_done, 0, sizeof(uint32_t), e->stream));
  // no head has run yet: best() before the first step gives zeros, not an earlier solve's rows
  NLSG_HIP(hipMemsetAsync(e->p.best_x, 0, B * D * 8, e->stream));
  NLSG_HIP(hipStreamSynchronize(e->stream));  // the host buffers are borrowed for this call only
  launch_init(e);
  NLSG_HIP(launches_status());
  e->initialised = true;
  return NLSG_OK;
}

// launches of at most turns_per_launch turns until every solve is done; one word read per launch
int run_to_done(nlsg_de_batch *e) {
  const uint64_t B = e->p.batch, tpl = e->turns_per_launch;
  // head k stops at k >= max_iter: max_iter + 1 turns end every solve
  const uint64_t bound = e->cfg.max_iter / tpl + 2;
  for (uint64_t launched = 1;; launched++) {
    launch_turns(e, tpl);
    NLSG_HIP(launches_status());
    uint32_t done = 0;
    NLSG_HIP(hipMemcpyAsync(&done, e->p.n_done, sizeof done, hipMemcpyDeviceToHost, e->stream));
    NLSG_HIP(hipStreamSynchronize(e->stream));
    if (done >= B) return NLSG_OK;
    if (launched > bound)
      return fail(NLSG_ERR_STATE, "resident DE: %llu of %llu solves unfinished after %llu launches",
                  (unsigned long long)(B - done), (unsigned long long)B, (unsigned long long)launched);
  }
}

void fill_status(const DeState &s, nlsg_status *out) {
  out->f_value = s.best_f;
  out->iteration = s.iter;
  out->function_calls_used = s.fcalls;
  out->gradient_evals_used = 0;
  out->hessian_evals_used = 0;
  out->best_index = s.best_id;
  out->val_no_change = s.val_no_change;
  out->std_err = s.std_err;
  out->done = s.done;
  out->reserved = 0;
}

int read_states(nlsg_de_batch *e, std::vector<DeState> &host) {
  host.resize(e->p.batch);
  NLSG_HIP(hipMemcpyAsync(host.data(), e->p.state, e->p.batch * sizeof(DeState), hipMemcpyDeviceToHost,
                          e->stream));
  NLSG_HIP(hipStreamSynchronize(e->stream));
  NLSG_HIP(launches_status());
  return NLSG_OK;
}

int de_batch_create(const nlsg_de_batch_config *cfg, const nlsg_custom_objective *custom,
                    nlsg_de_batch **out) {
  if (!cfg || !out) return fail(NLSG_ERR_INVALID_ARG, "null argument");
  *out = nullptr;
  if (cfg->struct_size != sizeof(nlsg_de_batch_config))
    return fail(NLSG_ERR_INVALID_ARG, "nlsg_de_batch_config size mismatch (%u vs %zu)", cfg->struct_size,
                sizeof(nlsg_de_batch_config));
  if (cfg->batch < 1) return fail(NLSG_ERR_INVALID_ARG, "batch must be >= 1");
  if (cfg->pop < 4 || cfg->pop > kDeBatchMaxPop)
    return fail(NLSG_ERR_UNSUPPORTED,
                "resident DE takes 4 <= pop <= %llu (one reduction tile; three donors besides the target), "
                "not pop %llu",
                (unsigned long long)kDeBatchMaxPop, (unsigned long long)cfg->pop);
  if (cfg->dim < 1 || cfg->dim > kDeBatchMaxDim)
    return fail(NLSG_ERR_UNSUPPORTED, "resident DE takes 1 <= dim <= %llu, not dim %llu",
                (unsigned long long)kDeBatchMaxDim, (unsigned long long)cfg->dim);
  const int32_t n_params = custom ? custom->n_params : 0;
  if (n_params < 0) return fail(NLSG_ERR_INVALID_ARG, "n_params must be >= 0, not %d", n_params);
  if (n_params > NLSG_CUSTOM_MAX_PARAMS)
    return fail(NLSG_ERR_UNSUPPORTED, "a custom objective takes at most %d parameters, not %d",
                NLSG_CUSTOM_MAX_PARAMS, n_params);
  const uint64_t lds = de_batch_lds_bytes(cfg->pop, cfg->dim);
  const uint64_t params_lds = custom_params_lds_bytes(n_params);  // static, in front of `lds`
  if (lds + params_lds > kDeBatchLdsBudget) {
    if (params_lds)
      return fail(NLSG_ERR_UNSUPPORTED,
                  "resident DE: pop %llu x dim %llu needs %llu bytes of LDS and %d parameters %llu more, "
                  "a workgroup has %llu",
                  (unsigned long long)cfg->pop, (unsigned long long)cfg->dim, (unsigned long long)lds,
                  n_params, (unsigned long long)params_lds, (unsigned long long)kDeBatchLdsBudget);
    return fail(NLSG_ERR_UNSUPPORTED,
                "resident DE: pop %llu x dim %llu needs %llu bytes of LDS, a workgroup has %llu",
                (unsigned long long)cfg->pop, (unsigned long long)cfg->dim, (unsigned long long)lds,
                (unsigned long long)kDeBatchLdsBudget);
  }
  if (cfg->batch >= (1ull << 23)) return fail(NLSG_ERR_UNSUPPORTED, "batch must be < 2^23 solves");
  if (!custom && (cfg->objective < 0 || cfg->objective > NLSG_OBJ_RASTRIGIN))
    return fail(NLSG_ERR_INVALID_ARG, "unknown objective %d", cfg->objective);
  if (cfg->strategy != NLSG_DE_BEST && cfg->strategy != NLSG_DE_RANDOM)
    return fail(NLSG_ERR_INVALID_ARG, "unknown strategy %d", cfg->strategy);
  nlsg_de_batch *e = nullptr;
  if (const int rc = open_engine(cfg->device, cfg->stream, &e)) return rc;
  e->cfg = *cfg;
  const uint64_t B = cfg->batch, n = cfg->pop, D = cfg->dim;
  e->lds = lds;
  e->n_params = n_params;
  e->group = D <= 8 ? 4 : D <= 16 ? 8 : D <= 32 ? 16 : D <= 64 ? 32 : 64;  // the turn engine's mappings
  e->turns_per_launch = cfg->turns_per_launch ? cfg->turns_per_launch : kDeBatchTurnsPerLaunch;
  DeBatchParams &p = e->p;
  std::memset(&p, 0, sizeof p);
  DeviceOwner &own = e->own;
  hipError_t &he = own.err;
  own.alloc(&p.rows, B * n * D * 8);
  own.alloc(&p.scores, B * n * 8);
  own.alloc(&p.best_x, B * D * 8);
  own.alloc(&p.state, B * sizeof(DeState));
  own.alloc(&p.n_done, 8);
  own.alloc(&e->seeds_dev, B * 8);
  own.alloc(&e->x0_dev, B * D * 8);
  e->alloc_params(B, n_params);
  e->timing_events();
  p.seeds = e->seeds_dev;
  p.params = e->params_dev;
  p.x0 = e->x0_dev;
  p.batch = B;
  p.pop = n;
  p.D = D;
  p.CR = cfg->CR;
  set_crossover_test(p, cfg->CR);
  p.F = cfg->F;
  p.eps = cfg->eps;
  p.fmul = cfg->minimize ? 1.0 : -1.0;  // f_multiplier, nlsolver.h:2418
  p.max_iter = cfg->max_iter;
  p.best_val_no_change = cfg->best_val_no_change;
  p.strategy = cfg->strategy;
  // The > 64 KiB dynamic-LDS opt-in belongs to the kernel instantiation (objective x G), which
  // every live engine of that class shares: it is set to the budget, never to one engine's size —
  // a later, smaller engine must not lower it under a kept larger one (as nlsg_nm.hip does).
  if (he == hipSuccess && !custom) {
    he = pick_kernels(e) ? hipFuncSetAttribute(e->turn_fn, hipFuncAttributeMaxDynamicSharedMemorySize,
                                               static_cast<int>(kDeBatchLdsBudget))
                         : hipErrorInvalidValue;
  }
  if (he == hipSuccess && custom) {
    const int rc2 = rtc_build_de_batch(custom, e->group, &e->rtc);
    if (rc2) {
      nlsg_de_batch_destroy(e);
      return rc2;
    }
    // this module is the engine's own; its static LDS (the parameter row) comes off the budget
    he = hipFuncSetAttribute(reinterpret_cast<const void *>(e->rtc.turns),
                             hipFuncAttributeMaxDynamicSharedMemorySize,
                             static_cast<int>(kDeBatchLdsBudget - params_lds));
  }
  if (const int rc = e->setup_status()) {
    nlsg_de_batch_destroy(e);
    return rc;
  }
  *out = e;
  return NLSG_OK;
}

}  // namespace

extern "C" {

uint64_t nlsg_de_batch_lds_bytes(uint64_t pop, uint64_t dim) { return de_batch_lds_bytes(pop, dim); }

int nlsg_de_batch_create(const nlsg_de_batch_config *cfg, nlsg_de_batch **out) {
  if (cfg && out && cfg->struct_size == sizeof(nlsg_de_batch_config) && cfg->objective == NLSG_OBJ_CUSTOM)
    return fail(NLSG_ERR_INVALID_ARG, "NLSG_OBJ_CUSTOM engines are made by nlsg_de_batch_create_custom");
  return timed_create([&] { return de_batch_create(cfg, nullptr, out); });
}

int nlsg_de_batch_create_custom(const nlsg_de_batch_config *cfg, const nlsg_custom_objective *obj,
                                nlsg_de_batch **out) {
  if (!cfg || !obj || !out) return fail(NLSG_ERR_INVALID_ARG, "null argument");
  if (cfg->struct_size == sizeof(nlsg_de_batch_config) && cfg->objective != NLSG_OBJ_CUSTOM)
    return fail(NLSG_ERR_INVALID_ARG, "cfg.objective must be NLSG_OBJ_CUSTOM");
  return timed_create([&] { return de_batch_create(cfg, obj, out); });
}

int nlsg_de_batch_destroy(nlsg_de_batch *e) {
  if (!e) return NLSG_OK;
  PhaseClock clk;
  e->drain();
  rtc_release(&e->rtc);
  e->close();
  delete e;
  call_timing().destroy_ms = clk.lap();
  return NLSG_OK;
}

int nlsg_de_batch_set_params(nlsg_de_batch *e, const double *params_host) {
  if (!e || !params_host) return fail(NLSG_ERR_INVALID_ARG, "null argument");
  return e->set_params(e->p.batch, params_host, "the engine's objective declares no parameters (n_params == 0)");
}

int nlsg_de_batch_init(nlsg_de_batch *e, const double *x0_host, const uint64_t *seeds_host) {
  if (!e || !x0_host || !seeds_host) return fail(NLSG_ERR_INVALID_ARG, "null argument");
  if (int rc = params_ready(e)) return rc;
  NLSG_HIP(hipSetDevice(e->cfg.device));
  return start(e, x0_host, seeds_host);
}

int nlsg_de_batch_step(nlsg_de_batch *e, uint64_t turns) {
  if (!e) return fail(NLSG_ERR_INVALID_ARG, "null engine");
  if (!e->initialised) return fail(NLSG_ERR_STATE, "nlsg_de_batch_init has not been called");
  NLSG_HIP(hipSetDevice(e->cfg.device));
  while (turns) {
    const uint64_t t = std::min(turns, e->turns_per_launch);
    launch_turns(e, t);
    turns -= t;
  }
  NLSG_HIP(launches_status());
  return NLSG_OK;
}

int nlsg_de_batch_status(nlsg_de_batch *e, nlsg_status *out) {
  if (!e || !out) return fail(NLSG_ERR_INVALID_ARG, "null argument");
  if (!e->initialised) return fail(NLSG_ERR_STATE, "nlsg_de_batch_init has not been called");
  NLSG_HIP(hipSetDevice(e->cfg.device));
  std::vector<DeState> s;
  int rc = read_states(e, s);
  if (rc) return rc;
  for (uint64_t b = 0; b < e->p.batch; b++) fill_status(s[b], out + b);
  return NLSG_OK;
}

int nlsg_de_batch_best(nlsg_de_batch *e, double *x_host, double *f, uint64_t *index) {
  if (!e) return fail(NLSG_ERR_INVALID_ARG, "null engine");
  if (!e->initialised) return fail(NLSG_ERR_STATE, "nlsg_de_batch_init has not been called");
  NLSG_HIP(hipSetDevice(e->cfg.device));
  std::vector<DeState> s;
  int rc = read_states(e, s);
  if (rc) return rc;
  if (x_host) NLSG_HIP(hipMemcpy(x_host, e->p.best_x, e->p.batch * e->p.D * 8, hipMemcpyDeviceToHost));
  for (uint64_t b = 0; b < e->p.batch; b++) {
    if (f) f[b] = s[b].best_f;
    if (index) index[b] = s[b].best_id;
  }
  return NLSG_OK;
}

int nlsg_de_batch_download(nlsg_de_batch *e, uint64_t b, double *pop_host, double *scores_host) {
  if (!e) return fail(NLSG_ERR_INVALID_ARG, "null engine");
  if (!e->initialised) return fail(NLSG_ERR_STATE, "nlsg_de_batch_init has not been called");
  if (b >= e->p.batch) return fail(NLSG_ERR_INVALID_ARG, "solve %llu out of range", (unsigned long long)b);
  NLSG_HIP(hipSetDevice(e->cfg.device));
  NLSG_HIP(hipStreamSynchronize(e->stream));
  NLSG_HIP(launches_status());
  const uint64_t n = e->p.pop, D = e->p.D;
  if (pop_host) NLSG_HIP(hipMemcpy(pop_host, e->p.rows + b * n * D, n * D * 8, hipMemcpyDeviceToHost));
  if (scores_host) NLSG_HIP(hipMemcpy(scores_host, e->p.scores + b * n, n * 8, hipMemcpyDeviceToHost));
  return NLSG_OK;
}

int nlsg_de_batch_upload(nlsg_de_batch *e, const double *pops_host, const double *scores_host) {
  if (!e || !pops_host || !scores_host) return fail(NLSG_ERR_INVALID_ARG, "null argument");
  if (!e->initialised) return fail(NLSG_ERR_STATE, "nlsg_de_batch_init has not been called");
  NLSG_HIP(hipSetDevice(e->cfg.device));
  const uint64_t B = e->p.batch, n = e->p.pop, D = e->p.D;
  NLSG_HIP(hipMemcpyAsync(e->p.rows, pops_host, B * n * D * 8, hipMemcpyHostToDevice, e->stream));
  NLSG_HIP(hipMemcpyAsync(e->p.scores, scores_host, B * n * 8, hipMemcpyHostToDevice, e->stream));
  NLSG_HIP(hipStreamSynchronize(e->stream));
  return NLSG_OK;
}

int nlsg_de_batch_minimize(nlsg_de_batch *e, double *x_inout_host, const uint64_t *seeds_host,
                           nlsg_status *status_host) {
  if (!e || !x_inout_host || !seeds_host) return fail(NLSG_ERR_INVALID_ARG, "null argument");
  if (int rc = params_ready(e)) return rc;
  NLSG_HIP(hipSetDevice(e->cfg.device));
  PhaseClock clk;
  int rc = start(e, x_inout_host, seeds_host);
  if (rc) return rc;
  call_timing().init_ms = clk.lap();
  rc = run_to_done(e);
  if (rc) return rc;
  call_timing().iterate_ms = clk.lap();
  // x = agents[best_id] (nlsolver.h:2444)
  NLSG_HIP(hipMemcpyAsync(x_inout_host, e->p.best_x, e->p.batch * e->p.D * 8, hipMemcpyDeviceToHost,
                          e->stream));
  if (status_host) {
    std::vector<DeState> s;
    rc = read_states(e, s);
    if (rc) return rc;
    for (uint64_t b = 0; b < e->p.batch; b++) fill_status(s[b], status_host + b);
  } else {
    NLSG_HIP(hipStreamSynchronize(e->stream));
  }
  call_timing().readback_ms = clk.lap();
  return NLSG_OK;
}

int nlsg_de_batch_time_solve(nlsg_de_batch *e, const double *x0_host, const uint64_t *seeds_host,
                             uint32_t repeats, float *ms_total) {
  if (!e || !x0_host || !seeds_host || !ms_total) return fail(NLSG_ERR_INVALID_ARG, "null argument");
  if (int rc = params_ready(e)) return rc;
  NLSG_HIP(hipSetDevice(e->cfg.device));
  const uint64_t B = e->p.batch, D = e->p.D;
  NLSG_HIP(hipMemcpyAsync(e->x0_dev, x0_host, B * D * 8, hipMemcpyHostToDevice, e->stream));
  NLSG_HIP(hipMemcpyAsync(e->seeds_dev, seeds_host, B * 8, hipMemcpyHostToDevice, e->stream));
  NLSG_HIP(hipStreamSynchronize(e->stream));
  return time_repeats(
      e->stream, e->ev0, e->ev1, repeats, ms_total,
      [&]() -> int {
        launch_init(e);
        e->initialised = true;
        return run_to_done(e);
      },
      [&]() -> int {  // the state reset, outside the interval
        NLSG_HIP(hipMemsetAsync(e->p.n_done, 0, sizeof(uint32_t), e->stream));
        NLSG_HIP(hipMemsetAsync(e->p.best_x, 0, B * D * 8, e->stream));
        return NLSG_OK;
      });
}

}  // extern "C"
