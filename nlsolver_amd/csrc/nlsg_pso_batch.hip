// nlsolver_amd/csrc/nlsg_pso_batch.hip — host side of the resident batch PSO engine + its C-ABI
// (include/nlsg_c_api.h, nlsg_pso_batch_*): `batch` keyed solves of one shape, one workgroup each,
// the turn loop inside pso_batch_kernel (nlsg_pso_batch_kernels.h). Solve b equals the turn engine
// (nlsg_pso_*) with seed seeds[b] and bounds lower[b] / upper[b] bit for bit. No global-memory
// fallback: a shape whose swarm does not fit a workgroup's LDS is NLSG_ERR_UNSUPPORTED.
#include <algorithm>
#include <cmath>
#include <vector>

#include "nlsg_engine.h"
// nlsg_pso_kernels.h defines the turn engine's non-template kernels with external linkage, and
// nlsg_pso.hip owns them. This file needs the header's types and device functions only
// (PsoState, PsoParams, pso_apply_pending, pso_finish_turn, pso_inertia_at), so here its kernels
// get internal linkage and are dropped unused; the header itself stays as it is.
#pragma push_macro("__global__")
#undef __global__
#define __global__ static __attribute__((global))
#include "nlsg_pso_kernels.h"
#pragma pop_macro("__global__")
#include "nlsg_pso_batch_kernels.h"
#include "nlsg_rtc.h"

using namespace nlsg;

struct nlsg_pso_batch : EngineBase {  // (n_params: a row per solve, nlsg_pso_batch_set_params)
  nlsg_pso_batch_config cfg;
  PsoBatchParams p;
  size_t lds = 0;
  int group = 0;  // lanes per particle: 4 / 8 / 16 / 32, or 64 = one wave per particle
  const void *init_fn = nullptr, *turn_fn = nullptr;  // built-in objectives
  PsoBatchRtcKernels rtc;                             // objective == NLSG_OBJ_CUSTOM
  uint64_t turns_per_launch = 0;
  uint64_t *seeds_dev = nullptr;
  double *lower_dev = nullptr, *upper_dev = nullptr, *tab_dev = nullptr;
  bool initialised = false;
};

namespace {

// No launch runs unbounded: step / minimize are cut into launches of at most this many turns
// (nlsg_pso_batch_config.turns_per_launch = 0)
constexpr uint64_t kPsoBatchTurnsPerLaunch = 1024;

// the two kernels of a built-in objective; false (and nothing picked) for a value outside the lists
bool pick_kernels(nlsg_pso_batch *e) {
  return with_objective(e->cfg.objective, [&](auto O) {
    e->init_fn = reinterpret_cast<const void *>(pso_batch_init_kernel<O>);
    return with_value<NLSG_PSO_VANILLA, NLSG_PSO_ACCELERATED>(e->cfg.type, [&](auto T) {
      return with_batch_groups(e->group, [&](auto G) {
        e->turn_fn = reinterpret_cast<const void *>(pso_batch_kernel<O, G, T>);
      });
    });
  });
}

void launch_init(nlsg_pso_batch *e) {
  uint32_t per = static_cast<uint32_t>((e->p.q.shard_n + 3) / 4);
  const unsigned grid = static_cast<unsigned>(e->p.batch * per);
  void *args[] = {&e->p, &per};
  if (e->cfg.objective == NLSG_OBJ_CUSTOM) {
    launch_module_kernel(e->rtc.init, grid, 256, 0, e->stream, args);
    return;
  }
  (void)hipLaunchKernel(e->init_fn, dim3(grid), dim3(256), args, 0, e->stream);
}

void launch_turns(nlsg_pso_batch *e, uint64_t turns) {
  const unsigned grid = static_cast<unsigned>(e->p.batch);
  void *args[] = {&e->p, &turns};
  if (e->cfg.objective == NLSG_OBJ_CUSTOM) {
    launch_module_kernel(e->rtc.turns, grid, 256, static_cast<unsigned>(e->lds), e->stream, args);
    return;
  }
  (void)hipLaunchKernel(e->turn_fn, dim3(grid), dim3(256), args, e->lds, e->stream);
}

int params_ready(const nlsg_pso_batch *e) {
  return e->params_ready("the objective has %d parameters: nlsg_pso_batch_set_params has not been called");
}

int upload_inputs(nlsg_pso_batch *e, const double *lower_host, const double *upper_host,
                  const uint64_t *seeds_host) {
  const uint64_t B = e->p.batch, D = e->p.q.D;
  NLSG_HIP(hipMemcpyAsync(e->lower_dev, lower_host, B * D * 8, hipMemcpyHostToDevice, e->stream));
  NLSG_HIP(hipMemcpyAsync(e->upper_dev, upper_host, B * D * 8, hipMemcpyHostToDevice, e->stream));
  NLSG_HIP(hipMemcpyAsync(e->seeds_dev, seeds_host, B * 8, hipMemcpyHostToDevice, e->stream));
  NLSG_HIP(hipStreamSynchronize(e->stream));  // the host buffers are borrowed for this call only
  return NLSG_OK;
}

// state reset, the swarms seeded and scored. Asynchronous.
int start(nlsg_pso_batch *e) {
  const uint64_t B = e->p.batch, D = e->p.q.D;
  NLSG_HIP(hipMemsetAsync(e->p.n_done, 0, sizeof(uint32_t), e->stream));
  // no head has run yet: best() before the first step gives zeros, not an earlier solve's rows
  NLSG_HIP(hipMemsetAsync(e->p.q.gbest_x, 0, B * D * 8, e->stream));
  launch_init(e);
  NLSG_HIP(launches_status());
  e->initialised = true;
  return NLSG_OK;
}

// launches of at most turns_per_launch turns until every solve is done; one word read per launch
int run_to_done(nlsg_pso_batch *e) {
  const uint64_t B = e->p.batch, tpl = e->turns_per_launch;
  // the head after max_iter moves stops at iter >= max_iter: max_iter + 1 turns end every solve
  const uint64_t bound = e->cfg.max_iter / tpl + 2;
  for (uint64_t launched = 1;; launched++) {
    launch_turns(e, tpl);
    NLSG_HIP(launches_status());
    uint32_t done = 0;
    NLSG_HIP(hipMemcpyAsync(&done, e->p.n_done, sizeof done, hipMemcpyDeviceToHost, e->stream));
    NLSG_HIP(hipStreamSynchronize(e->stream));
    if (done >= B) return NLSG_OK;
    if (launched > bound)
      return fail(NLSG_ERR_STATE, "resident PSO: %llu of %llu solves unfinished after %llu launches",
                  (unsigned long long)(B - done), (unsigned long long)B, (unsigned long long)launched);
  }
}

void fill_status(const PsoState &s, nlsg_status *out) {
  out->f_value = s.gbest_val;
  out->iteration = s.iter;
  out->function_calls_used = s.fevals;
  out->gradient_evals_used = 0;
  out->hessian_evals_used = 0;
  out->best_index = s.gbest_idx;
  out->val_no_change = s.val_no_change;
  out->std_err = s.std_err;
  out->done = s.done;
  out->reserved = 0;
}

int read_states(nlsg_pso_batch *e, std::vector<PsoState> &host) {
  host.resize(e->p.batch);
  NLSG_HIP(hipMemcpyAsync(host.data(), e->p.q.state, e->p.batch * sizeof(PsoState), hipMemcpyDeviceToHost,
                          e->stream));
  NLSG_HIP(hipStreamSynchronize(e->stream));
  NLSG_HIP(launches_status());
  return NLSG_OK;
}

int pso_batch_create(const nlsg_pso_batch_config *cfg, const nlsg_custom_objective *custom,
                     nlsg_pso_batch **out) {
  if (!cfg || !out) return fail(NLSG_ERR_INVALID_ARG, "null argument");
  *out = nullptr;
  if (cfg->struct_size != sizeof(nlsg_pso_batch_config))
    return fail(NLSG_ERR_INVALID_ARG, "nlsg_pso_batch_config size mismatch (%u vs %zu)", cfg->struct_size,
                sizeof(nlsg_pso_batch_config));
  if (cfg->batch < 1) return fail(NLSG_ERR_INVALID_ARG, "batch must be >= 1");
  if (cfg->type != NLSG_PSO_VANILLA && cfg->type != NLSG_PSO_ACCELERATED)
    return fail(NLSG_ERR_INVALID_ARG, "unknown PSO type %d", cfg->type);
  if (cfg->n_particles < 1 || cfg->n_particles > kPsoBatchMaxN)
    return fail(NLSG_ERR_UNSUPPORTED, "resident PSO takes 1 <= n_particles <= %llu (one reduction tile), not %llu",
                (unsigned long long)kPsoBatchMaxN, (unsigned long long)cfg->n_particles);
  if (cfg->dim < 1 || cfg->dim > kPsoBatchMaxDim)
    return fail(NLSG_ERR_UNSUPPORTED, "resident PSO takes 1 <= dim <= %llu, not dim %llu",
                (unsigned long long)kPsoBatchMaxDim, (unsigned long long)cfg->dim);
  const int32_t n_params = custom ? custom->n_params : 0;
  if (n_params < 0) return fail(NLSG_ERR_INVALID_ARG, "n_params must be >= 0, not %d", n_params);
  if (n_params > NLSG_CUSTOM_MAX_PARAMS)
    return fail(NLSG_ERR_UNSUPPORTED, "a custom objective takes at most %d parameters, not %d",
                NLSG_CUSTOM_MAX_PARAMS, n_params);
  const uint64_t lds = pso_batch_lds_bytes(cfg->n_particles, cfg->dim, cfg->type);
  const uint64_t params_lds = custom_params_lds_bytes(n_params);  // static, in front of `lds`
  if (lds + params_lds > kPsoBatchLdsBudget) {
    if (params_lds)
      return fail(NLSG_ERR_UNSUPPORTED,
                  "resident PSO: %llu particles x dim %llu need %llu bytes of LDS and %d parameters %llu "
                  "more, a workgroup has %llu",
                  (unsigned long long)cfg->n_particles, (unsigned long long)cfg->dim,
                  (unsigned long long)lds, n_params, (unsigned long long)params_lds,
                  (unsigned long long)kPsoBatchLdsBudget);
    return fail(NLSG_ERR_UNSUPPORTED,
                "resident PSO: %llu particles x dim %llu need %llu bytes of LDS, a workgroup has %llu",
                (unsigned long long)cfg->n_particles, (unsigned long long)cfg->dim, (unsigned long long)lds,
                (unsigned long long)kPsoBatchLdsBudget);
  }
  if (cfg->batch >= (1ull << 23)) return fail(NLSG_ERR_UNSUPPORTED, "batch must be < 2^23 solves");
  if (!custom && (cfg->objective < 0 || cfg->objective > NLSG_OBJ_RASTRIGIN))
    return fail(NLSG_ERR_INVALID_ARG, "unknown objective %d", cfg->objective);
  nlsg_pso_batch *e = nullptr;
  if (const int rc = open_engine(cfg->device, cfg->stream, &e)) return rc;
  e->cfg = *cfg;
  const uint64_t B = cfg->batch, n = cfg->n_particles, D = cfg->dim;
  const bool vanilla = cfg->type == NLSG_PSO_VANILLA;
  e->lds = lds;
  e->n_params = n_params;
  e->group = D <= 8 ? 4 : D <= 16 ? 8 : D <= 32 ? 16 : D <= 64 ? 32 : 64;  // the turn engine's mappings
  e->turns_per_launch = cfg->turns_per_launch ? cfg->turns_per_launch : kPsoBatchTurnsPerLaunch;
  PsoBatchParams &p = e->p;
  std::memset(&p, 0, sizeof p);
  PsoParams &q = p.q;
  DeviceOwner &own = e->own;
  hipError_t &he = own.err;
  own.alloc(&q.pos, B * n * D * 8);
  if (vanilla) own.alloc(&q.vel, B * n * D * 8);
  if (vanilla) own.alloc(&q.pbest_pos, B * n * D * 8);
  own.alloc(&q.pbest_val, B * n * 8);
  own.alloc(&q.cur_val, B * n * 8);
  own.alloc(&q.gbest_x, B * D * 8);
  own.alloc(&q.state, B * sizeof(PsoState));
  own.alloc(&p.n_done, 8);
  own.alloc(&e->seeds_dev, B * 8);
  own.alloc(&e->lower_dev, B * D * 8);
  own.alloc(&e->upper_dev, B * D * 8);
  e->alloc_params(B, n_params);
  // the inertia schedule pow(inertia, iter) (:2613) from the host libm, exactly as nlsg_pso_create
  // builds it (max_iter + 1 entries, or up to the first fixed point; at most 2^22)
  const uint64_t want = cfg->max_iter == ~0ull ? ~0ull : cfg->max_iter + 1;
  const uint64_t cap = std::min<uint64_t>(want, 1u << 22);
  std::vector<double> tab;
  tab.reserve(std::min<uint64_t>(cap, 4096));
  q.tab_fixed = 0;
  for (uint64_t k = 0; k < cap; k++) {
    tab.push_back(std::pow(cfg->inertia, static_cast<double>(k)));
    if (k >= 2 && std::memcmp(&tab[k], &tab[k - 1], 8) == 0 && std::memcmp(&tab[k], &tab[k - 2], 8) == 0 &&
        (tab[k] == 0.0 || tab[k] == 1.0 || std::isinf(tab[k]))) {
      q.tab_fixed = 1;
      break;
    }
  }
  q.tab_len = tab.size();
  own.alloc(&e->tab_dev, q.tab_len * 8);
  if (he == hipSuccess) he = hipMemcpy(e->tab_dev, tab.data(), q.tab_len * 8, hipMemcpyHostToDevice);
  e->timing_events();
  p.seeds = e->seeds_dev;
  p.params = e->params_dev;
  p.batch = B;
  q.lower = e->lower_dev;
  q.upper = e->upper_dev;
  q.inertia_tab = e->tab_dev;
  q.ntiles = 1;
  q.n = n;
  q.D = D;
  q.shard_lo = 0;
  q.shard_n = n;
  q.inertia = cfg->inertia;
  q.cog = cfg->cognitive;
  q.soc = cfg->social;
  q.eps = cfg->eps;
  q.fmul = cfg->minimize ? 1.0 : -1.0;
  q.max_iter = cfg->max_iter;
  q.best_val_no_change = cfg->best_val_no_change;
  q.type = cfg->type;
  q.bounded = cfg->bounded ? 1 : 0;
  // The > 64 KiB dynamic-LDS opt-in belongs to the kernel instantiation (objective x G x type),
  // which every live engine of that class shares: it is set to the budget, never to one engine's
  // size — a later, smaller engine must not lower it under a kept larger one.
  if (he == hipSuccess && !custom) {
    he = pick_kernels(e) ? hipFuncSetAttribute(e->turn_fn, hipFuncAttributeMaxDynamicSharedMemorySize,
                                               static_cast<int>(kPsoBatchLdsBudget))
                         : hipErrorInvalidValue;
  }
  if (he == hipSuccess && custom) {
    const int rc2 = rtc_build_pso_batch(custom, e->group, cfg->type, &e->rtc);
    if (rc2) {
      nlsg_pso_batch_destroy(e);
      return rc2;
    }
    // this module is the engine's own; its static LDS (the parameter row) comes off the budget
    he = hipFuncSetAttribute(reinterpret_cast<const void *>(e->rtc.turns),
                             hipFuncAttributeMaxDynamicSharedMemorySize,
                             static_cast<int>(kPsoBatchLdsBudget - params_lds));
  }
  if (const int rc = e->setup_status()) {
    nlsg_pso_batch_destroy(e);
    return rc;
  }
  *out = e;
  return NLSG_OK;
}

}  // namespace

extern "C" {

uint64_t nlsg_pso_batch_lds_bytes(uint64_t n_particles, uint64_t dim, int32_t type) {
  return pso_batch_lds_bytes(n_particles, dim, type);
}

int nlsg_pso_batch_create(const nlsg_pso_batch_config *cfg, nlsg_pso_batch **out) {
  if (cfg && out && cfg->struct_size == sizeof(nlsg_pso_batch_config) && cfg->objective == NLSG_OBJ_CUSTOM)
    return fail(NLSG_ERR_INVALID_ARG, "NLSG_OBJ_CUSTOM engines are made by nlsg_pso_batch_create_custom");
  return timed_create([&] { return pso_batch_create(cfg, nullptr, out); });
}

int nlsg_pso_batch_create_custom(const nlsg_pso_batch_config *cfg, const nlsg_custom_objective *obj,
                                 nlsg_pso_batch **out) {
  if (!cfg || !obj || !out) return fail(NLSG_ERR_INVALID_ARG, "null argument");
  if (cfg->struct_size == sizeof(nlsg_pso_batch_config) && cfg->objective != NLSG_OBJ_CUSTOM)
    return fail(NLSG_ERR_INVALID_ARG, "cfg.objective must be NLSG_OBJ_CUSTOM");
  return timed_create([&] { return pso_batch_create(cfg, obj, out); });
}

int nlsg_pso_batch_destroy(nlsg_pso_batch *e) {
  if (!e) return NLSG_OK;
  PhaseClock clk;
  e->drain();
  rtc_release(&e->rtc);
  e->close();
  delete e;
  call_timing().destroy_ms = clk.lap();
  return NLSG_OK;
}

int nlsg_pso_batch_set_params(nlsg_pso_batch *e, const double *params_host) {
  if (!e || !params_host) return fail(NLSG_ERR_INVALID_ARG, "null argument");
  return e->set_params(e->p.batch, params_host, "the engine's objective declares no parameters (n_params == 0)");
}

int nlsg_pso_batch_init(nlsg_pso_batch *e, const double *lower_host, const double *upper_host,
                        const uint64_t *seeds_host) {
  if (!e || !lower_host || !upper_host || !seeds_host) return fail(NLSG_ERR_INVALID_ARG, "null argument");
  if (int rc = params_ready(e)) return rc;
  NLSG_HIP(hipSetDevice(e->cfg.device));
  int rc = upload_inputs(e, lower_host, upper_host, seeds_host);
  if (rc) return rc;
  return start(e);
}

int nlsg_pso_batch_step(nlsg_pso_batch *e, uint64_t turns) {
  if (!e) return fail(NLSG_ERR_INVALID_ARG, "null engine");
  if (!e->initialised) return fail(NLSG_ERR_STATE, "nlsg_pso_batch_init has not been called");
  NLSG_HIP(hipSetDevice(e->cfg.device));
  while (turns) {
    const uint64_t t = std::min(turns, e->turns_per_launch);
    launch_turns(e, t);
    turns -= t;
  }
  NLSG_HIP(launches_status());
  return NLSG_OK;
}

int nlsg_pso_batch_status(nlsg_pso_batch *e, nlsg_status *out) {
  if (!e || !out) return fail(NLSG_ERR_INVALID_ARG, "null argument");
  if (!e->initialised) return fail(NLSG_ERR_STATE, "nlsg_pso_batch_init has not been called");
  NLSG_HIP(hipSetDevice(e->cfg.device));
  std::vector<PsoState> s;
  int rc = read_states(e, s);
  if (rc) return rc;
  for (uint64_t b = 0; b < e->p.batch; b++) fill_status(s[b], out + b);
  return NLSG_OK;
}

int nlsg_pso_batch_best(nlsg_pso_batch *e, double *x_host, double *f, uint64_t *index) {
  if (!e) return fail(NLSG_ERR_INVALID_ARG, "null engine");
  if (!e->initialised) return fail(NLSG_ERR_STATE, "nlsg_pso_batch_init has not been called");
  NLSG_HIP(hipSetDevice(e->cfg.device));
  std::vector<PsoState> s;
  int rc = read_states(e, s);
  if (rc) return rc;
  if (x_host)
    NLSG_HIP(hipMemcpy(x_host, e->p.q.gbest_x, e->p.batch * e->p.q.D * 8, hipMemcpyDeviceToHost));
  for (uint64_t b = 0; b < e->p.batch; b++) {
    if (f) f[b] = s[b].gbest_val;
    if (index) index[b] = s[b].gbest_idx;
  }
  return NLSG_OK;
}

int nlsg_pso_batch_download(nlsg_pso_batch *e, uint64_t b, double *pos_host, double *vel_host,
                            double *pbest_val_host, double *cur_val_host) {
  if (!e) return fail(NLSG_ERR_INVALID_ARG, "null engine");
  if (!e->initialised) return fail(NLSG_ERR_STATE, "nlsg_pso_batch_init has not been called");
  if (b >= e->p.batch) return fail(NLSG_ERR_INVALID_ARG, "solve %llu out of range", (unsigned long long)b);
  NLSG_HIP(hipSetDevice(e->cfg.device));
  NLSG_HIP(hipStreamSynchronize(e->stream));
  NLSG_HIP(launches_status());
  const PsoParams &q = e->p.q;
  const uint64_t n = q.shard_n, D = q.D;
  if (pos_host) NLSG_HIP(hipMemcpy(pos_host, q.pos + b * n * D, n * D * 8, hipMemcpyDeviceToHost));
  if (vel_host) {
    if (!q.vel) return fail(NLSG_ERR_STATE, "velocities exist only for Vanilla PSO");
    NLSG_HIP(hipMemcpy(vel_host, q.vel + b * n * D, n * D * 8, hipMemcpyDeviceToHost));
  }
  if (pbest_val_host) NLSG_HIP(hipMemcpy(pbest_val_host, q.pbest_val + b * n, n * 8, hipMemcpyDeviceToHost));
  if (cur_val_host) NLSG_HIP(hipMemcpy(cur_val_host, q.cur_val + b * n, n * 8, hipMemcpyDeviceToHost));
  return NLSG_OK;
}

int nlsg_pso_batch_minimize(nlsg_pso_batch *e, double *x_out_host, const double *lower_host,
                            const double *upper_host, const uint64_t *seeds_host,
                            nlsg_status *status_host) {
  if (!e || !x_out_host || !lower_host || !upper_host || !seeds_host)
    return fail(NLSG_ERR_INVALID_ARG, "null argument");
  if (int rc = params_ready(e)) return rc;
  NLSG_HIP(hipSetDevice(e->cfg.device));
  PhaseClock clk;
  int rc = upload_inputs(e, lower_host, upper_host, seeds_host);
  if (rc) return rc;
  rc = start(e);
  if (rc) return rc;
  call_timing().init_ms = clk.lap();
  rc = run_to_done(e);
  if (rc) return rc;
  call_timing().iterate_ms = clk.lap();
  // x = swarm_best_position (nlsolver.h:2601)
  NLSG_HIP(hipMemcpyAsync(x_out_host, e->p.q.gbest_x, e->p.batch * e->p.q.D * 8, hipMemcpyDeviceToHost,
                          e->stream));
  if (status_host) {
    std::vector<PsoState> s;
    rc = read_states(e, s);
    if (rc) return rc;
    for (uint64_t b = 0; b < e->p.batch; b++) fill_status(s[b], status_host + b);
  } else {
    NLSG_HIP(hipStreamSynchronize(e->stream));
  }
  call_timing().readback_ms = clk.lap();
  return NLSG_OK;
}

int nlsg_pso_batch_time_solve(nlsg_pso_batch *e, const double *lower_host, const double *upper_host,
                              const uint64_t *seeds_host, uint32_t repeats, float *ms_total) {
  if (!e || !lower_host || !upper_host || !seeds_host || !ms_total)
    return fail(NLSG_ERR_INVALID_ARG, "null argument");
  if (int rc = params_ready(e)) return rc;
  NLSG_HIP(hipSetDevice(e->cfg.device));
  int rc = upload_inputs(e, lower_host, upper_host, seeds_host);
  if (rc) return rc;
  const uint64_t B = e->p.batch, D = e->p.q.D;
  return time_repeats(
      e->stream, e->ev0, e->ev1, repeats, ms_total,
      [&]() -> int {
        launch_init(e);
        e->initialised = true;
        return run_to_done(e);
      },
      [&]() -> int {  // the state reset, outside the interval
        NLSG_HIP(hipMemsetAsync(e->p.n_done, 0, sizeof(uint32_t), e->stream));
        NLSG_HIP(hipMemsetAsync(e->p.q.gbest_x, 0, B * D * 8, e->stream));
        return NLSG_OK;
      });
}

}  // extern "C"
