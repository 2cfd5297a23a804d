// nlsolver_amd/csrc/nlsg_pso_batch.hip — host side of the resident batch PSO engine + its C-ABI
// (include/nlsg_c_api.h, nlsg_pso_batch_*): `batch` keyed solves of one shape, one workgroup each,
// the turn loop inside pso_batch_kernel (nlsg_pso_batch_kernels.h). Solve b equals the turn engine
// (nlsg_pso_*) with seed seeds[b] and bounds lower[b] / upper[b] bit for bit. No global-memory
// fallback: a shape whose swarm does not fit a workgroup's LDS is NLSG_ERR_UNSUPPORTED.
// What the engine shares with the resident DE engine is in nlsg_resident.h.
#include "nlsg_pso_batch_kernels.h"
#include "nlsg_resident.h"

using namespace nlsg;

struct nlsg_pso_batch : ResidentEngine {
  nlsg_pso_batch_config cfg;
  PsoBatchParams p;
  double *lower_dev = nullptr, *upper_dev = nullptr, *tab_dev = nullptr;
};

namespace {

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

int upload_inputs(nlsg_pso_batch *e, const double *lower_host, const double *upper_host,
                  const uint64_t *seeds_host) {
  const uint64_t B = e->batch, D = e->dim;
  NLSG_HIP(hipMemcpyAsync(e->lower_dev, lower_host, B * D * 8, hipMemcpyHostToDevice, e->stream));
  NLSG_HIP(hipMemcpyAsync(e->upper_dev, upper_host, B * D * 8, hipMemcpyHostToDevice, e->stream));
  NLSG_HIP(hipMemcpyAsync(e->seeds_dev, seeds_host, B * 8, hipMemcpyHostToDevice, e->stream));
  NLSG_HIP(hipStreamSynchronize(e->stream));  // the host buffers are borrowed for this call only
  return NLSG_OK;
}

// the bounds and the seeds in, state reset, the swarms seeded and scored. Asynchronous after the copies.
int start(nlsg_pso_batch *e, const double *lower_host, const double *upper_host, const uint64_t *seeds_host) {
  if (const int rc = upload_inputs(e, lower_host, upper_host, seeds_host)) return rc;
  if (const int rc = reset_state(e)) return rc;
  return begin(e, &e->p);
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
  const uint64_t lds = pso_batch_lds_bytes(cfg->n_particles, cfg->dim, cfg->type);
  if (const int rc = resident_checks(cfg, custom, "PSO", "%llu particles x dim %llu need", cfg->n_particles, lds,
                                     kPsoBatchLdsBudget))
    return rc;
  nlsg_pso_batch *e = nullptr;
  if (const int rc = open_engine(cfg->device, cfg->stream, "nlsg_pso_batch", &e)) return rc;
  CreateGuard<nlsg_pso_batch> guard(e, nlsg_pso_batch_destroy);
  resident_shape(e, cfg, "PSO", cfg->n_particles, lds);
  const uint64_t B = cfg->batch, n = cfg->n_particles, D = cfg->dim;
  const bool vanilla = cfg->type == NLSG_PSO_VANILLA;
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
  own.alloc(&e->best_x, B * D * 8);
  own.alloc(&q.state, B * sizeof(PsoState));
  own.alloc(&e->n_done, 8);
  own.alloc(&e->seeds_dev, B * 8);
  own.alloc(&e->lower_dev, B * D * 8);
  own.alloc(&e->upper_dev, B * D * 8);
  e->alloc_params(B, custom ? custom->n_params : 0);
  // the turn engine's inertia schedule, one table for every solve
  const std::vector<double> tab = pso_inertia_table(cfg->inertia, cfg->max_iter, &q.tab_fixed);
  q.tab_len = tab.size();
  own.alloc(&e->tab_dev, q.tab_len * 8);
  if (he == hipSuccess) he = hipMemcpy(e->tab_dev, tab.data(), q.tab_len * 8, hipMemcpyHostToDevice);
  e->timing_events();
  p.seeds = e->seeds_dev;
  p.params = e->params_dev;
  p.n_done = e->n_done;
  p.batch = B;
  q.gbest_x = e->best_x;
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
  if (const int rc = resident_kernels(e, custom != nullptr, kPsoBatchLdsBudget, pick_kernels, [&](ResidentRtcKernels *k) {
        return rtc_build_pso_batch(custom, e->group, cfg->type, k);
      }))
    return rc;
  *out = guard.release();
  return NLSG_OK;
}

}  // namespace

extern "C" {

uint64_t nlsg_pso_batch_lds_bytes(uint64_t n_particles, uint64_t dim, int32_t type) {
  return pso_batch_lds_bytes(n_particles, dim, type);
}

int nlsg_pso_batch_create(const nlsg_pso_batch_config *cfg, nlsg_pso_batch **out) {
  if (const int rc = builtin_door(cfg, "nlsg_pso_batch")) return rc;
  return timed_create([&] { return pso_batch_create(cfg, nullptr, out); });
}

int nlsg_pso_batch_create_custom(const nlsg_pso_batch_config *cfg, const nlsg_custom_objective *obj,
                                 nlsg_pso_batch **out) {
  if (const int rc = runtime_door(cfg, obj, out)) return rc;  // (takes the objective's parameters itself)
  return timed_create([&] { return pso_batch_create(cfg, obj, out); });
}

int nlsg_pso_batch_destroy(nlsg_pso_batch *e) { return timed_destroy(e); }

int nlsg_pso_batch_set_params(nlsg_pso_batch *e, const double *params_host) { return set_params_entry(e, params_host); }

int nlsg_pso_batch_init(nlsg_pso_batch *e, const double *lower_host, const double *upper_host,
                        const uint64_t *seeds_host) {
  if (!e || !lower_host || !upper_host || !seeds_host) return fail(NLSG_ERR_INVALID_ARG, "null argument");
  if (const int rc = e->params_ready()) return rc;
  NLSG_HIP(hipSetDevice(e->cfg.device));
  return start(e, lower_host, upper_host, seeds_host);
}

int nlsg_pso_batch_step(nlsg_pso_batch *e, uint64_t turns) { return resident_step(e, turns); }

int nlsg_pso_batch_status(nlsg_pso_batch *e, nlsg_status *out) {
  return resident_status(e, e ? e->p.q.state : nullptr, out);
}

int nlsg_pso_batch_best(nlsg_pso_batch *e, double *x_host, double *f, uint64_t *index) {
  return resident_best(e, e ? e->p.q.state : nullptr, x_host, f, index);
}

int nlsg_pso_batch_download(nlsg_pso_batch *e, uint64_t b, double *pos_host, double *vel_host,
                            double *pbest_val_host, double *cur_val_host) {
  if (!e) return fail(NLSG_ERR_INVALID_ARG, "null engine");
  if (const int rc = e->ready()) return rc;
  if (b >= e->batch) return fail(NLSG_ERR_INVALID_ARG, "solve %llu out of range", (unsigned long long)b);
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
  if (const int rc = e->params_ready()) return rc;
  NLSG_HIP(hipSetDevice(e->cfg.device));
  return resident_minimize(e, [&] { return start(e, lower_host, upper_host, seeds_host); }, x_out_host,
                           e->p.q.state, status_host);
}

int nlsg_pso_batch_time_solve(nlsg_pso_batch *e, const double *lower_host, const double *upper_host,
                              const uint64_t *seeds_host, uint32_t repeats, float *ms_total) {
  if (!e || !lower_host || !upper_host || !seeds_host || !ms_total)
    return fail(NLSG_ERR_INVALID_ARG, "null argument");
  if (const int rc = e->params_ready()) return rc;
  NLSG_HIP(hipSetDevice(e->cfg.device));
  if (const int rc = upload_inputs(e, lower_host, upper_host, seeds_host)) return rc;
  return resident_time_solve(e, repeats, ms_total);
}

}  // extern "C"
