// nlsolver_amd/csrc/nlsg_de_batch.hip — host side of the resident batch DE engine + its C-ABI
// (include/nlsg_c_api.h, nlsg_de_batch_*): `batch` keyed solves of one shape, one workgroup each,
// the turn loop inside de_batch_kernel (nlsg_de_batch_kernels.h). Solve b equals the turn engine
// (nlsg_de_*) with seed seeds[b] bit for bit. No global-memory fallback: a shape whose population
// does not fit a workgroup's LDS is NLSG_ERR_UNSUPPORTED.
// What the engine shares with the resident PSO engine is in nlsg_resident.h.
#include "nlsg_de_batch_kernels.h"
#include "nlsg_resident.h"

using namespace nlsg;

struct nlsg_de_batch : ResidentEngine {
  nlsg_de_batch_config cfg;
  DeBatchParams p;
  double *x0_dev = nullptr;
};

namespace {

// the two kernels of a built-in objective; false (and nothing picked) for a value outside the lists
bool pick_kernels(nlsg_de_batch *e) {
  return with_objective(e->cfg.objective, [&](auto O) {
    e->init_fn = reinterpret_cast<const void *>(de_batch_init_kernel<O>);
    return with_batch_groups(e->group, [&](auto G) {
      e->turn_fn = reinterpret_cast<const void *>(de_batch_kernel<O, G>);
    });
  });
}

// x0 and the seeds on their way in. Asynchronous: the caller synchronises before it returns
int upload_inputs(nlsg_de_batch *e, const double *x0_host, const uint64_t *seeds_host) {
  const uint64_t B = e->batch, D = e->dim;
  NLSG_HIP(hipMemcpyAsync(e->x0_dev, x0_host, B * D * 8, hipMemcpyHostToDevice, e->stream));
  NLSG_HIP(hipMemcpyAsync(e->seeds_dev, seeds_host, B * 8, hipMemcpyHostToDevice, e->stream));
  return NLSG_OK;
}

// x0 and the seeds in, state reset, generation 0 scored. Asynchronous after the copies.
int start(nlsg_de_batch *e, const double *x0_host, const uint64_t *seeds_host) {
  if (const int rc = upload_inputs(e, x0_host, seeds_host)) return rc;
  if (const int rc = reset_state(e)) return rc;
  NLSG_HIP(hipStreamSynchronize(e->stream));  // the host buffers are borrowed for this call only
  return begin(e, &e->p);
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
  const uint64_t lds = de_batch_lds_bytes(cfg->pop, cfg->dim);
  if (const int rc = resident_checks(cfg, custom, "DE", "pop %llu x dim %llu needs", cfg->pop, lds, kDeBatchLdsBudget))
    return rc;
  if (cfg->strategy != NLSG_DE_BEST && cfg->strategy != NLSG_DE_RANDOM)
    return fail(NLSG_ERR_INVALID_ARG, "unknown strategy %d", cfg->strategy);
  nlsg_de_batch *e = nullptr;
  if (const int rc = open_engine(cfg->device, cfg->stream, "nlsg_de_batch", &e)) return rc;
  CreateGuard<nlsg_de_batch> guard(e, nlsg_de_batch_destroy);
  resident_shape(e, cfg, "DE", cfg->pop, lds);
  const uint64_t B = cfg->batch, n = cfg->pop, D = cfg->dim;
  DeBatchParams &p = e->p;
  std::memset(&p, 0, sizeof p);
  DeviceOwner &own = e->own;
  own.alloc(&p.rows, B * n * D * 8);
  own.alloc(&p.scores, B * n * 8);
  own.alloc(&e->best_x, B * D * 8);
  own.alloc(&p.state, B * sizeof(DeState));
  own.alloc(&e->n_done, 8);
  own.alloc(&e->seeds_dev, B * 8);
  own.alloc(&e->x0_dev, B * D * 8);
  e->alloc_params(B, custom ? custom->n_params : 0);
  e->timing_events();
  p.best_x = e->best_x;
  p.n_done = e->n_done;
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
  if (const int rc = resident_kernels(e, custom != nullptr, kDeBatchLdsBudget, pick_kernels, [&](ResidentRtcKernels *k) {
        return rtc_build_de_batch(custom, e->group, k);
      }))
    return rc;
  *out = guard.release();
  return NLSG_OK;
}

}  // namespace

extern "C" {

uint64_t nlsg_de_batch_lds_bytes(uint64_t pop, uint64_t dim) { return de_batch_lds_bytes(pop, dim); }

int nlsg_de_batch_create(const nlsg_de_batch_config *cfg, nlsg_de_batch **out) {
  if (const int rc = builtin_door(cfg, "nlsg_de_batch")) return rc;
  return timed_create([&] { return de_batch_create(cfg, nullptr, out); });
}

int nlsg_de_batch_create_custom(const nlsg_de_batch_config *cfg, const nlsg_custom_objective *obj,
                                nlsg_de_batch **out) {
  if (const int rc = runtime_door(cfg, obj, out)) return rc;  // (takes the objective's parameters itself)
  return timed_create([&] { return de_batch_create(cfg, obj, out); });
}

int nlsg_de_batch_destroy(nlsg_de_batch *e) { return timed_destroy(e); }

int nlsg_de_batch_set_params(nlsg_de_batch *e, const double *params_host) { return set_params_entry(e, params_host); }

int nlsg_de_batch_init(nlsg_de_batch *e, const double *x0_host, const uint64_t *seeds_host) {
  if (!e || !x0_host || !seeds_host) return fail(NLSG_ERR_INVALID_ARG, "null argument");
  if (const int rc = e->params_ready()) return rc;
  NLSG_HIP(hipSetDevice(e->cfg.device));
  return start(e, x0_host, seeds_host);
}

int nlsg_de_batch_step(nlsg_de_batch *e, uint64_t turns) { return resident_step(e, turns); }

int nlsg_de_batch_status(nlsg_de_batch *e, nlsg_status *out) {
  return resident_status(e, e ? e->p.state : nullptr, out);
}

int nlsg_de_batch_best(nlsg_de_batch *e, double *x_host, double *f, uint64_t *index) {
  return resident_best(e, e ? e->p.state : nullptr, x_host, f, index);
}

int nlsg_de_batch_download(nlsg_de_batch *e, uint64_t b, double *pop_host, double *scores_host) {
  if (!e) return fail(NLSG_ERR_INVALID_ARG, "null engine");
  if (const int rc = e->ready()) return rc;
  if (b >= e->batch) return fail(NLSG_ERR_INVALID_ARG, "solve %llu out of range", (unsigned long long)b);
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
  if (const int rc = e->ready()) return rc;
  NLSG_HIP(hipSetDevice(e->cfg.device));
  const uint64_t B = e->batch, n = e->p.pop, D = e->p.D;
  NLSG_HIP(hipMemcpyAsync(e->p.rows, pops_host, B * n * D * 8, hipMemcpyHostToDevice, e->stream));
  NLSG_HIP(hipMemcpyAsync(e->p.scores, scores_host, B * n * 8, hipMemcpyHostToDevice, e->stream));
  NLSG_HIP(hipStreamSynchronize(e->stream));
  return NLSG_OK;
}

int nlsg_de_batch_minimize(nlsg_de_batch *e, double *x_inout_host, const uint64_t *seeds_host,
                           nlsg_status *status_host) {
  if (!e || !x_inout_host || !seeds_host) return fail(NLSG_ERR_INVALID_ARG, "null argument");
  if (const int rc = e->params_ready()) return rc;
  NLSG_HIP(hipSetDevice(e->cfg.device));
  return resident_minimize(e, [&] { return start(e, x_inout_host, seeds_host); }, x_inout_host, e->p.state,
                           status_host);
}

int nlsg_de_batch_time_solve(nlsg_de_batch *e, const double *x0_host, const uint64_t *seeds_host,
                             uint32_t repeats, float *ms_total) {
  if (!e || !x0_host || !seeds_host || !ms_total) return fail(NLSG_ERR_INVALID_ARG, "null argument");
  if (const int rc = e->params_ready()) return rc;
  NLSG_HIP(hipSetDevice(e->cfg.device));
  if (const int rc = upload_inputs(e, x0_host, seeds_host)) return rc;
  NLSG_HIP(hipStreamSynchronize(e->stream));
  return resident_time_solve(e, repeats, ms_total);
}

}  // extern "C"
