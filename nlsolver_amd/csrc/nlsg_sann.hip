// nlsolver_amd/csrc/nlsg_sann.hip — host side of the batched simulated-annealing engine + C-ABI.
#include "nlsg_engine.h"
#include "nlsg_rtc.h"
#include "nlsg_sann_kernels.h"

using namespace nlsg;

struct nlsg_sann : EngineBase {  // (n_params: nlsg_sann_create_params, a row per chain)
  nlsg_sann_config cfg;
  SannParams p;
  double *zero_dev = nullptr;
  int chunks = 0;
  int group = 0;  // lanes per chain when several chains share a wave (dim <= 64), else 0
  SannRtcKernels rtc;  // objective == NLSG_OBJ_CUSTOM: the kernel hiprtc built for it
  unsigned lds = 0;  // dynamic LDS of a launch: the parameter rows (0 without parameters)
};

namespace {

constexpr uint64_t kSannLdsBudget = 160ull * 1024;                      // a workgroup's LDS
constexpr uint64_t kSannTableBytes = 8ull * kRnormTabDoubles;           // rn_tab, static, in every kernel
// dynamic LDS of the packed kernel with `group` lanes per chain: a row per group, 4 * (64 / group) to the block
uint64_t sann_group_rows_bytes(int group, int64_t n_params) {
  return 4ull * (64 / group) * 8 * custom_params_group_stride(n_params);
}
// Lanes per chain of the kernel a shape gets: the packing by dim, unless the group rows of a
// parametrised objective do not fit next to rn_tab — then one chain per wave (0), whose four rows always do.
// A chain's history does not depend on the packing, so the rule moves no bit.
int sann_group_for(uint64_t D, int64_t n_params) {
  const int group = lane_group_of(D, false);
  if (group && n_params > 0 && kSannTableBytes + sann_group_rows_bytes(group, n_params) > kSannLdsBudget) return 0;
  return group;
}
void launch_anneal(nlsg_sann *e, uint64_t iter_begin, uint64_t iter_end) {
  // waves: one per chain, or one per 64 / group chains
  const uint64_t per_wave = e->group ? 64 / e->group : 1;
  const uint64_t waves = (e->p.batch + per_wave - 1) / per_wave;
  const dim3 grid(static_cast<unsigned>((waves + 3) / 4)), block(256);
  const bool vec = e->p.D % 2 == 0;
  if (e->cfg.objective == NLSG_OBJ_CUSTOM) {
    void *args[] = {&e->p, &iter_begin, &iter_end};
    launch_module_kernel(e->rtc.anneal, grid.x, 256, e->lds, e->stream, args);
    return;
  }
  routed(with_objective(e->cfg.objective, [&](auto O) {
    if (e->group)  // (dim <= 64)
      return with_groups(e->group, [&](auto G) {
        hipLaunchKernelGGL((sann_anneal_groups_kernel<O, G>), grid, block, 0, e->stream, e->p, iter_begin, iter_end);
      });
    return with_bool(vec, [&](auto V) {
      if (e->p.D > 1024) {  // chains streamed in segments
        hipLaunchKernelGGL((sann_anneal_long_kernel<O, V>), grid, block, 0, e->stream, e->p, iter_begin, iter_end);
        return true;
      }
      return with_chunks(e->chunks, [&](auto C) {
        hipLaunchKernelGGL((sann_anneal_kernel<O, C, V>), grid, block, 0, e->stream, e->p, iter_begin, iter_end);
      });
    });
  }));
}

// The whole schedule; long schedules are cut into launches of a bounded number of trial points so
// that no single kernel runs for seconds (the chain's state waits in HBM between launches).
void launch_solve(nlsg_sann *e) {
  const uint64_t max_iter = e->cfg.max_iter;
  const uint64_t per_iter = e->p.inner ? e->p.inner : 1;
  uint64_t span = (1u << 16) / per_iter;
  if (span == 0) span = 1;
  uint64_t it = 0;
  do {  // max_iter == 0 still scores the start (:2781)
    const uint64_t end = max_iter - it < span ? max_iter : it + span;
    launch_anneal(e, it, end);
    it = end;
  } while (it < max_iter);
}

}  // namespace

static int sann_create(const nlsg_sann_config *cfg, const nlsg_custom_objective *custom,
                       nlsg_sann **out, bool with_params = false);

extern "C" {

int nlsg_sann_create(const nlsg_sann_config *cfg, nlsg_sann **out) {
  if (const int rc = builtin_door(cfg, "nlsg_sann")) return rc;
  return sann_create(cfg, nullptr, out);
}

int nlsg_sann_create_custom(const nlsg_sann_config *cfg, const nlsg_custom_objective *obj,
                            nlsg_sann **out) {
  if (const int rc = custom_door(cfg, obj, out)) return rc;
  return sann_create(cfg, obj, out);
}

int nlsg_sann_create_params(const nlsg_sann_config *cfg, const nlsg_custom_objective *obj,
                            nlsg_sann **out) {
  if (const int rc = runtime_door(cfg, obj, out)) return rc;
  return sann_create(cfg, obj, out, true);
}

// 1, or the 64 / G chains that share a wave. 0 for dim == 0 or an n_params outside 0 .. NLSG_CUSTOM_MAX_PARAMS.
uint32_t nlsg_sann_chains_per_wave(uint64_t dim, int32_t n_params) {
  if (dim < 1 || n_params < 0 || n_params > NLSG_CUSTOM_MAX_PARAMS) return 0;
  const int group = sann_group_for(dim, n_params);
  return group ? 64 / group : 1;
}

// The dynamic LDS of a launch: the parameter rows (rn_tab is static and not counted). 0 without parameters
// and outside the ranges above.
uint64_t nlsg_sann_lds_bytes(uint64_t dim, int32_t n_params) {
  if (dim < 1 || n_params < 1 || n_params > NLSG_CUSTOM_MAX_PARAMS) return 0;
  const int group = sann_group_for(dim, n_params);
  return group ? sann_group_rows_bytes(group, n_params) : 4 * custom_params_lds_bytes(n_params);
}

int nlsg_sann_set_params(nlsg_sann *e, const double *params_host) { return set_params_entry(e, params_host); }

}  // extern "C"

static int sann_create(const nlsg_sann_config *cfg, const nlsg_custom_objective *custom,
                       nlsg_sann **out, bool with_params) {
  if (!cfg || !out) return fail(NLSG_ERR_INVALID_ARG, "null argument");
  *out = nullptr;
  if (cfg->struct_size != sizeof(nlsg_sann_config))
    return fail(NLSG_ERR_INVALID_ARG, "nlsg_sann_config size mismatch (%u vs %zu)",
                cfg->struct_size, sizeof(nlsg_sann_config));
  if (!custom && (cfg->objective < 0 || cfg->objective > NLSG_OBJ_RASTRIGIN))
    return fail(NLSG_ERR_INVALID_ARG, "unknown objective %d", cfg->objective);
  if (cfg->dim < 1 || cfg->batch < 1) return fail(NLSG_ERR_INVALID_ARG, "dim and batch must be >= 1");
  if (cfg->dim > 1024 && custom && custom->chain == NLSG_CUSTOM_VECTOR)
    return fail(NLSG_ERR_UNSUPPORTED,
                "dim %llu > 1024: a whole-vector objective needs the point in the wave's registers",
                (unsigned long long)cfg->dim);
  if (cfg->dim > 0xffffffffull) return fail(NLSG_ERR_UNSUPPORTED, "dim beyond 2^32");
  if (cfg->batch > 0x7fffffffull) return fail(NLSG_ERR_UNSUPPORTED, "batch too large");
  if (with_params)  // (a row per wave, four to the block, always fits; the packed kernel's rows: sann_group_for)
    if (const int prc = check_custom_params(custom, kSannTableBytes, "nlsg_sann", "nlsg_sann_create_custom", 4))
      return prc;
  nlsg_sann *e = nullptr;
  if (const int rc = open_engine(cfg->device, cfg->stream, "nlsg_sann", &e)) return rc;
  CreateGuard<nlsg_sann> guard(e, nlsg_sann_destroy);
  e->cfg = *cfg;
  const uint64_t B = cfg->batch, D = cfg->dim;
  e->chunks = row_chunks(D);
  e->n_params = with_params ? custom->n_params : 0;
  e->group = sann_group_for(D, e->n_params);
  e->lds = static_cast<unsigned>(nlsg_sann_lds_bytes(D, e->n_params));
  SannParams &p = e->p;
  std::memset(&p, 0, sizeof p);
  DeviceOwner &own = e->own;
  own.alloc(&p.x, B * D * 8);
  own.alloc(&p.p, B * D * 8);
  if (D > 1024) own.alloc(&p.trial, B * D * 8);
  own.alloc(&p.prob, B * sizeof(SannProblem));
  e->alloc_params(B, e->n_params);
  own.zeroed(&e->zero_dev, 16);
  e->timing_events();
  if (const int rc = e->setup_status()) return rc;
  if (custom) {
    if (const int rc = rtc_build_sann(custom, D > 1024 ? 0 : e->chunks, D % 2 == 0, e->group, &e->rtc)) return rc;
    // (the rows can pass the 64 KiB a launch may take without the opt-in)
    if (const int rc = module_kernel_lds(e->rtc.anneal, e->lds, "raising the kernel's dynamic LDS limit failed: %s", true))
      return rc;
  }
  p.params = e->params_dev;
  p.zero = e->zero_dev;
  p.batch = B;
  p.D = D;
  p.seed = cfg->seed;
  p.chain_lo = cfg->chain_lo;
  p.inner = cfg->temperature_iter ? cfg->temperature_iter - 1 : 0;  // for (j = 1; j < t_iter; j++)
  p.temp_max = cfg->temperature_max;
  p.fmul = cfg->minimize ? 1.0 : -1.0;
  *out = guard.release();
  return NLSG_OK;
}

extern "C" {

int nlsg_sann_destroy(nlsg_sann *e) { return destroy_engine(e); }

int nlsg_sann_minimize(nlsg_sann *e, double *x_inout_host, nlsg_status *status_host) {
  if (!e || !x_inout_host) return fail(NLSG_ERR_INVALID_ARG, "null argument");
  if (const int prc = e->params_ready()) return prc;
  NLSG_HIP(hipSetDevice(e->cfg.device));
  const uint64_t B = e->p.batch;
  return one_launch_minimize(e, e->p.x, B * e->p.D, x_inout_host, [&] { launch_solve(e); }, [&] {
    return download_rows(e->p.prob, B, status_host, [](const SannProblem &pr, uint64_t b) {
      return status_row(pr.best, pr.iter, pr.fcalls, b);
    });
  });
}

int nlsg_sann_time_solve(nlsg_sann *e, const double *x0_host, uint32_t repeats, float *ms_total) {
  if (!e || !x0_host || !ms_total) return fail(NLSG_ERR_INVALID_ARG, "null argument");
  if (const int prc = e->params_ready()) return prc;
  NLSG_HIP(hipSetDevice(e->cfg.device));
  return one_launch_time_solve(e, e->p.x, e->p.batch * e->p.D, x0_host, repeats, ms_total, [&] { launch_solve(e); });
}

}  // extern "C"
