// nlsolver_amd/csrc/nlsg_nmpso.hip — host side of the batched Nelder-Mead / PSO hybrid + C-ABI.
#include "nlsg_engine.h"
#include "nlsg_nmpso_kernels.h"
#include "nlsg_rtc.h"

using namespace nlsg;

struct nlsg_nmpso : EngineBase {  // (n_params: nlsg_nmpso_create_params, a row per instance)
  nlsg_nmpso_config cfg;
  HybParams p;
  double *upper_dev = nullptr, *lower_dev = nullptr, *zero_dev = nullptr;
  HybRtcKernels rtc;  // objective == NLSG_OBJ_CUSTOM: the kernel hiprtc built for it
};

namespace {

int wide_chunks(uint64_t n) { return n <= kHybMaxN ? 0 : n <= 256 ? 2 : n <= 512 ? 4 : 8; }

// the wide kernel <OBJ, C> of a built-in objective at n > kHybMaxN: f(O, C)
template <typename F>
bool with_wide_kernel(int objective, uint64_t n, F &&f) {
  return with_objective(objective, [&](auto O) {
    return with_value<2, 4, 8>(wide_chunks(n), [&](auto C) { return dispatch_call(f, O, C); });
  });
}

void launch(nlsg_nmpso *e) {
  const bool wide = e->p.n > kHybMaxN;
  const dim3 grid(static_cast<unsigned>(e->p.batch)),
      block(wide ? hyb_wide_threads(wide_chunks(e->p.n)) : hyb_block_threads(e->p.n));
  if (e->cfg.objective == NLSG_OBJ_CUSTOM) {
    void *args[] = {&e->p};
    launch_module_kernel(e->rtc.solve, grid.x, block.x,
                         wide ? static_cast<unsigned>(hyb_view_bytes(e->p.n)) : 0, e->stream, args);
    return;
  }
  if (wide) {
    const unsigned lds = static_cast<unsigned>(hyb_view_bytes(e->p.n));
    routed(with_wide_kernel(e->cfg.objective, e->p.n, [&](auto O, auto C) {
      hipLaunchKernelGGL((nmpso_solve_wide_kernel<O, C>), grid, block, lds, e->stream, e->p);
    }));
    return;
  }
  routed(with_objective(e->cfg.objective, [&](auto O) {
    hipLaunchKernelGGL(nmpso_solve_kernel<O>, grid, block, 0, e->stream, e->p);
  }));
}

int upload_bounds(nlsg_nmpso *e, const double *lower_host, const double *upper_host) {
  if (!e->p.bounded) return NLSG_OK;
  if (!lower_host || !upper_host)
    return fail(NLSG_ERR_INVALID_ARG, "a bounded engine needs lower and upper");
  NLSG_HIP(hipMemcpy(e->lower_dev, lower_host, e->p.n * 8, hipMemcpyHostToDevice));
  NLSG_HIP(hipMemcpy(e->upper_dev, upper_host, e->p.n * 8, hipMemcpyHostToDevice));
  return NLSG_OK;
}

}  // namespace

static int hyb_create(const nlsg_nmpso_config *cfg, const nlsg_custom_objective *custom,
                      nlsg_nmpso **out, bool with_params = false);

extern "C" {

int nlsg_nmpso_create(const nlsg_nmpso_config *cfg, nlsg_nmpso **out) {
  if (const int rc = builtin_door(cfg, "nlsg_nmpso")) return rc;
  return hyb_create(cfg, nullptr, out);
}

int nlsg_nmpso_create_custom(const nlsg_nmpso_config *cfg, const nlsg_custom_objective *obj,
                             nlsg_nmpso **out) {
  if (const int rc = custom_door(cfg, obj, out)) return rc;
  return hyb_create(cfg, obj, out);
}

int nlsg_nmpso_create_params(const nlsg_nmpso_config *cfg, const nlsg_custom_objective *obj,
                             nlsg_nmpso **out) {
  if (const int rc = runtime_door(cfg, obj, out)) return rc;
  return hyb_create(cfg, obj, out, true);
}

// the workgroup's LDS: the packed kernel's static block (n <= 128), the wide kernels' dynamic view beyond
uint64_t nlsg_nmpso_lds_bytes(uint64_t dim) {
  if (dim < 2 || dim > kHybWideMaxN) return 0;
  return dim <= kHybMaxN ? sizeof(HybShared) : hyb_view_bytes(dim);
}

int nlsg_nmpso_set_params(nlsg_nmpso *e, const double *params_host) { return set_params_entry(e, params_host); }

}  // extern "C"

static int hyb_create(const nlsg_nmpso_config *cfg, const nlsg_custom_objective *custom,
                      nlsg_nmpso **out, bool with_params) {
  if (!cfg || !out) return fail(NLSG_ERR_INVALID_ARG, "null argument");
  *out = nullptr;
  if (cfg->struct_size != sizeof(nlsg_nmpso_config))
    return fail(NLSG_ERR_INVALID_ARG, "nlsg_nmpso_config size mismatch (%u vs %zu)",
                cfg->struct_size, sizeof(nlsg_nmpso_config));
  if (!custom && (cfg->objective < 0 || cfg->objective > NLSG_OBJ_RASTRIGIN))
    return fail(NLSG_ERR_INVALID_ARG, "unknown objective %d", cfg->objective);
  if (cfg->batch < 1) return fail(NLSG_ERR_INVALID_ARG, "batch must be >= 1");
  if (cfg->dim < 2)  // the reference refuses it too (3627-3637)
    return fail(NLSG_ERR_INVALID_ARG, "dim must be >= 2: the hybrid does not support one dimension");
  if (cfg->dim > kHybWideMaxN)
    return fail(NLSG_ERR_UNSUPPORTED, "dim %llu > %d (an instance's sort keys, orders and trial "
                "points live in one workgroup's shared memory)", (unsigned long long)cfg->dim,
                kHybWideMaxN);
  if (cfg->batch > 0x7fffffffull) return fail(NLSG_ERR_UNSUPPORTED, "batch too large");
  if (with_params)
    if (const int prc = check_custom_params(custom, nlsg_nmpso_lds_bytes(cfg->dim), "nlsg_nmpso",
                                            "nlsg_nmpso_create_custom"))
      return prc;
  nlsg_nmpso *e = nullptr;
  if (const int rc = open_engine(cfg->device, cfg->stream, "nlsg_nmpso", &e)) return rc;
  CreateGuard<nlsg_nmpso> guard(e, nlsg_nmpso_destroy);
  e->cfg = *cfg;
  e->n_params = with_params ? custom->n_params : 0;
  HybParams &p = e->p;
  std::memset(&p, 0, sizeof p);
  const uint64_t B = cfg->batch, n = cfg->dim, rows = B * (3 * n + 1);
  DeviceOwner &own = e->own;
  hipError_t &he = own.err;
  own.alloc(&p.x, B * n * 8);
  own.alloc(&p.pos, rows * n * 8);
  own.alloc(&p.vel, rows * n * 8);
  own.alloc(&p.prob, B * sizeof(HybProblem));
  own.alloc(&e->upper_dev, n * 8);
  own.alloc(&e->lower_dev, n * 8);
  own.zeroed(&e->zero_dev, 16);
  e->alloc_params(B, e->n_params);
  e->timing_events();
  if (he == hipSuccess && n > kHybMaxN && !custom) {  // past 64 KiB the dynamic allocation has to be announced
    // the attribute belongs to the instantiation, shared by every engine of the chunk class: the class
    // maximum, so that an engine created later with a smaller n cannot lower an earlier one's limit
    he = hipErrorInvalidValue;  // (what a value outside the lists leaves)
    with_wide_kernel(cfg->objective, n, [&](auto O, auto C) {
      he = hipFuncSetAttribute(reinterpret_cast<const void *>(nmpso_solve_wide_kernel<O, C>),
                               hipFuncAttributeMaxDynamicSharedMemorySize,
                               static_cast<int>(hyb_view_bytes(128ull * C)));
    });
  }
  if (const int rc = e->setup_status()) return rc;
  if (custom)
    if (const int rc = rtc_build_nmpso(custom, wide_chunks(n), &e->rtc)) return rc;
  p.upper = e->upper_dev;
  p.lower = e->lower_dev;
  p.zero = e->zero_dev;
  p.params = e->params_dev;
  p.batch = B;
  p.n = n;
  p.max_iter = cfg->max_iter;
  p.no_change_iter = cfg->no_change_best_iter;
  p.seed = cfg->seed;
  p.inst_lo = cfg->inst_lo;
  p.alpha = cfg->alpha;
  p.gamma = cfg->gamma;
  p.rho = cfg->rho;
  p.sigma = cfg->sigma;
  p.inertia = cfg->inertia;
  p.cog = cfg->cognitive;
  p.soc = cfg->social;
  p.eps = cfg->eps;
  p.fmul = cfg->minimize ? 1.0 : -1.0;
  p.bounded = cfg->bounded ? 1 : 0;
  *out = guard.release();
  return NLSG_OK;
}

extern "C" {

int nlsg_nmpso_destroy(nlsg_nmpso *e) { return destroy_engine(e); }

int nlsg_nmpso_minimize(nlsg_nmpso *e, double *x_inout_host, const double *lower_host,
                        const double *upper_host, nlsg_status *status_host) {
  if (!e || !x_inout_host) return fail(NLSG_ERR_INVALID_ARG, "null argument");
  if (const int prc = e->params_ready()) return prc;
  NLSG_HIP(hipSetDevice(e->cfg.device));
  if (const int rc = upload_bounds(e, lower_host, upper_host)) return rc;
  const uint64_t B = e->p.batch;
  return one_launch_minimize(e, e->p.x, B * e->p.n, x_inout_host, [&] { launch(e); }, [&] {
    return download_rows(e->p.prob, B, status_host,
                         [](const HybProblem &pr, uint64_t b) { return status_row(pr.f, pr.iter, pr.fcalls, b); });
  });
}

int nlsg_nmpso_time_solve(nlsg_nmpso *e, const double *x0_host, uint32_t repeats, float *ms_total) {
  if (!e || !x0_host || !ms_total) return fail(NLSG_ERR_INVALID_ARG, "null argument");
  if (const int prc = e->params_ready()) return prc;
  if (e->p.bounded) return fail(NLSG_ERR_UNSUPPORTED, "timing aid of the unbounded overloads");
  NLSG_HIP(hipSetDevice(e->cfg.device));
  return one_launch_time_solve(e, e->p.x, e->p.batch * e->p.n, x0_host, repeats, ms_total, [&] { launch(e); });
}

}  // extern "C"
