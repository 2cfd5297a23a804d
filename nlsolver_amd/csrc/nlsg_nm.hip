// nlsolver_amd/csrc/nlsg_nm.hip — host side of the batched Nelder-Mead engine + C-ABI.
#include <cstdlib>

#include "nlsg_engine.h"
#include "nlsg_nm_kernels.h"
#include "nlsg_rtc.h"

using namespace nlsg;

struct nlsg_nm : EngineBase {  // (n_params: nlsg_nm_create_params, a row per start)
  NmRtcKernels rtc;  // objective == NLSG_OBJ_CUSTOM: the kernel hiprtc built for it
  nlsg_nm_config cfg;
  NmParams p;
  double *upper_dev = nullptr, *lower_dev = nullptr;
  size_t lds = 0;
  bool driver = false;  // n <= 128: nm_solve_driver_kernel (NLSG_NM_DRIVER=0: the phase-per-barrier kernel)
  unsigned long long *phase_dev = nullptr;  // from the first nlsg_nm_phase_cycles on
};

namespace {
// The opt-in for more than 64 KiB of dynamic LDS belongs to the kernel instantiation <OBJ, CHUNKS>,
// which every engine of that chunk class shares: it is set to the class maximum (the largest n the
// instantiation serves), never to one engine's size — a later, smaller engine must not lower it.
template <int OBJ>
hipError_t prepare(int chunks) {
  hipError_t he = hipErrorInvalidValue;  // (what a chunk count outside the list leaves)
  with_chunks(chunks, [&](auto C) {
    he = hipFuncSetAttribute(reinterpret_cast<const void *>(nm_solve_kernel<OBJ, C>),
                             hipFuncAttributeMaxDynamicSharedMemorySize,
                             160 * 1024);  // (reference order adds term buffers behind the image)
  });
  return he;
}
template <int OBJ>
hipError_t prepare_driver() {
  hipError_t he = hipFuncSetAttribute(reinterpret_cast<const void *>(nm_solve_driver_kernel<OBJ>),
                                      hipFuncAttributeMaxDynamicSharedMemorySize,
                                      static_cast<int>(nm_lds_bytes(128)));
  if constexpr (OBJ != NLSG_OBJ_RASTRIGIN)  // (reference order: term buffers behind the image)
    if (he == hipSuccess)
      he = hipFuncSetAttribute(reinterpret_cast<const void *>(nm_solve_driver_kernel<OBJ, true>),
                               hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
  return he;
}
void launch(nlsg_nm *e) {
  const dim3 grid(static_cast<unsigned>(e->p.batch)), block(nm_block_threads(e->p.n));
  if (e->cfg.objective == NLSG_OBJ_CUSTOM) {
    void *args[] = {&e->p};
    launch_module_kernel(e->rtc.solve, grid.x, block.x, static_cast<unsigned>(e->lds), e->stream, args);
    return;
  }
  routed(with_objective(e->cfg.objective, [&](auto O) {
    if (e->driver) {
      if constexpr (O != NLSG_OBJ_RASTRIGIN) {
        if (e->p.seq) {
          hipLaunchKernelGGL((nm_solve_driver_kernel<O, true>), grid, block, e->lds, e->stream, e->p);
          return true;
        }
      }
      hipLaunchKernelGGL(nm_solve_driver_kernel<O>, grid, block, e->lds, e->stream, e->p);
      return true;
    }
    return with_chunks(nm_chunks(e->p.n), [&](auto C) {
      hipLaunchKernelGGL((nm_solve_kernel<O, C>), grid, block, e->lds, e->stream, e->p);
    });
  }));
}

int upload_bounds(nlsg_nm *e, const double *upper_host, const double *lower_host) {
  if (!e->cfg.bounded) return NLSG_OK;
  if (!upper_host || !lower_host)
    return fail(NLSG_ERR_INVALID_ARG, "bounded solver needs upper and lower");
  NLSG_HIP(hipMemcpy(e->upper_dev, upper_host, e->p.n * 8, hipMemcpyHostToDevice));
  NLSG_HIP(hipMemcpy(e->lower_dev, lower_host, e->p.n * 8, hipMemcpyHostToDevice));
  return NLSG_OK;
}
}  // namespace

extern "C" {

static int nm_create(const nlsg_nm_config *cfg, const nlsg_custom_objective *custom, nlsg_nm **out,
                     bool with_params = false);

int nlsg_nm_create(const nlsg_nm_config *cfg, nlsg_nm **out) {
  if (const int rc = builtin_door(cfg, "nlsg_nm")) return rc;
  return nm_create(cfg, nullptr, out);
}

int nlsg_nm_create_custom(const nlsg_nm_config *cfg, const nlsg_custom_objective *obj, nlsg_nm **out) {
  if (const int rc = custom_door(cfg, obj, out)) return rc;
  return nm_create(cfg, obj, out);
}

int nlsg_nm_create_params(const nlsg_nm_config *cfg, const nlsg_custom_objective *obj, nlsg_nm **out) {
  if (const int rc = runtime_door(cfg, obj, out)) return rc;
  return nm_create(cfg, obj, out, true);
}

// The least dynamic LDS a launch of this shape takes (nm_launch_lds_bytes): the image, and in reference
// order one term buffer behind it — the driver wave's own; more waves get one as far as the CU's LDS goes.
uint64_t nlsg_nm_lds_bytes(uint64_t dim, uint32_t flags) {
  if (dim < 1 || dim > 1024 || (flags & ~NLSG_NM_REFERENCE_ORDER)) return 0;
  return nm_launch_lds_bytes(dim, 1, (flags & NLSG_NM_REFERENCE_ORDER) != 0);
}

int nlsg_nm_set_params(nlsg_nm *e, const double *params_host) { return set_params_entry(e, params_host); }

static int nm_create(const nlsg_nm_config *cfg, const nlsg_custom_objective *custom, nlsg_nm **out,
                     bool with_params) {
  if (!cfg || !out) return fail(NLSG_ERR_INVALID_ARG, "null argument");
  *out = nullptr;
  if (cfg->struct_size != sizeof(nlsg_nm_config))
    return fail(NLSG_ERR_INVALID_ARG, "nlsg_nm_config size mismatch (%u vs %zu)", cfg->struct_size,
                sizeof(nlsg_nm_config));
  if (!custom && (cfg->objective < 0 || cfg->objective > NLSG_OBJ_RASTRIGIN))
    return fail(NLSG_ERR_INVALID_ARG, "unknown objective %d", cfg->objective);
  if (cfg->dim < 1 || cfg->batch < 1) return fail(NLSG_ERR_INVALID_ARG, "dim and batch must be >= 1");
  if (cfg->dim > 1024)
    return fail(NLSG_ERR_UNSUPPORTED, "dim %llu > 1024 is not covered by the device path",
                (unsigned long long)cfg->dim);
  if (cfg->batch > 0x7fffffffull) return fail(NLSG_ERR_UNSUPPORTED, "batch too large");
  if (cfg->flags & ~NLSG_NM_REFERENCE_ORDER) return fail(NLSG_ERR_INVALID_ARG, "unknown flags 0x%x", cfg->flags);
  if ((cfg->flags & NLSG_NM_REFERENCE_ORDER) &&
      (cfg->objective == NLSG_OBJ_RASTRIGIN || (custom && custom->chain == NLSG_CUSTOM_VECTOR)))
    return fail(NLSG_ERR_UNSUPPORTED,
                "NLSG_NM_REFERENCE_ORDER needs an objective given by its terms whose arithmetic the device "
                "shares with the reference (not Rastrigin: its cosine is the device's own; not a whole-vector body)");
  if (with_params)
    if (const int prc = check_custom_params(custom, nlsg_nm_lds_bytes(cfg->dim, cfg->flags), "nlsg_nm",
                                            "nlsg_nm_create_custom"))
      return prc;
  nlsg_nm *e = nullptr;
  if (const int rc = open_engine(cfg->device, cfg->stream, "nlsg_nm", &e)) return rc;
  CreateGuard<nlsg_nm> guard(e, nlsg_nm_destroy);
  e->cfg = *cfg;
  NmParams &p = e->p;
  std::memset(&p, 0, sizeof p);
  const uint64_t B = cfg->batch, n = cfg->dim;
  const bool seq = (cfg->flags & NLSG_NM_REFERENCE_ORDER) != 0;
  // (the parameter row is static LDS of the run-time compiled module, in front of this dynamic block)
  e->n_params = with_params ? custom->n_params : 0;
  e->lds = nm_launch_lds_bytes(n, nm_block_threads(n) / 64, seq, custom_params_lds_bytes(e->n_params));
  DeviceOwner &own = e->own;
  hipError_t &he = own.err;
  const int chunks = nm_chunks(n);
  if (chunks > 1) own.alloc(&p.simplex, B * (n + 1) * n * 8);  // the simplexes themselves: past what LDS holds
  own.alloc(&p.x, B * n * 8);
  own.alloc(&p.prob, B * sizeof(NmProblem));
  own.alloc(&e->upper_dev, n * 8);
  own.alloc(&e->lower_dev, n * 8);
  e->alloc_params(B, e->n_params);
  e->timing_events();
  {
    const char *sw = std::getenv("NLSG_NM_DRIVER");
    e->driver = chunks == 1 && !(sw && sw[0] == '0');
  }
  if (he == hipSuccess) he = prepare_driver<NLSG_OBJ_ROSENBROCK>();
  if (he == hipSuccess) he = prepare_driver<NLSG_OBJ_SPHERE>();
  if (he == hipSuccess) he = prepare_driver<NLSG_OBJ_STYBLINSKI_TANG>();
  if (he == hipSuccess) he = prepare_driver<NLSG_OBJ_RASTRIGIN>();
  if (he == hipSuccess) he = prepare<NLSG_OBJ_ROSENBROCK>(chunks);
  if (he == hipSuccess) he = prepare<NLSG_OBJ_SPHERE>(chunks);
  if (he == hipSuccess) he = prepare<NLSG_OBJ_STYBLINSKI_TANG>(chunks);
  if (he == hipSuccess) he = prepare<NLSG_OBJ_RASTRIGIN>(chunks);
  if (he == hipSuccess && custom) {
    if (const int rc = rtc_build_nm(custom, e->driver ? 0 : chunks, seq, &e->rtc)) return rc;
    // the module API's counterpart of prepare<>(): allow the simplex-sized dynamic LDS
    if (const int rc = module_kernel_lds(e->rtc.solve, e->lds, "device setup failed: %s")) return rc;
  }
  if (const int rc = e->setup_status()) return rc;
  p.upper = e->upper_dev;
  p.lower = e->lower_dev;
  p.params = e->params_dev;
  p.batch = B;
  p.n = n;
  p.max_iter = cfg->max_iter;
  p.no_change_tol = cfg->no_change_best_tol;
  p.restarts = cfg->restarts;
  p.step = cfg->step;
  p.alpha = cfg->alpha;
  p.gamma = cfg->gamma;
  p.rho = cfg->rho;
  p.sigma = cfg->sigma;
  p.eps = cfg->eps;
  p.fmul = cfg->minimize ? 1.0 : -1.0;
  p.bounded = cfg->bounded ? 1 : 0;
  p.seq = 0;
  if (seq) {
    const char *sw = std::getenv("NLSG_NM_SEQ_WAVES");
    const int w = sw ? std::atoi(sw) : 16;
    p.seq = w < 1 ? 1 : (w > 16 ? 16 : w);
  }
  *out = guard.release();
  return NLSG_OK;
}

int nlsg_nm_destroy(nlsg_nm *e) { return destroy_engine(e); }

int nlsg_nm_minimize(nlsg_nm *e, double *x_inout_host, const double *upper_host,
                     const double *lower_host, nlsg_status *status_host, double *eps_out_host) {
  if (!e || !x_inout_host) return fail(NLSG_ERR_INVALID_ARG, "null argument");
  if (const int prc = e->params_ready()) return prc;
  NLSG_HIP(hipSetDevice(e->cfg.device));
  if (const int rc = upload_bounds(e, upper_host, lower_host)) return rc;
  const uint64_t B = e->p.batch;
  return one_launch_minimize(e, e->p.x, B * e->p.n, x_inout_host, [&] { launch(e); }, [&] {
    return download_rows(
        e->p.prob, B, status_host,
        [](const NmProblem &pr, uint64_t b) {
          nlsg_status st = status_row(pr.f, pr.iter, pr.fcalls, b);
          st.std_err = pr.eps;
          return st;
        },
        [&](const NmProblem &pr, uint64_t b) {
          if (eps_out_host) eps_out_host[b] = pr.eps;
        });
  });
}

int nlsg_nm_phase_cycles(nlsg_nm *e, const double *x0_host, uint64_t *cycles_host) {
  if (!e || !x0_host || !cycles_host) return fail(NLSG_ERR_INVALID_ARG, "null argument");
  if (const int prc = e->params_ready()) return prc;
  NLSG_HIP(hipSetDevice(e->cfg.device));
  const uint64_t B = e->p.batch;
  // a measurement aid: its buffer exists from its first use on, and it profiles the unbounded
  // solve only (a bounded engine would run on whatever bounds its last minimize left behind)
  if (e->cfg.bounded) return fail(NLSG_ERR_UNSUPPORTED, "nlsg_nm_phase_cycles profiles unbounded engines");
  if (!e->phase_dev) NLSG_HIP(e->own.take(&e->phase_dev, B * kNmPhases * 8));
  NLSG_HIP(hipMemcpy(e->p.x, x0_host, B * e->p.n * 8, hipMemcpyHostToDevice));
  NLSG_HIP(hipMemset(e->phase_dev, 0, B * kNmPhases * 8));
  e->p.phase = e->phase_dev;
  launch(e);
  e->p.phase = nullptr;
  NLSG_HIP(launches_status());
  NLSG_HIP(hipStreamSynchronize(e->stream));
  NLSG_HIP(hipMemcpy(cycles_host, e->phase_dev, B * kNmPhases * 8, hipMemcpyDeviceToHost));
  return NLSG_OK;
}

int nlsg_nm_time_solve(nlsg_nm *e, const double *x0_host, uint32_t repeats, float *ms_total) {
  if (!e || !x0_host || !ms_total) return fail(NLSG_ERR_INVALID_ARG, "null argument");
  if (const int prc = e->params_ready()) return prc;
  NLSG_HIP(hipSetDevice(e->cfg.device));
  return one_launch_time_solve(e, e->p.x, e->p.batch * e->p.n, x0_host, repeats, ms_total, [&] { launch(e); });
}

}  // extern "C"
