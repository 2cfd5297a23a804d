// nlsolver_amd/csrc/nlsg_bfgs.hip — host side of the batched BFGS engine + C-ABI.
#include <algorithm>
#include <vector>

#include "nlsg_bfgs_kernels.h"
#include "nlsg_engine.h"
#include "nlsg_rtc.h"

using namespace nlsg;

struct nlsg_bfgs : EngineBase {  // (n_params: nlsg_bfgs_create_params, a row per problem)
  BfgsRtcKernels rtc;  // objective == NLSG_OBJ_CUSTOM: the kernels hiprtc built (finite differences, or the
                       // objective's gradient body: nlsg_bfgs_create_gradient)
  nlsg_bfgs_config cfg;
  BfgsParams p;
  double *qd_dev = nullptr, *qb_dev = nullptr, *zero_dev = nullptr;
  unsigned long long *count_dev = nullptr;
  int chunks = 0;
  bool vec = false, initialised = false;
  uint32_t bpp = 0;  // blocks per problem in the H-streaming kernels
  bool symmetric = false;  // NLSG_BFGS_SYMMETRIC: upper blocks of H only
  hipEvent_t ev2 = nullptr, ev3 = nullptr;  // around the H kernels of a timed iteration
  unsigned fd_lds = 0;  // dynamic LDS of the module's search / init launches: the reference-order buffers,
                        // and behind them a parameter row per wave
  bool resident = false;   // NLSG_BFGS_RESIDENT: the whole loop in bfgs_resident_kernel, H in LDS
  BfgsResidentLayout res{};  // its dynamic LDS block (doubles)
};

namespace {

// the row width class and the row alignment of an engine's kernels: f(C, V)
template <typename F>
bool with_row_shape(const nlsg_bfgs *e, F &&f) {
  return with_chunks(e->chunks, [&](auto C) {
    return with_bool(e->vec, [&](auto V) { return dispatch_call(f, C, V); });
  });
}

// what is minimised, for the kernels that evaluate it: the quadratic or a built-in objective
template <typename F>
bool with_model(int model, F &&f) {
  return with_value<kBfgsQuad, NLSG_OBJ_ROSENBROCK, NLSG_OBJ_SPHERE, NLSG_OBJ_STYBLINSKI_TANG, NLSG_OBJ_RASTRIGIN>(
      model, std::forward<F>(f));
}

// search / init kernels depend on the row shape and on what is minimised: launch(C, V, M, lds)
template <typename Launch>
bool with_model_kernel(const nlsg_bfgs *e, Launch &&launch) {
  return with_row_shape(e, [&](auto C, auto V) {
    const unsigned fd_lds = e->p.seq ? static_cast<unsigned>(bfgs_fd_seq_lds_bytes(C)) : 0u;
    return with_model(e->p.model, [&](auto M) { launch(C, V, M, fd_lds); });
  });
}

// one resident launch: every unfinished problem makes up to `iters` turns
// (the resident kernel: CHUNKS = 1 only, a 64-lane workgroup per problem)
void launch_resident(nlsg_bfgs *e, uint32_t iters) {
  const unsigned lds_ = e->res.total * static_cast<unsigned>(sizeof(double));
  if (e->p.model == NLSG_OBJ_CUSTOM) {
    void *args[] = {&e->p, &iters, &e->res.h_at, &e->res.vec_at};
    launch_module_kernel(e->rtc.resident, static_cast<unsigned>(e->p.batch), 64, lds_, e->stream, args);
    return;
  }
  routed(with_bool(e->vec, [&](auto V) {
    return with_model(e->p.model, [&](auto M) {
      hipLaunchKernelGGL((bfgs_resident_kernel<1, V, M>), dim3(static_cast<unsigned>(e->p.batch)), dim3(64), lds_,
                         e->stream, e->p, iters, e->res.h_at, e->res.vec_at);
    });
  }));
}

void launch_iteration(nlsg_bfgs *e, bool timed) {
  const unsigned wave_grid = static_cast<unsigned>((e->p.batch + 3) / 4);
  const unsigned row_grid = static_cast<unsigned>(e->p.batch * e->bpp);
  if (e->p.model == NLSG_OBJ_CUSTOM) {
    void *args[] = {&e->p};
    launch_module_kernel(e->rtc.search, wave_grid, 256, e->fd_lds, e->stream, args);
  } else {
    routed(with_model_kernel(e, [&](auto C, auto V, auto M, unsigned fd_lds) {
      hipLaunchKernelGGL((bfgs_search_kernel<C, V, M>), dim3(wave_grid), dim3(256), fd_lds, e->stream, e->p);
    }));
  }
  if (timed) hipEventRecord(e->ev2, e->stream);
  if (e->symmetric) {
    const dim3 blocks(static_cast<unsigned>(e->p.batch * e->p.nstored)), probs(static_cast<unsigned>(e->p.batch));
    hipLaunchKernelGGL(bfgs_sym_hy_kernel, blocks, dim3(256), 0, e->stream, e->p);
    hipLaunchKernelGGL(bfgs_sym_reduce_kernel<false>, probs, dim3(256), 0, e->stream, e->p);
    hipLaunchKernelGGL(bfgs_sym_update_kernel, blocks, dim3(256), 0, e->stream, e->p);
    hipLaunchKernelGGL(bfgs_sym_reduce_kernel<true>, probs, dim3(256), 0, e->stream, e->p);
  } else if (e->p.seq) {  // reference order: a lane per row (nlsg_bfgs_kernels.h "at streaming speed")
    const uint64_t n = e->p.n;
    const uint32_t bpp = bfgs_seq_blocks_per_problem(n);
    const dim3 grid(static_cast<unsigned>(e->p.batch * bpp)), probs(static_cast<unsigned>(e->p.batch));
    const unsigned lds1 = static_cast<unsigned>(bfgs_seq_h_lds_bytes(n, kBfgsSeqColsHy));
    const unsigned lds3 = static_cast<unsigned>(bfgs_seq_h_lds_bytes(n, kBfgsSeqColsUpdate));
    if (e->vec) {
      hipLaunchKernelGGL(bfgs_hy_seq_kernel<true>, grid, dim3(256), lds1, e->stream, e->p, bpp);
      hipLaunchKernelGGL(bfgs_denom_seq_kernel, probs, dim3(64), static_cast<unsigned>(n * sizeof(double)), e->stream, e->p);
      hipLaunchKernelGGL(bfgs_update_seq_kernel<true>, grid, dim3(256), lds3, e->stream, e->p, bpp);
    } else {
      hipLaunchKernelGGL(bfgs_hy_seq_kernel<false>, grid, dim3(256), lds1, e->stream, e->p, bpp);
      hipLaunchKernelGGL(bfgs_denom_seq_kernel, probs, dim3(64), static_cast<unsigned>(n * sizeof(double)), e->stream, e->p);
      hipLaunchKernelGGL(bfgs_update_seq_kernel<false>, grid, dim3(256), lds3, e->stream, e->p, bpp);
    }
  } else {
    routed(with_row_shape(e, [&](auto C, auto V) {
      hipLaunchKernelGGL((bfgs_hy_kernel<C, V>), dim3(row_grid), dim3(256), 0, e->stream, e->p, e->bpp);
      hipLaunchKernelGGL((bfgs_update_kernel<C, V>), dim3(row_grid), dim3(256), 0, e->stream, e->p, e->bpp);
    }));
  }
  if (timed) hipEventRecord(e->ev3, e->stream);
}

// the unfinished problems a kernel counts into count_dev (kernel(p, count_dev), a thread per problem)
template <typename Kernel>
int count_problems(nlsg_bfgs *e, Kernel kernel, uint64_t *count) {
  if (!e || !count) return fail(NLSG_ERR_INVALID_ARG, "null argument");
  if (!e->initialised) return fail(NLSG_ERR_STATE, "nlsg_bfgs_init has not been called");
  NLSG_HIP(hipSetDevice(e->cfg.device));
  return device_count(e->stream, e->count_dev, count, [&] {
    hipLaunchKernelGGL(kernel, dim3(static_cast<unsigned>((e->p.batch + 255) / 256)), dim3(256), 0, e->stream, e->p,
                       e->count_dev);
  });
}

}  // namespace

extern "C" {

static int bfgs_create(const nlsg_bfgs_config *cfg, const double *diag_host, const double *lin_host,
                       const nlsg_custom_objective *custom, nlsg_bfgs **out, bool with_params = false,
                       const char *grad_body = nullptr);

int nlsg_bfgs_create(const nlsg_bfgs_config *cfg, const double *diag_host, const double *lin_host,
                     nlsg_bfgs **out) {
  if (const int rc = builtin_door(cfg, "nlsg_bfgs")) return rc;
  return timed_create([&] { return bfgs_create(cfg, diag_host, lin_host, nullptr, out); });
}

int nlsg_bfgs_create_custom(const nlsg_bfgs_config *cfg, const nlsg_custom_objective *obj,
                            nlsg_bfgs **out) {
  if (const int rc = custom_door(cfg, obj, out)) return rc;
  return timed_create([&] { return bfgs_create(cfg, nullptr, nullptr, obj, out); });
}

int nlsg_bfgs_create_params(const nlsg_bfgs_config *cfg, const nlsg_custom_objective *obj,
                            nlsg_bfgs **out) {
  if (const int rc = runtime_door(cfg, obj, out)) return rc;
  return timed_create([&] { return bfgs_create(cfg, nullptr, nullptr, obj, out, true); });
}

// The objective with its gradient as a second body: the kernels evaluate it instead of finite differences.
// Parameters are optional here (n_params == 0 is an objective without any).
int nlsg_bfgs_create_gradient(const nlsg_bfgs_config *cfg, const nlsg_custom_objective *obj,
                              const nlsg_bfgs_gradient *grad, nlsg_bfgs **out) {
  if (!grad) return fail(NLSG_ERR_INVALID_ARG, "null argument");
  if (const int rc = runtime_door(cfg, obj, out)) return rc;
  if (grad->struct_size != sizeof(nlsg_bfgs_gradient))
    return fail(NLSG_ERR_INVALID_ARG, "nlsg_bfgs_gradient size mismatch (%u vs %zu)", grad->struct_size,
                sizeof(nlsg_bfgs_gradient));
  if (!grad->grad_body || !grad->grad_body[0])
    return fail(NLSG_ERR_INVALID_ARG, "nlsg_bfgs_create_gradient needs a gradient body (finite differences are "
                "nlsg_bfgs_create_custom's)");
  return timed_create([&] { return bfgs_create(cfg, nullptr, nullptr, obj, out, obj->n_params != 0, grad->grad_body); });
}

// The dynamic LDS of a search / init launch without parameter rows: the four waves' reference-order
// buffers, or nothing. 0 also outside 1 <= dim <= 1024, for unknown flags and for reference order with
// the symmetric restatement (which the engine rejects).
// With NLSG_BFGS_RESIDENT: the resident workgroup's block without its parameter row — never 0 for a shape the
// engine takes, 0 for dim > 64 and with the symmetric restatement (a library older than the mode answers 0 to
// the flag it does not know: the probe for the mode is nlsg_bfgs_lds_bytes(2, NLSG_BFGS_RESIDENT) != 0).
uint64_t nlsg_bfgs_lds_bytes(uint64_t dim, uint32_t flags) {
  if (dim < 1 || dim > 1024 ||
      (flags & ~(NLSG_BFGS_SYMMETRIC | NLSG_BFGS_REFERENCE_ORDER | NLSG_BFGS_RESIDENT)))
    return 0;
  if (flags & NLSG_BFGS_RESIDENT) {
    if (dim > kBfgsResidentMaxDim || (flags & NLSG_BFGS_SYMMETRIC)) return 0;
    return bfgs_resident_layout(dim, (flags & NLSG_BFGS_REFERENCE_ORDER) ? 1 : 0, 0).total * sizeof(double);
  }
  if (!(flags & NLSG_BFGS_REFERENCE_ORDER) || (flags & NLSG_BFGS_SYMMETRIC)) return 0;
  return bfgs_fd_seq_lds_bytes(row_chunks(dim));
}

int nlsg_bfgs_set_params(nlsg_bfgs *e, const double *params_host) { return set_params_entry(e, params_host); }

static int bfgs_create(const nlsg_bfgs_config *cfg, const double *diag_host, const double *lin_host,
                       const nlsg_custom_objective *custom, nlsg_bfgs **out, bool with_params,
                       const char *grad_body) {
  if (!cfg || !out) return fail(NLSG_ERR_INVALID_ARG, "null argument");
  *out = nullptr;
  if (cfg->struct_size != sizeof(nlsg_bfgs_config))
    return fail(NLSG_ERR_INVALID_ARG, "nlsg_bfgs_config size mismatch (%u vs %zu)",
                cfg->struct_size, sizeof(nlsg_bfgs_config));
  const bool quad = cfg->objective == NLSG_OBJ_QUAD_DIAG_RANK1;
  const bool fd = cfg->objective == NLSG_OBJ_ROSENBROCK || cfg->objective == NLSG_OBJ_SPHERE ||
                  cfg->objective == NLSG_OBJ_STYBLINSKI_TANG || cfg->objective == NLSG_OBJ_RASTRIGIN ||
                  custom != nullptr;
  if (!quad && !fd) return fail(NLSG_ERR_INVALID_ARG, "unknown objective %d", cfg->objective);
  if (quad && (!diag_host || !lin_host))
    return fail(NLSG_ERR_INVALID_ARG, "the quadratic needs its d and b vectors");
  if (cfg->dim < 1 || cfg->batch < 1) return fail(NLSG_ERR_INVALID_ARG, "dim and batch must be >= 1");
  if (cfg->dim > 1024)
    return fail(NLSG_ERR_UNSUPPORTED, "dim %llu > 1024 is not covered by the device path",
                (unsigned long long)cfg->dim);
  const bool seq = (cfg->flags & NLSG_BFGS_REFERENCE_ORDER) != 0;
  if (cfg->flags & ~(NLSG_BFGS_SYMMETRIC | NLSG_BFGS_REFERENCE_ORDER | NLSG_BFGS_RESIDENT))
    return fail(NLSG_ERR_INVALID_ARG, "unknown flags 0x%x", cfg->flags);
  const bool resident = (cfg->flags & NLSG_BFGS_RESIDENT) != 0;
  if (seq && (cfg->flags & NLSG_BFGS_SYMMETRIC))
    return fail(NLSG_ERR_INVALID_ARG,
                "NLSG_BFGS_REFERENCE_ORDER reproduces the reference's literal arithmetic; the symmetric "
                "restatement is a different one");
  if (seq && custom && custom->chain == NLSG_CUSTOM_VECTOR)
    return fail(NLSG_ERR_UNSUPPORTED,
                "NLSG_BFGS_REFERENCE_ORDER needs an objective given by its terms (x.sum() of a "
                "whole-vector body adds in the lane-tree order)");
  if (seq && cfg->objective == NLSG_OBJ_RASTRIGIN)
    return fail(NLSG_ERR_UNSUPPORTED,
                "NLSG_BFGS_REFERENCE_ORDER: Rastrigin's cosine is the device's deterministic one, not "
                "libm's — there is no reference arithmetic to reproduce");
  if (resident && (cfg->flags & NLSG_BFGS_SYMMETRIC))
    return fail(NLSG_ERR_INVALID_ARG,
                "NLSG_BFGS_RESIDENT keeps the literal update's whole matrix in LDS; the symmetric restatement "
                "is the streaming engine's");
  if (resident && cfg->dim > kBfgsResidentMaxDim)
    return fail(NLSG_ERR_UNSUPPORTED, "NLSG_BFGS_RESIDENT holds a problem of at most %d coordinates in LDS, not %llu",
                kBfgsResidentMaxDim, (unsigned long long)cfg->dim);
  if (grad_body && custom->n_params < 0)  // (zero is an objective without parameters: no row, no check)
    return fail(NLSG_ERR_INVALID_ARG, "n_params = %d: nlsg_bfgs_create_gradient takes 0 .. %d parameters",
                custom->n_params, NLSG_CUSTOM_MAX_PARAMS);
  if (with_params)  // (a row per wave, four to the block, behind the reference-order buffers; the resident
                    // workgroup is one wave with one row)
    if (const int prc = check_custom_params(custom, nlsg_bfgs_lds_bytes(cfg->dim, cfg->flags), "nlsg_bfgs",
                                            "nlsg_bfgs_create_custom", resident ? 1 : 4))
      return prc;
  nlsg_bfgs *e = nullptr;
  if (const int rc = open_engine(cfg->device, cfg->stream, "nlsg_bfgs", &e)) return rc;
  CreateGuard<nlsg_bfgs> guard(e, nlsg_bfgs_destroy);
  e->cfg = *cfg;
  const uint64_t n = cfg->dim, B = cfg->batch;
  e->chunks = row_chunks(n);
  e->n_params = with_params ? custom->n_params : 0;
  // the launch's dynamic block: the reference-order buffers, then the rows — ONE layout, from which both the
  // launch size and the offset the kernels are compiled with (NLSG_PARAMS_PER_WAVE) are taken
  const size_t rows_at = seq ? bfgs_fd_seq_lds_bytes(e->chunks) : 0;
  e->fd_lds = static_cast<unsigned>(rows_at + 4 * custom_params_lds_bytes(e->n_params));
  // (the resident kernel's row sits where the init kernel's first wave has its own: bfgs_resident_layout)
  e->resident = resident;
  e->res = bfgs_resident_layout(n, seq ? 1 : 0, custom_params_lds_bytes(e->n_params) / sizeof(double));
  e->vec = n % 2 == 0;
  e->bpp = static_cast<uint32_t>((n + 4 * kBfgsRowsPerWave - 1) / (4 * kBfgsRowsPerWave));
  e->symmetric = (cfg->flags & NLSG_BFGS_SYMMETRIC) != 0;
  const uint32_t nb = static_cast<uint32_t>((n + kBfgsSymB - 1) / kBfgsSymB), nstored = nb * (nb + 1) / 2;
  if (B * e->bpp > 0x7fffffffull || B * nstored > 0x7fffffffull)
    return fail(NLSG_ERR_UNSUPPORTED, "batch * dim too large for one launch grid");
  BfgsParams &p = e->p;
  std::memset(&p, 0, sizeof p);
  p.ldh = seq && (n * sizeof(double)) % 4096 == 0 ? n + 16 : n;  // (BfgsParams::ldh)
  DeviceOwner &own = e->own;
  hipError_t &he = own.err;
  auto alloc = [&](auto **ptr, size_t bytes) { own.alloc(ptr, bytes ? bytes : 8); };
  const size_t vec_bytes = B * n * sizeof(double);
  if (!e->symmetric) alloc(&p.H, B * n * p.ldh * sizeof(double));
  if (e->symmetric) alloc(&p.Hs, B * nstored * kBfgsSymB * kBfgsSymB * sizeof(double));
  if (e->symmetric) alloc(&p.part, B * nb * nb * kBfgsSymB * sizeof(double));
  alloc(&p.x, vec_bytes);
  alloc(&p.g, vec_bytes);
  alloc(&p.dir, vec_bytes);
  alloc(&p.s, vec_bytes);
  alloc(&p.y, vec_bytes);
  alloc(&p.t, vec_bytes);
  if (he == hipSuccess) he = hipMemset(p.dir, 0, vec_bytes);
  alloc(&p.prob, B * sizeof(BfgsProblem));
  alloc(&e->qd_dev, n * sizeof(double));
  alloc(&e->qb_dev, n * sizeof(double));
  own.zeroed(&e->zero_dev, 16);
  alloc(&e->count_dev, 8);
  e->alloc_params(B, e->n_params);
  if (he == hipSuccess)
    he = quad ? hipMemcpy(e->qd_dev, diag_host, n * sizeof(double), hipMemcpyHostToDevice)
              : hipMemset(e->qd_dev, 0, n * sizeof(double));
  if (he == hipSuccess)
    he = quad ? hipMemcpy(e->qb_dev, lin_host, n * sizeof(double), hipMemcpyHostToDevice)
              : hipMemset(e->qb_dev, 0, n * sizeof(double));
  e->timing_events();
  own.event(&e->ev2);
  own.event(&e->ev3);
  if (const int rc = e->setup_status("device allocation failed: %s")) return rc;
  p.qd = e->qd_dev;
  p.qb = e->qb_dev;
  p.zero = e->zero_dev;
  p.params = e->params_dev;
  p.batch = B;
  p.n = n;
  p.max_iter = cfg->max_iter;
  p.grad_eps = cfg->grad_eps;
  p.alpha = cfg->alpha;
  p.qc = cfg->quad_c;
  p.model = quad ? kBfgsQuad : cfg->objective;
  p.seq = seq ? 1 : 0;
  p.nb = nb;
  p.nstored = nstored;
  if (custom) {
    if (const int rc = rtc_build_bfgs(custom, e->chunks, e->vec, static_cast<long>(rows_at / sizeof(double)), &e->rtc,
                                      grad_body, resident))
      return rc;
    // four rows of parameters go past the 64 KiB a launch may take without the opt-in
    const char *raising = "raising the kernels' dynamic LDS limit failed: %s";
    if (const int rc = module_kernel_lds(e->rtc.search, e->fd_lds, raising, true)) return rc;
    if (const int rc = module_kernel_lds(e->rtc.init, e->fd_lds, raising, true)) return rc;
    // (only a module kernel has a parameter row: the built-in resident kernels stay below 64 KiB)
    if (resident)
      if (const int rc = module_kernel_lds(e->rtc.resident, e->res.total * sizeof(double),
                                           "raising the resident kernel's dynamic LDS limit failed: %s", true))
        return rc;
  }
  *out = guard.release();
  return NLSG_OK;
}

int nlsg_bfgs_destroy(nlsg_bfgs *e) { return timed_destroy(e); }

int nlsg_bfgs_init(nlsg_bfgs *e, const double *x0_host) {
  if (!e || !x0_host) return fail(NLSG_ERR_INVALID_ARG, "null argument");
  if (const int prc = e->params_ready()) return prc;
  NLSG_HIP(hipSetDevice(e->cfg.device));
  NLSG_HIP(hipMemcpyAsync(e->p.x, x0_host, e->p.batch * e->p.n * sizeof(double),
                          hipMemcpyHostToDevice, e->stream));
  NLSG_HIP(hipStreamSynchronize(e->stream));
  if (e->p.model == NLSG_OBJ_CUSTOM) {
    void *args[] = {&e->p};
    launch_module_kernel(e->rtc.init, static_cast<unsigned>((e->p.batch + 3) / 4), 256, e->fd_lds, e->stream,
                         args);
  } else {
    routed(with_model_kernel(e, [&](auto C, auto V, auto M, unsigned fd_lds) {
      hipLaunchKernelGGL((bfgs_init_kernel<C, V, M>), dim3(static_cast<unsigned>((e->p.batch + 3) / 4)), dim3(256),
                         fd_lds, e->stream, e->p);
    }));
  }
  NLSG_HIP(launches_status());
  e->initialised = true;
  return NLSG_OK;
}

int nlsg_bfgs_step(nlsg_bfgs *e, uint64_t iters) {
  if (!e) return fail(NLSG_ERR_INVALID_ARG, "null engine");
  if (const int prc = e->params_ready()) return prc;
  if (!e->initialised) return fail(NLSG_ERR_STATE, "nlsg_bfgs_init has not been called");
  NLSG_HIP(hipSetDevice(e->cfg.device));
  if (e->resident) {  // the host cuts at a constant number of turns per launch
    for (uint64_t left = iters; left > 0;) {
      const uint32_t cut = static_cast<uint32_t>(std::min<uint64_t>(left, kBfgsResidentCut));
      launch_resident(e, cut);
      left -= cut;
    }
  } else {
    for (uint64_t k = 0; k < iters; k++) launch_iteration(e, false);
  }
  NLSG_HIP(launches_status());
  return NLSG_OK;
}

int nlsg_bfgs_unfinished(nlsg_bfgs *e, uint64_t *count) {
  return count_problems(e, bfgs_count_unfinished_kernel, count);
}

int nlsg_bfgs_identity_count(nlsg_bfgs *e, uint64_t *count) {
  return count_problems(e, bfgs_count_identity_kernel, count);
}

int nlsg_bfgs_download(nlsg_bfgs *e, double *x_host, nlsg_status *status_host) {
  if (!e) return fail(NLSG_ERR_INVALID_ARG, "null engine");
  if (!e->initialised) return fail(NLSG_ERR_STATE, "nlsg_bfgs_init has not been called");
  NLSG_HIP(hipSetDevice(e->cfg.device));
  NLSG_HIP(hipStreamSynchronize(e->stream));
  const uint64_t B = e->p.batch, n = e->p.n;
  if (x_host) NLSG_HIP(hipMemcpy(x_host, e->p.x, B * n * sizeof(double), hipMemcpyDeviceToHost));
  return download_rows(e->p.prob, B, status_host, [](const BfgsProblem &pr, uint64_t b) {
    nlsg_status st = status_row(pr.fval, pr.iter, pr.fcalls, b);
    st.gradient_evals_used = pr.gcalls;
    st.std_err = pr.cur_norm;  // gradient norm at the last iterate
    st.done = pr.done;
    return st;
  });
}

int nlsg_bfgs_download_state(nlsg_bfgs *e, double *g_host, double *h_host) {
  if (!e) return fail(NLSG_ERR_INVALID_ARG, "null engine");
  if (!e->initialised) return fail(NLSG_ERR_STATE, "nlsg_bfgs_init has not been called");
  NLSG_HIP(hipSetDevice(e->cfg.device));
  NLSG_HIP(hipStreamSynchronize(e->stream));
  const uint64_t B = e->p.batch, n = e->p.n;
  if (g_host) NLSG_HIP(hipMemcpy(g_host, e->p.g, B * n * sizeof(double), hipMemcpyDeviceToHost));
  if (h_host && !e->symmetric)
    NLSG_HIP(hipMemcpy2D(h_host, n * sizeof(double), e->p.H, e->p.ldh * sizeof(double), n * sizeof(double),
                         B * n, hipMemcpyDeviceToHost));
  if (h_host && e->symmetric) {  // the full matrix from its upper blocks
    const uint64_t tile = kBfgsSymB * kBfgsSymB;
    std::vector<double> blk(e->p.nstored * tile);
    for (uint64_t b = 0; b < B; b++) {
      NLSG_HIP(hipMemcpy(blk.data(), e->p.Hs + b * e->p.nstored * tile, blk.size() * sizeof(double),
                         hipMemcpyDeviceToHost));
      for (uint64_t i = 0; i < n; i++)
        for (uint64_t j = 0; j < n; j++) {
          const uint64_t r = i <= j ? i : j, c = i <= j ? j : i;  // (r, c) in the upper triangle
          const uint32_t I = static_cast<uint32_t>(r / kBfgsSymB), J = static_cast<uint32_t>(c / kBfgsSymB);
          h_host[(b * n + i) * n + j] = blk[bfgs_sym_block(I, J, e->p.nb) * tile +
                                            (r % kBfgsSymB) * kBfgsSymB + c % kBfgsSymB];
        }
    }
  }
  return NLSG_OK;
}

int nlsg_bfgs_minimize(nlsg_bfgs *e, double *x_inout_host, nlsg_status *status_host) {
  if (!e || !x_inout_host) return fail(NLSG_ERR_INVALID_ARG, "null argument");
  if (const int prc = e->params_ready()) return prc;
  PhaseClock clk;
  int rc = nlsg_bfgs_init(e, x_inout_host);
  if (rc) return rc;
  call_timing().init_ms = clk.lap();
  // every problem stops after at most max_iter + 1 turns (the last one only fires the stop test)
  uint64_t left = e->cfg.max_iter + 1;
  for (;;) {
    const uint64_t chunk = std::min<uint64_t>(left ? left : 1, e->resident ? kBfgsResidentCut : 8);
    rc = nlsg_bfgs_step(e, chunk);
    if (rc) return rc;
    left = left > chunk ? left - chunk : 0;
    uint64_t open = 0;
    rc = nlsg_bfgs_unfinished(e, &open);
    if (rc) return rc;
    if (open == 0) break;
  }
  call_timing().iterate_ms = clk.lap();
  rc = nlsg_bfgs_download(e, x_inout_host, status_host);
  call_timing().readback_ms = clk.lap();
  return rc;
}

int nlsg_bfgs_time_steps(nlsg_bfgs *e, uint64_t iters, float *ms_total, float *ms_hessian) {
  if (!e || !ms_total) return fail(NLSG_ERR_INVALID_ARG, "null argument");
  if (const int prc = e->params_ready()) return prc;
  if (!e->initialised) return fail(NLSG_ERR_STATE, "nlsg_bfgs_init has not been called");
  if (e->resident)
    return fail(NLSG_ERR_UNSUPPORTED, "a resident engine has no separate H kernels to bracket: time nlsg_bfgs_step");
  NLSG_HIP(hipSetDevice(e->cfg.device));
  float hess = 0.f;
  const int rc = time_repeats(e->stream, e->ev0, e->ev1, 1, ms_total, [&]() -> int {
    for (uint64_t k = 0; k < iters; k++) {
      // one timed iteration per sync: the two inner events are reused
      launch_iteration(e, true);
      NLSG_HIP(hipEventSynchronize(e->ev3));
      float ms = 0.f;
      NLSG_HIP(hipEventElapsedTime(&ms, e->ev2, e->ev3));
      hess += ms;
    }
    return NLSG_OK;
  });
  if (rc) return rc;
  if (ms_hessian) *ms_hessian = hess;
  return NLSG_OK;
}

}  // extern "C"
