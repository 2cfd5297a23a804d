// nlsolver_amd/csrc/nlsg_lm.hip — host side of the batched LM engine + C-ABI.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdlib>
#include <vector>

#include "nlsg_engine.h"
#include "nlsg_lm_kernels.h"
#include "nlsg_rtc.h"

using namespace nlsg;

struct nlsg_lm : EngineBase {  // (n_params: nlsg_lm_create_params, a row per problem)
  nlsg_lm_config cfg;
  LmParams p;
  double *A_dev = nullptr, *y_dev = nullptr, *zero_dev = nullptr;
  unsigned long long *count_dev = nullptr;
  bool has_data = false;
  bool wide = false;   // n > 64: the workgroup-per-problem kernels (lm_wide_*)
  bool wide_valu = false;  // NLSG_LM_WIDE_MFMA=0: the VALU contraction at every n > 64 (A/B switch)
  bool wide256 = true;     // NLSG_LM_WIDE256=0: the super-block evaluation at 128 < n <= 256 too (A/B switch)
  bool wide_chol = true;   // NLSG_LM_WIDE_CHOL=0: the steps before the blocked one — LDS-resident at
                           // n <= 128, column by column beyond (A/B switch)
  uint64_t ldt = kLmN; // row stride of theta / gg on the device: 64, or n when wide
  LmRtcKernels rtc;  // objective == NLSG_OBJ_CUSTOM: the kernel hiprtc built for it;
                     // NLSG_OBJ_LINK_REGRESSION: the Gauss-Newton evaluation kernel on the user's link
  bool link = false;  // nlsg_lm_create_link
  bool resident = false;  // NLSG_LM_RESIDENT: the whole loop in rtc.resident (cfg.solver holds the low byte only)
  uint32_t curve_k = 0;  // nlsg_lm_create_curve: data per observation (0: no curve engine); rtc.iter is
                         // lm_curve_iter_kernel, A_dev the repacked (t, y) of nlsg_lm_set_curve_data
};

namespace {
int upload_theta(nlsg_lm *e, const double *theta_host) {
  const uint64_t B = e->p.batch, n = e->p.n;
  if (e->wide) {
    NLSG_HIP(hipMemcpy(e->p.theta, theta_host, B * n * sizeof(double), hipMemcpyHostToDevice));
    return NLSG_OK;
  }
  std::vector<double> padded(B * kLmN, 0.0);
  for (uint64_t b = 0; b < B; b++)
    for (uint64_t j = 0; j < n; j++) padded[b * kLmN + j] = theta_host[b * n + j];
  NLSG_HIP(hipMemcpy(e->p.theta, padded.data(), padded.size() * sizeof(double),
                     hipMemcpyHostToDevice));
  return NLSG_OK;
}
// its inverse: the padding taken off again
int download_theta(nlsg_lm *e, double *theta_host) {
  const uint64_t B = e->p.batch, n = e->p.n;
  if (e->wide) {
    NLSG_HIP(hipMemcpy(theta_host, e->p.theta, B * n * 8, hipMemcpyDeviceToHost));
    return NLSG_OK;
  }
  std::vector<double> padded(B * kLmN);
  NLSG_HIP(hipMemcpy(padded.data(), e->p.theta, padded.size() * 8, hipMemcpyDeviceToHost));
  for (uint64_t b = 0; b < B; b++)
    for (uint64_t j = 0; j < n; j++) theta_host[b * n + j] = padded[b * kLmN + j];
  return NLSG_OK;
}

// All problems in lock step; the host polls the number of unfinished problems every few
// iterations. Cholesky solver: one launch per iteration (step k, then evaluation k + 1, one wave
// per problem). QR solver: the step is a kernel of its own (one workgroup per problem) between
// two evaluation launches.
bool lm_fd_objective(int objective) {
  return objective == NLSG_OBJ_ROSENBROCK || objective == NLSG_OBJ_SPHERE ||
         objective == NLSG_OBJ_STYBLINSKI_TANG || objective == NLSG_OBJ_RASTRIGIN ||
         objective == NLSG_OBJ_CUSTOM;
}

// dynamic LDS of the launch that evaluates an objective of n parameters (lm_fd_iter_kernel up to 64,
// the wide kernels beyond: none in tree order)
// (+ 66: the point and a zero behind it, for the reference-order evaluation's lanes)
size_t lm_fd_launch_lds_bytes(uint64_t n, bool ref_order) {
  if (n <= kLmN) return (64 * static_cast<size_t>(lm_fd_chunks(n)) + 128 + 66) * sizeof(double);
  return ref_order ? lm_wide_fd_lanes_lds_bytes(n) : 0;
}

// the call that hands the engine its data
const char *data_call(const nlsg_lm *e) { return e->curve_k ? "nlsg_lm_set_curve_data" : "nlsg_lm_set_data"; }

// finite-difference model: step k + evaluation k + 1 (first: the evaluation at x0 only)
void launch_fd_iter(nlsg_lm *e, int first) {
  const dim3 grid(static_cast<unsigned>(e->p.batch));
  const unsigned lds = static_cast<unsigned>(lm_fd_launch_lds_bytes(e->p.n, false));
  if (e->cfg.objective == NLSG_OBJ_CUSTOM) {
    void *args[] = {&e->p, &first};
    launch_module_kernel(e->rtc.iter, grid.x, 64, lds, e->stream, args);
    return;
  }
  if (e->cfg.solver == NLSG_LM_CHOLESKY_REFERENCE_ORDER) {  // (Rastrigin is rejected at creation)
    routed(with_value<NLSG_OBJ_ROSENBROCK, NLSG_OBJ_SPHERE, NLSG_OBJ_STYBLINSKI_TANG>(e->cfg.objective, [&](auto O) {
      hipLaunchKernelGGL((lm_fd_iter_kernel<O, true>), grid, dim3(64), lds, e->stream, e->p, first);
    }));
    return;
  }
  routed(with_objective(e->cfg.objective, [&](auto O) {
    hipLaunchKernelGGL(lm_fd_iter_kernel<O>, grid, dim3(64), lds, e->stream, e->p, first);
  }));
}

// Gauss-Newton model up to 64 parameters: step k (with_step) + evaluation k + 1, one wave per problem
void launch_gn_iter(nlsg_lm *e, int first, int with_step) {
  const unsigned grid = static_cast<unsigned>(e->p.batch);
  if (e->link || e->curve_k) {  // (a curve engine's kernel takes the same arguments)
    void *args[] = {&e->p, &first, &with_step};
    launch_module_kernel(e->rtc.iter, grid, 64, 0, e->stream, args);
    return;
  }
  hipLaunchKernelGGL(lm_iter_kernel<>, dim3(grid), dim3(64), 0, e->stream, e->p, first, with_step);
}

// the blocked Cholesky step, by the threads of its workgroup and the parity of n
void launch_wide_chol_step(nlsg_lm *e, dim3 grid) {
  routed(with_value<256, 512, 1024>(lm_wchol_threads(e->p.n), [&](auto T) {
    return with_bool(!(e->p.n & 1), [&](auto EVEN) {
      hipLaunchKernelGGL((lm_wide_chol_step_kernel<T, EVEN>), grid, dim3(T), lm_wchol_lds_bytes(T), e->stream, e->p);
    });
  }));
}
// n > 64: evaluation (f, g, H at the current point) as one launch, a workgroup per problem
void launch_wide_eval(nlsg_lm *e, int first) {
  // finite-difference model: enough workgroups per problem to fill the device when the batch is small
  const unsigned split = e->p.fd ? static_cast<unsigned>(std::min<uint64_t>(
                                       64, std::max<uint64_t>(1, 2048 / e->p.batch))) : 1u;
  const dim3 grid(static_cast<unsigned>(e->p.batch), split);
  if (e->link) {  // the built-in selection below, on the module's one kernel
    void *args[] = {&e->p, &first};
    const bool one_pass = e->p.n <= 256;
    launch_module_kernel(e->rtc.iter, grid.x, one_pass ? 512 : 256,
                         e->p.n > 128 && one_pass ? static_cast<unsigned>(sizeof(LmWide256Shared)) : 0u,
                         e->stream, args);
    return;
  }
  if (!e->p.fd) {
    // up to 128 parameters: one pass over A, J^T J on the matrix cores
    if (e->wide_valu)
      hipLaunchKernelGGL(lm_wide_tanh_eval_kernel, grid, dim3(kLmWideThreads), 0, e->stream, e->p, first);
    else if (e->p.n <= 128)
      hipLaunchKernelGGL(lm_wide128x8_tanh_eval_kernel<>, grid, dim3(512), 0, e->stream, e->p, first);
    else if (e->p.n <= 256 && e->wide256)  // one pass over A still: 136 tiles on eight waves
      hipLaunchKernelGGL(lm_wide256x8_tanh_eval_kernel<>, grid, dim3(512), sizeof(LmWide256Shared), e->stream, e->p, first);
    else  // super-blocks of 128 x 128, each on the matrix cores
      hipLaunchKernelGGL(lm_wide_mfma_tanh_eval_kernel<>, grid, dim3(256), 0, e->stream, e->p, first);
    return;
  }
  if (e->cfg.objective == NLSG_OBJ_CUSTOM) {
    void *args[] = {&e->p, &first};
    if (e->cfg.solver == NLSG_LM_CHOLESKY_REFERENCE_ORDER)
      launch_module_kernel(e->rtc.iter, grid.x, 256, static_cast<unsigned>(lm_wide_fd_lanes_lds_bytes(e->p.n)),
                           e->stream, args, grid.y);
    else
      launch_module_kernel(e->rtc.iter, grid.x, lm_wide_fd_threads(lm_wide_chunks(e->p.n)), 0, e->stream,
                           args, grid.y);
    return;
  }
  if (e->cfg.solver == NLSG_LM_CHOLESKY_REFERENCE_ORDER) {  // past 64 parameters (Rastrigin is rejected at creation)
    routed(with_value<NLSG_OBJ_ROSENBROCK, NLSG_OBJ_SPHERE, NLSG_OBJ_STYBLINSKI_TANG>(e->cfg.objective, [&](auto O) {
      hipLaunchKernelGGL((lm_wide_fd_lanes_kernel<O>), grid, dim3(256),
                         static_cast<unsigned>(lm_wide_fd_lanes_lds_bytes(e->p.n)), e->stream, e->p, first);
    }));
    return;
  }
  routed(with_objective(e->cfg.objective, [&](auto O) {
    return with_chunks(lm_wide_chunks(e->p.n), [&](auto C) {
      hipLaunchKernelGGL((lm_wide_fd_eval_kernel<O, C>), grid, dim3(lm_wide_fd_threads(C)), 0, e->stream, e->p, first);
    });
  }));
}

// A solver argument of the C-ABI: the nlsg_lm_solver in the low byte, NLSG_LM_RESIDENT above it. A value
// below 256 (negative ones included) is a plain solver, known or not, and answers as it always did.
struct LmSolverArg {
  int32_t solver;
  bool resident, unknown_bits;
};
LmSolverArg lm_solver_arg(int32_t v) {
  if (v < 256) return {v, false, false};
  return {v & 0xff, (v & NLSG_LM_RESIDENT) != 0, (v & ~(0xff | NLSG_LM_RESIDENT)) != 0};
}
// the rules of the flag, behind every check of the plain value; nothing here touches the device
int lm_resident_door(const LmSolverArg &a, int32_t given, bool fd, bool ref_order, uint64_t n) {
  if (a.unknown_bits)
    return fail(NLSG_ERR_INVALID_ARG, "unknown bits in solver 0x%x: above the low byte only NLSG_LM_RESIDENT (256) "
                                      "is defined", static_cast<unsigned>(given));
  if (!a.resident) return NLSG_OK;
  if (a.solver == NLSG_LM_QR)
    return fail(NLSG_ERR_UNSUPPORTED, "NLSG_LM_RESIDENT runs the Cholesky step: the tinyqr step is a 512-thread "
                                      "workgroup of its own (NLSG_LM_QR)");
  if (ref_order)
    return fail(NLSG_ERR_UNSUPPORTED, "NLSG_LM_RESIDENT restates the tree-order turn: not with "
                                      "NLSG_LM_CHOLESKY_REFERENCE_ORDER");
  if (fd)
    return fail(NLSG_ERR_UNSUPPORTED, "NLSG_LM_RESIDENT covers the Gauss-Newton models (tanh, link, curve): a "
                                      "finite-difference objective runs in lock step");
  if (n > kLmN)
    return fail(NLSG_ERR_UNSUPPORTED, "NLSG_LM_RESIDENT runs one wave per problem: n = %llu > %d",
                (unsigned long long)n, kLmN);
  return NLSG_OK;
}
// the resident kernel of the engine's model: a link or curve module has it already, a tanh engine builds its
// own here (hiprtc; the code object is kept by its source)
int lm_resident_kernel_ready(nlsg_lm *e) {
  if (e->rtc.resident) return NLSG_OK;
  if (const int rc = rtc_build_lm_tanh_resident(&e->rtc)) {
    if (rc == NLSG_ERR_UNSUPPORTED)
      return fail(NLSG_ERR_UNSUPPORTED, "NLSG_LM_RESIDENT needs the run-time compiler, and hiprtc cannot be "
                                        "loaded in this process (nlsg_rtc_load): the lock-step driver runs without it");
    return rc;
  }
  return NLSG_OK;
}

// NLSG_LM_RESIDENT: every unfinished problem makes up to kLmResidentCut turns per launch; the host counts the
// unfinished ones between launches only
int launch_resident_solve(nlsg_lm *e) {
  const uint64_t total = e->p.max_iter + 1;  // max_iter iterations plus the turn whose stop test fires
  const unsigned grid = static_cast<unsigned>(e->p.batch);
  uint64_t made = 0;
  for (int first = 1;; first = 0) {
    uint32_t turns = static_cast<uint32_t>(std::min<uint64_t>(total - made, kLmResidentCut));
    void *args[] = {&e->p, &first, &turns};
    launch_module_kernel(e->rtc.resident, grid, 64, 0, e->stream, args);
    made += turns;
    if (made >= total) break;
    uint64_t open = 0;
    if (const int rc = device_count(e->stream, e->count_dev, &open, [&] {
          hipLaunchKernelGGL(lm_count_unfinished_kernel, dim3(static_cast<unsigned>((e->p.batch + 255) / 256)),
                             dim3(256), 0, e->stream, e->p, e->count_dev);
        }))
      return rc;
    if (open == 0) break;
  }
  return NLSG_OK;
}

int launch_solve(nlsg_lm *e) {
  if (e->resident) return launch_resident_solve(e);
  const dim3 grid(static_cast<unsigned>(e->p.batch));
  const bool qr = e->cfg.solver == NLSG_LM_QR, fd = e->p.fd != 0;
  if (e->wide)
    launch_wide_eval(e, 1);
  else if (fd)
    launch_fd_iter(e, 1);
  else
    launch_gn_iter(e, 1, 0);
  uint64_t launched = 0;
  for (;;) {
    // max_iter iterations plus the turn whose stop test fires
    const uint64_t left = e->p.max_iter + 1 - launched;
    const uint64_t chunk = left < 8 ? left : 8;
    for (uint64_t i = 0; i < chunk; i++) {
      if (e->wide) {
        if (e->cfg.solver == NLSG_LM_CHOLESKY_REFERENCE_ORDER)  // the reference's own order of operations
          hipLaunchKernelGGL(lm_wide_step_kernel<true>, grid, dim3(kLmWideThreads), 0, e->stream, e->p);
        else if (e->wide_chol && !e->wide_valu)  // blocked, the panel sums on the matrix cores
          launch_wide_chol_step(e, grid);
        else if (e->p.n <= 128 && !e->wide_valu)  // the damped matrix in LDS, one thread per row
          hipLaunchKernelGGL(lm_wide128_step_kernel, grid, dim3(128), sizeof(LmWide128StepShared),
                             e->stream, e->p);
        else
          hipLaunchKernelGGL(lm_wide_step_kernel<false>, grid, dim3(kLmWideThreads), 0, e->stream, e->p);
        launch_wide_eval(e, 0);
      } else if (fd) {
        launch_fd_iter(e, 0);
      } else if (qr) {
        hipLaunchKernelGGL(lm_qr_step_kernel<kLmQrThreads>, grid, dim3(kLmQrThreads), sizeof(LmQrShared), e->stream, e->p);
        launch_gn_iter(e, 0, 0);
      } else {
        launch_gn_iter(e, 0, 1);
      }
    }
    launched += chunk;
    if (launched >= e->p.max_iter + 1) break;
    uint64_t open = 0;
    if (const int rc = device_count(e->stream, e->count_dev, &open, [&] {
          hipLaunchKernelGGL(lm_count_unfinished_kernel, dim3(static_cast<unsigned>((e->p.batch + 255) / 256)),
                             dim3(256), 0, e->stream, e->p, e->count_dev);
        }))
      return rc;
    if (open == 0) break;
  }
  return NLSG_OK;
}
}  // namespace

static int lm_create(const nlsg_lm_config *cfg, const nlsg_custom_objective *custom, nlsg_lm **out,
                     bool with_params = false, const nlsg_lm_link *link = nullptr,
                     const nlsg_lm_curve *curve = nullptr);

extern "C" {

int nlsg_lm_create(const nlsg_lm_config *cfg, nlsg_lm **out) {
  if (const int rc = builtin_door(cfg, "nlsg_lm")) return rc;
  if (const int rc = builtin_door(cfg, "nlsg_lm", NLSG_OBJ_LINK_REGRESSION, "NLSG_OBJ_LINK_REGRESSION", "link")) return rc;
  if (const int rc = builtin_door(cfg, "nlsg_lm", NLSG_OBJ_CURVE_MODEL, "NLSG_OBJ_CURVE_MODEL", "curve")) return rc;
  return timed_create([&] { return lm_create(cfg, nullptr, out); });
}

int nlsg_lm_create_custom(const nlsg_lm_config *cfg, const nlsg_custom_objective *obj, nlsg_lm **out) {
  if (const int rc = custom_door(cfg, obj, out)) return rc;
  return timed_create([&] { return lm_create(cfg, obj, out); });
}

int nlsg_lm_create_params(const nlsg_lm_config *cfg, const nlsg_custom_objective *obj, nlsg_lm **out) {
  if (const int rc = runtime_door(cfg, obj, out)) return rc;
  return timed_create([&] { return lm_create(cfg, obj, out, true); });
}

int nlsg_lm_create_link(const nlsg_lm_config *cfg, const nlsg_lm_link *link, nlsg_lm **out) {
  if (const int rc = runtime_door(cfg, link, out, NLSG_OBJ_LINK_REGRESSION, "NLSG_OBJ_LINK_REGRESSION")) return rc;
  return timed_create([&] { return lm_create(cfg, nullptr, out, false, link); });
}

int nlsg_lm_create_curve(const nlsg_lm_config *cfg, const nlsg_lm_curve *curve, nlsg_lm **out) {
  if (const int rc = runtime_door(cfg, curve, out, NLSG_OBJ_CURVE_MODEL, "NLSG_OBJ_CURVE_MODEL")) return rc;
  return timed_create([&] { return lm_create(cfg, nullptr, out, false, nullptr, curve); });
}

// The dynamic LDS of the launch that evaluates an objective (the finite-difference model, which is what a
// custom objective runs): 0 for a shape that model rejects (n outside 1 .. 1024, the QR solver, an
// unknown solver) — and for tree order past 64 parameters, whose evaluation kernel takes none.
uint64_t nlsg_lm_lds_bytes(uint64_t n, int32_t solver) {
  if (solver >= 256)  // the resident workgroup of a regression model: the lock-step kernel's block
    return solver == (NLSG_LM_CHOLESKY | NLSG_LM_RESIDENT) && n >= 1 && n <= kLmN
               ? (kLmTri + 128) * sizeof(double) : 0;
  if (n < 1 || n > kLmWideMaxN) return 0;
  if (solver != NLSG_LM_CHOLESKY && solver != NLSG_LM_CHOLESKY_REFERENCE_ORDER) return 0;
  return lm_fd_launch_lds_bytes(n, solver == NLSG_LM_CHOLESKY_REFERENCE_ORDER);
}

int nlsg_lm_set_params(nlsg_lm *e, const double *params_host) {
  if (!e || !params_host) return fail(NLSG_ERR_INVALID_ARG, "null argument");
  if (e->curve_k)
    return fail(NLSG_ERR_INVALID_ARG, "a curve model has no p(k): per-problem constants ride in columns of t "
                                      "(nlsg_lm_set_curve_data)");
  return e->set_params(params_host);
}

}  // extern "C"

static int lm_create(const nlsg_lm_config *cfg, const nlsg_custom_objective *custom, nlsg_lm **out,
                     bool with_params, const nlsg_lm_link *link, const nlsg_lm_curve *curve) {
  if (!cfg || !out) return fail(NLSG_ERR_INVALID_ARG, "null argument");
  *out = nullptr;
  if (cfg->struct_size != sizeof(nlsg_lm_config))
    return fail(NLSG_ERR_INVALID_ARG, "nlsg_lm_config size mismatch (%u vs %zu)", cfg->struct_size,
                sizeof(nlsg_lm_config));
  const bool fd = lm_fd_objective(cfg->objective);
  const LmSolverArg arg = lm_solver_arg(cfg->solver);
  const int32_t solver = arg.solver;
  if (cfg->objective != NLSG_OBJ_TANH_REGRESSION && !(link && cfg->objective == NLSG_OBJ_LINK_REGRESSION) &&
      !(curve && cfg->objective == NLSG_OBJ_CURVE_MODEL) && !fd)
    return fail(NLSG_ERR_INVALID_ARG, "unknown objective %d", cfg->objective);
  const bool ref_order = solver == NLSG_LM_CHOLESKY_REFERENCE_ORDER;
  if (solver != NLSG_LM_CHOLESKY && solver != NLSG_LM_QR && !ref_order)
    return fail(NLSG_ERR_INVALID_ARG, "unknown solver %d", solver);
  if (fd && solver == NLSG_LM_QR)
    return fail(NLSG_ERR_UNSUPPORTED,
                "the finite-difference model runs the reference's own solve (Cholesky) only");
  if (ref_order && (!fd || cfg->objective == NLSG_OBJ_RASTRIGIN ||
                    (custom && custom->chain == NLSG_CUSTOM_VECTOR)))
    return fail(NLSG_ERR_UNSUPPORTED,
                "NLSG_LM_CHOLESKY_REFERENCE_ORDER covers the default functors on objectives given by "
                "their terms (Rosenbrock / Sphere / Styblinski-Tang, custom term bodies): Rastrigin's "
                "cosine is the device's own, a whole-vector body's x.sum() adds in the lane-tree order");
  if (cfg->n < 1 || (!fd && cfg->m < 1) || cfg->batch < 1)
    return fail(NLSG_ERR_INVALID_ARG, "need n >= 1, m >= 1, batch >= 1");
  if (curve && cfg->n > kLmN)
    return fail(NLSG_ERR_UNSUPPORTED, "curve models run one wave per problem: n = %llu > %d",
                (unsigned long long)cfg->n, kLmN);
  const bool wide = cfg->n > kLmN;
  if (cfg->n > kLmWideMaxN)
    return fail(NLSG_ERR_UNSUPPORTED, "n = %llu > %d (a thread of the step follows at most four rows)",
                (unsigned long long)cfg->n, kLmWideMaxN);
  if (wide && solver == NLSG_LM_QR)
    return fail(NLSG_ERR_UNSUPPORTED, "the tinyqr solve is built for n <= 64; n = %llu runs the "
                "class's own Cholesky solve", (unsigned long long)cfg->n);
  if (cfg->batch > 0x7fffffffull) return fail(NLSG_ERR_UNSUPPORTED, "batch too large");
  if (with_params)  // (the row is static LDS of the run-time compiled module, next to the launch's dynamic block)
    if (const int prc = check_custom_params(custom, nlsg_lm_lds_bytes(cfg->n, solver), "nlsg_lm",
                                            "nlsg_lm_create_custom"))
      return prc;
  if (link && (!link->value_body || !link->value_body[0] || !link->slope_body || !link->slope_body[0]))
    return fail(NLSG_ERR_INVALID_ARG, "a link needs a value body and a slope body (nlsg_lm_link)");
  if (curve && (curve->k < 1 || curve->k > 16))
    return fail(NLSG_ERR_INVALID_ARG, "a curve model takes 1 .. 16 data per observation: k = %u", curve->k);
  if (curve && (!curve->body || !curve->body[0]))
    return fail(NLSG_ERR_INVALID_ARG, "a curve model needs a body (nlsg_lm_curve)");
  if (const int rc = lm_resident_door(arg, cfg->solver, fd, ref_order, cfg->n)) return rc;
  nlsg_lm *e = nullptr;
  if (const int rc = open_engine(cfg->device, cfg->stream, "nlsg_lm", &e)) return rc;
  CreateGuard<nlsg_lm> guard(e, nlsg_lm_destroy);
  e->cfg = *cfg;
  e->cfg.solver = solver;
  e->resident = arg.resident;
  e->wide = wide;
  e->n_params = with_params ? custom->n_params : 0;
  e->link = link != nullptr;
  e->curve_k = curve ? curve->k : 0;
  if (!e->link) {  // (a link engine has one evaluation kernel per shape, and the blocked step: no A/B forms)
    const char *sw = std::getenv("NLSG_LM_WIDE_MFMA");
    e->wide_valu = sw && sw[0] == '0';
    const char *w2 = std::getenv("NLSG_LM_WIDE256");
    e->wide256 = !(w2 && w2[0] == '0');
    const char *wc = std::getenv("NLSG_LM_WIDE_CHOL");
    e->wide_chol = !(wc && wc[0] == '0');
  }
  e->ldt = wide ? cfg->n : kLmN;
  LmParams &p = e->p;
  std::memset(&p, 0, sizeof p);
  const uint64_t B = cfg->batch, m = fd ? 0 : cfg->m;  // no design matrix behind an objective
  DeviceOwner &own = e->own;
  hipError_t &he = own.err;
  // row groups of 16 (design matrices), or super-steps of 64 observations (curve data)
  const uint64_t nstep = wide ? 0 : curve ? (m + 63) / 64 : (m + 15) / 16;
  p.nstep = nstep;
  if (curve) own.alloc(&e->A_dev, nstep * B * (curve->k + 1) * 64 * 8);  // [super-step][batch][k + 1][64], y in the last row
  if (nstep && !curve) own.alloc(&e->A_dev, nstep * B * 16 * kLmN * 8);
  if (nstep && !curve) own.alloc(&e->y_dev, nstep * B * 16 * 8);
  if (wide && m) {  // the caller's layout, [batch][m][n]
    own.alloc(&e->A_dev, B * m * cfg->n * 8);
    own.alloc(&e->y_dev, B * m * 8);
    own.alloc(&p.rw, B * 2 * m * 8);
  }
  if (wide) own.alloc(&p.Hw, B * cfg->n * cfg->n * 8);
  own.alloc(&p.theta, B * e->ldt * 8);
  own.alloc(&p.prob, B * sizeof(LmProblem));
  if (!wide) own.zeroed(&p.Hg, B * kLmTri * 8);  // rows past n are never written
  own.alloc(&p.gg, B * e->ldt * 8);
  own.alloc(&e->count_dev, 8);
  own.zeroed(&e->zero_dev, 16);
  e->alloc_params(B, e->n_params);
  e->timing_events();
  if (he == hipSuccess)
    he = hipFuncSetAttribute(reinterpret_cast<const void *>(lm_qr_step_kernel<kLmQrThreads>),
                             hipFuncAttributeMaxDynamicSharedMemorySize, sizeof(LmQrShared));
  if (he == hipSuccess)
    he = hipFuncSetAttribute(reinterpret_cast<const void *>(lm_wide128_step_kernel),
                             hipFuncAttributeMaxDynamicSharedMemorySize, sizeof(LmWide128StepShared));
  if (he == hipSuccess)
    he = hipFuncSetAttribute(reinterpret_cast<const void *>(lm_wide256x8_tanh_eval_kernel<>),
                             hipFuncAttributeMaxDynamicSharedMemorySize, sizeof(LmWide256Shared));
  for (int ev = 0; ev < 2 && he == hipSuccess; ev++) {  // 139 KB at 1024 threads, 70 KB at 512
    he = hipFuncSetAttribute(ev ? reinterpret_cast<const void *>(lm_wide_chol_step_kernel<1024, true>)
                                : reinterpret_cast<const void *>(lm_wide_chol_step_kernel<1024, false>),
                             hipFuncAttributeMaxDynamicSharedMemorySize, lm_wchol_lds_bytes(1024));
    if (he == hipSuccess)
      he = hipFuncSetAttribute(ev ? reinterpret_cast<const void *>(lm_wide_chol_step_kernel<512, true>)
                                  : reinterpret_cast<const void *>(lm_wide_chol_step_kernel<512, false>),
                               hipFuncAttributeMaxDynamicSharedMemorySize, lm_wchol_lds_bytes(512));
  }
  if (const int rc = e->setup_status()) return rc;
  if (custom)
    if (const int rc = rtc_build_lm(custom, !wide ? 0 : lm_wide_chunks(cfg->n), ref_order, &e->rtc)) return rc;
  if (link) {
    if (const int rc = rtc_build_lm_link(link, cfg->n, &e->rtc)) return rc;
    if (cfg->n > 128 && cfg->n <= 256)  // 70 KB of dynamic LDS: the module API's opt-in
      if (const int rc = module_kernel_lds(e->rtc.iter, sizeof(LmWide256Shared), "device setup failed: %s")) return rc;
  }
  if (curve)
    if (const int rc = rtc_build_lm_curve(curve, cfg->n, &e->rtc)) return rc;
  if (e->resident)
    if (const int rc = lm_resident_kernel_ready(e)) return rc;
  p.A = e->A_dev;
  p.y = e->y_dev;
  p.Aw = e->A_dev;
  p.yw = e->y_dev;
  p.zero = e->zero_dev;
  p.params = e->params_dev;
  p.batch = B;
  p.m = m;
  p.n = cfg->n;
  p.max_iter = cfg->max_iter;
  p.lambda0 = cfg->lambda;
  p.up = cfg->up;
  p.down = cfg->down;
  p.f_delta = cfg->f_delta;
  p.fd = fd ? 1 : 0;
  // the matrix-core evaluations (but the four-wave A/B form) hand is_diagonal's verdict to the step
  p.verdict = (wide && !fd && !e->wide_valu) ? 1 : 0;
  p.eps_h = std::pow(DBL_EPSILON, 1.0 / 4.0);  // fin_diff_h's step (:1454)
  e->has_data = fd;  // the model is the objective itself
  *out = guard.release();
  return NLSG_OK;
}

extern "C" {

int nlsg_lm_destroy(nlsg_lm *e) { return timed_destroy(e); }

int nlsg_lm_set_data(nlsg_lm *e, const double *a_host, const double *y_host) {
  if (!e || !a_host || !y_host) return fail(NLSG_ERR_INVALID_ARG, "null argument");
  if (e->p.fd) return fail(NLSG_ERR_STATE, "this engine minimises a built-in objective: no data");
  if (e->curve_k)
    return fail(NLSG_ERR_INVALID_ARG, "a curve model's data are t and y: nlsg_lm_set_curve_data");
  NLSG_HIP(hipSetDevice(e->cfg.device));
  PhaseClock clk;
  const uint64_t B = e->p.batch, m = e->p.m, n = e->p.n;
  if (e->wide) {  // kept as handed over
    NLSG_HIP(hipMemcpy(e->A_dev, a_host, B * m * n * 8, hipMemcpyHostToDevice));
    NLSG_HIP(hipMemcpy(e->y_dev, y_host, B * m * 8, hipMemcpyHostToDevice));
    e->has_data = true;
    call_timing().upload_ms = clk.lap();
    return NLSG_OK;
  }
  // host layout [problem][m][n] -> device layout [row group][problem][16][64] (zero padded):
  // problems that run side by side read one contiguous stretch of HBM per row group instead
  // of addresses a whole problem (m * 512 bytes) apart, which camp on a few channels.
  // The matrices cross PCIe in chunks of problems through two staging buffers on a copy stream
  // of their own while the previous chunk is repacked: from pinned host memory (nlsg_host_alloc)
  // the copies are plain DMA at the link's rate; from pageable memory the runtime stages them.
  const uint64_t per = m * n * 8;
  uint64_t chunk = std::max<uint64_t>(1, (64ull << 20) / per);  // ~64 MiB per staging buffer
  if (chunk > B) chunk = B;
  double *raw[2] = {nullptr, nullptr}, *y_raw = nullptr;
  hipStream_t copy = nullptr;
  hipEvent_t landed[2] = {nullptr, nullptr}, packed[2] = {nullptr, nullptr};
  DeviceOwner tmp(e->cfg.device);  // the staging buffers, the copy stream and its events: this call's only
  hipError_t &he = tmp.err;
  tmp.watch(e->stream);
  tmp.stream(&copy);
  for (int k = 0; k < 2; k++) {
    tmp.alloc(&raw[k], chunk * per);
    tmp.event(&landed[k], hipEventDisableTiming);
    tmp.event(&packed[k], hipEventDisableTiming);
  }
  tmp.alloc(&y_raw, B * m * 8);
  if (he == hipSuccess) he = hipMemcpyAsync(y_raw, y_host, B * m * 8, hipMemcpyHostToDevice, copy);
  uint64_t k = 0;
  for (uint64_t b0 = 0; b0 < B && he == hipSuccess; b0 += chunk, k++) {
    const uint64_t nbp = std::min(chunk, B - b0);
    const int slot = static_cast<int>(k & 1);
    if (k >= 2) he = hipStreamWaitEvent(copy, packed[slot], 0);  // the buffer's previous chunk is repacked
    if (he == hipSuccess)
      he = hipMemcpyAsync(raw[slot], a_host + b0 * m * n, nbp * per, hipMemcpyHostToDevice, copy);
    if (he == hipSuccess) he = hipEventRecord(landed[slot], copy);
    if (he == hipSuccess) he = hipStreamWaitEvent(e->stream, landed[slot], 0);
    if (he == hipSuccess) {
      const uint64_t total = e->p.nstep * nbp * 16 * kLmN;
      hipLaunchKernelGGL(lm_repack_kernel, dim3(static_cast<unsigned>((total + 255) / 256)), dim3(256),
                         0, e->stream, e->p, raw[slot], y_raw, e->A_dev, e->y_dev, b0, nbp);
      he = hipGetLastError();
    }
    if (he == hipSuccess) he = hipEventRecord(packed[slot], e->stream);
  }
  if (he == hipSuccess) he = hipStreamSynchronize(e->stream);  // the host buffers are borrowed for this call only
  tmp.release();  // (drains the copy stream, and the engine's on a failed path, before the buffers go back)
  NLSG_HIP(he);
  e->has_data = true;
  call_timing().upload_ms = clk.lap();
  return NLSG_OK;
}

// host layout t [problem][m][k], y [problem][m] -> device layout [super-step][problem][k + 1][64] (zero
// padded past m, y in row k): a lane per observation reads its data coalesced (lm_curve_repack_kernel)
int nlsg_lm_set_curve_data(nlsg_lm *e, const double *t_host, const double *y_host) {
  if (!e || !t_host || !y_host) return fail(NLSG_ERR_INVALID_ARG, "null argument");
  if (!e->curve_k)
    return fail(NLSG_ERR_INVALID_ARG, "not a curve engine (nlsg_lm_create_curve): its data go by nlsg_lm_set_data");
  NLSG_HIP(hipSetDevice(e->cfg.device));
  PhaseClock clk;
  const uint64_t B = e->p.batch, m = e->p.m, K = e->curve_k;
  double *t_raw = nullptr, *y_raw = nullptr;
  DeviceOwner tmp(e->cfg.device);
  hipError_t &he = tmp.err;
  tmp.watch(e->stream);
  tmp.alloc(&t_raw, B * m * K * 8);
  tmp.alloc(&y_raw, B * m * 8);
  if (he == hipSuccess) he = hipMemcpyAsync(t_raw, t_host, B * m * K * 8, hipMemcpyHostToDevice, e->stream);
  if (he == hipSuccess) he = hipMemcpyAsync(y_raw, y_host, B * m * 8, hipMemcpyHostToDevice, e->stream);
  if (he == hipSuccess) {
    const uint64_t total = e->p.nstep * B * (K + 1) * 64;
    hipLaunchKernelGGL(lm_curve_repack_kernel, dim3(static_cast<unsigned>((total + 255) / 256)), dim3(256), 0,
                       e->stream, e->p, e->curve_k, t_raw, y_raw, e->A_dev);
    he = hipGetLastError();
  }
  if (he == hipSuccess) he = hipStreamSynchronize(e->stream);  // the host buffers are borrowed for this call only
  tmp.release();
  NLSG_HIP(he);
  e->has_data = true;
  call_timing().upload_ms = clk.lap();
  return NLSG_OK;
}

// Page-locked host memory for buffers that cross PCIe at the boundary (design matrices, start
// points): what lives there is copied by DMA at the link's rate instead of being staged.
int nlsg_host_alloc(void **out, uint64_t bytes) {
  if (!out) return fail(NLSG_ERR_INVALID_ARG, "null argument");
  *out = nullptr;
  NLSG_HIP(hipHostMalloc(out, bytes ? bytes : 8, hipHostMallocDefault));
  return NLSG_OK;
}
int nlsg_host_free(void *ptr) {
  if (ptr) NLSG_HIP(hipHostFree(ptr));
  return NLSG_OK;
}

int nlsg_lm_set_solver(nlsg_lm *e, int32_t solver) {
  if (!e) return fail(NLSG_ERR_INVALID_ARG, "null engine");
  const int32_t given = solver;
  const LmSolverArg arg = lm_solver_arg(given);
  solver = arg.solver;
  if (solver != NLSG_LM_CHOLESKY && solver != NLSG_LM_QR)
    return fail(NLSG_ERR_INVALID_ARG, "unknown solver %d (the reference-order mode is chosen at creation)",
                solver);
  if (e->cfg.solver == NLSG_LM_CHOLESKY_REFERENCE_ORDER)  // the bit-for-bit parity mode is a property of
    return fail(NLSG_ERR_STATE,                           // the engine: it is not left silently
                "this engine was created in NLSG_LM_CHOLESKY_REFERENCE_ORDER; create another engine "
                "for a different solver");
  if (e->wide && solver != NLSG_LM_CHOLESKY)
    return fail(NLSG_ERR_UNSUPPORTED, "the tinyqr solve is built for n <= 64");
  if (e->p.fd && solver != NLSG_LM_CHOLESKY)
    return fail(NLSG_ERR_UNSUPPORTED,
                "the finite-difference model runs the reference's own solve (Cholesky) only");
  if (const int rc = lm_resident_door(arg, given, e->p.fd != 0, false, e->p.n)) return rc;
  if (arg.resident) {
    NLSG_HIP(hipSetDevice(e->cfg.device));
    if (const int rc = lm_resident_kernel_ready(e)) return rc;
  }
  e->cfg.solver = solver;
  e->resident = arg.resident;
  return NLSG_OK;
}

int nlsg_lm_minimize(nlsg_lm *e, double *theta_inout_host, nlsg_status *status_host,
                     double *lambda_out_host) {
  if (!e || !theta_inout_host) return fail(NLSG_ERR_INVALID_ARG, "null argument");
  if (!e->has_data) return fail(NLSG_ERR_STATE, "%s has not been called", data_call(e));
  if (const int prc = e->params_ready()) return prc;
  NLSG_HIP(hipSetDevice(e->cfg.device));
  PhaseClock clk;
  int rc = upload_theta(e, theta_inout_host);
  if (rc) return rc;
  call_timing().init_ms = clk.lap();
  rc = launch_solve(e);
  if (rc) return rc;
  NLSG_HIP(launches_status());
  NLSG_HIP(hipStreamSynchronize(e->stream));
  call_timing().iterate_ms = clk.lap();
  rc = download_theta(e, theta_inout_host);
  if (rc) return rc;
  // f, grad and hess are evaluated together; behind the default functors every probe of
  // fin_diff (4 n) and fin_diff_h (16 n^2) is a call of the objective
  const uint64_t n = e->p.n, calls_per_eval = e->p.fd ? 1 + 4 * n + 16 * n * n : 1;
  rc = download_rows(
      e->p.prob, e->p.batch, status_host,
      [&](const LmProblem &pr, uint64_t b) {
        nlsg_status st = status_row(pr.f, pr.iter, pr.fcalls * calls_per_eval, b);
        st.gradient_evals_used = pr.fcalls;
        st.hessian_evals_used = pr.fcalls;
        st.std_err = pr.lambda;
        st.done = pr.done;
        return st;
      },
      [&](const LmProblem &pr, uint64_t b) {
        if (lambda_out_host) lambda_out_host[b] = pr.lambda;
      });
  if (rc) return rc;
  call_timing().readback_ms = clk.lap();
  return NLSG_OK;
}

// cov = c (J^T J)^-1 at theta: the solve's own first launch (evaluation at theta, which also resets
// LmProblem), then lm_cov_kernel on the Hg and f it left. The output block is the pool's: it goes back
// only after the stream has drained, whatever failed in between.
int nlsg_lm_covariance(nlsg_lm *e, const double *theta_host, int32_t scale, double *cov_out_host,
                       double *s2_out_host, int32_t *ok_out_host) {
  if (!e || !theta_host || !cov_out_host) return fail(NLSG_ERR_INVALID_ARG, "null argument");
  if (!e->has_data) return fail(NLSG_ERR_STATE, "%s has not been called", data_call(e));
  if (e->wide)
    return fail(NLSG_ERR_UNSUPPORTED, "the covariance kernel runs one wave per problem: n = %llu > %d",
                (unsigned long long)e->p.n, kLmN);
  if (e->p.fd)
    return fail(NLSG_ERR_UNSUPPORTED, "Gauss-Newton models only: behind the default functors the engine's "
                                      "matrix is a finite-difference Hessian, not J^T J");
  if (scale != NLSG_LM_COV_RESIDUAL && scale != NLSG_LM_COV_ABSOLUTE)
    return fail(NLSG_ERR_INVALID_ARG, "unknown scale %d", scale);
  if (scale == NLSG_LM_COV_RESIDUAL && e->p.m <= e->p.n)
    return fail(NLSG_ERR_INVALID_ARG, "the residual variance f / (m - n) needs m > n: m = %llu, n = %llu "
                                      "(NLSG_LM_COV_ABSOLUTE takes m <= n)",
                (unsigned long long)e->p.m, (unsigned long long)e->p.n);
  NLSG_HIP(hipSetDevice(e->cfg.device));
  PhaseClock clk;
  const uint64_t B = e->p.batch, n = e->p.n;
  // cov [B][n][n] | s2 [B] | ok [B]
  const uint64_t cov_bytes = B * n * n * 8;
  unsigned char *block = nullptr;
  DeviceOwner tmp(e->cfg.device);  // drains the engine's stream before the block goes back, on every path
  tmp.watch(e->stream);
  NLSG_HIP(tmp.take(&block, cov_bytes + B * 8 + B * 4));
  double *cov_dev = reinterpret_cast<double *>(block);
  double *s2_dev = reinterpret_cast<double *>(block + cov_bytes);
  int32_t *ok_dev = reinterpret_cast<int32_t *>(block + cov_bytes + B * 8);
  int rc = upload_theta(e, theta_host);
  if (rc) return rc;
  call_timing().init_ms = clk.lap();
  launch_gn_iter(e, 1, 0);
  if (scale == NLSG_LM_COV_RESIDUAL)
    hipLaunchKernelGGL(lm_cov_kernel<true>, dim3(static_cast<unsigned>(B)), dim3(64), 0, e->stream, e->p,
                       cov_dev, s2_dev, ok_dev);
  else
    hipLaunchKernelGGL(lm_cov_kernel<false>, dim3(static_cast<unsigned>(B)), dim3(64), 0, e->stream, e->p,
                       cov_dev, s2_dev, ok_dev);
  hipError_t he = launches_status();
  const hipError_t se = hipStreamSynchronize(e->stream);
  if (he == hipSuccess) he = se;
  call_timing().iterate_ms = clk.lap();
  if (he == hipSuccess) he = hipMemcpy(cov_out_host, cov_dev, cov_bytes, hipMemcpyDeviceToHost);
  if (he == hipSuccess && s2_out_host) he = hipMemcpy(s2_out_host, s2_dev, B * 8, hipMemcpyDeviceToHost);
  if (he == hipSuccess && ok_out_host) he = hipMemcpy(ok_out_host, ok_dev, B * 4, hipMemcpyDeviceToHost);
  tmp.release();
  NLSG_HIP(he);
  call_timing().readback_ms = clk.lap();
  return NLSG_OK;
}

int nlsg_lm_time_solve(nlsg_lm *e, const double *theta0_host, uint32_t repeats, float *ms_total) {
  if (!e || !theta0_host || !ms_total) return fail(NLSG_ERR_INVALID_ARG, "null argument");
  if (const int prc = e->params_ready()) return prc;
  if (!e->has_data) return fail(NLSG_ERR_STATE, "%s has not been called", data_call(e));
  NLSG_HIP(hipSetDevice(e->cfg.device));
  return time_repeats(
      e->stream, e->ev0, e->ev1, repeats, ms_total, [&]() -> int { return launch_solve(e); },
      [&]() -> int { return upload_theta(e, theta0_host); });  // the start point again, outside the interval
}

// Times `repeats` launches of the dominant kernel of the Cholesky pipeline (f, g, H at theta0
// for every problem) on the engine's stream, HIP events around each launch.
int nlsg_lm_time_eval_kernel(nlsg_lm *e, const double *theta0_host, uint32_t repeats, float *ms_total) {
  if (!e || !theta0_host || !ms_total) return fail(NLSG_ERR_INVALID_ARG, "null argument");
  if (const int prc = e->params_ready()) return prc;  // (before anything that could launch an evaluation)
  if (e->p.fd) return fail(NLSG_ERR_UNSUPPORTED, "Gauss-Newton model only");
  if (!e->has_data) return fail(NLSG_ERR_STATE, "%s has not been called", data_call(e));
  NLSG_HIP(hipSetDevice(e->cfg.device));
  int rc = upload_theta(e, theta0_host);
  if (rc) return rc;
  return time_repeats(e->stream, e->ev0, e->ev1, repeats, ms_total, [&]() -> int {
    if (e->wide)
      launch_wide_eval(e, 1);
    else
      launch_gn_iter(e, 1, 0);
    return NLSG_OK;
  });
}

// Times `repeats` launches of the QR step kernel alone (stop tests, damped matrix, Givens QR,
// back-substitution, update) after one evaluation at theta0 has produced H and g.
int nlsg_lm_time_qr_kernel(nlsg_lm *e, const double *theta0_host, uint32_t repeats, float *ms_total) {
  if (!e || !theta0_host || !ms_total) return fail(NLSG_ERR_INVALID_ARG, "null argument");
  if (const int prc = e->params_ready()) return prc;  // (before anything that could launch an evaluation)
  if (e->p.fd) return fail(NLSG_ERR_UNSUPPORTED, "Gauss-Newton model only");
  if (e->wide) return fail(NLSG_ERR_UNSUPPORTED, "the tinyqr step kernel: n <= 64 only");
  if (!e->has_data) return fail(NLSG_ERR_STATE, "%s has not been called", data_call(e));
  NLSG_HIP(hipSetDevice(e->cfg.device));
  int rc = upload_theta(e, theta0_host);
  if (rc) return rc;
  const dim3 grid(static_cast<unsigned>(e->p.batch));
  launch_gn_iter(e, 1, 0);
  return time_repeats(e->stream, e->ev0, e->ev1, repeats, ms_total, [&]() -> int {
    hipLaunchKernelGGL(lm_qr_step_kernel<kLmQrThreads>, grid, dim3(kLmQrThreads), sizeof(LmQrShared),
                       e->stream, e->p);
    return NLSG_OK;
  });
}

}  // extern "C"
