// tests/cpp/stub_nlsg.cpp — a stand-in libnlsolver_hip.so for tests/test_header_calls_cpu.py: every
// entry point that include/nlsolver_mi/nlsolver.h (device::api) and tinyqr.h (tinyqr::device) bind,
// defined with the prototypes of include/nlsg_c_api.h (a drifted signature fails to compile) and no
// HIP at all. It records what the headers ask of the library, so that the order of calls and every
// config field are pinned without a GPU.
//   $NLSG_STUB_LOG   every call appends one line here: the symbol, the config as hex over struct_size
//                    bytes, source bodies, parameter rows, start vectors, bounds, seeds, and for a
//                    destroy the engine's serial number; at exit, "live_engines N" (created - destroyed)
//   $NLSG_STUB_FAIL  the symbol named returns NLSG_ERR_HIP with last_error "stub: <symbol>"; every
//                    *_destroy overwrites last_error, so a message read after the destroy shows up
//   -DNLSG_STUB_OLD  leaves out the entry points the header binds as optional: "the library predates ..."
// minimize answers deterministically: x + 1 in every coordinate, f_value 1.5, iteration 2, the calls /
// gradient / Hessian counters 3 / 4 / 5, eps_after 0.125, lambda 0.25, and a fixed next generator state.
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "nlsg_c_api.h"

namespace {
std::string g_error = "stub: no error";
uint64_t g_serial = 0;
long g_live = 0;

void emit(const std::string &line) {
  const char *path = std::getenv("NLSG_STUB_LOG");
  if (!path || !*path) return;
  if (FILE *fp = std::fopen(path, "a")) {
    std::fprintf(fp, "%s\n", line.c_str());
    std::fclose(fp);
  }
}

std::string fmt(const char *f, ...) {
  char buf[256];
  va_list ap;
  va_start(ap, f);
  std::vsnprintf(buf, sizeof buf, f, ap);
  va_end(ap);
  return buf;
}
std::string hex(const void *p, size_t bytes) {
  if (!p) return "null";
  std::string out;
  for (size_t i = 0; i < bytes; i++) out += fmt("%02x", static_cast<const unsigned char *>(p)[i]);
  return out;
}
template <typename Cfg>
std::string config(const Cfg *cfg) {
  return cfg ? " cfg=" + hex(cfg, cfg->struct_size) : " cfg=null";
}
std::string text(const char *name, const char *s) {
  return std::string(" ") + name + "=" + (s ? "\"" + std::string(s) + "\"" : "null");
}
std::string doubles(const char *name, const double *v, uint64_t n) {
  std::string out = std::string(" ") + name + "=";
  if (!v) return out + "null";
  out += "[";
  for (uint64_t i = 0; i < n; i++) out += fmt(i ? ",%a" : "%a", v[i]);
  return out + "]";
}
[[maybe_unused]] std::string words(const char *name, const uint64_t *v, uint64_t n) {
  std::string out = std::string(" ") + name + "=";
  if (!v) return out + "null";
  out += "[";
  for (uint64_t i = 0; i < n; i++) out += fmt(i ? ",%016llx" : "%016llx", static_cast<unsigned long long>(v[i]));
  return out + "]";
}
std::string custom(const nlsg_custom_objective *obj) {
  if (!obj) return " obj=null";
  return text("term", obj->term_body) + text("finish", obj->finish_body) +
         fmt(" chain=%d n_params=%d", obj->chain, obj->n_params);
}

// logs the call and says whether $NLSG_STUB_FAIL names it
int called(const char *symbol, const std::string &args = "") {
  emit(std::string(symbol) + args);
  const char *fail = std::getenv("NLSG_STUB_FAIL");
  if (!fail || std::strcmp(fail, symbol) != 0) return NLSG_OK;
  g_error = std::string("stub: ") + symbol;
  return NLSG_ERR_HIP;
}

struct engine {
  uint64_t serial = 0, batch = 1, dim = 0, m = 0, k = 0;
  int32_t n_params = 0;
};
}  // namespace

struct nlsg_de : engine {};
struct nlsg_pso : engine {};
struct nlsg_bfgs : engine {};
struct nlsg_lm : engine {};
struct nlsg_nm : engine {};
struct nlsg_sann : engine {};
struct nlsg_nmpso : engine {};
struct nlsg_de_ref : engine {};
struct nlsg_de_batch : engine {};
struct nlsg_pso_batch : engine {};

namespace {
struct at_exit {
  ~at_exit() { emit(fmt("live_engines %ld", g_live)); }
} g_at_exit;

template <typename E>
int create(const char *symbol, const std::string &args, uint64_t batch, uint64_t dim,
           const nlsg_custom_objective *obj, E **out, uint64_t m = 0, uint64_t k = 0) {
  if (const int rc = called(symbol, args)) return rc;
#ifdef NLSG_STUB_OLD
  if (obj && obj->n_params != 0) {
    g_error = std::string("stub: ") + symbol + ": run-time parameters are unsupported";
    return NLSG_ERR_UNSUPPORTED;
  }
#endif
  E *e = new E;
  e->serial = ++g_serial;
  e->batch = batch;
  e->dim = dim;
  e->m = m;
  e->k = k;
  e->n_params = obj ? obj->n_params : 0;
  g_live++;
  *out = e;
  return NLSG_OK;
}
template <typename E>
int destroy(const char *symbol, E *e) {
  emit(std::string(symbol) + fmt(" serial=%llu", static_cast<unsigned long long>(e ? e->serial : 0)));
  g_error = std::string("stub: overwritten by ") + symbol;
  if (e) g_live--;
  delete e;
  return NLSG_OK;
}
template <typename E>
[[maybe_unused]] int set_params(const char *symbol, E *e, const double *rows) {
  return called(symbol, fmt(" serial=%llu", static_cast<unsigned long long>(e->serial)) +
                            doubles("params", rows, e->batch * static_cast<uint64_t>(e->n_params)));
}
std::string start(const engine *e, const double *x) {
  return fmt(" serial=%llu", static_cast<unsigned long long>(e->serial)) + doubles("x", x, e->batch * e->dim);
}
void answer(const engine *e, double *x, nlsg_status *st) {
  for (uint64_t i = 0; x && i < e->batch * e->dim; i++) x[i] += 1.0;
  for (uint64_t b = 0; st && b < e->batch; b++) {
    st[b] = nlsg_status{};
    st[b].f_value = 1.5;
    st[b].iteration = 2;
    st[b].function_calls_used = 3;
    st[b].gradient_evals_used = 4;
    st[b].hessian_evals_used = 5;
    st[b].done = 1;
  }
}
}  // namespace

extern "C" {
const char *nlsg_last_error(void) { return g_error.c_str(); }
int nlsg_abi_version(void) { return NLSG_ABI_VERSION; }
int nlsg_rtc_load(const char *hiprtc_path) { return called("nlsg_rtc_load", text("path", hiprtc_path)); }

// --- DE, turn engine
int nlsg_de_create(const nlsg_de_config *cfg, nlsg_de **out) {
  return create("nlsg_de_create", config(cfg), 1, cfg->dim, nullptr, out);
}
int nlsg_de_create_custom(const nlsg_de_config *cfg, const nlsg_custom_objective *obj, nlsg_de **out) {
  return create("nlsg_de_create_custom", config(cfg) + custom(obj), 1, cfg->dim, obj, out);
}
int nlsg_de_destroy(nlsg_de *e) { return destroy("nlsg_de_destroy", e); }
int nlsg_de_minimize(nlsg_de *e, double *x, uint64_t poll_every, nlsg_status *out) {
  if (const int rc = called("nlsg_de_minimize", start(e, x) + fmt(" poll_every=%llu",
                                                                static_cast<unsigned long long>(poll_every))))
    return rc;
  answer(e, x, out);
  return NLSG_OK;
}

// --- PSO, turn engine
int nlsg_pso_create(const nlsg_pso_config *cfg, nlsg_pso **out) {
  return create("nlsg_pso_create", config(cfg), 1, cfg->dim, nullptr, out);
}
int nlsg_pso_create_custom(const nlsg_pso_config *cfg, const nlsg_custom_objective *obj, nlsg_pso **out) {
  return create("nlsg_pso_create_custom", config(cfg) + custom(obj), 1, cfg->dim, obj, out);
}
int nlsg_pso_destroy(nlsg_pso *e) { return destroy("nlsg_pso_destroy", e); }
int nlsg_pso_minimize(nlsg_pso *e, double *x, const double *lower, const double *upper, uint64_t poll_every,
                      nlsg_status *out) {
  if (const int rc = called("nlsg_pso_minimize",
                            start(e, x) + doubles("lower", lower, e->dim) + doubles("upper", upper, e->dim) +
                                fmt(" poll_every=%llu", static_cast<unsigned long long>(poll_every))))
    return rc;
  answer(e, x, out);
  return NLSG_OK;
}

// --- BFGS
int nlsg_bfgs_create(const nlsg_bfgs_config *cfg, const double *diag, const double *lin, nlsg_bfgs **out) {
  return create("nlsg_bfgs_create", config(cfg) + doubles("diag", diag, cfg->dim) + doubles("lin", lin, cfg->dim),
                cfg->batch, cfg->dim, nullptr, out);
}
int nlsg_bfgs_create_custom(const nlsg_bfgs_config *cfg, const nlsg_custom_objective *obj, nlsg_bfgs **out) {
  return create("nlsg_bfgs_create_custom", config(cfg) + custom(obj), cfg->batch, cfg->dim, obj, out);
}
int nlsg_bfgs_destroy(nlsg_bfgs *e) { return destroy("nlsg_bfgs_destroy", e); }
int nlsg_bfgs_minimize(nlsg_bfgs *e, double *x, nlsg_status *st) {
  if (const int rc = called("nlsg_bfgs_minimize", start(e, x))) return rc;
  answer(e, x, st);
  return NLSG_OK;
}

// --- Levenberg-Marquardt
int nlsg_lm_create(const nlsg_lm_config *cfg, nlsg_lm **out) {
  return create("nlsg_lm_create", config(cfg), cfg->batch, cfg->n, nullptr, out, cfg->m);
}
int nlsg_lm_create_custom(const nlsg_lm_config *cfg, const nlsg_custom_objective *obj, nlsg_lm **out) {
  return create("nlsg_lm_create_custom", config(cfg) + custom(obj), cfg->batch, cfg->n, obj, out, cfg->m);
}
int nlsg_lm_destroy(nlsg_lm *e) { return destroy("nlsg_lm_destroy", e); }
int nlsg_lm_set_data(nlsg_lm *e, const double *a, const double *y) {
  return called("nlsg_lm_set_data", fmt(" serial=%llu", static_cast<unsigned long long>(e->serial)) +
                                        doubles("A", a, e->batch * e->m * e->dim) + doubles("y", y, e->batch * e->m));
}
int nlsg_lm_minimize(nlsg_lm *e, double *theta, nlsg_status *st, double *lambda_out) {
  if (const int rc = called("nlsg_lm_minimize", start(e, theta))) return rc;
  answer(e, theta, st);
  for (uint64_t b = 0; lambda_out && b < e->batch; b++) lambda_out[b] = 0.25;
  return NLSG_OK;
}

// --- Nelder-Mead
int nlsg_nm_create(const nlsg_nm_config *cfg, nlsg_nm **out) {
  return create("nlsg_nm_create", config(cfg), cfg->batch, cfg->dim, nullptr, out);
}
int nlsg_nm_create_custom(const nlsg_nm_config *cfg, const nlsg_custom_objective *obj, nlsg_nm **out) {
  return create("nlsg_nm_create_custom", config(cfg) + custom(obj), cfg->batch, cfg->dim, obj, out);
}
int nlsg_nm_destroy(nlsg_nm *e) { return destroy("nlsg_nm_destroy", e); }
int nlsg_nm_minimize(nlsg_nm *e, double *x, const double *upper, const double *lower, nlsg_status *st,
                     double *eps_out) {
  if (const int rc = called("nlsg_nm_minimize", start(e, x) + doubles("upper", upper, e->dim) +
                                                    doubles("lower", lower, e->dim)))
    return rc;
  answer(e, x, st);
  for (uint64_t b = 0; eps_out && b < e->batch; b++) eps_out[b] = 0.125;
  return NLSG_OK;
}

// --- the NM/PSO hybrid
int nlsg_nmpso_create(const nlsg_nmpso_config *cfg, nlsg_nmpso **out) {
  return create("nlsg_nmpso_create", config(cfg), cfg->batch, cfg->dim, nullptr, out);
}
int nlsg_nmpso_create_custom(const nlsg_nmpso_config *cfg, const nlsg_custom_objective *obj, nlsg_nmpso **out) {
  return create("nlsg_nmpso_create_custom", config(cfg) + custom(obj), cfg->batch, cfg->dim, obj, out);
}
int nlsg_nmpso_destroy(nlsg_nmpso *e) { return destroy("nlsg_nmpso_destroy", e); }
int nlsg_nmpso_minimize(nlsg_nmpso *e, double *x, const double *lower, const double *upper, nlsg_status *st) {
  if (const int rc = called("nlsg_nmpso_minimize", start(e, x) + doubles("lower", lower, e->dim) +
                                                       doubles("upper", upper, e->dim)))
    return rc;
  answer(e, x, st);
  return NLSG_OK;
}

// --- simulated annealing
int nlsg_sann_create(const nlsg_sann_config *cfg, nlsg_sann **out) {
  return create("nlsg_sann_create", config(cfg), cfg->batch, cfg->dim, nullptr, out);
}
int nlsg_sann_create_custom(const nlsg_sann_config *cfg, const nlsg_custom_objective *obj, nlsg_sann **out) {
  return create("nlsg_sann_create_custom", config(cfg) + custom(obj), cfg->batch, cfg->dim, obj, out);
}
int nlsg_sann_destroy(nlsg_sann *e) { return destroy("nlsg_sann_destroy", e); }
int nlsg_sann_minimize(nlsg_sann *e, double *x, nlsg_status *st) {
  if (const int rc = called("nlsg_sann_minimize", start(e, x))) return rc;
  answer(e, x, st);
  return NLSG_OK;
}

// --- tinyqr::device
int nlsg_tinyqr_lm(const double *X, const double *y, uint64_t batch, uint64_t n, uint64_t p, double tol,
                   int32_t device, double *beta, float *ms_kernel) {
  if (const int rc = called("nlsg_tinyqr_lm",
                            fmt(" batch=%llu n=%llu p=%llu tol=%a device=%d ms_kernel=%s",
                                static_cast<unsigned long long>(batch), static_cast<unsigned long long>(n),
                                static_cast<unsigned long long>(p), tol, device, ms_kernel ? "set" : "null") +
                                doubles("X", X, batch * n * p) + doubles("y", y, batch * n)))
    return rc;
  for (uint64_t i = 0; i < batch * p; i++) beta[i] = 0.5 + static_cast<double>(i);
  return NLSG_OK;
}

#ifndef NLSG_STUB_OLD
// --- what the header binds as optional
int nlsg_de_ref_create(const nlsg_de_ref_config *cfg, nlsg_de_ref **out) {
  return create("nlsg_de_ref_create", config(cfg), cfg->batch, cfg->dim, nullptr, out);
}
int nlsg_de_ref_create_custom(const nlsg_de_ref_config *cfg, const nlsg_custom_objective *obj,
                              nlsg_de_ref **out) {
  return create("nlsg_de_ref_create_custom", config(cfg) + custom(obj), cfg->batch, cfg->dim, obj, out);
}
int nlsg_de_ref_destroy(nlsg_de_ref *e) { return destroy("nlsg_de_ref_destroy", e); }
int nlsg_de_ref_minimize(nlsg_de_ref *e, double *x, uint64_t *rng_state, nlsg_status *st) {
  if (const int rc = called("nlsg_de_ref_minimize", start(e, x) + words("state", rng_state, 2 * e->batch)))
    return rc;
  answer(e, x, st);
  for (uint64_t b = 0; b < e->batch; b++) {
    rng_state[2 * b] = 0x0123456789abcdefull;
    rng_state[2 * b + 1] = 0xfedcba9876543210ull;
  }
  return NLSG_OK;
}

uint64_t nlsg_de_batch_lds_bytes(uint64_t pop, uint64_t dim) {
  const uint64_t need = pop < 4 || pop > 1024 || dim > 128 ? 0 : 4096 + 8 * pop * (dim + 2);
  emit(fmt("nlsg_de_batch_lds_bytes pop=%llu dim=%llu -> %llu", static_cast<unsigned long long>(pop),
           static_cast<unsigned long long>(dim), static_cast<unsigned long long>(need)));
  return need;
}
int nlsg_de_batch_create(const nlsg_de_batch_config *cfg, nlsg_de_batch **out) {
  return create("nlsg_de_batch_create", config(cfg), cfg->batch, cfg->dim, nullptr, out);
}
int nlsg_de_batch_create_custom(const nlsg_de_batch_config *cfg, const nlsg_custom_objective *obj,
                                nlsg_de_batch **out) {
  return create("nlsg_de_batch_create_custom", config(cfg) + custom(obj), cfg->batch, cfg->dim, obj, out);
}
int nlsg_de_batch_set_params(nlsg_de_batch *e, const double *rows) {
  return set_params("nlsg_de_batch_set_params", e, rows);
}
int nlsg_de_batch_destroy(nlsg_de_batch *e) { return destroy("nlsg_de_batch_destroy", e); }
int nlsg_de_batch_minimize(nlsg_de_batch *e, double *x, const uint64_t *seeds, nlsg_status *st) {
  if (const int rc = called("nlsg_de_batch_minimize", start(e, x) + words("seeds", seeds, e->batch))) return rc;
  answer(e, x, st);
  return NLSG_OK;
}

uint64_t nlsg_pso_batch_lds_bytes(uint64_t n_particles, uint64_t dim, int32_t type) {
  const uint64_t rows = type == NLSG_PSO_VANILLA ? 3 : 1;
  const uint64_t need = n_particles == 0 || n_particles > 1024 || dim > 128 ? 0 : 4096 + 8 * rows * n_particles * dim;
  emit(fmt("nlsg_pso_batch_lds_bytes n_particles=%llu dim=%llu type=%d -> %llu",
           static_cast<unsigned long long>(n_particles), static_cast<unsigned long long>(dim), type,
           static_cast<unsigned long long>(need)));
  return need;
}
int nlsg_pso_batch_create(const nlsg_pso_batch_config *cfg, nlsg_pso_batch **out) {
  return create("nlsg_pso_batch_create", config(cfg), cfg->batch, cfg->dim, nullptr, out);
}
int nlsg_pso_batch_create_custom(const nlsg_pso_batch_config *cfg, const nlsg_custom_objective *obj,
                                 nlsg_pso_batch **out) {
  return create("nlsg_pso_batch_create_custom", config(cfg) + custom(obj), cfg->batch, cfg->dim, obj, out);
}
int nlsg_pso_batch_set_params(nlsg_pso_batch *e, const double *rows) {
  return set_params("nlsg_pso_batch_set_params", e, rows);
}
int nlsg_pso_batch_destroy(nlsg_pso_batch *e) { return destroy("nlsg_pso_batch_destroy", e); }
int nlsg_pso_batch_minimize(nlsg_pso_batch *e, double *x, const double *lower, const double *upper,
                            const uint64_t *seeds, nlsg_status *st) {
  if (const int rc = called("nlsg_pso_batch_minimize",
                            start(e, x) + doubles("lower", lower, e->dim) + doubles("upper", upper, e->dim) +
                                words("seeds", seeds, e->batch)))
    return rc;
  answer(e, x, st);
  return NLSG_OK;
}

uint64_t nlsg_custom_params_lds_bytes(int32_t n_params) {
  const uint64_t need = n_params <= 0 || n_params > NLSG_CUSTOM_MAX_PARAMS ? 0 : 8 * static_cast<uint64_t>(n_params);
  emit(fmt("nlsg_custom_params_lds_bytes n_params=%d -> %llu", n_params, static_cast<unsigned long long>(need)));
  return need;
}

int nlsg_nm_create_params(const nlsg_nm_config *cfg, const nlsg_custom_objective *obj, nlsg_nm **out) {
  return create("nlsg_nm_create_params", config(cfg) + custom(obj), cfg->batch, cfg->dim, obj, out);
}
int nlsg_nm_set_params(nlsg_nm *e, const double *rows) { return set_params("nlsg_nm_set_params", e, rows); }
int nlsg_nmpso_create_params(const nlsg_nmpso_config *cfg, const nlsg_custom_objective *obj, nlsg_nmpso **out) {
  return create("nlsg_nmpso_create_params", config(cfg) + custom(obj), cfg->batch, cfg->dim, obj, out);
}
int nlsg_nmpso_set_params(nlsg_nmpso *e, const double *rows) { return set_params("nlsg_nmpso_set_params", e, rows); }
int nlsg_bfgs_create_params(const nlsg_bfgs_config *cfg, const nlsg_custom_objective *obj, nlsg_bfgs **out) {
  return create("nlsg_bfgs_create_params", config(cfg) + custom(obj), cfg->batch, cfg->dim, obj, out);
}
int nlsg_bfgs_set_params(nlsg_bfgs *e, const double *rows) { return set_params("nlsg_bfgs_set_params", e, rows); }
int nlsg_lm_create_params(const nlsg_lm_config *cfg, const nlsg_custom_objective *obj, nlsg_lm **out) {
  return create("nlsg_lm_create_params", config(cfg) + custom(obj), cfg->batch, cfg->n, obj, out, cfg->m);
}
int nlsg_lm_set_params(nlsg_lm *e, const double *rows) { return set_params("nlsg_lm_set_params", e, rows); }

int nlsg_lm_create_link(const nlsg_lm_config *cfg, const nlsg_lm_link *link, nlsg_lm **out) {
  return create("nlsg_lm_create_link", config(cfg) + text("value", link->value_body) + text("slope", link->slope_body),
                cfg->batch, cfg->n, nullptr, out, cfg->m);
}
int nlsg_lm_create_curve(const nlsg_lm_config *cfg, const nlsg_lm_curve *curve, nlsg_lm **out) {
  return create("nlsg_lm_create_curve", config(cfg) + text("body", curve->body) + fmt(" k=%u", curve->k), cfg->batch,
                cfg->n, nullptr, out, cfg->m, curve->k);
}
int nlsg_lm_set_curve_data(nlsg_lm *e, const double *t, const double *y) {
  return called("nlsg_lm_set_curve_data", fmt(" serial=%llu", static_cast<unsigned long long>(e->serial)) +
                                              doubles("t", t, e->batch * e->m * e->k) +
                                              doubles("y", y, e->batch * e->m));
}
int nlsg_bfgs_create_gradient(const nlsg_bfgs_config *cfg, const nlsg_custom_objective *obj,
                              const nlsg_bfgs_gradient *grad, nlsg_bfgs **out) {
  return create("nlsg_bfgs_create_gradient",
                config(cfg) + custom(obj) + fmt(" grad_size=%u grad_reserved=%u", grad->struct_size, grad->reserved) +
                    text("grad", grad->grad_body),
                cfg->batch, cfg->dim, obj, out);
}
uint64_t nlsg_bfgs_lds_bytes(uint64_t dim, uint32_t flags) {
  const uint64_t need = (flags & NLSG_BFGS_RESIDENT) ? (dim <= 64 ? 1024 + 8 * dim * dim : 0) : 512;
  emit(fmt("nlsg_bfgs_lds_bytes dim=%llu flags=%u -> %llu", static_cast<unsigned long long>(dim), flags,
           static_cast<unsigned long long>(need)));
  return need;
}
#endif  // NLSG_STUB_OLD
}  // extern "C"
