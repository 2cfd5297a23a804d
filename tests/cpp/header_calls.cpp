// tests/cpp/header_calls.cpp — every device branch of include/nlsolver_mi/nlsolver.h and
// tinyqr::device::lm, run against the stand-in library of stub_nlsg.cpp (tests/test_header_calls_cpu.py).
// One case per run; the case is one word whose parts are separated by ':' (the driver modes, the
// summation order, the failing symbol and the library come from the environment). Prints what the class
// handed back: x, every solver_status field, the eps or lambda it kept, the generator's state.
//   header_calls de:rosenbrock|custom|params:random|best:min|max[:big]
//   header_calls pso:rosenbrock|custom|params:vanilla|accel:free|bounded:min|max[:big]
//   header_calls nm:rosenbrock|rastrigin|custom|vector|params:free|bounded:min|max
//   header_calls bfgs:quad|rosenbrock|custom|params|grad|gradparams|gradempty:one|batch|alloc[:n65]
//   header_calls lm:tanh|link|curve|rosenbrock|custom|params:one|batch|mismatch|alloc
//   header_calls sann:rosenbrock|custom|params:one|batch|alloc:min|max
//   header_calls nmpso:rosenbrock|custom|params:one|batch|bounded|alloc:min|max
//   header_calls tinyqr
// `alloc`: the first allocation of the solve's flat start vector throws std::bad_alloc (operator new
// below), which is after the engine was made: the engine must still be destroyed.
#include <cstdio>
#include <cstdlib>
#include <new>
#include <sstream>
#include <string>
#include <vector>

#include "nlsolver_mi/nlsolver.h"

namespace nl = nlsolver;
namespace dev = nlsolver::device;
using vec = std::vector<double>;

// (noinline: an inlined pair makes g++ 11 report malloc / free as mismatched with new / delete)
static size_t g_refuse_bytes = 0;  // operator new throws for a request of exactly this size
__attribute__((noinline)) void *operator new(size_t bytes) {
  if (g_refuse_bytes != 0 && bytes == g_refuse_bytes) throw std::bad_alloc();
  if (void *p = std::malloc(bytes ? bytes : 1)) return p;
  throw std::bad_alloc();
}
__attribute__((noinline)) void operator delete(void *p) noexcept { std::free(p); }
__attribute__((noinline)) void operator delete(void *p, size_t) noexcept { std::free(p); }

static void show_x(const vec &x) {
  std::printf(" x=[");
  for (size_t i = 0; i < x.size(); i++) std::printf(i ? ",%a" : "%a", x[i]);
  std::printf("]");
}
static void show(const char *tag, const nl::solver_status<double> &st, const vec &x) {
  auto [fcalls, iters, f, g, h] = st.get_summary();
  std::printf("%s f=%a iters=%zu fcalls=%zu gcalls=%zu hcalls=%zu", tag, f, iters, fcalls, g, h);
  show_x(x);
  std::printf("\n");
}
static void show_batch(const std::vector<nl::solver_status<double>> &st, const std::vector<vec> &xs) {
  for (size_t b = 0; b < xs.size(); b++) show(("start " + std::to_string(b)).c_str(), st[b], xs[b]);
}
static void show_rng(const nl::rng::xorshift<double> &gen) {
  const auto s = gen.raw_state();
  std::printf("rng %016llx %016llx\n", static_cast<unsigned long long>(s[0]), static_cast<unsigned long long>(s[1]));
}

static const char *kChain = "double t1 = 1 - xi; double t2 = xn - xi * xi; return t1 * t1 + 100 * t2 * t2;";
static const char *kTerms = "double r = xi - p(0); return p(1) * r * r;";

// the Custom objective a case names: custom (a chain, no parameters), vector (whole-vector body),
// params (terms that read two parameters)
static dev::Custom<double> custom_of(const std::string &kind) {
  if (kind == "vector") return dev::Custom<double>::vector("return x(0) * x(0) + x(1);");
  if (kind == "params" || kind == "gradparams") {
    dev::Custom<double> f(kTerms, false, "return s + D;");
    f.params = {1.5, 2.0};
    if (kind == "gradparams") f.grad_body = "return 2.0 * p(1) * (xi - p(0));";
    return f;
  }
  dev::Custom<double> f(kChain, true);
  if (kind == "grad") f.grad_body = "return 2.0 * xi;";
  return f;
}
static vec ramp(size_t n, double x0, double step) {
  vec x(n);
  for (size_t i = 0; i < n; i++) x[i] = x0 + step * static_cast<double>(i);
  return x;
}

template <typename F, nl::RecombinationStrategy S>
static void run_de(F &f, bool minimize, bool big) {
  nl::rng::xorshift<double> gen;
  nl::DE<F, nl::rng::xorshift<double>, double, S> solver(f, gen, 0.75, 0.5, 1e-3, big ? 2000 : 12, 34, 5);
  vec x = {5, 7, -2};
  show("de", minimize ? solver.minimize(x) : solver.maximize(x), x);
  show_rng(gen);
}
template <typename F>
static void case_de(F &f, const std::vector<std::string> &a) {
  const bool big = a.size() > 4 && a[4] == "big";
  if (a[2] == "best")
    run_de<F, nl::best>(f, a[3] == "min", big);
  else
    run_de<F, nl::random>(f, a[3] == "min", big);
}

template <typename F, nl::PSOType T>
static void run_pso(F &f, bool bounded, bool minimize, bool big) {
  nl::rng::xorshift<double> gen;
  nl::PSO<F, nl::rng::xorshift<double>, double, T> solver(f, gen, 0.75, 1.5, 1.25, big ? 2000 : 9, 33, 4, 1e-3);
  vec x = {3, -4, 0.5};
  const vec lower = {-1, -2, -3}, upper = {1.5, 2.5, 3.5};
  if (bounded)
    show("pso", minimize ? solver.minimize(x, lower, upper) : solver.maximize(x, lower, upper), x);
  else
    show("pso", minimize ? solver.minimize(x) : solver.maximize(x), x);
  show_rng(gen);
}
template <typename F>
static void case_pso(F &f, const std::vector<std::string> &a) {
  const bool big = a.size() > 5 && a[5] == "big";
  if (a[2] == "accel")
    run_pso<F, nl::Accelerated>(f, a[3] == "bounded", a[4] == "min", big);
  else
    run_pso<F, nl::Vanilla>(f, a[3] == "bounded", a[4] == "min", big);
}

template <typename F>
static void case_nm(F &f, const std::vector<std::string> &a) {
  nl::NelderMead<F, double> solver(f, 0.5, 1.25, 2.5, 0.25, 0.75, 1e-4, 77, 6, 2);
  vec x = {0.5, 1.5, -2.5};
  const vec upper = {4, 5, 6}, lower = {-4, -5, -6};
  for (int call = 0; call < 2; call++) {  // the second call starts from the eps the first one left
    nl::solver_status<double> st = a[2] == "bounded"
                                       ? (a[3] == "min" ? solver.minimize(x, upper, lower) : solver.maximize(x, upper, lower))
                                       : (a[3] == "min" ? solver.minimize(x) : solver.maximize(x));
    show("nm", st, x);
  }
}

template <typename F, typename Grad>
static void run_bfgs(F &f, const std::vector<std::string> &a) {
  const size_t n = a.size() > 3 && a[3] == "n65" ? 65 : 3;
  nl::BFGS<F, double, Grad> solver(f, Grad(), 41, 1e-4, 0.5);
  if (a[2] == "one") {
    vec x = ramp(n, 0.5, 0.25);
    show("bfgs", solver.minimize(x), x);
  } else if (a[2] == "batch") {
    std::vector<vec> xs = {ramp(n, 0.5, 0.25), ramp(n, -1.0, 0.5)};
    show_batch(solver.minimize_batch(xs), xs);
  } else {  // alloc: one start of 12345 coordinates, whose flat copy is refused
    std::vector<vec> xs = {ramp(12345, 0.0, 1.0)};
    g_refuse_bytes = 12345 * sizeof(double);
    solver.minimize_batch(xs);
  }
}

template <typename F>
static void run_lm(F &f, const std::vector<std::string> &a, size_t n) {
  nl::LevenbergMarquardt<F, double> solver(f, 8, 4, 2, 21, 1e-9);
  if (a[2] == "one") {
    vec x = ramp(n, 0.5, 0.25);
    show("lm", solver.minimize(x), x);
    show("lm again", solver.minimize(x), x);  // with the lambda the first call wrote back
  } else if (a[2] == "alloc") {
    std::vector<vec> xs = {ramp(n, 0.0, 1.0)};
    g_refuse_bytes = n * sizeof(double);
    solver.minimize_batch(xs);
  } else {  // batch, or mismatch: three starts for a model of two problems
    std::vector<vec> xs = {ramp(n, 0.5, 0.25), ramp(n, -1.0, 0.5)};
    if (a[2] == "mismatch") xs.push_back(ramp(n, 0.0, 1.0));
    show_batch(solver.minimize_batch(xs), xs);
    xs.resize(2);
    show_batch(solver.minimize_batch(xs), xs);  // lambda is not written back by a batch
  }
}
static void case_lm(const std::vector<std::string> &a) {
  const size_t B = a[2] == "one" || a[2] == "alloc" ? 1 : 2, m = 3;
  const size_t n = a[2] == "alloc" ? 12345 : 2;
  if (a[1] == "tanh") {
    dev::TanhRegression<double> f(m, n, ramp(B * m * n, 0.125, 0.125), ramp(B * m, -0.5, 0.25));
    run_lm(f, a, n);
  } else if (a[1] == "link") {
    dev::LinkRegression<double> f(m, n, ramp(B * m * n, 0.125, 0.125), ramp(B * m, -0.5, 0.25),
                                  "return 1.0 / (1.0 + det_exp(-z));", "return v * (1.0 - v);");
    run_lm(f, a, n);
  } else if (a[1] == "curve") {
    dev::CurveModel<double> f(m, n, 2, ramp(B * m * 2, 1.0, 0.5), ramp(B * m, -0.5, 0.25),
                              "r = y - th(0) * t(0) - th(1) * t(1); J(0) = -t(0); J(1) = -t(1);");
    run_lm(f, a, n);
  } else if (a[1] == "rosenbrock") {
    dev::Rosenbrock<double> f;
    run_lm(f, a, n);
  } else {
    dev::Custom<double> f = custom_of(a[1]);
    run_lm(f, a, n);
  }
}

template <typename F>
static void case_sann(F &f, const std::vector<std::string> &a) {
  nl::rng::xorshift<double> gen;
  nl::SANN<F, nl::rng::xorshift<double>, double> solver(f, gen, 55, 7, 12.5);
  if (a[2] == "one") {
    vec x = {0.5, 1.5, -2.5};
    show("sann", a[3] == "min" ? solver.minimize(x) : solver.maximize(x), x);
  } else if (a[2] == "alloc") {
    std::vector<vec> xs = {ramp(12345, 0.0, 1.0)};
    g_refuse_bytes = 12345 * sizeof(double);
    solver.minimize_batch(xs);
  } else {
    std::vector<vec> xs = {{0.5, 1.5, -2.5}, {1, 2, 3}};
    show_batch(a[3] == "min" ? solver.minimize_batch(xs) : solver.maximize_batch(xs), xs);
  }
  show_rng(gen);
}

template <typename F>
static void case_nmpso(F &f, const std::vector<std::string> &a) {
  nl::rng::xorshift<double> gen;
  nl::NelderMeadPSO<F, nl::rng::xorshift<double>, double> solver(f, gen, 1.25, 2.5, 0.25, 0.75, 0.625, 1.5, 1.75,
                                                                 1e-5, 66, 8);
  vec x = {0.5, 1.5, -2.5};
  const vec lower = {-4, -5, -6}, upper = {4, 5, 6};
  if (a[2] == "batch") {
    std::vector<vec> xs = {x, {1, 2, 3}};
    show_batch(solver.minimize_batch(xs), xs);
  } else if (a[2] == "alloc") {
    std::vector<vec> xs = {ramp(12345, 0.0, 1.0)};
    g_refuse_bytes = 12345 * sizeof(double);
    solver.minimize_batch(xs);
  } else if (a[2] == "bounded") {
    show("nmpso", a[3] == "min" ? solver.minimize(x, lower, upper) : solver.maximize(x, lower, upper), x);
  } else {
    show("nmpso", a[3] == "min" ? solver.minimize(x) : solver.maximize(x), x);
  }
  show_rng(gen);
}

// the objective a case names, handed to `body` as its own type
template <typename Body>
static void with_objective(const std::string &kind, Body body) {
  if (kind == "rosenbrock") {
    dev::Rosenbrock<double> f;
    body(f);
  } else if (kind == "rastrigin") {
    dev::Rastrigin<double> f;
    body(f);
  } else {
    dev::Custom<double> f = custom_of(kind);
    body(f);
  }
}

static int run_case(const std::vector<std::string> &a) {
  const std::string &cls = a[0];
  if (cls == "de") {
    with_objective(a[1], [&](auto &f) { case_de(f, a); });
  } else if (cls == "pso") {
    with_objective(a[1], [&](auto &f) { case_pso(f, a); });
  } else if (cls == "nm") {
    with_objective(a[1], [&](auto &f) { case_nm(f, a); });
  } else if (cls == "sann") {
    with_objective(a[1], [&](auto &f) { case_sann(f, a); });
  } else if (cls == "nmpso") {
    with_objective(a[1], [&](auto &f) { case_nmpso(f, a); });
  } else if (cls == "bfgs") {
    if (a[1] == "quad") {
      const size_t n = a.size() > 3 && a[3] == "n65" ? 65 : a[2] == "alloc" ? 12345 : 3;
      dev::QuadDiagRank1<double> f(ramp(n, 1.0, 0.5), ramp(n, -1.0, 0.25), 0.375);
      run_bfgs<decltype(f), dev::analytic_grad>(f, a);
    } else if (a[1] == "rosenbrock") {
      dev::Rosenbrock<double> f;
      run_bfgs<decltype(f), nl::fin_diff<decltype(f), double>>(f, a);
    } else if (a[1] == "custom" || a[1] == "params") {
      dev::Custom<double> f = custom_of(a[1]);
      run_bfgs<decltype(f), nl::fin_diff<decltype(f), double>>(f, a);
    } else {  // grad, gradparams, gradempty
      dev::Custom<double> f = custom_of(a[1] == "gradempty" ? "custom" : a[1]);
      run_bfgs<decltype(f), dev::analytic_grad>(f, a);
    }
  } else if (cls == "lm") {
    case_lm(a);
  } else if (cls == "tinyqr") {
    const vec beta = tinyqr::device::lm(ramp(2 * 3 * 2, 1.0, 0.5), ramp(2 * 3, -1.0, 0.75), 2, 1e-10, 1);
    std::printf("tinyqr");
    show_x(beta);
    std::printf("\n");
  } else {
    return 2;
  }
  return 0;
}

int main(int argc, char **argv) {
  if (argc != 2) {
    std::fprintf(stderr, "usage: header_calls CASE\n");
    return 2;
  }
  std::vector<std::string> parts;
  std::stringstream in(argv[1]);
  for (std::string part; std::getline(in, part, ':');) parts.push_back(part);
  parts.resize(std::max<size_t>(parts.size(), 6));
  int rc = 0;
  try {
    rc = run_case(parts);
  } catch (const nl::device_error &e) {
    g_refuse_bytes = 0;
    std::printf("device_error: %s\n", e.what());
    rc = 3;
  } catch (const tinyqr::device::device_error &e) {
    std::printf("tinyqr device_error: %s\n", e.what());
    rc = 3;
  } catch (const std::bad_alloc &) {
    g_refuse_bytes = 0;
    std::printf("bad_alloc\n");
    rc = 4;
  }
  return rc;
}
