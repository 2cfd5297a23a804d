// tests/cpp/header_bfgs_resident.cpp — the drop-in header's BFGS under device::bfgs_driver_mode(): the
// Rosenbrock chain as a device::Custom<double> objective, solved from the starts given on the command line.
//   header_bfgs_resident analytic X0 X1 ...        one solve with the objective's gradient body
//   header_bfgs_resident default  X0 X1 ...        one solve with the default finite differences
//   header_bfgs_resident batch D X0 ... X(kD-1)    minimize_batch of k starts of D coordinates: a JSON list
// The driver comes from the environment (NLSG_BFGS_DRIVER = turns | resident): either must print the same x,
// f and counts, and so must the Python drop-in; a misspelt value is a device_error, exit code 3.
// Built by tests/test_bfgs_resident_gpu.py itself (g++ -std=c++17).
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "nlsolver_mi/nlsolver.h"

namespace dev = nlsolver::device;

static const char *kTerm = "double t1 = 1 - xi; double t2 = xn - xi * xi; return t1 * t1 + 100 * t2 * t2;";
static const char *kGrad =
    "double g = 0.0; if (i + 1 < D) g = -2.0 * (1.0 - xi) - 400.0 * xi * (xn - xi * xi); "
    "if (i > 0) g = g + 200.0 * (xi - xm * xm); return g;";

static void print(const nlsolver::solver_status<double> &res, const std::vector<double> &x) {
  auto [fcalls, iters, f, g, h] = res.get_summary();
  (void)h;
  std::printf("{\"fcalls\":%zu,\"gcalls\":%zu,\"iters\":%zu,\"f\":\"%a\",\"x\":[", fcalls, static_cast<size_t>(g),
              iters, f);
  for (size_t i = 0; i < x.size(); i++) std::printf("%s\"%a\"", i ? "," : "", x[i]);
  std::printf("]}\n");
}

int main(int argc, char **argv) {
  if (argc < 3) {
    std::fprintf(stderr, "usage: header_bfgs_resident analytic|default|batch ...\n");
    return 2;
  }
  try {
    dev::Custom<double> prob(kTerm, /*chain=*/true);
    if (std::strcmp(argv[1], "batch") == 0) {
      const size_t D = std::strtoul(argv[2], nullptr, 10);
      std::vector<double> v;
      for (int k = 3; k < argc; k++) v.push_back(std::strtod(argv[k], nullptr));
      if (D == 0 || v.empty() || v.size() % D != 0) {
        std::fprintf(stderr, "batch needs D and k starts of D coordinates\n");
        return 2;
      }
      std::vector<std::vector<double>> xs;
      for (size_t b = 0; b < v.size() / D; b++) xs.emplace_back(v.begin() + b * D, v.begin() + (b + 1) * D);
      auto solver = nlsolver::BFGS<dev::Custom<double>, double>(prob);
      const auto res = solver.minimize_batch(xs);
      std::printf("[");
      for (size_t b = 0; b < xs.size(); b++) {
        if (b) std::printf(",");
        print(res[b], xs[b]);
      }
      std::printf("]\n");
      return 0;
    }
    std::vector<double> x;
    for (int k = 2; k < argc; k++) x.push_back(std::strtod(argv[k], nullptr));
    if (std::strcmp(argv[1], "analytic") == 0) {
      prob.grad_body = kGrad;
      auto solver = nlsolver::BFGS<dev::Custom<double>, double, dev::analytic_grad>(prob);
      print(solver.minimize(x), x);
    } else {
      auto solver = nlsolver::BFGS<dev::Custom<double>, double>(prob);
      print(solver.minimize(x), x);
    }
  } catch (const nlsolver::device_error &e) {
    std::fprintf(stderr, "device_error: %s\n", e.what());
    return 3;
  }
  return 0;
}
