// tests/cpp/header_bfgs_gradient.cpp — a device::Custom<double> objective that carries its analytic
// gradient (Custom::grad_body) through the drop-in header's BFGS: one solve of the Rosenbrock chain from
// the start given on the command line, as one JSON object.
//   header_bfgs_gradient analytic X0 X1 ...   BFGS<Custom, double, device::analytic_grad>: the gradient body
//   header_bfgs_gradient default  X0 X1 ...   the same Custom under the default Grad: finite differences
//   header_bfgs_gradient empty    X0 X1 ...   analytic_grad without a body: device_error, exit code 3
//   header_bfgs_gradient batch P0 X0 ... X(2D-1)   minimize_batch of two starts of a quartic whose coefficient
//                                                   is Custom::params[0], under analytic_grad: a JSON list
// The Python drop-ins on the same objective must give the same x and status.
// Built by tests/test_bfgs_gradient_gpu.py itself (g++ -std=c++17).
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "nlsolver_mi/nlsolver.h"

namespace dev = nlsolver::device;

static const char *kTerm = "double t1 = 1 - xi; double t2 = xn - xi * xi; return t1 * t1 + 100 * t2 * t2;";
static const char *kGrad =
    "double g = 0.0; if (i + 1 < D) g = -2.0 * (1.0 - xi) - 400.0 * xi * (xn - xi * xi); "
    "if (i > 0) g = g + 200.0 * (xi - xm * xm); return g;";

static const char *kQuartic = "double q = xi * xi; return 0.5 * (q * q - p(0) * q + 5.0 * xi);";
static const char *kQuarticGrad = "return 0.5 * (4.0 * xi * xi * xi - 2.0 * p(0) * xi + 5.0);";

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
    std::fprintf(stderr, "usage: header_bfgs_gradient analytic|default|empty|batch X0 X1 ...\n");
    return 2;
  }
  std::vector<double> x;
  for (int k = 2; k < argc; k++) x.push_back(std::strtod(argv[k], nullptr));
  try {
    if (std::strcmp(argv[1], "batch") == 0) {
      if (x.size() < 3 || x.size() % 2 == 0) {
        std::fprintf(stderr, "batch needs P0 and two starts of equal length\n");
        return 2;
      }
      dev::Custom<double> prob(kQuartic);
      prob.grad_body = kQuarticGrad;
      prob.params = {x[0]};
      const size_t D = (x.size() - 1) / 2;
      std::vector<std::vector<double>> xs = {std::vector<double>(x.begin() + 1, x.begin() + 1 + D),
                                             std::vector<double>(x.begin() + 1 + D, x.end())};
      auto solver = nlsolver::BFGS<dev::Custom<double>, double, dev::analytic_grad>(prob);
      const auto res = solver.minimize_batch(xs);
      std::printf("[");
      for (size_t b = 0; b < xs.size(); b++) {
        if (b) std::printf(",");
        print(res[b], xs[b]);
      }
      std::printf("]\n");
      return 0;
    }
    dev::Custom<double> prob(kTerm, /*chain=*/true);
    if (std::strcmp(argv[1], "empty") != 0) prob.grad_body = kGrad;
    if (std::strcmp(argv[1], "default") == 0) {
      auto solver = nlsolver::BFGS<dev::Custom<double>, double>(prob);
      print(solver.minimize(x), x);
    } else {
      auto solver = nlsolver::BFGS<dev::Custom<double>, double, dev::analytic_grad>(prob);
      print(solver.minimize(x), x);
    }
  } catch (const nlsolver::device_error &e) {
    std::fprintf(stderr, "device_error: %s\n", e.what());
    return 3;
  }
  return 0;
}
