// tests/cpp/header_lm_bfgs_params.cpp — a device::Custom<double> objective that owns run-time data
// (Custom::params, read in the body as p(k)) through the drop-in header's BFGS and
// LevenbergMarquardt: one solve each from x0 = (5, 7), as one JSON object. Both create their engine
// with the library's *_create_params and send the one row; the Python drop-ins with params= must give
// the same x and status.
//   header_lm_bfgs_params P0 P1 P2
// Built by tests/test_lm_bfgs_params_gpu.py itself (g++ -std=c++17).
#include <cstdio>
#include <cstdlib>

#include "nlsolver_mi/nlsolver.h"

namespace dev = nlsolver::device;

static const char *kTerms = "double r = xi - p(0); return p(1) * r * r + r / p(2);";

static void print(const char *name, const nlsolver::solver_status<double> &res, const std::vector<double> &x,
                  bool last) {
  auto [fcalls, iters, f, g, h] = res.get_summary();
  (void)g;
  (void)h;
  std::printf("\"%s\":{\"fcalls\":%zu,\"iters\":%zu,\"f\":\"%a\",\"x\":[\"%a\",\"%a\"]}%s", name, fcalls, iters,
              f, x[0], x[1], last ? "" : ",");
}

int main(int argc, char **argv) {
  if (argc != 4) {
    std::fprintf(stderr, "usage: header_lm_bfgs_params P0 P1 P2\n");
    return 2;
  }
  try {
    dev::Custom<double> prob(kTerms);
    for (int k = 1; k < argc; k++) prob.params.push_back(std::strtod(argv[k], nullptr));
    std::printf("{");
    {
      auto solver = nlsolver::BFGS<dev::Custom<double>, double>(prob);
      std::vector<double> x = {5, 7};
      print("bfgs", solver.minimize(x), x, false);
    }
    {
      auto solver = nlsolver::LevenbergMarquardt<dev::Custom<double>, double>(prob);
      std::vector<double> x = {5, 7};
      print("lm", solver.minimize(x), x, true);
    }
    std::printf("}\n");
  } catch (const nlsolver::device_error &e) {
    std::fprintf(stderr, "device_error: %s\n", e.what());
    return 3;
  }
  return 0;
}
