// tests/cpp/header_batch_params.cpp — a device::Custom<double> objective that owns run-time data
// (Custom::params, read in the body as p(k)) through the drop-in header: one DE solve (40 agents)
// and one PSO solve (Vanilla, 10 particles, 300 iterations at most) from x0 = (5, 7), as one JSON
// object. Such an objective runs through the resident batch engine whatever the driver mode, and
// the Python drop-ins with params= must give the same x and status.
//   header_batch_params P0 P1 P2         the two solves with params = {P0, P1, P2}
//   header_batch_params sann P0 P1 P2    a solver whose engine takes no parameters: the library's
//                                        "unsupported" message, exit code 3
// Built by tests/test_batch_params_gpu.py itself (g++ -std=c++17).
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "nlsolver_mi/nlsolver.h"

namespace dev = nlsolver::device;
using xorshift = nlsolver::rng::xorshift<double>;

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
  const bool other = argc == 5 && !std::strcmp(argv[1], "sann");
  if (argc != 4 && !other) {
    std::fprintf(stderr, "usage: header_batch_params [sann] P0 P1 P2\n");
    return 2;
  }
  try {
    dev::Custom<double> prob(kTerms);
    for (int k = argc - 3; k < argc; k++) prob.params.push_back(std::strtod(argv[k], nullptr));
    if (other) {
      xorshift gen;
      auto solver = nlsolver::SANN<dev::Custom<double>, xorshift, double>(prob, gen);
      std::vector<double> x = {5, 7};
      solver.minimize(x);
      return 0;  // not reached: the engine rejects the parameters
    }
    std::printf("{");
    {
      xorshift gen;
      auto solver = nlsolver::DE<dev::Custom<double>, xorshift, double>(prob, gen, 0.9, 0.8, 10e-4, 40);
      std::vector<double> x = {5, 7};
      print("de", solver.minimize(x), x, false);
    }
    {
      xorshift gen;
      auto solver = nlsolver::PSO<dev::Custom<double>, xorshift, double, nlsolver::Vanilla>(prob, gen, 0.8, 1.8,
                                                                                           1.8, 10, 300);
      std::vector<double> x = {5, 7};
      print("pso", solver.minimize(x), x, true);
    }
    std::printf("}\n");
  } catch (const nlsolver::device_error &e) {
    std::fprintf(stderr, "device_error: %s\n", e.what());
    return 3;
  }
  return 0;
}
