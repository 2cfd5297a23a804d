// tests/cpp/header_pso_resident.cpp — PSO on a DEVICE objective through the drop-in header under
// NLSG_PSO_DRIVER: the class defaults (10 particles) on Rosenbrock from x0 = (5, 7), for both types
// and both overloads (minimize(x); minimize(x, lower, upper) with bounds -+3), as one JSON object;
// the resident driver and the turn driver must print the same one. An unknown driver name ends
// with the device_error's message and exit code 3. Built by tests/test_pso_batch_gpu.py itself
// (g++ -std=c++17).
#include <cstdio>

#include "nlsolver_mi/nlsolver.h"

namespace dev = nlsolver::device;

template <nlsolver::PSOType Type>
static void run(bool bounded, bool last) {
  dev::Rosenbrock<double> prob;
  nlsolver::rng::xorshift<double> gen;
  auto solver = nlsolver::PSO<dev::Rosenbrock<double>, nlsolver::rng::xorshift<double>, double, Type>(
      prob, gen, 0.8, 1.8, 1.8, 10, 300);
  std::vector<double> x = {5, 7};
  const std::vector<double> lower = {-3, -3}, upper = {3, 3};
  auto res = bounded ? solver.minimize(x, lower, upper) : solver.minimize(x);
  auto [fcalls, iters, f, g, h] = res.get_summary();
  (void)g;
  (void)h;
  std::printf("{\"type\":%d,\"bounded\":%d,\"fcalls\":%zu,\"iters\":%zu,\"f\":\"%a\",\"x\":[\"%a\",\"%a\"]}%s",
              static_cast<int>(Type), bounded ? 1 : 0, fcalls, iters, f, x[0], x[1], last ? "" : ",");
}

int main() {
  try {
    std::printf("{\"runs\":[");
    run<nlsolver::Vanilla>(false, false);
    run<nlsolver::Vanilla>(true, false);
    run<nlsolver::Accelerated>(false, false);
    run<nlsolver::Accelerated>(true, true);
    std::printf("]}\n");
  } catch (const nlsolver::device_error &e) {
    std::fprintf(stderr, "device_error: %s\n", e.what());
    return 3;
  }
  return 0;
}
