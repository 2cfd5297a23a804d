// tests/cpp/header_de_resident.cpp — DE on a DEVICE objective through the drop-in header under
// NLSG_DE_DRIVER: config C1 (DE(f, gen, 0.9, 0.8, 10e-4, 40) from x0 = (5, 7)) as one JSON object;
// the resident driver and the turn driver must print the same one. An unknown driver name ends
// with the device_error's message and exit code 3. Built by tests/test_de_batch_gpu.py itself
// (g++ -std=c++17).
#include <cstdio>

#include "nlsolver_mi/nlsolver.h"

namespace dev = nlsolver::device;

int main() {
  try {
    dev::Rosenbrock<double> prob;
    nlsolver::rng::xorshift<double> gen;
    auto solver = nlsolver::DE<dev::Rosenbrock<double>, nlsolver::rng::xorshift<double>, double>(
        prob, gen, 0.9, 0.8, 10e-4, 40);
    std::vector<double> x = {5, 7};
    auto res = solver.minimize(x);
    auto [fcalls, iters, f, g, h] = res.get_summary();
    (void)g;
    (void)h;
    std::printf("{\"fcalls\":%zu,\"iters\":%zu,\"f\":\"%a\",\"x\":[\"%a\",\"%a\"]}\n", fcalls, iters, f, x[0], x[1]);
  } catch (const nlsolver::device_error &e) {
    std::fprintf(stderr, "device_error: %s\n", e.what());
    return 3;
  }
  return 0;
}
