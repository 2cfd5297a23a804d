// tests/cpp/header_lm_cov_missing.cpp — LevenbergMarquardt::covariance against a library that has no
// nlsg_lm_covariance (the stand-in tests/cpp/stub_nlsg.cpp, named by $NLSG_LIBRARY): after an ordinary
// minimize, covariance must throw the device_error that names the missing symbol, before it makes an
// engine. Prints the exception text; exit status 3. Built by tests/test_lm_cov_cpu.py itself.
#include <cstdio>

#include "nlsolver_mi/nlsolver.h"

namespace dev = nlsolver::device;

int main() {
  const size_t m = 3, n = 2;
  std::vector<double> A(m * n), y(m), x(n, 0.25);
  for (size_t i = 0; i < A.size(); i++) A[i] = 0.125 * static_cast<double>(i + 1);
  for (size_t i = 0; i < m; i++) y[i] = 0.25 * static_cast<double>(i) - 0.5;
  try {
    dev::TanhRegression<double> model(m, n, A, y);
    auto solver = nlsolver::LevenbergMarquardt<dev::TanhRegression<double>, double>(model);
    solver.minimize(x);
    std::printf("minimized\n");
    std::fflush(stdout);
    const std::vector<double> cov = solver.covariance(x);
    std::printf("covariance returned %zu numbers\n", cov.size());
  } catch (const nlsolver::device_error &e) {
    std::printf("device_error: %s\n", e.what());
    return 3;
  }
  return 0;
}
