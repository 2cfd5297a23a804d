// tests/cpp/header_lm_link.cpp — a device::LinkRegression<double> model (the logistic link, given as
// source text) through the drop-in header's LevenbergMarquardt: one solve of one problem, as one JSON
// object. The Python drop-in on nlsolver_amd.LinkRegression.logistic must give the same x and status.
//   header_lm_link FILE      FILE: "m n" and then A (m * n), y (m), theta0 (n) as hexadecimal floats
// Built by tests/test_lm_link_gpu.py itself (g++ -std=c++17).
#include <cstdio>
#include <cstdlib>

#include "nlsolver_mi/nlsolver.h"

namespace dev = nlsolver::device;

int main(int argc, char **argv) {
  if (argc != 2) {
    std::fprintf(stderr, "usage: header_lm_link FILE\n");
    return 2;
  }
  std::FILE *fh = std::fopen(argv[1], "r");
  if (!fh) {
    std::fprintf(stderr, "cannot open %s\n", argv[1]);
    return 2;
  }
  size_t m = 0, n = 0;
  if (std::fscanf(fh, "%zu %zu", &m, &n) != 2 || m == 0 || n == 0) return 2;
  auto read = [&](size_t count) {
    std::vector<double> v(count);
    char word[64];
    for (double &d : v) {
      if (std::fscanf(fh, "%63s", word) != 1) std::exit(2);
      d = std::strtod(word, nullptr);
    }
    return v;
  };
  std::vector<double> A = read(m * n), y = read(m), x = read(n);
  std::fclose(fh);
  try {
    dev::LinkRegression<double> model(m, n, A, y, "return 1.0 / (1.0 + det_exp(-z));", "return v * (1.0 - v);");
    auto solver = nlsolver::LevenbergMarquardt<dev::LinkRegression<double>, double>(model);
    auto [fcalls, iters, f, g, h] = solver.minimize(x).get_summary();
    std::printf("{\"fcalls\":%zu,\"iters\":%zu,\"gcalls\":%zu,\"hcalls\":%zu,\"f\":\"%a\",\"x\":[", fcalls, iters, g,
                h, f);
    for (size_t j = 0; j < n; j++) std::printf("%s\"%a\"", j ? "," : "", x[j]);
    std::printf("]}\n");
  } catch (const nlsolver::device_error &e) {
    std::fprintf(stderr, "device_error: %s\n", e.what());
    return 3;
  }
  return 0;
}
