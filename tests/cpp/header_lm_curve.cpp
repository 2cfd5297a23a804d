// tests/cpp/header_lm_curve.cpp — a device::CurveModel<double> (exponential decay, residual and Jacobian
// row given as source text) through the drop-in header's LevenbergMarquardt: one solve of one problem, as
// one JSON object. The Python drop-in on nlsolver_amd.CurveModel.exp_decay must give the same x and status.
//   header_lm_curve FILE      FILE: "m" and then t (m), y (m), theta0 (3) as hexadecimal floats
// Built by tests/test_lm_curve_gpu.py itself (g++ -std=c++17).
#include <cstdio>
#include <cstdlib>

#include "nlsolver_mi/nlsolver.h"

namespace dev = nlsolver::device;

int main(int argc, char **argv) {
  if (argc != 2) {
    std::fprintf(stderr, "usage: header_lm_curve FILE\n");
    return 2;
  }
  std::FILE *fh = std::fopen(argv[1], "r");
  if (!fh) {
    std::fprintf(stderr, "cannot open %s\n", argv[1]);
    return 2;
  }
  size_t m = 0;
  const size_t n = 3;
  if (std::fscanf(fh, "%zu", &m) != 1 || m == 0) return 2;
  auto read = [&](size_t count) {
    std::vector<double> v(count);
    char word[64];
    for (double &d : v) {
      if (std::fscanf(fh, "%63s", word) != 1) std::exit(2);
      d = std::strtod(word, nullptr);
    }
    return v;
  };
  std::vector<double> t = read(m), y = read(m), x = read(n);
  std::fclose(fh);
  try {
    dev::CurveModel<double> model(m, n, 1, t, y,
                                  "const double e = det_exp(-th(1) * t(0));\n"
                                  "r = y - (th(0) * e + th(2));\n"
                                  "J(0) = -e;  J(1) = th(0) * t(0) * e;  J(2) = -1.0;");
    auto solver = nlsolver::LevenbergMarquardt<dev::CurveModel<double>, double>(model);
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
