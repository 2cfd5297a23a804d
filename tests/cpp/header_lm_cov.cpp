// tests/cpp/header_lm_cov.cpp — LevenbergMarquardt::covariance and covariance_batch of the drop-in header
// on a device::CurveModel<double> (exponential decay), as one JSON object of hexadecimal floats. The Python
// drop-in's LevenbergMarquardt(CurveModel.exp_decay(...)).covariance must give the same bits.
//   header_lm_cov FILE      FILE: "m" and then t (m), y (m), theta (3) as hexadecimal floats
// Built by tests/test_lm_cov_gpu.py itself (g++ -std=c++17).
#include <cstdio>
#include <cstdlib>

#include "nlsolver_mi/nlsolver.h"

namespace dev = nlsolver::device;

static void print_matrix(const char *name, const std::vector<double> &c) {
  std::printf("\"%s\":[", name);
  for (size_t j = 0; j < c.size(); j++) std::printf("%s\"%a\"", j ? "," : "", c[j]);
  std::printf("]");
}

int main(int argc, char **argv) {
  if (argc != 2) {
    std::fprintf(stderr, "usage: header_lm_cov FILE\n");
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
    std::printf("{");
    print_matrix("residual", solver.covariance(x));
    std::printf(",");
    print_matrix("absolute", solver.covariance(x, dev::cov_scale::absolute));
    auto [covs, ok] = solver.covariance_batch({x}, dev::cov_scale::residual);
    std::printf(",");
    print_matrix("batch", covs[0]);
    std::printf(",\"ok\":%d}\n", ok[0] ? 1 : 0);
  } catch (const nlsolver::device_error &e) {
    std::fprintf(stderr, "device_error: %s\n", e.what());
    return 3;
  }
  return 0;
}
