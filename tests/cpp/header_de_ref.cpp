// tests/cpp/header_de_ref.cpp — DE on DEVICE objectives through the drop-in header with
// NLSG_DE_GENERATION=reference: the reference's C1 runs (tests/golden/de_c1.json) bit for bit,
// including the caller's generator afterwards. Built by tests/test_de_ref_cpu.py /
// tests/test_de_ref_gpu.py themselves (g++ -std=c++17).
//   header_de_ref c1               the three C1 runs and the README objective as a Custom chain
//   header_de_ref mode             prints the generation mode the environment selects
//   header_de_ref reject-rng       splitmix generator in reference mode: must throw
//   header_de_ref reject-rastrigin Rastrigin in reference mode: must throw
//   header_de_ref reject-vector    whole-vector Custom in reference mode: must throw
#include <cstdio>
#include <cstring>

#include "nlsolver_mi/nlsolver.h"

using nlsolver::DE;
using nlsolver::rng::xorshift;
using DEStrat = nlsolver::RecombinationStrategy;
namespace dev = nlsolver::device;

template <typename S, typename G>
static void report(const char *name, S &solver, G &gen, std::vector<double> x, bool last = false) {
  auto res = solver.minimize(x);
  auto [fcalls, iters, f, g, h] = res.get_summary();
  (void)g;
  (void)h;
  std::printf("\"%s\":{\"fcalls\":%zu,\"iters\":%zu,\"f\":\"%a\",\"x\":[\"%a\",\"%a\"],", name, fcalls, iters, f,
              x[0], x[1]);
  const double a = gen(), b = gen();
  std::printf("\"rng_after\":[\"%a\",\"%a\"]}%s\n", a, b, last ? "" : ",");
}

template <typename F>
static int expect_throw(F &&run) {
  try {
    run();
  } catch (const nlsolver::device_error &e) {
    std::printf("device_error: %s\n", e.what());
    return 0;
  }
  std::printf("no exception\n");
  return 1;
}

int main(int argc, char **argv) {
  const char *cmd = argc > 1 ? argv[1] : "c1";
  if (!std::strcmp(cmd, "mode")) {
    try {
      std::printf("%s\n", dev::de_generation_mode() == dev::de_generation::reference ? "reference" : "keyed");
    } catch (const nlsolver::device_error &e) {
      std::printf("device_error: %s\n", e.what());
      return 3;
    }
    return 0;
  }
  if (!std::strcmp(cmd, "reject-rng")) {
    return expect_throw([] {
      dev::Rosenbrock<double> prob;
      nlsolver::rng::splitmix<double> gen;
      auto s = DE<dev::Rosenbrock<double>, nlsolver::rng::splitmix<double>, double>(prob, gen, 0.9, 0.8, 10e-4, 40);
      std::vector<double> x = {5, 7};
      s.minimize(x);
    });
  }
  if (!std::strcmp(cmd, "reject-rastrigin")) {
    return expect_throw([] {
      dev::Rastrigin<double> prob;
      xorshift<double> gen;
      auto s = DE<dev::Rastrigin<double>, xorshift<double>, double>(prob, gen, 0.9, 0.8, 10e-4, 40);
      std::vector<double> x = {5, 7};
      s.minimize(x);
    });
  }
  if (!std::strcmp(cmd, "reject-vector")) {
    return expect_throw([] {
      auto prob = dev::Custom<double>::vector("return x(0) * x(0) + x(1) * x(1);");
      xorshift<double> gen;
      auto s = DE<dev::Custom<double>, xorshift<double>, double>(prob, gen, 0.9, 0.8, 10e-4, 40);
      std::vector<double> x = {5, 7};
      s.minimize(x);
    });
  }
  std::printf("{\n");
  {
    dev::Rosenbrock<double> prob;
    xorshift<double> gen;
    auto s = DE<dev::Rosenbrock<double>, xorshift<double>, double, DEStrat::random>(prob, gen, 0.9, 0.8, 10e-4, 40);
    report("c1_random_pop40_x0_5_7", s, gen, {5, 7});
  }
  {
    dev::Rosenbrock<double> prob;
    xorshift<double> gen;
    auto s = DE<dev::Rosenbrock<double>, xorshift<double>, double>(prob, gen);  // all defaults
    report("random_pop50_x0_5_7", s, gen, {5, 7});
  }
  {
    dev::Rosenbrock<double> prob;
    xorshift<double> gen;
    auto s = DE<dev::Rosenbrock<double>, xorshift<double>, double, DEStrat::best>(prob, gen);
    report("example_best_pop50_x0_2_7", s, gen, {2, 7});
  }
  {
    // README.md's objective (t1 = x[0]) spelled as the reference's functor spells it
    dev::Custom<double> prob("double t1 = xi; double t2 = (xn - xi * xi); return t1 * t1 + 100 * t2 * t2;", true);
    xorshift<double> gen;
    auto s = DE<dev::Custom<double>, xorshift<double>, double>(prob, gen, 0.9, 0.8, 10e-4, 40);
    report("readme_objective_pop40", s, gen, {5, 7}, true);
  }
  std::printf("}\n");
  return 0;
}
