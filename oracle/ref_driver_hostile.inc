// oracle/ref_driver_hostile.inc — TEST INFRASTRUCTURE, NOT PRODUCT CODE; included by ref_driver.cpp.
//
// The unmodified reference's NelderMead on the hostile objective families of tests/_hostile.py
// (plateaus, NaN regions, +-inf walls, constant 0, all NaN, huge steps): the functor below is the
// driver's own code, the same statements as _hostile.TERM_SRC, summed left to right. Its values do
// not depend on the order of the sum (small integers or non-finite terms).
//   nm-hostile D family a b step max_iter eps no_change restarts x0 x0_step bounded upper lower minimize
// x_i = x0 + x0_step i. Even D only: for an odd D the reference's simplex constructor writes one
// element past a vector (SURVEY B1) and the run is not defined.
// tests/golden/gen_golden_hostile.py records the output in tests/golden/nm_hostile.json.

struct HostileFamily {
  double fam, a, b;
  double term(double xi) const {
    double q = std::floor(4.0 * xi);
    q = q < -64.0 ? -64.0 : (q > 64.0 ? 64.0 : q);
    const double pl = q * q;
    if (fam == 0.0) return pl;
    if (fam == 1.0) return 0.0;
    if (fam == 2.0) return xi > a ? __builtin_nan("") : pl;
    if (fam == 3.0) return __builtin_nan("");
    if (fam == 4.0) return xi < a ? __builtin_inf() : (xi > b ? -__builtin_inf() : pl);
    return pl * 0x1p1000;
  }
  double operator()(std::vector<double> &x) {
    double acc = 0.0;
    for (size_t i = 0; i < x.size(); i++) acc += term(x[i]);
    return acc;
  }
};

static int run_nm_hostile(int argc, char **argv) {
  if (argc < 17) {
    std::fprintf(stderr, "nm-hostile D family a b step max_iter eps no_change restarts x0 x0_step "
                         "bounded upper lower minimize\n");
    return 2;
  }
  const size_t D = std::strtoull(argv[2], nullptr, 10);
  if (D % 2) {
    std::fprintf(stderr, "nm-hostile: even D only (SURVEY B1)\n");
    return 2;
  }
  HostileFamily f{std::strtod(argv[3], nullptr), std::strtod(argv[4], nullptr), std::strtod(argv[5], nullptr)};
  const double step = std::strtod(argv[6], nullptr);
  const size_t max_iter = std::strtoull(argv[7], nullptr, 10);
  const double eps = std::strtod(argv[8], nullptr);
  const size_t no_change = std::strtoull(argv[9], nullptr, 10);
  const size_t restarts = std::strtoull(argv[10], nullptr, 10);
  const double x0 = std::strtod(argv[11], nullptr), x0_step = std::strtod(argv[12], nullptr);
  const bool bounded = std::atoi(argv[13]) != 0;
  const double up = std::strtod(argv[14], nullptr), lo = std::strtod(argv[15], nullptr);
  const bool minimize = std::atoi(argv[16]) != 0;
  auto solver = nlsolver::NelderMead<HostileFamily, double>(f, step, 1, 2, 0.5, 0.5, eps, max_iter,
                                                            no_change, restarts);
  std::vector<double> x(D), upper(D, up), lower(D, lo);
  for (size_t i = 0; i < D; i++) x[i] = x0 + x0_step * static_cast<double>(i);
  auto res = bounded ? (minimize ? solver.minimize(x, upper, lower) : solver.maximize(x, upper, lower))
                     : (minimize ? solver.minimize(x) : solver.maximize(x));
  auto [fcalls, iters, fval, g, h] = res.get_summary();
  (void)g;
  (void)h;
  std::printf("{\"fcalls\":%zu,\"iters\":%zu,\"f\":", fcalls, iters);
  put_hex(fval);
  std::printf(",\"x\":");
  put_vec(x);
  std::printf("}\n");
  return 0;
}
