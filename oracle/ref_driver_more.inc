// oracle/ref_driver_more.inc — TEST INFRASTRUCTURE (part of ref_driver.cpp).
// Additional sub-commands (PSO / NelderMead / BFGS / LM / tinyqr goldens).

using nlsolver::PSO;
using nlsolver::PSOType;

// pso <accelerated|vanilla> <D> <particles> <max_iter> <eps> <no_change> <x0> <trace>
//     [bounded lower upper] [inertia cognitive social]
template <PSOType T>
static int run_pso(size_t D, size_t np, size_t max_iter, double eps, size_t no_change,
                   std::vector<double> x, int trace, bool bounded, double lo, double hi,
                   double inertia, double cog, double soc) {
  RecordingRosenbrock f;
  xorshift<double> gen;
  auto solver = PSO<RecordingRosenbrock, xorshift<double>, double, T>(
      f, gen, inertia, cog, soc, np, max_iter, no_change, eps);
  std::vector<double> lower(D, lo), upper(D, hi);
  auto res = bounded ? solver.minimize(x, lower, upper) : solver.minimize(x);
  auto [fcalls, iters, fval, g, h] = res.get_summary();
  (void)g;
  (void)h;
  std::printf("{\"type\":\"%s\",\"D\":%zu,\"particles\":%zu,\"max_iter\":%zu,\"eps\":",
              T == PSOType::Accelerated ? "accelerated" : "vanilla", D, np, max_iter);
  put_hex(eps);
  std::printf(",\"no_change\":%zu,\"bounded\":%d,\"lower\":", no_change, bounded ? 1 : 0);
  put_hex(lo);
  std::printf(",\"upper\":");
  put_hex(hi);
  std::printf(",\"inertia\":");
  put_hex(inertia);
  std::printf(",\"cognitive\":");
  put_hex(cog);
  std::printf(",\"social\":");
  put_hex(soc);
  std::printf(",\"fcalls\":%zu,\"iters\":%zu,\"f\":", fcalls, iters);
  put_hex(fval);
  std::printf(",\"x\":");
  put_vec(x);
  std::printf(",\"rng_after\":[");
  put_hex(gen());
  std::printf(",");
  put_hex(gen());
  std::printf("]");
  if (trace >= 1) {
    std::printf(",\"eval_f\":");
    put_vec(f.fs);
    Fnv hh;
    for (auto &v : f.xs)
      for (double d : v) hh.add(d);
    std::printf(",\"eval_x_fnv\":\"%" PRIu64 "\"", hh.h);
  }
  if (trace >= 2) {
    std::printf(",\"eval_x\":[");
    for (size_t i = 0; i < f.xs.size(); i++) {
      if (i) std::printf(",");
      put_vec(f.xs[i]);
    }
    std::printf("]");
  }
  std::printf("}\n");
  return 0;
}

// bench-pso: time the reference Accelerated PSO on Rosenbrock-ND (unbounded overload).
static int bench_pso(size_t D, size_t np, size_t iters) {
  RosenbrockND f;
  xorshift<double> gen;
  auto solver = PSO<RosenbrockND, xorshift<double>, double, PSOType::Accelerated>(
      f, gen, 0.8, 1.8, 1.8, np, iters, iters + 1, 0.0);
  std::vector<double> x(D, 2.048);
  auto t0 = std::chrono::steady_clock::now();
  auto res = solver.minimize(x);
  auto t1 = std::chrono::steady_clock::now();
  const double s = std::chrono::duration<double>(t1 - t0).count();
  auto [fcalls, it, fval, g, h] = res.get_summary();
  (void)g;
  (void)h;
  std::printf("{\"D\":%zu,\"particles\":%zu,\"iterations\":%zu,\"fcalls\":%zu,"
              "\"seconds\":%.6f,\"particle_evals_per_s\":%.6e,\"f\":%.17g}\n",
              D, np, it, fcalls, s, static_cast<double>(fcalls) / s, fval);
  return 0;
}

// ---------------------------------------------------------------------------
// BFGS (nlsolver.h:3169-3286) on the convex quadratic of SURVEY.md §8c G6:
//   f(x) = 1/2 sum d_i x_i^2 + 1/2 c (sum x)^2 - sum b_i x_i,
//   d_i = 1 + 9 i/(n-1), b_i = sin(0.1 i), c = 0.01, analytic gradient functor.
// Every f / gradient call is recorded (point hash + value) so the golden pins the
// whole trajectory including the More-Thuente trial points.
// ---------------------------------------------------------------------------
struct QuadDR1 {
  std::vector<double> d, b;
  double c = 0.01;
  std::vector<double> f_vals;
  Fnv f_pts, g_pts;
  size_t g_calls = 0;
  explicit QuadDR1(size_t n) : d(n), b(n) {
    for (size_t i = 0; i < n; i++) {
      d[i] = n > 1 ? 1.0 + 9.0 * static_cast<double>(i) / static_cast<double>(n - 1) : 1.0;
      b[i] = std::sin(0.1 * static_cast<double>(i));
    }
  }
  double operator()(std::vector<double> &x) {
    double q = 0.0, sx = 0.0, lin = 0.0;
    for (size_t i = 0; i < x.size(); i++) {
      q += d[i] * x[i] * x[i];
      sx += x[i];
      lin += b[i] * x[i];
    }
    const double v = 0.5 * q + 0.5 * c * (sx * sx) - lin;
    f_vals.push_back(v);
    for (double t : x) f_pts.add(t);
    return v;
  }
};
struct QuadGrad {
  void operator()(QuadDR1 &f, std::vector<double> &x, std::vector<double> &g) {
    double sx = 0.0;
    for (size_t i = 0; i < x.size(); i++) sx += x[i];
    for (size_t i = 0; i < x.size(); i++) g[i] = f.d[i] * x[i] + f.c * sx - f.b[i];
    f.g_calls++;
    for (double t : x) f.g_pts.add(t);
  }
};

static int run_bfgs(size_t n, size_t max_iter, double grad_eps, double alpha, double x0,
                    double x0_step, int trace) {
  QuadDR1 f(n);
  QuadGrad g;
  auto solver = nlsolver::BFGS<QuadDR1, double, QuadGrad>(f, g, max_iter, grad_eps, alpha);
  std::vector<double> x(n);
  for (size_t i = 0; i < n; i++) x[i] = x0 + x0_step * static_cast<double>(i);
  auto res = solver.minimize(x);
  auto [fcalls, iters, fval, gcalls, h] = res.get_summary();
  (void)h;
  std::printf("{\"n\":%zu,\"max_iter\":%zu,\"grad_eps\":", n, max_iter);
  put_hex(grad_eps);
  std::printf(",\"alpha\":");
  put_hex(alpha);
  std::printf(",\"x0\":");
  put_hex(x0);
  std::printf(",\"x0_step\":");
  put_hex(x0_step);
  std::printf(",\"fcalls\":%zu,\"iters\":%zu,\"gcalls\":%zu,\"f\":", fcalls, iters, gcalls);
  put_hex(fval);
  Fnv hx;
  for (double t : x) hx.add(t);
  std::printf(",\"x_fnv\":\"%" PRIu64 "\",\"x_head\":", hx.h);
  put_vec(std::vector<double>(x.begin(), x.begin() + std::min<size_t>(n, 8)));
  std::printf(",\"f_pts_fnv\":\"%" PRIu64 "\",\"g_pts_fnv\":\"%" PRIu64 "\"", f.f_pts.h,
              f.g_pts.h);
  if (trace) {
    std::printf(",\"f_vals\":");
    put_vec(f.f_vals);
  }
  std::printf("}\n");
  return 0;
}

// BFGS on the line-search family (oracle/oracle_bfgs.c fam_f / fam_g say the same operation for operation):
// per coordinate, (a, b, c, d, e) = p[0..4],
//   q = x x, w = 1 + q;  f = ((a q + b x + c) x + d) x + e (q / w)
//                        g = ((4 a x + 3 b) x + 2 c) x + d + e ((2 x) / (w w))
// n = 1: f = 0.0 + f_0; n = 2: f = 0.0 + (f_0 + f_1), coordinate 1 under p[5..9]. At n = 1 the first turn of
// BFGS::solve (H = I, d = -g) is exactly one More-Thuente search on phi(t) = f(x0 - t g(x0)) from stp = alpha,
// so the members of this family pin the branches of cstep / cvsrch (tests/golden/bfgs_mt.json).
struct MtFamily {
  std::vector<double> p;  // 5 n
  std::vector<double> f_vals;
  size_t g_calls = 0;
  static double f1(double x, const double *p) {
    const double q = x * x, w = 1 + q;
    return ((p[0] * q + p[1] * x + p[2]) * x + p[3]) * x + p[4] * (q / w);
  }
  static double g1(double x, const double *p) {
    const double q = x * x, w = 1 + q;
    return ((4 * p[0] * x + 3 * p[1]) * x + 2 * p[2]) * x + p[3] + p[4] * ((2 * x) / (w * w));
  }
  double operator()(std::vector<double> &x) {
    const double v = x.size() == 1 ? 0.0 + f1(x[0], p.data())
                                   : 0.0 + (f1(x[0], p.data()) + f1(x[1], p.data() + 5));
    f_vals.push_back(v);
    return v;
  }
};
struct MtFamilyGrad {
  void operator()(MtFamily &f, std::vector<double> &x, std::vector<double> &g) {
    for (size_t i = 0; i < x.size(); i++) g[i] = MtFamily::g1(x[i], f.p.data() + 5 * i);
    f.g_calls++;
  }
};
static std::vector<double> parse_list(const char *s) {
  std::vector<double> out;
  std::stringstream ss(s);
  std::string tok;
  while (std::getline(ss, tok, ',')) out.push_back(std::strtod(tok.c_str(), nullptr));
  return out;
}

static int run_bfgs_mt(size_t n, const char *params, const char *x0, double alpha, size_t max_iter,
                       double grad_eps) {
  MtFamily f;
  f.p = parse_list(params);
  std::vector<double> x = parse_list(x0);
  if ((n != 1 && n != 2) || f.p.size() != 5 * n || x.size() != n) {
    std::fprintf(stderr, "bfgs-mt: n is 1 or 2, with 5 n parameters and n coordinates\n");
    return 2;
  }
  const std::vector<double> start = x;
  MtFamilyGrad g;
  auto solver = nlsolver::BFGS<MtFamily, double, MtFamilyGrad>(f, g, max_iter, grad_eps, alpha);
  auto res = solver.minimize(x);
  auto [fcalls, iters, fval, gcalls, h] = res.get_summary();
  (void)h;
  std::printf("{\"n\":%zu,\"params\":", n);
  put_vec(f.p);
  std::printf(",\"x0\":");
  put_vec(start);
  std::printf(",\"alpha\":");
  put_hex(alpha);
  std::printf(",\"max_iter\":%zu,\"grad_eps\":", max_iter);
  put_hex(grad_eps);
  std::printf(",\"fcalls\":%zu,\"iters\":%zu,\"gcalls\":%zu,\"g_calls_seen\":%zu,\"f\":", fcalls, iters,
              gcalls, f.g_calls);
  put_hex(fval);
  std::printf(",\"x\":");
  put_vec(x);
  std::printf(",\"f_vals\":");
  put_vec(f.f_vals);
  std::printf("}\n");
  return 0;
}

// BFGS with the reference's DEFAULT gradient (fin_diff -> finite_difference_gradient<.,.,1>,
// nlsolver.h:1385-1413, 2849-2855) on a built-in N-D objective; every objective value (the
// finite-difference probes included: they go through the counting wrapper, 3218-3224) is
// recorded.
struct CountedObjective {
  int kind;  // 0 Rosenbrock chain, 1 sphere, 2 Styblinski-Tang
  std::vector<double> f_vals;
  Fnv f_pts;
  double operator()(std::vector<double> &x) {
    double acc = 0.0;
    const size_t n = x.size();
    if (kind == 0) {
      for (size_t i = 0; i + 1 < n; i++) {
        const double t1 = 1 - x[i];
        const double t2 = (x[i + 1] - x[i] * x[i]);
        acc += t1 * t1 + 100 * t2 * t2;
      }
    } else if (kind == 1) {
      for (size_t i = 0; i < n; i++) acc += x[i] * x[i];
    } else {
      for (size_t i = 0; i < n; i++) {
        const double x2 = x[i] * x[i];
        acc += x2 * x2 - 16 * x2 + 5 * x[i];
      }
      acc = acc / 2.0;
    }
    f_vals.push_back(acc);
    for (double t : x) f_pts.add(t);
    return acc;
  }
};

static int run_bfgs_fd(int kind, size_t n, size_t max_iter, double grad_eps, double alpha, double x0,
                       double x0_step, size_t trace_cap) {
  CountedObjective f{kind, {}, {}};
  auto solver = nlsolver::BFGS<CountedObjective, double>(
      f, nlsolver::fin_diff<CountedObjective, double>(), max_iter, grad_eps, alpha);
  std::vector<double> x(n);
  for (size_t i = 0; i < n; i++) x[i] = x0 + x0_step * static_cast<double>(i);
  auto res = solver.minimize(x);
  auto [fcalls, iters, fval, gcalls, h] = res.get_summary();
  (void)h;
  std::printf("{\"objective\":%d,\"n\":%zu,\"max_iter\":%zu,\"grad_eps\":", kind, n, max_iter);
  put_hex(grad_eps);
  std::printf(",\"alpha\":");
  put_hex(alpha);
  std::printf(",\"x0\":");
  put_hex(x0);
  std::printf(",\"x0_step\":");
  put_hex(x0_step);
  std::printf(",\"fcalls\":%zu,\"iters\":%zu,\"gcalls\":%zu,\"f\":", fcalls, iters, gcalls);
  put_hex(fval);
  std::printf(",\"x\":");
  put_vec(x);
  Fnv hv;
  for (double t : f.f_vals) hv.add(t);
  std::printf(",\"f_count\":%zu,\"f_vals_fnv\":\"%" PRIu64 "\",\"f_pts_fnv\":\"%" PRIu64 "\"",
              f.f_vals.size(), hv.h, f.f_pts.h);
  std::printf(",\"f_vals_head\":");
  put_vec(std::vector<double>(f.f_vals.begin(),
                              f.f_vals.begin() + std::min(trace_cap, f.f_vals.size())));
  std::printf("}\n");
  return 0;
}

// LevenbergMarquardt with the reference's DEFAULT functors (fin_diff, fin_diff_h) on a built-in
// N-D objective; every objective value (all finite-difference probes included) is counted.
static int run_lm_fd(int kind, size_t n, size_t max_iter, double lambda, double f_delta, double x0,
                     double x0_step, size_t trace_cap) {
  CountedObjective f{kind, {}, {}};
  auto solver = nlsolver::LevenbergMarquardt<CountedObjective, double>(f, lambda, 10, 10, max_iter,
                                                                      f_delta);
  std::vector<double> x(n);
  for (size_t i = 0; i < n; i++) x[i] = x0 + x0_step * static_cast<double>(i);
  auto res = solver.minimize(x);
  auto [fcalls, iters, fval, gcalls, hcalls] = res.get_summary();
  std::printf("{\"objective\":%d,\"n\":%zu,\"max_iter\":%zu,\"lambda\":", kind, n, max_iter);
  put_hex(lambda);
  std::printf(",\"f_delta\":");
  put_hex(f_delta);
  std::printf(",\"x0\":");
  put_hex(x0);
  std::printf(",\"x0_step\":");
  put_hex(x0_step);
  std::printf(",\"fcalls\":%zu,\"iters\":%zu,\"gcalls\":%zu,\"hcalls\":%zu,\"f\":", fcalls, iters,
              gcalls, hcalls);
  put_hex(fval);
  std::printf(",\"x\":");
  put_vec(x);
  Fnv hv;
  for (double t : f.f_vals) hv.add(t);
  std::printf(",\"f_count\":%zu,\"f_vals_fnv\":\"%" PRIu64 "\",\"f_pts_fnv\":\"%" PRIu64 "\"",
              f.f_vals.size(), hv.h, f.f_pts.h);
  std::printf(",\"f_vals_head\":");
  put_vec(std::vector<double>(f.f_vals.begin(),
                              f.f_vals.begin() + std::min(trace_cap, f.f_vals.size())));
  std::printf("}\n");
  return 0;
}

// SANN (nlsolver.h:2744-2815) on a built-in N-D objective with the reference's xorshift
// generator; every objective value is recorded; the generator's next draw after the run pins
// the number of draws consumed.
static int run_sann(int kind, size_t n, size_t max_iter, size_t temp_iter, double temp_max, double x0,
                    double x0_step, int minimize, size_t trace_cap) {
  CountedObjective f{kind, {}, {}};
  nlsolver::rng::xorshift<double> gen;
  auto solver = nlsolver::SANN<CountedObjective, nlsolver::rng::xorshift<double>, double>(
      f, gen, max_iter, temp_iter, temp_max);
  std::vector<double> x(n);
  for (size_t i = 0; i < n; i++) x[i] = x0 + x0_step * static_cast<double>(i);
  auto res = minimize ? solver.minimize(x) : solver.maximize(x);
  auto [fcalls, iters, fval, gcalls, hcalls] = res.get_summary();
  (void)gcalls; (void)hcalls;
  std::printf("{\"objective\":%d,\"n\":%zu,\"max_iter\":%zu,\"temp_iter\":%zu,\"temp_max\":", kind, n,
              max_iter, temp_iter);
  put_hex(temp_max);
  std::printf(",\"x0\":");
  put_hex(x0);
  std::printf(",\"x0_step\":");
  put_hex(x0_step);
  std::printf(",\"minimize\":%d,\"fcalls\":%zu,\"iters\":%zu,\"f\":", minimize, fcalls, iters);
  put_hex(fval);
  std::printf(",\"x\":");
  put_vec(x);
  std::printf(",\"next_draw\":");
  put_hex(gen());
  Fnv hv;
  for (double t : f.f_vals) hv.add(t);
  std::printf(",\"f_count\":%zu,\"f_vals_fnv\":\"%" PRIu64 "\",\"f_pts_fnv\":\"%" PRIu64 "\"",
              f.f_vals.size(), hv.h, f.f_pts.h);
  std::printf(",\"f_vals_head\":");
  put_vec(std::vector<double>(f.f_vals.begin(),
                              f.f_vals.begin() + std::min(trace_cap, f.f_vals.size())));
  std::printf("}\n");
  return 0;
}

// NelderMeadPSO (nlsolver.h:3546-3920), unbounded overloads (bounds = -+|2.5 x|), with the
// reference's xorshift generator; every objective value is recorded.
static int run_nmpso(int kind, size_t n, size_t max_iter, double eps, size_t no_change, double x0,
                     double x0_step, int minimize, size_t trace_cap) {
  CountedObjective f{kind, {}, {}};
  nlsolver::rng::xorshift<double> gen;
  auto solver = nlsolver::NelderMeadPSO<CountedObjective, nlsolver::rng::xorshift<double>, double>(
      f, gen, 1, 2, 0.5, 0.5, 0.8, 1.8, 1.8, eps, max_iter, no_change);
  std::vector<double> x(n);
  for (size_t i = 0; i < n; i++) x[i] = x0 + x0_step * static_cast<double>(i);
  auto res = minimize ? solver.minimize(x) : solver.maximize(x);
  auto [fcalls, iters, fval, gcalls, hcalls] = res.get_summary();
  (void)gcalls; (void)hcalls;
  std::printf("{\"objective\":%d,\"n\":%zu,\"max_iter\":%zu,\"eps\":", kind, n, max_iter);
  put_hex(eps);
  std::printf(",\"no_change\":%zu,\"x0\":", no_change);
  put_hex(x0);
  std::printf(",\"x0_step\":");
  put_hex(x0_step);
  std::printf(",\"minimize\":%d,\"fcalls\":%zu,\"iters\":%zu,\"f\":", minimize, fcalls, iters);
  put_hex(fval);
  std::printf(",\"x\":");
  put_vec(x);
  std::printf(",\"next_draw\":");
  put_hex(gen());
  Fnv hv;
  for (double t : f.f_vals) hv.add(t);
  std::printf(",\"f_count\":%zu,\"f_vals_fnv\":\"%" PRIu64 "\",\"f_pts_fnv\":\"%" PRIu64 "\"",
              f.f_vals.size(), hv.h, f.f_pts.h);
  std::printf(",\"f_vals_head\":");
  put_vec(std::vector<double>(f.f_vals.begin(),
                              f.f_vals.begin() + std::min(trace_cap, f.f_vals.size())));
  std::printf("}\n");
  return 0;
}

// CPU baseline of bench.py --workload nmpso: `reps` instances of the reference's NelderMeadPSO
// on Rosenbrock-nD (n even), max_iter iterations each (eps = 0, no early stop).
static int bench_nmpso(size_t n, size_t reps, size_t max_iter) {
  RosenbrockND f;
  double evals = 0, fsum = 0;
  auto t0 = std::chrono::steady_clock::now();
  for (size_t r = 0; r < reps; r++) {
    nlsolver::rng::xorshift<double> gen;
    auto solver = nlsolver::NelderMeadPSO<RosenbrockND, nlsolver::rng::xorshift<double>, double>(
        f, gen, 1, 2, 0.5, 0.5, 0.8, 1.8, 1.8, 0.0, max_iter, static_cast<size_t>(-1));
    std::vector<double> x(n);
    for (size_t i = 0; i < n; i++) x[i] = 0.5 + 0.001 * static_cast<double>(i + r);
    auto res = solver.minimize(x);
    auto [fcalls, it, fval, g, h] = res.get_summary();
    (void)it; (void)g; (void)h;
    evals += static_cast<double>(fcalls);
    fsum += fval;
  }
  const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  std::printf("{\"n\":%zu,\"reps\":%zu,\"evals\":%.0f,\"seconds\":%.6f,"
              "\"evals_per_s\":%.6e,\"fsum\":%.17g}\n", n, reps, evals, sec, evals / sec, fsum);
  return 0;
}

// CPU baseline of bench.py --workload sann: `reps` chains of the reference's SANN on
// Rosenbrock-nD, max_iter temperatures x (temp_iter - 1) trial points each.
static int bench_sann(size_t n, size_t reps, size_t max_iter, size_t temp_iter) {
  RosenbrockND f;
  double trials = 0, fsum = 0;
  auto t0 = std::chrono::steady_clock::now();
  for (size_t r = 0; r < reps; r++) {
    nlsolver::rng::xorshift<double> gen;
    auto solver = nlsolver::SANN<RosenbrockND, nlsolver::rng::xorshift<double>, double>(
        f, gen, max_iter, temp_iter, 10.0);
    std::vector<double> x(n);
    for (size_t i = 0; i < n; i++) x[i] = 0.5 + 0.001 * static_cast<double>(i + r);
    auto res = solver.minimize(x);
    auto [fcalls, it, fval, g, h] = res.get_summary();
    (void)it; (void)g; (void)h;
    trials += static_cast<double>(fcalls);
    fsum += fval;
  }
  const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  std::printf("{\"n\":%zu,\"reps\":%zu,\"trials\":%.0f,\"seconds\":%.6f,"
              "\"trials_per_s\":%.6e,\"fsum\":%.17g}\n", n, reps, trials, sec, trials / sec, fsum);
  return 0;
}

// CPU baseline of bench.py --workload lm-fd: `reps` starts of the default-functor
// LevenbergMarquardt on Rosenbrock-nD, `iters` iterations each (f_delta = 0).
static uint64_t drv_key(uint64_t parent, uint64_t index);
static double drv_u(uint64_t key, uint64_t slot);
static int bench_lm_fd(size_t n, size_t reps, size_t iters) {
  RosenbrockND f;
  double total_iters = 0, fsum = 0;
  auto t0 = std::chrono::steady_clock::now();
  for (size_t r = 0; r < reps; r++) {
    auto solver = nlsolver::LevenbergMarquardt<RosenbrockND, double>(f, 10, 10, 10, iters, 0.0);
    std::vector<double> x(n);
    for (size_t i = 0; i < n; i++)
      x[i] = 0.8 + 0.4 * (drv_u(drv_key(12374563468ull, r), i) - 0.5);
    auto res = solver.minimize(x);
    auto [fcalls, it, fval, g, h] = res.get_summary();
    (void)fcalls; (void)g; (void)h;
    total_iters += static_cast<double>(it);
    fsum += fval;
  }
  const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  std::printf("{\"n\":%zu,\"reps\":%zu,\"iterations\":%.0f,\"seconds\":%.6f,"
              "\"iterations_per_s\":%.6e,\"fsum\":%.17g}\n", n, reps, total_iters, sec,
              total_iters / sec, fsum);
  return 0;
}

// update_inverse_hessian (nlsolver.h:3130-3168) on a small explicit system (B5 probe).
static int run_hess_update() {
  const size_t n = 3;
  std::vector<double> H = {2.0, 0.3, -0.1, 0.3, 1.5, 0.2, -0.1, 0.2, 1.1};
  std::vector<double> s = {0.3, -0.2, 0.5}, y = {0.7, 0.1, -0.4}, t(n);
  const double rho = 1.0 / nlsolver::math::dot(y.data(), s.data(), 3);
  nlsolver::update_inverse_hessian(H, s, y, t, rho);
  std::printf("{\"rho\":");
  put_hex(rho);
  std::printf(",\"H\":");
  put_vec(H);
  std::printf(",\"t\":");
  put_vec(t);
  std::printf("}\n");
  return 0;
}

static int bench_bfgs(size_t n, size_t reps) {
  double total_iters = 0;
  auto t0 = std::chrono::steady_clock::now();
  double fsum = 0;
  for (size_t r = 0; r < reps; r++) {
    QuadDR1 f(n);
    f.f_vals.reserve(4096);
    QuadGrad g;
    auto solver = nlsolver::BFGS<QuadDR1, double, QuadGrad>(f, g, 50, 0.0, 1.0);
    std::vector<double> x(n);
    for (size_t i = 0; i < n; i++) x[i] = 1.0 + 0.25 * std::sin(static_cast<double>(i + 31 * r));
    auto res = solver.minimize(x);
    auto [fcalls, iters, fval, gcalls, h] = res.get_summary();
    (void)fcalls; (void)gcalls; (void)h;
    total_iters += static_cast<double>(iters);
    fsum += fval;
  }
  auto t1 = std::chrono::steady_clock::now();
  const double sec = std::chrono::duration<double>(t1 - t0).count();
  std::printf("{\"n\":%zu,\"problems\":%zu,\"iterations\":%.0f,\"seconds\":%.6f,"
              "\"iterations_per_s\":%.6e,\"fsum\":%.17g}\n", n, reps, total_iters, sec,
              total_iters / sec, fsum);
  return 0;
}

static uint64_t drv_key(uint64_t parent, uint64_t index);
static double drv_u(uint64_t key, uint64_t slot);
// CPU baseline of the default-gradient BFGS path: Rosenbrock-nD, `reps` starts x `iters` iterations
static int bench_bfgs_fd(size_t n, size_t reps, size_t iters) {
  RosenbrockND f;
  double total_iters = 0, fsum = 0;
  auto t0 = std::chrono::steady_clock::now();
  for (size_t r = 0; r < reps; r++) {
    auto solver = nlsolver::BFGS<RosenbrockND, double>(f, nlsolver::fin_diff<RosenbrockND, double>(),
                                                       iters, 0.0, 1.0);
    std::vector<double> x(n);
    for (size_t i = 0; i < n; i++)
      x[i] = 0.8 + 0.4 * (drv_u(drv_key(12374563468ull, r), i) - 0.5);
    auto res = solver.minimize(x);
    auto [fcalls, it, fval, g, h] = res.get_summary();
    (void)fcalls; (void)g; (void)h;
    total_iters += static_cast<double>(it);
    fsum += fval;
  }
  const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  std::printf("{\"n\":%zu,\"reps\":%zu,\"iterations\":%.0f,\"seconds\":%.6f,"
              "\"iterations_per_s\":%.6e,\"fsum\":%.17g}\n", n, reps, total_iters, sec,
              total_iters / sec, fsum);
  return 0;
}

// ---------------------------------------------------------------------------
// Levenberg-Marquardt (nlsolver.h:3428-3545) driven as an NLLS solver with
// Gauss-Newton functors: f = sum r^2, Grad = 2 J^T r, Hess = 2 J^T J (SURVEY §0.3).
// Two residual models (all arithmetic below is the driver's own code):
//   exp  : r_i = y_i - p0 * exp(p1 * t_i)                         (SURVEY §8c G8)
//   tanh : r_i = y_i - tanh(sum_j A_ij theta_j), synthetic data keyed by (seed, problem)
//          from splitmix64 (SURVEY §8d C4)
// ---------------------------------------------------------------------------
static uint64_t drv_mix64(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
static uint64_t drv_key(uint64_t parent, uint64_t index) {
  return drv_mix64(parent + 0x9E3779B97F4A7C15ull * (index + 1));
}
static double drv_u(uint64_t key, uint64_t slot) {
  return static_cast<double>(drv_key(key, slot)) * 0x1p-64;
}

struct NllsModel {
  // kind 0: exp model (n = 2); kind 1: tanh regression
  int kind;
  size_t m, n;
  std::vector<double> A, y, t;  // A: m*n row-major (tanh); t: abscissae (exp)
  std::vector<double> f_vals;
  Fnv pts;
  void residual_and_jacobian(const std::vector<double> &x, std::vector<double> &r,
                             std::vector<double> &J) const {
    r.assign(m, 0.0);
    J.assign(m * n, 0.0);
    for (size_t i = 0; i < m; i++) {
      if (kind == 0) {
        const double e = std::exp(x[1] * t[i]);
        r[i] = y[i] - x[0] * e;
        J[i * n + 0] = -e;
        J[i * n + 1] = -(x[0] * t[i] * e);
      } else {
        double z = 0.0;
        for (size_t j = 0; j < n; j++) z += A[i * n + j] * x[j];
        const double th = std::tanh(z);
        r[i] = y[i] - th;
        const double w = 1 - th * th;
        for (size_t j = 0; j < n; j++) J[i * n + j] = -(w * A[i * n + j]);
      }
    }
  }
  double operator()(std::vector<double> &x) {
    std::vector<double> r, J;
    residual_and_jacobian(x, r, J);
    double acc = 0.0;
    for (size_t i = 0; i < m; i++) acc += r[i] * r[i];
    f_vals.push_back(acc);
    for (double v : x) pts.add(v);
    return acc;
  }
};
struct GNGrad {
  void operator()(NllsModel &f, std::vector<double> &x, std::vector<double> &g) {
    std::vector<double> r, J;
    f.residual_and_jacobian(x, r, J);
    for (size_t j = 0; j < f.n; j++) {
      double acc = 0.0;
      for (size_t i = 0; i < f.m; i++) acc += J[i * f.n + j] * r[i];
      g[j] = 2 * acc;
    }
  }
};
struct GNHess {
  void operator()(NllsModel &f, std::vector<double> &x, std::vector<double> &h) {
    std::vector<double> r, J;
    f.residual_and_jacobian(x, r, J);
    for (size_t j = 0; j < f.n; j++)
      for (size_t k = 0; k < f.n; k++) {
        double acc = 0.0;
        for (size_t i = 0; i < f.m; i++) acc += J[i * f.n + j] * J[i * f.n + k];
        h[j * f.n + k] = 2 * acc;
      }
  }
};

static NllsModel make_exp_model() {
  NllsModel f;
  f.kind = 0;
  f.m = 8;
  f.n = 2;
  for (size_t i = 0; i < f.m; i++) {
    const double ti = 0.25 * static_cast<double>(i);
    f.t.push_back(ti);
    f.y.push_back(2.0 * std::exp(-0.7 * ti) + 0.02 * std::sin(3.0 * static_cast<double>(i) + 1.0));
  }
  return f;
}
static NllsModel make_tanh_model(uint64_t seed, uint64_t problem, size_t m, size_t n,
                                 std::vector<double> &theta0) {
  NllsModel f;
  f.kind = 1;
  f.m = m;
  f.n = n;
  const uint64_t kp = drv_key(seed, problem);
  const uint64_t kA = drv_key(kp, 0), kT = drv_key(kp, 1), k0 = drv_key(kp, 2);
  const double scale = 1.0 / std::sqrt(static_cast<double>(n));
  f.A.resize(m * n);
  for (size_t e = 0; e < m * n; e++) f.A[e] = (2 * drv_u(kA, e) - 1) * scale;
  std::vector<double> star(n);
  for (size_t j = 0; j < n; j++) star[j] = 2 * drv_u(kT, j) - 1;
  f.y.resize(m);
  for (size_t i = 0; i < m; i++) {
    double z = 0.0;
    for (size_t j = 0; j < n; j++) z += f.A[i * n + j] * star[j];
    f.y[i] = std::tanh(z);
  }
  theta0.resize(n);
  for (size_t j = 0; j < n; j++) theta0[j] = 0.5 * star[j] + 0.1 * (2 * drv_u(k0, j) - 1);
  return f;
}

static int run_lm(NllsModel &f, std::vector<double> x, double lambda, double up, double down,
                  size_t max_iter, double f_delta) {
  GNGrad g;
  GNHess h;
  auto solver = nlsolver::LevenbergMarquardt<NllsModel, double, GNGrad, GNHess>(
      f, lambda, up, down, max_iter, f_delta, g, h);
  auto res = solver.minimize(x);
  auto [fcalls, iters, fval, gcalls, hcalls] = res.get_summary();
  std::printf("{\"m\":%zu,\"n\":%zu,\"lambda\":", f.m, f.n);
  put_hex(lambda);
  std::printf(",\"up\":");
  put_hex(up);
  std::printf(",\"down\":");
  put_hex(down);
  std::printf(",\"max_iter\":%zu,\"f_delta\":", max_iter);
  put_hex(f_delta);
  std::printf(",\"fcalls\":%zu,\"iters\":%zu,\"gcalls\":%zu,\"hcalls\":%zu,\"f\":", fcalls,
              iters, gcalls, hcalls);
  put_hex(fval);
  std::printf(",\"x\":");
  put_vec(x);
  std::printf(",\"f_vals\":");
  put_vec(f.f_vals);
  std::printf(",\"pts_fnv\":\"%" PRIu64 "\"}\n", f.pts.h);
  return 0;
}

// tinyqr (tinyqr.h:291-310, 437-470) and math::cholesky solve (nlsolver.h:251-330) probes
static int run_linalg(size_t n, uint64_t seed, double lambda) {
  // SPD system: M = B^T B + lambda I from a pseudo-random B (n x n), rhs b
  std::vector<double> B(n * n), M(n * n, 0.0), b(n);
  const uint64_t k = drv_key(seed, 77);
  for (size_t e = 0; e < n * n; e++) B[e] = 2 * drv_u(k, e) - 1;
  for (size_t i = 0; i < n; i++) b[i] = 2 * drv_u(k, n * n + i) - 1;
  for (size_t i = 0; i < n; i++)
    for (size_t j = 0; j < n; j++) {
      double acc = 0.0;
      for (size_t l = 0; l < n; l++) acc += B[l * n + i] * B[l * n + j];
      M[i * n + j] = acc + (i == j ? lambda : 0.0);
    }
  // Cholesky path of the reference LM (row-major M)
  std::vector<double> Mc = M, upd(n), bc = b;
  nlsolver::math::get_update_with_hessian(upd, Mc, bc);
  // tinyqr::lm takes X column-major n x p; M is symmetric up to rounding, pass M^T explicitly
  std::vector<double> X(n * n);
  for (size_t i = 0; i < n; i++)
    for (size_t j = 0; j < n; j++) X[j * n + i] = M[i * n + j];
  auto beta = tinyqr::lm(X, b);
  auto qr = tinyqr::qr_decomposition(X, n, n);
  Fnv hq, hr;
  for (double v : qr.Q) hq.add(v);
  for (double v : qr.R) hr.add(v);
  std::printf("{\"n\":%zu,\"seed\":%" PRIu64 ",\"lambda\":", n, seed);
  put_hex(lambda);
  std::printf(",\"cholesky_solution\":");
  put_vec(upd);
  std::printf(",\"qr_solution\":");
  put_vec(beta);
  std::printf(",\"Q_fnv\":\"%" PRIu64 "\",\"R_fnv\":\"%" PRIu64 "\"", hq.h, hr.h);
  if (n <= 4) {
    std::printf(",\"Q\":");
    put_vec(qr.Q);
    std::printf(",\"R\":");
    put_vec(qr.R);
  }
  std::printf("}\n");
  return 0;
}
static int run_tinyqr_example() {  // SURVEY §3.5: X = [1 1 1 1; 0 1 2 3]^T, y = (1,3,5,7.5)
  std::vector<double> X = {1, 1, 1, 1, 0, 1, 2, 3}, y = {1, 3, 5, 7.5};
  auto qr = tinyqr::qr_decomposition(X, 4, 2);
  auto beta = tinyqr::lm(X, y);
  std::printf("{\"Q\":");
  put_vec(qr.Q);
  std::printf(",\"R\":");
  put_vec(qr.R);
  std::printf(",\"beta\":");
  put_vec(beta);
  std::printf("}\n");
  return 0;
}

// tinyqr on a RECTANGULAR system (n >= p): qr_decomposition (tinyqr.h:291-310) and lm (:461-470)
// on pseudo-random X (column-major n x p, entries in [-1, 1]) and y
static int run_tinyqr_rect(size_t n, size_t p, uint64_t seed) {
  std::vector<double> X(n * p), y(n);
  const uint64_t k = drv_key(seed, 78);
  for (size_t e = 0; e < n * p; e++) X[e] = 2 * drv_u(k, e) - 1;
  for (size_t i = 0; i < n; i++) y[i] = 2 * drv_u(k, n * p + i) - 1;
  auto beta = tinyqr::lm(X, y);
  auto qr = tinyqr::qr_decomposition(X, n, p);
  auto beta2 = tinyqr::back_solve(qr.Q, qr.R, y, n, p);  // with qr_decomposition's default tol
  Fnv hq, hr;
  for (double v : qr.Q) hq.add(v);
  for (double v : qr.R) hr.add(v);
  std::printf("{\"n\":%zu,\"p\":%zu,\"seed\":%" PRIu64 ",\"beta\":", n, p, seed);
  put_vec(beta);
  std::printf(",\"beta_tol1e-8\":");
  put_vec(beta2);
  std::printf(",\"Q_fnv\":\"%" PRIu64 "\",\"R_fnv\":\"%" PRIu64 "\"", hq.h, hr.h);
  if (n * p <= 64) {
    std::printf(",\"Q\":");
    put_vec(qr.Q);
    std::printf(",\"R\":");
    put_vec(qr.R);
  }
  std::printf("}\n");
  return 0;
}

// tinyqr on a system GIVEN on stdin (tests/_tinyqr_cases.py: graded, zero-laden, non-finite, scaled):
// X (column-major n x p) and y as hexfloat / nan / inf tokens. Output as tinyqr-rect, plus beta at
// `tol`; the hashes read every NaN as the one quiet NaN (its sign and payload are not pinned).
static int run_tinyqr_hex(size_t n, size_t p, double tol) {
  std::vector<double> X(n * p), y(n);
  auto read = [](double &v) {
    char tok[64];
    if (std::scanf("%63s", tok) != 1) std::exit(3);
    v = std::strtod(tok, nullptr);
  };
  for (double &v : X) read(v);
  for (double &v : y) read(v);
  auto beta = tinyqr::lm(X, y);
  auto beta_t = tinyqr::lm(X, y, tol);
  auto qr = tinyqr::qr_decomposition(X, n, p);
  auto beta2 = tinyqr::back_solve(qr.Q, qr.R, y, n, p);  // with qr_decomposition's default tol
  Fnv hq, hr;
  const double qnan = std::strtod("nan", nullptr);
  for (double v : qr.Q) hq.add(v != v ? qnan : v);
  for (double v : qr.R) hr.add(v != v ? qnan : v);
  std::printf("{\"n\":%zu,\"p\":%zu,\"tol\":", n, p);
  put_hex(tol);
  std::printf(",\"beta\":");
  put_vec(beta);
  std::printf(",\"beta_tol\":");
  put_vec(beta_t);
  std::printf(",\"beta_tol1e-8\":");
  put_vec(beta2);
  std::printf(",\"Q_fnv\":\"%" PRIu64 "\",\"R_fnv\":\"%" PRIu64 "\"", hq.h, hr.h);
  if (n <= 40 && p <= 12) {
    std::printf(",\"Q\":");
    put_vec(qr.Q);
    std::printf(",\"R\":");
    put_vec(qr.R);
  }
  std::printf("}\n");
  return 0;
}

// timing of the reference's tinyqr::lm on `count` pseudo-random n x p systems, one thread
static int bench_tinyqr(size_t n, size_t p, size_t count) {
  double total = 0, acc = 0;
  std::vector<double> X(n * p), y(n);
  for (size_t c = 0; c < count; c++) {
    const uint64_t k = drv_key(12374563468ull + c, 78);
    for (size_t e = 0; e < n * p; e++) X[e] = 2 * drv_u(k, e) - 1;
    for (size_t i = 0; i < n; i++) y[i] = 2 * drv_u(k, n * p + i) - 1;
    auto t0 = std::chrono::steady_clock::now();
    auto beta = tinyqr::lm(X, y);
    total += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    acc += beta[0];
  }
  std::printf("{\"n\":%zu,\"p\":%zu,\"systems\":%zu,\"seconds\":%.6f,\"systems_per_s\":%.6g,\"checksum\":%.17g}\n",
              n, p, count, total, count / total, acc);
  return 0;
}

static int bench_lm(size_t m, size_t n, size_t problems, size_t iters) {
  double total = 0, fsum = 0;
  auto t0 = std::chrono::steady_clock::now();
  for (size_t p = 0; p < problems; p++) {
    std::vector<double> x0;
    NllsModel f = make_tanh_model(12374563468ull, p, m, n, x0);
    GNGrad g;
    GNHess h;
    auto solver = nlsolver::LevenbergMarquardt<NllsModel, double, GNGrad, GNHess>(
        f, 10, 10, 10, iters, 0.0, g, h);
    auto res = solver.minimize(x0);
    auto [fcalls, it, fval, gc, hc] = res.get_summary();
    (void)fcalls; (void)gc; (void)hc;
    total += static_cast<double>(it);
    fsum += fval;
  }
  auto t1 = std::chrono::steady_clock::now();
  const double sec = std::chrono::duration<double>(t1 - t0).count();
  std::printf("{\"m\":%zu,\"n\":%zu,\"problems\":%zu,\"iterations\":%.0f,\"seconds\":%.6f,"
              "\"iterations_per_s\":%.6e,\"fsum\":%.17g}\n", m, n, problems, total, sec,
              total / sec, fsum);
  return 0;
}

// ---------------------------------------------------------------------------
// NelderMead (nlsolver.h:2099-2300) on Rosenbrock-ND. Records every objective value;
// big runs are pinned by an FNV hash of the values and of the evaluated points.
//   nm D step max_iter eps no_change restarts x0 x0_step bounded(0/1) upper lower minimize trace
// ---------------------------------------------------------------------------
static int run_nm(size_t D, double step, size_t max_iter, double eps, size_t no_change,
                  size_t restarts, double x0, double x0_step, bool bounded, double up, double lo,
                  bool minimize, int trace) {
  RecordingRosenbrock f;
  auto solver = nlsolver::NelderMead<RecordingRosenbrock, double>(f, step, 1, 2, 0.5, 0.5, eps,
                                                                  max_iter, no_change, restarts);
  std::vector<double> x(D), upper(D, up), lower(D, lo);
  for (size_t i = 0; i < D; i++) x[i] = x0 + x0_step * static_cast<double>(i);
  auto res = bounded ? (minimize ? solver.minimize(x, upper, lower) : solver.maximize(x, upper, lower))
                     : (minimize ? solver.minimize(x) : solver.maximize(x));
  auto [fcalls, iters, fval, g, h] = res.get_summary();
  (void)g;
  (void)h;
  std::printf("{\"D\":%zu,\"step\":", D);
  put_hex(step);
  std::printf(",\"max_iter\":%zu,\"eps\":", max_iter);
  put_hex(eps);
  std::printf(",\"no_change\":%zu,\"restarts\":%zu,\"x0\":", no_change, restarts);
  put_hex(x0);
  std::printf(",\"x0_step\":");
  put_hex(x0_step);
  std::printf(",\"bounded\":%d,\"upper\":", bounded ? 1 : 0);
  put_hex(up);
  std::printf(",\"lower\":");
  put_hex(lo);
  std::printf(",\"minimize\":%d,\"fcalls\":%zu,\"iters\":%zu,\"f\":", minimize ? 1 : 0, fcalls,
              iters);
  put_hex(fval);
  std::printf(",\"x\":");
  put_vec(x);
  Fnv hf, hx;
  for (double v : f.fs) hf.add(v);
  for (auto &v : f.xs)
    for (double d : v) hx.add(d);
  std::printf(",\"eval_f_fnv\":\"%" PRIu64 "\",\"eval_x_fnv\":\"%" PRIu64 "\"", hf.h, hx.h);
  if (trace >= 1) {
    std::printf(",\"eval_f\":");
    put_vec(f.fs);
  }
  std::printf("}\n");
  return 0;
}
static int run_simplex_init() {  // SURVEY B1 probe: x = {1,2,3,4}, default step
  std::vector<double> x = {1, 2, 3, 4};
  nlsolver::simplex<double> s(x, -1);
  std::printf("{\"vals\":[");
  for (size_t i = 0; i < s.vals.size(); i++) {
    if (i) std::printf(",");
    put_vec(s.vals[i]);
  }
  std::printf("]}\n");
  return 0;
}
static int bench_nm(size_t D, size_t iters) {
  RosenbrockND f;
  auto solver = nlsolver::NelderMead<RosenbrockND, double>(f, -1, 1, 2, 0.5, 0.5, 0.0, iters,
                                                           iters + 1, 0);
  std::vector<double> x(D, 0.5);
  auto t0 = std::chrono::steady_clock::now();
  auto res = solver.minimize(x);
  auto t1 = std::chrono::steady_clock::now();
  const double s = std::chrono::duration<double>(t1 - t0).count();
  auto [fcalls, it, fval, g, h] = res.get_summary();
  (void)g;
  (void)h;
  std::printf("{\"D\":%zu,\"iterations\":%zu,\"fcalls\":%zu,\"seconds\":%.6f,"
              "\"iterations_per_s\":%.6e,\"f\":%.17g}\n", D, it, fcalls, s,
              static_cast<double>(it) / s, fval);
  return 0;
}

static int more_main(const std::string &cmd, int argc, char **argv) {
  if (cmd == "nm") {
    if (argc < 15) {
      std::fprintf(stderr, "nm D step max_iter eps no_change restarts x0 x0_step bounded upper "
                           "lower minimize trace\n");
      return 2;
    }
    return run_nm(std::strtoull(argv[2], nullptr, 10), std::strtod(argv[3], nullptr),
                  std::strtoull(argv[4], nullptr, 10), std::strtod(argv[5], nullptr),
                  std::strtoull(argv[6], nullptr, 10), std::strtoull(argv[7], nullptr, 10),
                  std::strtod(argv[8], nullptr), std::strtod(argv[9], nullptr),
                  std::atoi(argv[10]) != 0, std::strtod(argv[11], nullptr),
                  std::strtod(argv[12], nullptr), std::atoi(argv[13]) != 0, std::atoi(argv[14]));
  }
  if (cmd == "simplex-init") return run_simplex_init();
  if (cmd == "bench-nm")
    return bench_nm(argc > 2 ? std::strtoull(argv[2], nullptr, 10) : 128,
                    argc > 3 ? std::strtoull(argv[3], nullptr, 10) : 2000);
  if (cmd == "lm-exp") {
    NllsModel f = make_exp_model();
    return run_lm(f, {1.0, -0.1}, argc > 2 ? std::strtod(argv[2], nullptr) : 10, 10, 10,
                  argc > 3 ? std::strtoull(argv[3], nullptr, 10) : 100,
                  argc > 4 ? std::strtod(argv[4], nullptr) : 1e-12);
  }
  if (cmd == "lm-tanh") {  // lm-tanh seed problem m n lambda max_iter f_delta
    if (argc < 9) return 2;
    std::vector<double> x0;
    NllsModel f = make_tanh_model(std::strtoull(argv[2], nullptr, 10),
                                  std::strtoull(argv[3], nullptr, 10),
                                  std::strtoull(argv[4], nullptr, 10),
                                  std::strtoull(argv[5], nullptr, 10), x0);
    return run_lm(f, x0, std::strtod(argv[6], nullptr), 10, 10,
                  std::strtoull(argv[7], nullptr, 10), std::strtod(argv[8], nullptr));
  }
  if (cmd == "linalg")
    return run_linalg(std::strtoull(argv[2], nullptr, 10), std::strtoull(argv[3], nullptr, 10),
                      std::strtod(argv[4], nullptr));
  if (cmd == "tinyqr-example") return run_tinyqr_example();
  if (cmd == "tinyqr-rect") {
    if (argc < 5) return 2;
    return run_tinyqr_rect(std::strtoull(argv[2], nullptr, 10), std::strtoull(argv[3], nullptr, 10),
                           std::strtoull(argv[4], nullptr, 10));
  }
  if (cmd == "tinyqr-hex") {  // tinyqr-hex n p tol < X y
    if (argc < 5) return 2;
    return run_tinyqr_hex(std::strtoull(argv[2], nullptr, 10), std::strtoull(argv[3], nullptr, 10),
                          std::strtod(argv[4], nullptr));
  }
  if (cmd == "bench-tinyqr")
    return bench_tinyqr(argc > 2 ? std::strtoull(argv[2], nullptr, 10) : 576,
                        argc > 3 ? std::strtoull(argv[3], nullptr, 10) : 64,
                        argc > 4 ? std::strtoull(argv[4], nullptr, 10) : 16);
  if (cmd == "bench-lm")
    return bench_lm(argc > 2 ? std::strtoull(argv[2], nullptr, 10) : 512,
                    argc > 3 ? std::strtoull(argv[3], nullptr, 10) : 64,
                    argc > 4 ? std::strtoull(argv[4], nullptr, 10) : 4,
                    argc > 5 ? std::strtoull(argv[5], nullptr, 10) : 20);
  if (cmd == "bfgs") {
    if (argc < 9) {
      std::fprintf(stderr, "bfgs n max_iter grad_eps alpha x0 x0_step trace\n");
      return 2;
    }
    return run_bfgs(std::strtoull(argv[2], nullptr, 10), std::strtoull(argv[3], nullptr, 10),
                    std::strtod(argv[4], nullptr), std::strtod(argv[5], nullptr),
                    std::strtod(argv[6], nullptr), std::strtod(argv[7], nullptr),
                    std::atoi(argv[8]));
  }
  if (cmd == "bfgs-mt") {
    if (argc < 8) {
      std::fprintf(stderr, "bfgs-mt n params(5n, comma separated) x0(n) alpha max_iter grad_eps\n");
      return 2;
    }
    return run_bfgs_mt(std::strtoull(argv[2], nullptr, 10), argv[3], argv[4], std::strtod(argv[5], nullptr),
                       std::strtoull(argv[6], nullptr, 10), std::strtod(argv[7], nullptr));
  }
  if (cmd == "bfgs-fd") {
    if (argc < 10) {
      std::fprintf(stderr, "bfgs-fd objective n max_iter grad_eps alpha x0 x0_step trace_cap\n");
      return 2;
    }
    return run_bfgs_fd(std::atoi(argv[2]), std::strtoull(argv[3], nullptr, 10),
                       std::strtoull(argv[4], nullptr, 10), std::strtod(argv[5], nullptr),
                       std::strtod(argv[6], nullptr), std::strtod(argv[7], nullptr),
                       std::strtod(argv[8], nullptr), std::strtoull(argv[9], nullptr, 10));
  }
  if (cmd == "lm-fd") {
    if (argc < 10) {
      std::fprintf(stderr, "lm-fd objective n max_iter lambda f_delta x0 x0_step trace_cap\n");
      return 2;
    }
    return run_lm_fd(std::atoi(argv[2]), std::strtoull(argv[3], nullptr, 10),
                     std::strtoull(argv[4], nullptr, 10), std::strtod(argv[5], nullptr),
                     std::strtod(argv[6], nullptr), std::strtod(argv[7], nullptr),
                     std::strtod(argv[8], nullptr), std::strtoull(argv[9], nullptr, 10));
  }
  if (cmd == "bench-bfgs-fd")
    return bench_bfgs_fd(argc > 2 ? std::strtoull(argv[2], nullptr, 10) : 128,
                         argc > 3 ? std::strtoull(argv[3], nullptr, 10) : 8,
                         argc > 4 ? std::strtoull(argv[4], nullptr, 10) : 20);
  if (cmd == "sann") {
    if (argc < 11) {
      std::fprintf(stderr, "sann objective n max_iter temp_iter temp_max x0 x0_step minimize trace_cap\n");
      return 2;
    }
    return run_sann(std::atoi(argv[2]), std::strtoull(argv[3], nullptr, 10),
                    std::strtoull(argv[4], nullptr, 10), std::strtoull(argv[5], nullptr, 10),
                    std::strtod(argv[6], nullptr), std::strtod(argv[7], nullptr),
                    std::strtod(argv[8], nullptr), std::atoi(argv[9]),
                    std::strtoull(argv[10], nullptr, 10));
  }
  if (cmd == "nmpso") {
    if (argc < 11) {
      std::fprintf(stderr, "nmpso objective n max_iter eps no_change x0 x0_step minimize trace_cap\n");
      return 2;
    }
    return run_nmpso(std::atoi(argv[2]), std::strtoull(argv[3], nullptr, 10),
                     std::strtoull(argv[4], nullptr, 10), std::strtod(argv[5], nullptr),
                     std::strtoull(argv[6], nullptr, 10), std::strtod(argv[7], nullptr),
                     std::strtod(argv[8], nullptr), std::atoi(argv[9]),
                     std::strtoull(argv[10], nullptr, 10));
  }
  if (cmd == "bench-nmpso")
    return bench_nmpso(argc > 2 ? std::strtoull(argv[2], nullptr, 10) : 32,
                       argc > 3 ? std::strtoull(argv[3], nullptr, 10) : 8,
                       argc > 4 ? std::strtoull(argv[4], nullptr, 10) : 100);
  if (cmd == "bench-sann")
    return bench_sann(argc > 2 ? std::strtoull(argv[2], nullptr, 10) : 128,
                      argc > 3 ? std::strtoull(argv[3], nullptr, 10) : 8,
                      argc > 4 ? std::strtoull(argv[4], nullptr, 10) : 100,
                      argc > 5 ? std::strtoull(argv[5], nullptr, 10) : 10);
  if (cmd == "bench-lm-fd")
    return bench_lm_fd(argc > 2 ? std::strtoull(argv[2], nullptr, 10) : 16,
                       argc > 3 ? std::strtoull(argv[3], nullptr, 10) : 8,
                       argc > 4 ? std::strtoull(argv[4], nullptr, 10) : 10);
  if (cmd == "hess-update") return run_hess_update();
  if (cmd == "bench-bfgs")
    return bench_bfgs(argc > 2 ? std::strtoull(argv[2], nullptr, 10) : 1024,
                      argc > 3 ? std::strtoull(argv[3], nullptr, 10) : 8);
  if (cmd == "pso") {
    if (argc < 10) {
      std::fprintf(stderr, "pso <accelerated|vanilla> D particles max_iter eps no_change x0 trace "
                           "[bounded lower upper] [inertia cog soc]\n");
      return 2;
    }
    const std::string type = argv[2];
    const size_t D = std::strtoull(argv[3], nullptr, 10);
    const size_t np = std::strtoull(argv[4], nullptr, 10);
    const size_t max_iter = std::strtoull(argv[5], nullptr, 10);
    const double eps = std::strtod(argv[6], nullptr);
    const size_t no_change = std::strtoull(argv[7], nullptr, 10);
    auto x0 = parse_x0(argv[8], D);
    const int trace = std::atoi(argv[9]);
    const bool bounded = argc > 10 && std::atoi(argv[10]) != 0;
    const double lo = argc > 11 ? std::strtod(argv[11], nullptr) : 0.0;
    const double hi = argc > 12 ? std::strtod(argv[12], nullptr) : 0.0;
    const double inertia = argc > 13 ? std::strtod(argv[13], nullptr) : 0.8;
    const double cog = argc > 14 ? std::strtod(argv[14], nullptr) : 1.8;
    const double soc = argc > 15 ? std::strtod(argv[15], nullptr) : 1.8;
    if (type == "accelerated")
      return run_pso<PSOType::Accelerated>(D, np, max_iter, eps, no_change, x0, trace, bounded, lo,
                                           hi, inertia, cog, soc);
    return run_pso<PSOType::Vanilla>(D, np, max_iter, eps, no_change, x0, trace, bounded, lo, hi,
                                     inertia, cog, soc);
  }
  if (cmd == "bench-pso") {
    const size_t D = argc > 2 ? std::strtoull(argv[2], nullptr, 10) : 256;
    const size_t np = argc > 3 ? std::strtoull(argv[3], nullptr, 10) : 4096;
    const size_t it = argc > 4 ? std::strtoull(argv[4], nullptr, 10) : 10;
    return bench_pso(D, np, it);
  }
  std::fprintf(stderr, "unknown command %s\n", cmd.c_str());
  return 2;
}
