// nlsolver_amd/csrc/nlsg_bfgs_turn.h — the statements of one turn of BFGS::solve's loop (nlsolver.h:3238-3284)
// up to the two H passes, for the wave that owns the problem: stop tests, reset guard, the whole More-Thuente
// search (<= 20 f+g evaluations), s, x, g, y, rho. NOT a header of declarations: nlsg_bfgs_kernels.h includes it
// wherever a kernel runs a turn, so that ONE text decides the bits of the lock-step and the resident engine.
// In scope at the include: CHUNKS; p (BfgsParams); model (BfgsModel<MODEL, CHUNKS>); n = p.n; x, g, dir
// (double[CHUNKS][2]); iter, fcalls, gcalls (uint64_t); prev_norm, cur_norm (double); and two macros:
//   NLSG_BFGS_TURN_STOPPED(fv)  a stop test fired: fv is f(x), only fcalls moved; must leave the turn
//   NLSG_BFGS_TURN_ADVANCED     the turn ran: s, y (double[CHUNKS][2]), rho and identity (whether H was
//                               taken as I) are in scope; iter is NOT incremented here
  // stop tests, nlsolver.h:3239-3246
  if (iter >= p.max_iter || cur_norm < p.grad_eps || fabs(cur_norm - prev_norm) < p.grad_eps ||
      isinf(cur_norm)) {
    const double fv = model.f(x, fcalls);
    NLSG_BFGS_TURN_STOPPED(fv)
  }
  // direction: d = -H g, computed by the previous update pass (or -g while H = I)
  // H in memory is valid after the previous update pass; only the very first
  // iteration (H = I, :3212) and the reset guard below use the identity shortcut
  int identity = (iter == 0) ? 1 : 0;
  if (identity) {
#pragma unroll
    for (int c = 0; c < CHUNKS; c++) {
      dir[c][0] = -g[c][0];
      dir[c][1] = -g[c][1];
    }
  }
  const double phi = bfgs_dot<CHUNKS>(g, dir, n, p.seq, model.lds);
  if ((phi > 0) || isnan(phi) || cur_norm > prev_norm) {  // reset guard, :3253-3260
    identity = 1;
#pragma unroll
    for (int c = 0; c < CHUNKS; c++) {
      dir[c][0] = -g[c][0];
      dir[c][1] = -g[c][1];
    }
  }
  double pg[CHUNKS][2];
#pragma unroll
  for (int c = 0; c < CHUNKS; c++) {
    pg[c][0] = g[c][0];
    pg[c][1] = g[c][1];
  }
  // more_thuente_search (1880-1891) -> cvsrch (1673-1793)
  const double f0 = model.f(x, fcalls);
  double stp = p.alpha;
  {
    int info = 0, infoc = 1;
    const double xtol = 1e-15, ftol = 1e-4, gtol = 1e-2, stpmin = 1e-15, stpmax = 1e15, xtrapf = 4;
    const int maxfev = 20;
    int nfev = 0;
    const double dginit = bfgs_dot<CHUNKS>(g, dir, n, p.seq, model.lds);
    if (!(dginit >= 0.0)) {
      int brackt = 0, stage1 = 1;
      const double finit = f0, dgtest = ftol * dginit;
      double width = stpmax - stpmin, width1 = 2 * width;
      double stx = 0.0, fx = finit, dgx = dginit, sty = 0.0, fy = finit, dgy = dginit;
      double stmin, stmax;
      for (;;) {
        if (brackt) {
          stmin = mt_min(stx, sty);
          stmax = mt_max(stx, sty);
        } else {
          stmin = stx;
          stmax = stp + xtrapf * (stp - stx);
        }
        stp = mt_clamp(stp, stpmin, stpmax);
        if ((brackt && ((stp <= stmin) || (stp >= stmax))) || (nfev >= maxfev - 1) ||
            (infoc == 0) || (brackt && ((stmax - stmin) <= (xtol * stmax))))
          stp = stx;
        double tmp[CHUNKS][2];
#pragma unroll
        for (int c = 0; c < CHUNKS; c++) {
          tmp[c][0] = x[c][0] + stp * dir[c][0];
          tmp[c][1] = x[c][1] + stp * dir[c][1];
        }
        const double fcur = model.f(tmp, fcalls);
        model.grad(tmp, g, fcalls, gcalls);
        nfev++;
        const double dg = bfgs_dot<CHUNKS>(g, dir, n, p.seq, model.lds);
        const double ftest1 = finit + stp * dgtest;
        if ((brackt & ((stp <= stmin) | (stp >= stmax))) | (infoc == 0)) info = 6;
        if ((stp == stpmax) & (fcur <= ftest1) & (dg <= dgtest)) info = 5;
        if ((stp == stpmin) & ((fcur > ftest1) | (dg >= dgtest))) info = 4;
        if (nfev >= maxfev) info = 3;
        if (brackt & (stmax - stmin <= xtol * stmax)) info = 2;
        if ((fcur <= ftest1) & (fabs(dg) <= gtol * (-dginit))) info = 1;
        if (info != 0) break;
        if (stage1 & (fcur <= ftest1) & (dg >= mt_min(ftol, gtol) * dginit)) stage1 = 0;
        // ONE call site, on copies chosen by value: with two calls on different references the compiler
        // merges them into one call on a selected address, and the bracket then lives in scratch memory
        const bool modified = stage1 & (fcur <= fx) & (fcur > ftest1);  // the modified function of stage 1
        double fxm = fx, fym = fy, dgxm = dgx, dgym = dgy, fm = fcur, dgm = dg;
        if (modified) {
          fm = fcur - stp * dgtest;
          fxm = fx - stx * dgtest;
          fym = fy - sty * dgtest;
          dgm = dg - dgtest;
          dgxm = dgx - dgtest;
          dgym = dgy - dgtest;
        }
        mt_cstep(stx, fxm, dgxm, sty, fym, dgym, stp, fm, dgm, brackt, stmin, stmax, infoc);
        fx = fxm;
        fy = fym;
        dgx = dgxm;
        dgy = dgym;
        if (modified) {
          fx = fxm + stx * dgtest;
          fy = fym + sty * dgtest;
          dgx = dgxm + dgtest;
          dgy = dgym + dgtest;
        }
        if (brackt) {
          if (fabs(sty - stx) >= 0.66 * width1) stp = stx + 0.5 * (sty - stx);
          width1 = width;
          width = fabs(sty - stx);
        }
      }
    }
  }
  // s = rate d; x += s; g = grad(x); norms; y; rho  (3266-3278)
  double s[CHUNKS][2], y[CHUNKS][2];
#pragma unroll
  for (int c = 0; c < CHUNKS; c++) {
#pragma unroll
    for (int h = 0; h < 2; h++) {
      s[c][h] = dir[c][h] * stp;
      x[c][h] = x[c][h] + s[c][h];
    }
  }
  model.grad(x, g, fcalls, gcalls);
  prev_norm = cur_norm;
  cur_norm = sqrt(bfgs_dot<CHUNKS>(g, g, n, p.seq, model.lds));
#pragma unroll
  for (int c = 0; c < CHUNKS; c++) {
    y[c][0] = g[c][0] - pg[c][0];
    y[c][1] = g[c][1] - pg[c][1];
  }
  double rho = bfgs_dot<CHUNKS>(y, s, n, p.seq, model.lds);
  rho = 1 / rho;
  NLSG_BFGS_TURN_ADVANCED
