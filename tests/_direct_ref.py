"""Independent references for the three direct-search solvers (TEST INFRASTRUCTURE).

Plain Python floats, written from the cited lines of nlsolver.h. Nothing here imports the package
or a *solver* of the oracle, so a decision rule that the device kernels share with their C
restatement (oracle/oracle_nm.c, oracle_nmpso.c, oracle_sann.c) cannot hide behind it.

  RefNelderMead  nlsolver.h:1894-2052 and 2166-2299: the effective simplex of SURVEY B1, the eps
                 mutation B2, the serial best / worst / second-worst scan B3 exactly as written
                 (`if <` / `else if >`), the contraction B4; bounds, maximize, step, restarts
  RefHybrid      nlsolver.h:3623-3918 with the rules H1-H5 of oracle/oracle_nmpso.c; the sort is the
                 project's rule (stable, NaN last, -0 equal to +0) written with sorted()
  RefSANN        nlsolver.h:2777-2814, literally `difference <= 0 or u < exp(-difference / t)`:
                 no shortcut of any kind

Draws and elementary functions are not the subject here and have pins of their own
(tests/test_math_*.py, test_rng*.py): Prims takes them as black boxes from liboracle.so. Every
comparison, counter, sort, scan and stop rule below is Python.

Sums. The objective is a callable; std_err's two sums are taken in the device's lane-tree order
(tree=True: lane l adds elements l, l + 64, ... in order, then the xor butterfly) or in index
order (tree=False: the reference's own arithmetic, and the device's reference_order mode).

Every reference counts what it did (`.counts`), so that a test can assert that its cases reach
the rules they are meant to reach.
"""
import math
from collections import Counter

NAN = float("nan")
INF = float("inf")


def same_value(a, b):
    """== with every NaN equal to every NaN; -0.0 equals +0.0 (a sum that starts from +0.0 and a
    lane tree padded with +0.0 agree on a signed zero only by value)."""
    a, b = float(a), float(b)
    return (a != a and b != b) or a == b


def same_bits(a, b):
    """bit-equal, every NaN equal to every NaN"""
    a, b = float(a), float(b)
    if a != a or b != b:
        return a != a and b != b
    return a == b and math.copysign(1.0, a) == math.copysign(1.0, b)


class Prims:
    """The black-box primitives: keyed draws and the deterministic exp / log of liboracle.so."""

    def __init__(self, lib):
        self.key = lambda a, b: int(lib.orc_ctr_key(a & 0xFFFFFFFFFFFFFFFF, b & 0xFFFFFFFFFFFFFFFF))
        self.u01 = lambda z: float(lib.orc_u01(z))
        self.rnorm = lambda z: float(lib.orc_rnorm(z))
        self.exp = lambda v: float(lib.orc_exp(v))
        self.log = lambda v: float(lib.orc_log(v))
        self._lib = lib

    def _row(self, fn, parent, first, stride, count):
        import ctypes
        out = (ctypes.c_double * count)()
        fn(parent, first, stride, count, out)
        return list(out)

    def u01_row(self, parent, first, stride, count):
        """[u01(key(parent, first + stride i)) for i < count], in one call"""
        return self._row(self._lib.orc_u01_keys, parent, first, stride, count)

    def rnorm_row(self, parent, first, stride, count):
        return self._row(self._lib.orc_rnorm_keys, parent, first, stride, count)


def fdiv(a, b):
    """a / b in IEEE double: Python raises where C gives +-inf or NaN"""
    try:
        return a / b
    except ZeroDivisionError:
        if a != a or a == 0.0:
            return NAN
        return math.copysign(INF, a) * math.copysign(1.0, b)


def _sqrt(v):
    return math.sqrt(v) if v >= 0.0 else NAN  # sqrt of NaN or of a negative number: NaN


def _tree_sum(vals):
    lane = [0.0] * 64
    for i, v in enumerate(vals):
        lane[i % 64] = lane[i % 64] + v
    off = 32
    while off >= 1:
        lane = [lane[l] + lane[l ^ off] for l in range(64)]
        off >>= 1
    return lane[0]


def _serial_sum(vals):
    acc = 0.0
    for v in vals:
        acc = acc + v
    return acc


def std_err(x, tree):
    """nlsolver.h:2037-2052 / 3903-3918: mean, sum of squared deviations (pow(d, 2) is the rounded
    product), division by n - 1, square root. Overflow gives inf and inf - inf NaN, as in C."""
    total = _tree_sum if tree else _serial_sum
    n = len(x)
    mean = total(x) / float(n)
    sq = []
    for v in x:
        d = v - mean
        sq.append(d * d)
    return _sqrt(total(sq) / float(n - 1))


def clamp(v, lo, hi):
    """std::clamp(v, lo, hi): a NaN passes through"""
    return lo if v < lo else (hi if hi < v else v)


def transform(point, centroid, coef, reflect, bounds):
    """simplex_transform<reflect, bound>, nlsolver.h:1986-2007"""
    out = []
    for i in range(len(point)):
        if reflect:
            t = centroid[i] + coef * (centroid[i] - point[i])
        else:
            t = centroid[i] + coef * (point[i] - centroid[i])
        if bounds is not None:
            t = clamp(t, bounds[1][i], bounds[0][i])
        out.append(t)
    return out


def max_abs_vec(x):
    """nlsolver.h:1894-1904"""
    result = abs(x[0])
    for v in x[1:]:
        t = abs(v)
        if result < t:
            result = t
    return result


class Result:
    def __init__(self, x, f_value, iteration, fcalls, eps=None):
        self.x, self.f_value, self.iteration, self.function_calls_used = x, f_value, iteration, fcalls
        self.eps = eps


def scan_categories(scores, best, worst, second):
    """What made a best / worst / second-worst scan hostile (RefNelderMead counts these)."""
    cats = []
    real = [s for s in scores if s == s]
    if len(real) != len(scores):
        cats.append("nan_among_scores")
    if scores[0] != scores[0]:
        cats.append("frozen")  # nothing compares with a NaN at vertex 0: all three stay 0
        return cats
    if sum(1 for s in real if s == min(real)) > 1:
        cats.append("tied_min")
    if sum(1 for s in real if s == max(real)) > 1:
        cats.append("tied_max")
    if len(real) >= 2:
        second_largest = sorted(real)[-2]
        if scores[second] != second_largest:
            cats.append("b3_quirk")  # "second worst" is not the second-largest score
    return cats


class RefNelderMead:
    """NelderMead<Callable>(f, step, alpha, gamma, rho, sigma, eps, max_iter, no_change_best_tol,
    restarts), nlsolver.h:2099-2299. `f` maps a list of floats to a float. upper / lower: lists
    (the bounded overloads) or None. self.eps is the solver's member: every solve mutates it (B2)."""

    def __init__(self, f, *, minimize=True, upper=None, lower=None, step=-1.0, alpha=1.0, gamma=2.0,
                 rho=0.5, sigma=0.5, eps=1e-6, max_iter=500, no_change=20, restarts=0, tree=True,
                 stop_margin=True):
        self.f, self.fm = f, (1.0 if minimize else -1.0)
        self.bounds = None if upper is None else (list(upper), list(lower))
        self.step, self.alpha, self.gamma, self.rho, self.sigma = step, alpha, gamma, rho, sigma
        self.eps, self.max_iter, self.no_change, self.restarts = eps, max_iter, no_change, restarts
        self.tree, self.stop_margin = tree, stop_margin
        self.counts = Counter()

    def run(self, x):
        """minimize() / maximize() with restarts (2127-2163; status.add: 2084-2091)"""
        x = [float(v) for v in x]
        res = self.solve(x)
        for _ in range(self.restarts):
            more = self.solve(res.x)
            res = Result(more.x, more.f_value, res.iteration + more.iteration,
                         res.function_calls_used + more.function_calls_used)
        res.eps = self.eps
        return res

    def solve(self, x):
        n, nv = len(x), len(x) + 1
        calls = [0]

        def f_lam(pt):  # 2177-2182
            calls[0] += 1
            return self.fm * self.f(pt)

        # simplex ctor, 1910-1947. init_simplex[i][i] for i == n is one element past the vector
        # (B1): the effective simplex leaves the last vertex at x.
        S = [list(x) for _ in range(nv)]
        if self.step < 0:
            inf_norm = max_abs_vec(x)
            a = 1.0 if inf_norm < 1.0 else inf_norm
            scale = a if a < 10 else 10.0
            for i in range(1, n):
                S[i][i] = S[i][i] + scale
            nn = float(n)
            for i in range(n):
                S[0][i] = x[i] + ((1.0 - math.sqrt(nn + 1.0)) / nn * scale)
        else:
            for i in range(1, n):
                S[i][i] = S[i][i] + self.step
        scores = [f_lam(S[i]) for i in range(nv)]  # 2184-2186
        self.eps = self.eps * (scores[0] * self.eps)  # 2189 (B2)
        worst = second = 0
        last_best, no_change, it = 99999999, 0, 0
        centroid = [0.0] * n  # 2195: zeros until the first update
        shrunk = False
        while True:
            best, prev_worst, worst, second = 0, worst, 0, 0  # 2202-2207
            se = std_err(scores, self.tree)
            for i in range(1, nv):  # 2209-2221, as written
                if scores[i] < scores[best]:
                    best = i
                elif scores[i] > scores[worst]:
                    second = worst
                    worst = i
            for c in scan_categories(scores, best, worst, second):
                self.counts["scan:" + c] += 1
            if last_best == best:  # 2223-2230
                no_change += 1
            else:
                no_change, last_best = 0, best
            if self.stop_margin and se == se and 0.0 < se < INF and 0.0 < self.eps < INF:
                # no verdict may hang on the last bits of a tree sum
                assert se > 2.0 * self.eps or se < 0.5 * self.eps, (se, self.eps)
            if it >= self.max_iter or se < self.eps or no_change >= self.no_change:  # 2233-2237
                self.counts["stop:" + ("max_iter" if it >= self.max_iter else
                                       "std_err" if se < self.eps else "no_change")] += 1
                return Result(list(S[best]), scores[best], it, calls[0])
            it += 1
            if prev_worst != worst or shrunk:  # update_centroid, 1965-1984
                centroid = [0.0] * n
                for v in range(nv):
                    if v == worst:
                        continue
                    for j in range(n):
                        centroid[j] = centroid[j] + S[v][j]
                centroid = [c / float(nv - 1) for c in centroid]
                shrunk = False
            tr = transform(S[worst], centroid, self.alpha, True, self.bounds)  # 2245
            ref_score = f_lam(tr)
            if ref_score >= scores[best] and ref_score < scores[second]:  # 2251
                S[worst], scores[worst] = tr, ref_score
                self.counts["act:accept"] += 1
            elif ref_score < scores[best]:  # 2255-2264
                te = transform(tr, centroid, self.gamma, False, self.bounds)
                exp_score = f_lam(te)
                S[worst] = te if exp_score < ref_score else tr
                scores[worst] = exp_score if exp_score < ref_score else ref_score
                self.counts["act:expand"] += 1
            else:  # 2266-2296 (B4: the reflect transform for both kinds of contraction)
                outside = ref_score < scores[worst]
                tc = transform(tr if outside else S[worst], centroid, self.rho, True, self.bounds)
                cont_score = f_lam(tc)
                if cont_score < (ref_score if outside else scores[worst]):
                    S[worst], scores[worst] = tc, cont_score
                    self.counts["act:contract_outside" if outside else "act:contract_inside"] += 1
                else:  # shrink 2009-2035, rescoring 2288-2294
                    bv = S[best]
                    for v in range(nv):
                        if v != best:
                            S[v] = [bv[j] + self.sigma * (S[v][j] - bv[j]) for j in range(n)]
                    for v in range(nv):
                        if v != best:
                            scores[v] = f_lam(S[v])
                    shrunk = True
                    self.counts["act:shrink"] += 1


def sort_key(v):
    """the project's order of particle values: NaN last, -0 equal to +0 (oracle_nmpso.c)"""
    return (1, 0.0) if v != v else (0, v)


class RefHybrid:
    """NelderMeadPSO, nlsolver.h:3546-3918, with draws keyed as orc_nmpso_sync's comment says:
    kc = key(seed, instance); the initialisation uses key(kc, 0), iteration it key(kc, it + 1); the
    PSO particle of rank r (0 .. 2n-1) has kp = key(that, r) and coordinate j takes draws 2j, 2j+1."""

    def __init__(self, f, prims, *, seed, instance, minimize=True, upper=None, lower=None, alpha=1.0,
                 gamma=2.0, rho=0.5, sigma=0.5, inertia=0.8, cog=1.8, soc=1.8, eps=1e-6, max_iter=1000,
                 no_change=20, tree=True, stop_margin=True):
        self.f, self.P, self.fm = f, prims, (1.0 if minimize else -1.0)
        self.kc = prims.key(seed, instance)
        self.bounds = None if upper is None else (list(upper), list(lower))
        self.alpha, self.gamma, self.rho, self.sigma = alpha, gamma, rho, sigma
        self.inertia, self.cog, self.soc = inertia, cog, soc
        self.eps, self.max_iter, self.no_change, self.tree = eps, max_iter, no_change, tree
        self.stop_margin = stop_margin
        self.counts = Counter()

    def _sorted(self, order, val, ns):
        out = sorted(order, key=lambda i: sort_key(val[i]))  # stable
        head = [sort_key(val[i]) for i in out[:ns]]
        if any(head[i] == head[i + 1] for i in range(ns - 1)):
            self.counts["sort:tied_in_simplex"] += 1
        if any(val[i] != val[i] for i in order):
            self.counts["sort:nan_key"] += 1
        plus = False
        for i in out:  # a +0.0 kept ahead of a -0.0: the two are one key, and the sort is stable
            if val[i] == 0.0:
                if math.copysign(1.0, val[i]) > 0.0:
                    plus = True
                elif plus:
                    self.counts["sort:plus_zero_before_minus_zero"] += 1
                    break
        return out

    def run(self, x):
        P, n = self.P, len(x)
        x = [float(v) for v in x]
        if n < 2:  # 3627-3636
            return Result(x, 999999.0, 0, 0)
        ns, np_, total = n + 1, 2 * n, 3 * n + 1
        calls = [0]

        def f_lam(pt):
            calls[0] += 1
            return self.fm * self.f(pt)

        bound = self.bounds is not None
        if bound:
            upper, lower = self.bounds
        else:  # 3587-3593
            lower = [-abs(2.5 * v) for v in x]
            upper = [abs(2.5 * v) for v in x]
        bounds = (upper, lower) if bound else None
        # init_solver_state, 3688-3741; particle_positions[n][n] is out of bounds (H1)
        inf_norm = max_abs_vec(x)
        a = 1.0 if inf_norm < 1.0 else inf_norm
        scale = a if a < 10 else 10.0
        pos = [list(x) for _ in range(ns)]
        for i in range(1, n):
            pos[i][i] = x[i] + scale
        nn = float(n)
        for i in range(n):
            pos[0][i] = x[i] + ((1.0 - math.sqrt(nn + 1.0)) / nn * scale)
        vel = [[0.0] * n for _ in range(ns)]
        kinit = P.key(self.kc, 0)
        for r in range(np_):
            kp = P.key(kinit, r)
            row, vrow = [], []
            u = P.u01_row(kp, 0, 1, 2 * n)  # coordinate j: draws 2j and 2j + 1
            for j in range(n):
                temp = abs(upper[j] - lower[j])
                row.append(lower[j] + ((upper[j] - lower[j]) * u[2 * j]))
                vrow.append(-temp + (u[2 * j + 1] * temp))
            pos.append(row)
            vel.append(vrow)
        val = [f_lam(p) for p in pos]
        order = list(range(total))
        it = no_change = 0
        best_val = val[0]  # 3649, never updated (H2)
        self.first_value = best_val
        while True:
            order = self._sorted(order, val, ns)  # 3653
            same = best_val == val[order[0]]  # 3659
            no_change = no_change + 1 if same else 0
            self.counts["h2:" + ("same" if same else "differs")] += 1
            if same and best_val == 0.0:
                self.counts["h2:same_at_zero"] += 1
            se = std_err([val[i] for i in order[:ns]], self.tree)
            if self.stop_margin and se == se and 0.0 < se < INF and 0.0 < self.eps < INF:
                assert se > 2.0 * self.eps or se < 0.5 * self.eps, (se, self.eps)
            if it >= self.max_iter or no_change >= self.no_change or se < self.eps:  # 3665-3669
                self.counts["stop:" + ("max_iter" if it >= self.max_iter else "no_change"
                                       if no_change >= self.no_change else "std_err")] += 1
                return Result(list(pos[order[0]]), val[order[0]], it, calls[0])
            # apply_simplex, 3742-3823
            best_score = val[order[0]]
            worst, second = order[ns - 1], order[ns - 2]
            centroid = [0.0] * n
            for i in range(ns - 1):
                pi = pos[order[i]]
                for j in range(n):
                    centroid[j] = centroid[j] + pi[j]
            centroid = [c / float(ns - 1) for c in centroid]
            tr = transform(pos[worst], centroid, self.alpha, True, bounds)
            ref_score = f_lam(tr)
            if ref_score >= best_score and ref_score < val[second]:
                pos[worst], val[worst] = tr, ref_score
                self.counts["act:accept"] += 1
            elif ref_score < best_score:
                te = transform(tr, centroid, self.gamma, False, bounds)
                exp_score = f_lam(te)
                pos[worst] = te if exp_score < ref_score else tr
                val[worst] = exp_score if exp_score < ref_score else ref_score
                self.counts["act:expand"] += 1
            else:
                worst_score = val[worst]
                outside = ref_score < worst_score
                tc = transform(tr if outside else pos[worst], centroid, self.rho, False, bounds)
                cont_score = f_lam(tc)
                # std::min(ref_score, worst_score) = worst_score < ref_score ? worst_score : ref_score
                if cont_score < (worst_score if worst_score < ref_score else ref_score):
                    pos[worst], val[worst] = tc, cont_score
                    self.counts["act:contract_outside" if outside else "act:contract_inside"] += 1
                else:  # shrink 3887-3903, rescoring and the second sort 3810-3820
                    bv = pos[order[0]]
                    for i in range(1, ns):
                        cur = pos[order[i]]
                        pos[order[i]] = [bv[j] + self.sigma * (cur[j] - bv[j]) for j in range(n)]
                    for i in range(1, ns):
                        val[order[i]] = f_lam(pos[order[i]])
                    order = self._sorted(order, val, ns)
                    self.counts["act:shrink"] += 1
            # apply_pso, 3824-3868
            kit = P.key(self.kc, it + 1)
            flip = False
            best_in_pair = order[ns]
            best = pos[order[0]]
            for i in range(ns, total):
                pid = order[i]
                if flip:
                    best_in_pair = order[i + 1]  # H4
                flip = bool((i - ns) % 2)
                particle, velocity = pos[pid], vel[pid]  # H3: the velocity is never written back
                pair = list(pos[best_in_pair])
                kp = P.key(kit, i - ns)
                u = P.u01_row(kp, 0, 1, 2 * n)
                for j in range(n):
                    r_p, r_g = u[2 * j], u[2 * j + 1]
                    temp = (self.inertia * velocity[j]) + self.cog * r_p * (pair[j] - particle[j]) + \
                        self.soc * r_g * (best[j] - particle[j])
                    if bound:
                        temp = clamp(temp, lower[j], upper[j])  # H5
                    particle[j] = particle[j] + temp
                val[pid] = f_lam(particle)
            it += 1


class RefSANN:
    """SANN::solve, nlsolver.h:2777-2814, with the keying of orc_sann_sync: kc = key(seed, chain);
    inner step s = iter (temperature_iter - 1) + (j - 1) has ks = key(kc, s); coordinate e takes
    rnorm(key(ks, 2e)), the acceptance test u01(key(ks, 2D))."""

    def __init__(self, f, prims, *, seed, chain, minimize=True, max_iter=5000, temp_iter=10,
                 temp_max=10.0):
        self.f, self.P, self.fm = f, prims, (1.0 if minimize else -1.0)
        self.kc = prims.key(seed, chain)
        self.max_iter, self.temp_iter, self.temp_max = max_iter, temp_iter, temp_max
        self.counts = Counter()

    def run(self, x):
        P, D = self.P, len(x)
        x = [float(v) for v in x]
        e_minus_1 = 1.7182818
        best_val = self.fm * self.f(x)  # 2780
        scale = fdiv(1.0, self.temp_max)
        evals = 1
        p, it = list(x), 0
        while True:
            if it >= self.max_iter:  # 2787-2790
                return Result(x, best_val, it, evals)
            t = fdiv(self.temp_max, P.log(float(it) + e_minus_1))  # 2792-2793
            for j in range(1, self.temp_iter):
                ks = P.key(self.kc, it * (self.temp_iter - 1) + (j - 1))
                current_scale = t * scale
                z = P.rnorm_row(ks, 0, 2, D)  # coordinate e: rnorm(key(ks, 2e))
                ptry = [p[i] + current_scale * z[i] for i in range(D)]
                current_val = self.fm * self.f(ptry)
                evals += 1
                difference = current_val - best_val  # 2803
                if difference != difference or abs(difference) == INF:
                    self.counts["diff:" + ("nan" if difference != difference else
                                           "+inf" if difference > 0 else "-inf")] += 1
                if difference > 710.0 * t > 0.0:
                    self.counts["diff:beyond_710t"] += 1
                # 2804, literally
                if difference <= 0.0 or P.u01(P.key(ks, 2 * D)) < P.exp(fdiv(-difference, t)):
                    self.counts["accepted_" + ("better" if difference < 0.0 else "equal"
                                               if difference == 0.0 else "worse")] += 1
                    p = ptry
                    if current_val <= best_val:  # 2806
                        x, best_val = list(p), current_val
                        self.counts["best_taken_" + ("lower" if difference < 0.0 else "equal")] += 1
                    else:
                        self.counts["best_kept"] += 1
                else:
                    self.counts["rejected"] += 1
            it += 1
