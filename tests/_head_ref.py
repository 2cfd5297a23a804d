"""Independent references for the head of a population turn (TEST INFRASTRUCTURE).

Plain Python: nothing here imports tests._oracle or the package, so an error that the device
kernels share with their C restatement (oracle/oracle_de.c, oracle/oracle_pso.c) cannot hide.

  RefDEHead      the best scan, the counter and the stop tests of nlsolver.h:2428-2447
  RefPSOHead     update_best_positions, nlsolver.h:2716-2741, with the two documented repairs
                 (+inf sentinels, B9: "no change" means that no update happened)
  literal_std_err  nlsolver.h:2037-2052 in double, serially, as written there
  exact_std_err  the same statistic in exact rational arithmetic, rounded once
  families(...)  hostile score vectors: ties, non-finite values, conditioning
"""
import math
from fractions import Fraction

import numpy as np

NAN = float("nan")
INF = float("inf")
U = 2.0 ** -53  # unit roundoff of binary64


def same_double(a, b):
    """Bit-equal with every NaN equal to every NaN: -0.0 and +0.0 differ."""
    a, b = float(a), float(b)
    if a != a or b != b:
        return a != a and b != b
    return a == b and math.copysign(1.0, a) == math.copysign(1.0, b)


def literal_std_err(x):
    """nlsolver.h:2037-2052 as written: a serial mean, a serial sum of squared deviations,
    division by n - 1, square root; IEEE double throughout (overflow gives inf, not an error)."""
    a = np.asarray(x, dtype=np.float64)
    n = a.size
    with np.errstate(all="ignore"):  # np.add.accumulate adds strictly left to right
        mean = float(np.add.accumulate(a)[-1]) / n
        d = a - mean
        res = float(np.add.accumulate(d * d)[-1]) / (n - 1)  # pow(d, 2) is the rounded product
    return math.sqrt(res)  # res is >= 0, +inf or NaN


def exact_std_err(x):
    """(std_err, kappa) of finite doubles. The sums of nlsolver.h:2037-2052 are taken exactly
    (every double is an integer times a power of two; the variance is one Fraction), the square
    root with mpmath at 400 bits, and the result is rounded to double once.
    kappa = sqrt(sum x^2 / M2): how much a relative error of the mean is amplified in M2.
    M2 == 0 (all equal): (0.0, inf)."""
    import mpmath
    a = np.asarray(x, dtype=np.float64)
    assert a.ndim == 1 and a.size >= 2 and np.all(np.isfinite(a))
    n = int(a.size)
    mant, expo = np.frexp(a)
    m = np.ldexp(mant, 53).astype(np.int64).astype(object)  # exact: |mant| < 1 has 53 bits
    e = expo.astype(np.int64) - 53
    nz = a != 0.0
    emin = int(e[nz].min()) if nz.any() else 0
    sh = np.where(nz, e - emin, 0).astype(np.int64).astype(object)
    v = m * (2 ** sh)  # python integers: x_i = v_i * 2^emin
    s1 = int(v.sum())
    s2 = int((v * v).sum())
    m2n = n * s2 - s1 * s1  # n * M2 >= 0, exactly
    if m2n == 0:
        return 0.0, INF
    var = Fraction(m2n, n * (n - 1))  # in units of 2^(2 emin)
    with mpmath.workprec(400):
        root = mpmath.sqrt(mpmath.mpf(var.numerator) / mpmath.mpf(var.denominator))
        se = root * mpmath.mpf(2) ** emin
        kappa = mpmath.sqrt(mpmath.mpf(n * s2) / mpmath.mpf(m2n))
        # one rounding to double, subnormal results included (Fraction -> float rounds correctly)
        mt, ex = mpmath.frexp(se)
        q = Fraction(int(mpmath.floor(mpmath.ldexp(mt, 300)))) * Fraction(2) ** (int(ex) - 300)
        return float(q), float(kappa)


def std_err_bound(kappa, L):
    """A-priori relative error of the one-pass tile-merged std_err whose longest path has L
    roundings: first-order sensitivity of the merge to the rounded means, plus the two-pass
    residual. (Standard model of arithmetic: valid while nothing underflows.)"""
    return L * U * (2.0 + 2.0 * kappa) + (L * U * kappa) ** 2


# A statistic below STD_ERR_TINY comes from squared deviations that underflow (denormal scores):
# no double evaluation of the formula, the literal one included, keeps a relative accuracy there.
# Every squared deviation may lose up to 2^-1074, M2 then n * 2^-1074 and the statistic
# sqrt(n / (n-1) * 2^-1074) <= 2^-536: below STD_ERR_TINY, and only there, that absolute term
# is added to the bound. Everywhere else the bound is purely relative.
STD_ERR_TINY = 1e-150
STD_ERR_UNDERFLOW = 2.0 ** -536


class RefDEHead:
    """nlsolver.h:2428-2447. `iter` counts the generations made so far; a head that fires a stop
    test freezes the state (the reference returns there)."""

    def __init__(self, max_iter=1000, best_val_no_change=50, eps=0.0):
        self.max_iter, self.best_val_no_change, self.eps = max_iter, best_val_no_change, eps
        self.best_id = 0  # :2428
        self.val_no_change = 0
        self.iter = 0  # :2427
        self.done = False
        self.f_value = None
        self.std_err = NAN

    def turn(self, scores, std_err=None):
        """One head on `scores`. `std_err`: the statistic to test against eps (default: the
        literal formula on `scores`). Returns (best_id, val_no_change, done, f_value)."""
        if not self.done:
            s = np.asarray(scores, dtype=np.float64).tolist()
            best_id = self.best_id
            not_updated = True
            for i in range(len(s)):  # :2432-2437
                if s[i] < s[best_id]:
                    best_id = i
                    not_updated = False
            self.best_id = best_id
            self.val_no_change = (self.val_no_change + 1) if not_updated else 0  # :2439
            self.f_value = s[best_id]
            stop = self.iter >= self.max_iter or self.val_no_change >= self.best_val_no_change
            if not stop and self.eps > 0:  # `std_err < eps` is false for every eps <= 0 or NaN
                self.std_err = literal_std_err(s) if std_err is None else std_err
                stop = self.std_err < self.eps  # :2443
            if stop:
                self.done = True  # :2444-2446
            else:
                self.iter += 1  # the generation follows
        return self.best_id, self.val_no_change, self.done, self.f_value


class RefPSOHead:
    """update_best_positions (nlsolver.h:2716-2741) followed by the stop tests of the loop's next
    trip (:2597-2600), with SURVEY B8 (sentinels are +inf) and B9 (val_no_change resets when an
    update happened, not when the best index is non-zero)."""

    def __init__(self, n, max_iter=5000, best_val_no_change=50, eps=0.0):
        self.n = n
        self.max_iter, self.best_val_no_change, self.eps = max_iter, best_val_no_change, eps
        self.swarm_best_value = INF  # :2631 with B8
        self.swarm_best_index = 0
        self.particle_best_values = [INF] * n  # :2655-2656 with B8
        self.val_no_change = 0
        self.iter = 0
        self.done = False
        self.std_err = NAN

    def turn(self, values, std_err=None):
        """`values`: f_multiplier * f(position) of every particle. Returns (gbest index,
        gbest value, val_no_change, done)."""
        if not self.done:
            best_index, update_happened = self.swarm_best_index, False
            for i in range(self.n):
                temp = float(values[i])  # :2722
                if temp < self.swarm_best_value:  # :2723-2729
                    self.swarm_best_value = temp
                    best_index = i
                    update_happened = True
                if temp < self.particle_best_values[i]:  # :2730-2732
                    self.particle_best_values[i] = temp
            self.swarm_best_index = best_index
            self.val_no_change = 0 if update_happened else self.val_no_change + 1  # :2740, B9
            stop = self.iter >= self.max_iter or self.val_no_change >= self.best_val_no_change
            if not stop and self.eps > 0:
                self.std_err = (literal_std_err(self.particle_best_values) if std_err is None
                                else std_err)
                stop = self.std_err < self.eps
            if stop:
                self.done = True
            else:
                self.iter += 1
        return self.swarm_best_index, self.swarm_best_value, self.val_no_change, self.done


def std_err_precondition(x):
    """finite scores whose sum of squares does not overflow: the bound applies"""
    a = np.asarray(x, dtype=np.float64)
    return bool(np.all(np.isfinite(a))) and float(np.max(np.abs(a))) < 1e150


def _cls(v):
    return "nan" if v != v else "+inf" if v == INF else "-inf" if v == -INF else "finite"


def judge_std_err(got, x, L):
    """Holds `got`, a double evaluation of std_err(x) with at most L roundings on its longest
    path, against the exact statistic. Returns (ok, ratio, text): `ratio` is the error as a
    fraction of the bound's linear term (None where the bound does not apply).
      bound applies : |got - exact| <= exact * std_err_bound(kappa, L)
                      (+ STD_ERR_UNDERFLOW where exact < STD_ERR_TINY)
      exact == 0    : kappa is infinite and the bound says nothing; got must be finite, >= 0
      otherwise     : got falls in the class (NaN or +inf) of the literal formula"""
    if not std_err_precondition(x):
        want = _cls(literal_std_err(x))
        return _cls(got) == want, None, f"class {_cls(got)} vs literal {want}"
    exact, kappa = exact_std_err(x)
    if exact == 0.0:
        return _cls(got) == "finite" and got >= 0.0, None, f"got {got!r}, exact 0"
    err = abs(got - exact)
    allowed = exact * std_err_bound(kappa, L)
    if exact < STD_ERR_TINY:
        allowed += STD_ERR_UNDERFLOW
    lin = exact * L * U * (2.0 + 2.0 * kappa)
    ratio = err / lin if lin > 0.0 else None  # a subnormal statistic: only the absolute term
    return err <= allowed, ratio, (f"got {got!r} exact {exact!r} kappa {kappa:.3g} rel err "
                                   f"{err / exact:.3g} bound {std_err_bound(kappa, L):.3g}")


# ---- score families ---------------------------------------------------------------------------
# family(n, inc, shards, rng) -> list of (name, vector). `inc` is where the incumbent will sit
# when the head scans the vector, `shards` the number of equal shards the vector is cut into
# (1: none). Values around the incumbent are chosen so that each rule decides something.
TILE = 1024


def _base(n, rng):
    """distinct finite scores in [2, 3): whatever a family plants below 2 is the minimum"""
    return 2.0 + rng.permutation(n) / float(n)


def _landmarks(n):
    return sorted({i for i in (0, 255, 256, 257, 1023, 1024, 1025, n - 1) if 0 <= i < n})


def fam_ties(n, inc, shards, rng):
    out = [("ties/all_equal", np.full(n, 1.5))]
    for at in _landmarks(n):
        v = np.full(n, 2.0)  # two-valued
        v[at] = 1.0
        out.append((f"ties/two_valued_min_at_{at}", v))
    v = np.full(n, 2.0)
    v[0] = v[n - 1] = 1.0
    out.append(("ties/two_valued_min_first_and_last", v))
    # the minimum duplicated below and above the incumbent, which holds it too / does not
    lo, hi = max(inc - 1, 0), min(inc + 1, n - 1)
    v = _base(n, rng)
    v[[lo, hi]] = 1.0
    v[inc] = 1.0
    out.append(("ties/dup_around_incumbent_tied", v))
    v = _base(n, rng)
    v[[0, lo, hi, n - 1]] = 1.0
    if inc not in (0, lo, hi, n - 1):
        v[inc] = 1.25
    out.append(("ties/dup_around_incumbent_beaten", v))
    # -0.0 == +0.0: equal values, so the incumbent or the lower index wins, never the sign
    v = np.full(n, 0.0)
    v[inc] = -0.0
    out.append(("ties/neg_zero_incumbent_among_pos_zero", v.copy()))
    v = np.full(n, -0.0)
    v[inc] = 0.0
    out.append(("ties/pos_zero_incumbent_among_neg_zero", v.copy()))
    v = _base(n, rng)
    v[inc] = 0.0
    v[(inc + 1) % n] = -0.0
    v[(inc - 1) % n] = -0.0
    out.append(("ties/neg_zero_beside_zero_incumbent", v))
    if shards > 1:  # equal minima in several shards; incumbent in an earlier / later / no such shard
        m = n // shards
        owner = inc // m
        for name, ranks in (("all_shards", range(shards)), ("later_shards", range(owner + 1, shards)),
                            ("earlier_shards", range(0, owner)), ("first_and_last", (0, shards - 1))):
            ranks = list(ranks)
            if not ranks:
                continue
            for inc_val, tag in ((1.0, "incumbent_tied"), (1.5, "incumbent_beaten")):
                v = _base(n, rng)
                for r in ranks:
                    v[r * m + (m - 1 if r % 2 else m // 2)] = 1.0
                if owner not in ranks or v[inc] != 1.0:
                    v[inc] = inc_val
                out.append((f"ties/equal_minima_{name}_{tag}", v))
    return out


def fam_nonfinite(n, inc, shards, rng):
    out = []
    v = _base(n, rng)
    v[inc] = NAN
    out.append(("nonfinite/nan_at_incumbent", v))
    for keep in sorted({0, inc, n - 1}):
        v = np.full(n, NAN)
        v[keep] = 1.0
        out.append((f"nonfinite/nan_everywhere_but_{keep}", v))
    if n > TILE:
        for t in sorted({0, inc // TILE, (n - 1) // TILE}):
            v = _base(n, rng)
            v[t * TILE:(t + 1) * TILE] = NAN
            out.append((f"nonfinite/nan_tile_{t}", v))
    if shards > 1:
        m = n // shards
        owner = inc // m
        for r in sorted({0, owner, (owner + 1) % shards, shards - 1}):
            v = _base(n, rng)
            v[r * m:(r + 1) * m] = NAN
            tag = "owning" if r == owner else "not_owning"
            out.append((f"nonfinite/nan_shard_{r}_{tag}_incumbent", v))
        if owner > 0:  # a NaN incumbent in rank r > 0 while rank 0 holds finite scores
            v = _base(n, rng)
            v[inc] = NAN
            v[0] = 0.5
            out.append(("nonfinite/nan_incumbent_behind_finite_rank0", v))
            v = np.full(n, NAN)
            v[:m] = _base(m, rng)
            out.append(("nonfinite/only_rank0_finite", v))
    out.append(("nonfinite/all_nan", np.full(n, NAN)))
    out.append(("nonfinite/all_pos_inf", np.full(n, INF)))
    v = np.full(n, INF)
    v[n - 1] = 1.0
    out.append(("nonfinite/pos_inf_but_last", v))
    for at in sorted({0, n // 2, n - 1}):
        v = _base(n, rng)
        v[at] = -INF
        out.append((f"nonfinite/neg_inf_at_{at}", v))
    v = _base(n, rng)
    v[[0, n - 1]] = -INF
    out.append(("nonfinite/neg_inf_twice", v))
    out.append(("nonfinite/all_1e308", np.full(n, 1e308)))
    return out


def fam_conditioning(n, inc, shards, rng):
    out = []
    for mean, spread in ((0.0, 1.0), (50.0, 10.0), (1e4, 1e-2), (-1e8, 1.0)):
        out.append((f"conditioning/normal_{mean:g}_{spread:g}", rng.normal(mean, spread, n)))
    out.append(("conditioning/denormals", rng.integers(1, 2 ** 40, n).astype(np.float64) * 2.0 ** -1074))
    v = rng.uniform(0.5, 1.5, n)
    v[rng.integers(0, n)] = 1e12
    out.append(("conditioning/outlier_1e12", v))
    return out


FAMILIES = {"ties": fam_ties, "nonfinite": fam_nonfinite, "conditioning": fam_conditioning}


def families(n, inc, shards=1, seed=0, which=("ties", "nonfinite", "conditioning")):
    """[(name, vector)] of every family member that exists at this size; seeded."""
    out = []
    for k, key in enumerate(which):
        rng = np.random.default_rng([seed, n, inc, shards, k])
        out += FAMILIES[key](n, inc, shards, rng)
    return out


def placement(n, j, scale=1.0):
    """Scores whose unique minimum is at j and whose std_err is about scale * n / 3.5: one head
    on them moves the incumbent to j without the eps test firing for any eps < scale."""
    v = scale * (2.0 + np.arange(n, dtype=np.float64))
    v[j] = scale
    return v


def fuzz_vector(n, rng):
    """scores drawn from the six values on which the comparison rules differ"""
    return rng.choice(np.array([NAN, -INF, -0.0, 0.0, 1.0, INF]), size=n)


# ---- two-turn cases: place the incumbent, then scan a hostile vector ---------------------------
EPS_TINY = 1e-300  # > 0, so std_err is evaluated; only an exactly zero statistic is below it


def incumbents(n, shards=1):
    """where the incumbent sits: first, middle, last agent; per shard layout a first, a middle and
    the last shard; in a population of many tiles one agent inside a middle tile"""
    if shards > 1:
        m = n // shards
        return sorted({r * m + m // 3 for r in (0, shards // 2, shards - 1)})
    if n > 4096:
        return [100 * TILE + 5]
    return sorted({0, n // 2, n - 1})


class Case:
    """`place` puts the incumbent at `inc` (turn 1), `vec` is scanned from there (turn 2);
    `want` = (best_id, val_no_change, iter, done) and `f_value` of RefDEHead after both turns.
    `judge`: whether std_err is held against the exact statistic for this vector (always at
    n <= 4096 and for the conditioning family; the exact sums of the rest are skipped above that)."""

    def __init__(self, name, inc, place, vec, head, judge):
        self.name, self.inc, self.place, self.vec, self.judge = name, inc, place, vec, judge
        self.want = (head.best_id, head.val_no_change, head.iter, head.done)
        self.f_value = head.f_value


_CASES = {}


def cases(n, shards=1, which=("ties", "nonfinite", "conditioning"), eps=EPS_TINY,
          best_val_no_change=10 ** 6):
    """Every family member at this size for every incumbent position, with RefDEHead's verdict;
    computed once per argument set and shared by the tests of a session."""
    import copy
    key = (n, shards, tuple(which), eps, best_val_no_change)
    if key not in _CASES:
        if len(_CASES) > 8:
            _CASES.clear()
        out = []
        for inc in incumbents(n, shards):
            place = placement(n, inc)
            placed = RefDEHead(eps=eps, best_val_no_change=best_val_no_change)
            placed.turn(place)
            assert placed.best_id == inc and not placed.done
            for name, vec in families(n, inc, shards, which=which):
                head = copy.copy(placed)
                head.turn(vec)
                judge = (n <= 4096 or name.startswith("conditioning") or
                         not std_err_precondition(vec))
                out.append(Case(name, inc, place, vec, head, judge))
        _CASES[key] = out
    return _CASES[key]
