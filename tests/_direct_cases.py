"""The case list of the direct-search rule tests (TEST INFRASTRUCTURE): shared by
tests/test_direct_rules_cpu.py (coverage conditions, goldens), tests/test_direct_rules_gpu.py (the
device runs) and tests/golden/gen_golden_hostile.py (the unmodified reference's runs).

A batch is one engine launch: a shape, a solver configuration and one (parameter row, start) per
batch row. Starts are x_i = x0 + dx i, which is also what the reference driver takes.
References are computed once per (batch, summation order) and shared (reference()).
"""
import functools
from collections import Counter, namedtuple

from tests import _direct_ref as R
from tests import _hostile as H

NAN, INF = H.NAN, H.INF

# ---- Nelder-Mead ---------------------------------------------------------------------------------
NMBatch = namedtuple("NMBatch", "name n minimize bounded upper lower step restarts eps max_iter "
                                "no_change rows source")
Row = namedtuple("Row", "family a b x0 dx")

# (family, a, b, x0, dx). With dx = 0 the vertices 1 .. n-1 of the initial simplex all score the
# same: ties from the first scan on.
NM_ROWS = [
    Row(H.PLATEAU, 0.0, 0.0, 0.3, 0.0),       # 0 ties everywhere, vertex n = x is the unique best
    Row(H.PLATEAU, 0.0, 0.0, -1.1, 0.37),     # 1
    Row(H.ZERO, 0.0, 0.0, 0.5, 0.1),          # 2 all scores equal: std_err 0 < eps... if eps > 0
    Row(H.NAN_BEYOND, 1.0, 0.0, 0.3, 0.0),    # 3 the bumped vertices are NaN, vertices 0 and n are not
    Row(H.NAN_BEYOND, 0.9, 0.0, 0.8, 0.0),    # 4 only vertex 0 (shifted down) is finite
    Row(H.ALL_NAN, 0.0, 0.0, 0.5, 0.1),       # 5 NaN at vertex 0: nothing ever compares
    Row(H.WALLS, 0.25, 0.5, 0.3, 0.45),       # 6 vertex 0 crosses the +inf wall and keeps the -inf well: NaN
    Row(H.WALLS, -0.5, 3.0, 0.3, 0.0),        # 7 finite start between a +inf wall and a -inf well
    Row(H.WALLS, 0.0, 1.0e9, 0.6, 0.0),       # 8 +inf at vertex 0 only: eps becomes inf
    Row(H.WALLS, -1.0e9, 1.1, 0.3, 0.0),      # 9 -inf at every bumped vertex: a tied -inf minimum
    Row(H.HUGE, 0.0, 0.0, 0.3, 0.0),          # 10 std_err's squares overflow
    Row(H.HUGE, 0.0, 0.0, 7.9, 0.3),          # 11 ... and its mean
    Row(H.PLATEAU, 0.0, 0.0, 0.0, 0.0),       # 12 scores[0] = 0: eps becomes 0 and never stops
    # found by search: starts from which long simplices contract outside and expand
    Row(H.PLATEAU, 0.0, 0.0, -2.01, 0.0),     # 13
    Row(H.WALLS, -1.45, 2.43, 1.16, -0.0019),  # 14
    Row(H.PLATEAU, 0.0, 0.0, 0.48, -0.0259),  # 15
    Row(H.NAN_BEYOND, 1.69, 0.0, -1.09, 0.0173),  # 16
    Row(H.NAN_BEYOND, 2.03, 0.0, -2.27, 0.0),  # 17
    Row(H.PLATEAU, 0.0, 0.0, 20.0, 0.0),      # 18 the clamped plateau: all scores equal, std_err 0 < eps
]
_SMALL = (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 15, 17)
_LARGE = (0, 2, 3, 5, 6, 8, 10, 13, 14, 15, 17, 18)
_LARGEST = (2, 5, 6, 8, 13, 14, 15, 16, 17, 18)
NM_SIZES = (1, 2, 3, 16, 63, 64, 128, 129, 257)
# kernel classes: one score per lane | a second ballot round | the third | nm_solve_kernel on the
# global workspace
NM_CLASSES = {"one_round": (1, 2, 3, 16), "two_rounds": (63, 64), "three_rounds": (128,),
              "workspace": (129, 257)}


def _nm_iters(n):
    return 60 if n <= 16 else 40 if n <= 64 else 24 if n <= 129 else 12


def _nm_rows(n):
    return [NM_ROWS[i] for i in (_SMALL if n <= 16 else _LARGE if n <= 129 else _LARGEST)]


def nm_batches():
    out = []
    for n in NM_SIZES:
        out.append(NMBatch(f"n{n}_min", n, True, False, 0.0, 0.0, -1.0, 0, 1e-3, _nm_iters(n),
                           30 if n <= 16 else 1000,
                           tuple(_nm_rows(n)), "family"))
    for n in (2, 16, 64, 129):
        out.append(NMBatch(f"n{n}_max_bounded", n, False, True, 3.0, -3.0, -1.0, 0, 1e-3, _nm_iters(n),
                           30, tuple(_nm_rows(n)), "family"))
    for n in (3, 16, 63, 128):
        out.append(NMBatch(f"n{n}_restarts_step", n, True, True, 4.0, -2.0, 0.75, 2, 1e-5,
                           _nm_iters(n) // 2, 12, tuple(_nm_rows(n)), "family"))
    # the path without a parameter row, and the whole-vector body with its signed zeros
    lit = tuple(Row(NAN, 2.25, -2.5, x0, dx) for x0, dx in
                ((0.3, 0.0), (-1.1, 0.37), (1.4, 0.0), (-2.2, 0.05), (2.0, 0.02), (0.0, 0.0), (-3.0, 0.4),
                 (1.2, -0.3)))
    out.append(NMBatch("n16_literal", 16, True, False, 0.0, 0.0, -1.0, 0, 1e-3, 60, 30, lit, "literal"))
    vec = tuple(Row(0.0, b, 0.0, x0, dx) for b, x0, dx in
                ((2.0, -0.2, 0.0), (2.0, 0.1, 0.0), (1.0, -1.3, 0.3), (8.0, 0.6, 0.1), (0.0, 0.3, 0.0),
                 (3.0, -0.05, 0.01), (2.0, 1.1, -0.2), (64.0, 0.4, 0.2)))
    for n in (3, 64):
        out.append(NMBatch(f"n{n}_vector", n, True, False, 0.0, 0.0, -1.0, 0, 1e-3, 40, 30, vec, "vector"))
    return out


def start(row, n):
    return [row.x0 + row.dx * float(i) for i in range(n)]


def objective(source, row):
    if source == "literal":
        return H.literal
    if source == "vector":
        return H.vector((row.family, row.a, row.b))
    return H.family((row.family, row.a, row.b))


@functools.lru_cache(maxsize=None)
def nm_reference(batch, tree):
    """[(Result, counts)] of a batch's rows in one summation order"""
    out = []
    for row in batch.rows:
        ref = R.RefNelderMead(objective(batch.source, row), minimize=batch.minimize,
                              upper=[batch.upper] * batch.n if batch.bounded else None,
                              lower=[batch.lower] * batch.n if batch.bounded else None,
                              step=batch.step, eps=batch.eps, max_iter=batch.max_iter,
                              no_change=batch.no_change, restarts=batch.restarts, tree=tree)
        out.append((ref.run(start(row, batch.n)), ref.counts))
    return out


def total_counts(results):
    c = Counter()
    for _, counts in results:
        c.update(counts)
    return c


def nm_golden_only():
    """even sizes that only the goldens of the unmodified reference use (CPU)"""
    rows = tuple(_nm_rows(4))
    return [NMBatch("n4_min", 4, True, False, 0.0, 0.0, -1.0, 0, 1e-3, 60, 30, rows, "family"),
            NMBatch("n8_max_bounded_restart", 8, False, True, 3.0, -3.0, -1.0, 1, 1e-5, 40, 30, rows, "family")]


def batch_by_name(name):
    return next(b for b in nm_batches() + nm_golden_only() if b.name == name)


def golden_runs():
    """the runs of the unmodified reference in tests/golden/nm_hostile.json: (batch name, row index).
    Even n only: for an odd n the reference writes out of bounds."""
    picks = []
    for b in nm_batches() + nm_golden_only():
        if b.n % 2 or b.source != "family" or b.n > 64:
            continue
        step = 2 if b.n <= 8 else 3
        picks += [(b.name, r) for r in range(len(b.name) % step, len(b.rows), step)]
    return picks


# ---- SANN ------------------------------------------------------------------------------------------
SANNBatch = namedtuple("SANNBatch", "name D minimize max_iter temp_iter temp_max seed chain_lo rows source")
SEED = 0x5EEDC0FFEE

# Neighbouring chains take different families, so the lanes of a packed wave are in different states
# when the acceptance ballot is taken.
SANN_ROWS = (
    Row(H.PLATEAU, 0.0, 0.0, 0.3, 0.0),      # near the minimum: equal and worse trials, both `<=`
    Row(H.ZERO, 0.0, 0.0, 0.5, 0.1),         # every trial equal: accepted and taken as the best
    Row(H.PLATEAU, 0.0, 0.0, 2.6, 0.01),     # downhill: better trials
    Row(H.ALL_NAN, 0.0, 0.0, 0.5, 0.1),      # NaN start: nothing is ever accepted, x untouched
    Row(H.NAN_BEYOND, 1.0, 0.0, 0.3, 0.0),   # finite start, NaN trials are rejected
    Row(H.NAN_BEYOND, 0.2, 0.0, 0.5, 0.0),   # the start is NaN
    Row(H.WALLS, 0.5, 1.0e9, 0.2, 0.0),      # +inf start: a finite trial is accepted, a +inf trial is inf - inf
    Row(H.WALLS, -1.0e9, 2.0, 0.3, 0.0),     # reaches -inf: an equal -inf later is not taken
    Row(H.WALLS, -0.5, 1.5, 0.3, 0.0),
    Row(H.HUGE, 0.0, 0.0, 0.3, 0.0),         # differences beyond 710 t
    Row(H.HUGE, 0.0, 0.0, 3.1, 0.0),
    Row(H.PLATEAU, 0.0, 0.0, -1.1, 0.37),
)
# a streamed point: x = 16.2 lies on the clamped plateau (q = 64), from which most trials are better
SANN_STREAMED = SANN_ROWS[:2] + (Row(H.PLATEAU, 0.0, 0.0, 16.2, 0.0),) + SANN_ROWS[4:10:2] + SANN_ROWS[9:10] + \
    SANN_ROWS[2:3]
# layouts: several chains per wave | the packing boundary | register-resident | streamed
SANN_CLASSES = {"packed": (1, 2, 16), "boundary": (64, 65), "resident": (130,), "streamed": (1026,)}
# t scales with temperature_max while the step size t / temperature_max does not: a longer point has
# larger differences and needs a hotter chain for its worse trials to be accepted
_SANN_TEMP = {1: 10.0, 2: 10.0, 16: 50.0, 64: 500.0, 65: 500.0, 130: 2000.0, 1026: 1.0e5}


def sann_batches():
    out = []
    for D in (1, 2, 16, 64, 65, 130, 1026):
        iters = 40 if D <= 16 else 24 if D <= 130 else 10
        rows = SANN_ROWS if D <= 130 else SANN_STREAMED
        out.append(SANNBatch(f"D{D}_min", D, True, iters, 6, _SANN_TEMP[D], SEED, 3, tuple(rows), "family"))
    for D in (2, 65):
        out.append(SANNBatch(f"D{D}_max", D, False, 30, 6, _SANN_TEMP[D], SEED + 1, 0, SANN_ROWS, "family"))
    for D in (2, 130):  # a negative temperature_max: t < 0, every worse trial is accepted (exp of a positive number)
        out.append(SANNBatch(f"D{D}_negative_t", D, True, 12, 6, -10.0, SEED + 2, 0, SANN_ROWS[:4] + SANN_ROWS[9:],
                             "family"))
    # ... and a packed wave in which no chain has a NaN difference: the ballot then rests on
    # sann_sure_reject alone
    finite = (SANN_ROWS[0], SANN_ROWS[2], SANN_ROWS[9], SANN_ROWS[11], SANN_ROWS[10], Row(H.PLATEAU, 0.0, 0.0, 1.3, 0.2),
              Row(H.PLATEAU, 0.0, 0.0, -2.2, 0.1), Row(H.HUGE, 0.0, 0.0, -1.0, 0.5))
    out.append(SANNBatch("D2_negative_t_finite", 2, True, 12, 6, -10.0, SEED + 6, 0, finite, "family"))
    # temperature_max = 0: t = 0 and the step 0 * inf is NaN, so every trial point is NaN. Constant 0 still
    # scores it 0: an equal trial, and exp(-0.0 / 0.0) is NaN -- only `difference <= 0.0` accepts it (at
    # any other temperature exp(-0 / t) = 1 accepts an equal trial too, whichever comparison is written)
    zero_t = (SANN_ROWS[1], SANN_ROWS[0], Row(H.ZERO, 0.0, 0.0, -1.5, 0.2), SANN_ROWS[3], SANN_ROWS[1], SANN_ROWS[9],
              Row(H.ZERO, 0.0, 0.0, 3.0, 0.0), SANN_ROWS[2])
    for D in (2, 130, 1026):
        out.append(SANNBatch(f"D{D}_zero_t", D, True, 4, 6, 0.0, SEED + 5, 0, zero_t, "family"))
    lit = tuple(Row(NAN, 2.25, -2.5, x0, dx) for x0, dx in
                ((0.3, 0.0), (2.1, 0.0), (-2.4, 0.0), (2.3, 0.0), (-2.6, 0.01), (0.0, 0.0), (1.0, 0.05), (-1.0, 0.1)))
    out.append(SANNBatch("D16_literal", 16, True, 40, 6, 50.0, SEED + 3, 0, lit, "literal"))
    vec = tuple(Row(0.0, b, 0.0, x0, dx) for b, x0, dx in
                ((2.0, -0.2, 0.0), (2.0, 0.1, 0.0), (1.0, -1.3, 0.3), (8.0, 0.6, 0.1), (0.0, 0.3, 0.0),
                 (3.0, -0.05, 0.01), (2.0, 1.1, -0.2), (64.0, 0.4, 0.2)))
    for D in (3, 130):
        out.append(SANNBatch(f"D{D}_vector", D, True, 30, 6, 10.0, SEED + 4, 0, vec, "vector"))
    return out


_PRIMS = []


def prims():
    if not _PRIMS:
        from tests import _oracle as O
        _PRIMS.append(R.Prims(O.load()))
    return _PRIMS[0]


@functools.lru_cache(maxsize=None)
def sann_reference(batch):
    out = []
    for c, row in enumerate(batch.rows):
        ref = R.RefSANN(objective(batch.source, row), prims(), seed=batch.seed, chain=batch.chain_lo + c,
                        minimize=batch.minimize, max_iter=batch.max_iter, temp_iter=batch.temp_iter,
                        temp_max=batch.temp_max)
        out.append((ref.run(start(row, batch.D)), ref.counts))
    return out


# ---- the NM / PSO hybrid -----------------------------------------------------------------------------
HybBatch = namedtuple("HybBatch", "name n minimize bounded upper lower eps max_iter no_change seed inst_lo "
                                  "rows source")
HYB_ROWS = (
    Row(H.PLATEAU, 0.0, 0.0, 0.3, 0.0),      # tied keys in the simplex ranks from the first sort on
    Row(H.PLATEAU, 0.0, 0.0, -1.1, 0.37),
    Row(H.ZERO, 0.0, 0.0, 0.5, 0.1),         # every key equal: the sort must keep the order; std_err 0 stops
    Row(H.NAN_BEYOND, 1.0, 0.0, 0.3, 0.0),   # NaN keys among finite ones
    Row(H.ALL_NAN, 0.0, 0.0, 0.5, 0.1),      # the first particle's value is NaN: H2 can never count
    Row(H.WALLS, 0.25, 0.5, 0.3, 0.45),      # the first particle is NaN (+inf and -inf), the others are not
    Row(H.WALLS, -0.5, 3.0, 0.3, 0.0),
    Row(H.WALLS, -1.0e9, 1.1, 0.3, 0.0),     # tied -inf keys
    Row(H.HUGE, 0.0, 0.0, 0.3, 0.0),
    Row(H.PLATEAU, 0.0, 0.0, 0.0, 0.0),      # x = 0: the unbounded overloads derive the bounds [-0, 0]
    Row(H.NAN_BEYOND, 2.03, 0.0, -2.27, 0.0),
    Row(H.PLATEAU, 0.0, 0.0, 2.6, -0.21),
)
# found by search: starts near 0 (the unbounded overloads then draw the PSO particles within +-2.5 |x|, a
# few plateau steps) from which a long simplex contracts outside within its first iterations
HYB_OUTSIDE = (
    Row(H.PLATEAU, 0.0, 0.0, -0.231, 0.0),
    Row(H.NAN_BEYOND, 2.99, 0.0, -0.224, 0.0),
    Row(H.HUGE, 0.0, 0.0, 0.064, 0.0),
    Row(H.PLATEAU, 0.0, 0.0, -0.025, 0.0013),
)
HYB_CLASSES = {"thread_per_particle": (2, 3, 8, 33, 64, 128), "wave_per_particle": (129, 200)}


def _hyb_shape(n):
    """(rows, iterations): a reference run draws 8 n^2 uniforms per iteration"""
    if n <= 8:
        return HYB_ROWS, 40
    if n <= 33:
        return HYB_ROWS, 16
    if n <= 64:
        return HYB_ROWS[:9], 8
    if n <= 129:
        return HYB_ROWS[:8] + HYB_OUTSIDE[:2], 4
    return HYB_ROWS[:8:2] + HYB_ROWS[5:8:2] + HYB_OUTSIDE[2:], 3


def hyb_batches():
    out = []
    for n in (2, 3, 8, 33, 64, 128, 129, 200):
        rows, iters = _hyb_shape(n)
        out.append(HybBatch(f"n{n}_min", n, True, False, 0.0, 0.0, 1e-3, iters, 20, SEED + 10, 5, tuple(rows),
                            "family"))
    for n in (3, 33, 129):
        rows, iters = _hyb_shape(n)
        out.append(HybBatch(f"n{n}_max_bounded", n, False, True, 3.0, -3.0, 1e-3, iters, 20, SEED + 11, 0,
                            tuple(rows), "family"))
    lit = tuple(Row(NAN, 2.25, -2.5, x0, dx) for x0, dx in
                ((0.3, 0.0), (-1.1, 0.37), (1.4, 0.0), (-2.2, 0.05), (2.0, 0.02), (0.0, 0.0), (-3.0, 0.4),
                 (1.2, -0.3)))
    out.append(HybBatch("n8_literal", 8, True, False, 0.0, 0.0, 1e-3, 40, 20, SEED + 12, 0, lit, "literal"))
    # -0.0 at the first particle (x(0) < 0) against +0.0 elsewhere: H2 compares them with ==
    vec = tuple(Row(0.0, b, 0.0, x0, dx) for b, x0, dx in
                ((64.0, 0.1, 0.0), (64.0, 0.05, 0.0), (64.0, 0.2, 0.0), (8.0, 0.6, 0.1), (0.0, 0.3, 0.0),
                 (3.0, -0.05, 0.01), (2.0, 1.1, -0.2), (64.0, -1.0, 0.7)))
    for n, mini in ((3, True), (8, False)):
        out.append(HybBatch(f"n{n}_vector", n, mini, False, 0.0, 0.0, 1e-3, 40, 20, SEED + 13, 0, vec, "vector"))
    return out


@functools.lru_cache(maxsize=None)
def hyb_reference(batch):
    out = []
    for b, row in enumerate(batch.rows):
        ref = R.RefHybrid(objective(batch.source, row), prims(), seed=batch.seed, instance=batch.inst_lo + b,
                          minimize=batch.minimize,
                          upper=[batch.upper] * batch.n if batch.bounded else None,
                          lower=[batch.lower] * batch.n if batch.bounded else None,
                          eps=batch.eps, max_iter=batch.max_iter, no_change=batch.no_change)
        res = ref.run(start(row, batch.n))
        res.first_value = ref.first_value  # the first particle's initial value (H2 compares with it)
        out.append((res, ref.counts))
    return out
