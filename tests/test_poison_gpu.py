"""Every engine family against its oracle on poisoned device memory, and a second solve on a used
engine against a fresh engine's.

The pool (nlsolver_amd/csrc/nlsg_pool.h) promises nothing about what a block holds, and a fresh
hipMalloc in a fresh process reads as zero, which is usually the harmless value: a kernel that reads
a padding column, a tail row, a counter or a done flag it never wrote passes every parity test and
fails in a long-lived process. Here each family runs once in a child process whose pool fills every
block it hands out, fresh or recycled, with one byte (NLSG_POOL_POISON):

  1     0xFF bytes: NaN as a double, -1 / 2^32 - 1 / 2^64 - 1 as an integer;
  0xC0  the finite double -8577.5019..., which wins every min-scan over honest scores of Rosenbrock,
        sphere or Rastrigin (NaN is invisible to `v < best`, fmin and `err < eps`), and a negative
        int32.

A child asserts first that the byte is in force (nlsg_pool_poison()), then runs the family's cases
once each -- the shapes are the smallest at which each kernel and each padding rule is live, not the
benchmark's -- and compares with the oracle exactly as the named parity test does: the cases CALL
those tests' own bodies and helpers with these shapes. The first failed assertion ends the child.

The reuse tests are the same class of bug seen from the other side: the stale contents are the
engine's own (done flags, n_done, best_x, val_no_change, LM's lambda, the simplex, a chain's state).
Problem A is solved to its stop, then problem B on the same engine: B's points, statuses and every
downloadable state equal, bit for bit, those of a fresh engine that solved only B. No engine documents
that it cannot be re-run, so none asserts an error instead. They run in this process and once more
inside a poisoned child.

Wall time of each child on an MI355X (python start-up, library load, run-time compilations and the
CPU oracle included), measured once, pattern 1 / pattern 0xC0, in seconds: batches 4.7 / 2.2,
bfgs 2.3 / 2.2, de_ref 0.5 / 0.6, de_turns 2.3 / 2.4, lm_narrow 0.6 / 0.6, lm_wide 9.5 / 3.7,
nm 4.2 / 2.6, nmpso 4.6 / 2.2, pso_turns 2.3 / 2.4, sann 0.6 / 0.6, tinyqr 0.6 / 0.5, the reuse child
8.0 / 2.4 (the first child of a family pays the run-time compilations that the second finds cached).
None is near 20 s.
de_turns and pso_turns start with `import torch`: their sharded cases borrow its stream, and loaded
after this library it finds no device.

That a child can fail was shown once on scratch builds of the library (the pool's
paragraph): LM's memset of Hg and BFGS's of dir initialise bytes that are loaded but never used, so
removing them changes nothing under either pattern; removing BFGS's memset of its zero word (what
padded lanes load) fails the bfgs child in its first case under both patterns, and without poison only
in its last case, on a recycled block.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import _oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 12374563468
PATTERNS = {"1": 0xFF, "0xC0": 0xC0}

# ---- helpers -----------------------------------------------------------------------------------------
def _same(a, b):
    """equal bit for bit (NaNs by their bits); None only equals None"""
    if a is None or b is None:
        return a is None and b is None
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype == np.float64:
        a, b = a.view(np.uint64), b.view(np.uint64)
    return np.array_equal(a, b)


def _status(st):
    """every field of a Status, the doubles as their bit patterns"""
    out = []
    for name, _ in type(st)._fields_:
        v = getattr(st, name)
        out.append(int(np.float64(v).view(np.uint64)) if isinstance(v, float) else int(v))
    return tuple(out)


# ---- the families ------------------------------------------------------------------------------------
def family_de_turns(m, oracle):
    """D 24: several agents per wave; 65: a wave per agent, odd rows, scalar loads; 1026: rows streamed
    in segments. pop 70: no multiple of the tile, the wave or the agents per wave."""
    from tests.test_de_home_gpu import accepting_generations, shards_on_one_gpu
    # (accepted > 0: rows moved to the other buffer, so both `home` parities were read)
    for D, CR in ((24, 0.2), (65, 0.2), (1026, 0.01)):
        assert accepting_generations(m, oracle, 70, D, 0, CR) > 0               # best
        assert accepting_generations(m, oracle, 70, D, 1, CR) > 0               # random, head and generation apart
        assert accepting_generations(m, oracle, 70, D, 1, CR, trace=False) > 0  # random, the fused turn (D <= 1024)
    assert accepting_generations(m, oracle, 70, 24, 1, 0.2, minimize=False, trace=False) > 0
    shards_on_one_gpu(m, oracle, 2, 35, 24, 1)
    shards_on_one_gpu(m, oracle, 2, 35, 24, 0)


def family_pso_turns(m, oracle):
    from tests import test_pso_gpu as T
    for type_ in (O.PSO_ACCELERATED, O.PSO_VANILLA):
        for bounded in (False, True):
            T.test_pso_turns_bit_exact(m, oracle, 70, 24, type_, bounded)
            T.test_pso_turns_bit_exact(m, oracle, 70, 65, type_, bounded)
            T.test_pso_particles_longer_than_1024_coordinates_bit_exact(m, oracle, 70, 1026, type_, bounded)
    T.test_pso_sharded_path_on_one_gpu_bit_exact(m, oracle, O.PSO_ACCELERATED, 0.0, 24)


def family_de_ref(m, oracle):
    """(40, 8): population, scores and trial in LDS. (70, 117): 80 008 bytes, just past the 78 KiB
    budget (70 x 116 still fits): agents and the trial row in memory, scores in LDS. (8400, 2): the
    (pop + 8)-long score rows in memory too (past 8368 agents they alone exceed the budget)."""
    from nlsolver_amd import DE_BEST, DE_RANDOM
    from tests.test_de_ref_gpu import shape_case
    for pop, D, batch, gens, strategy, minimize in ((40, 8, 2, 5, DE_RANDOM, True), (40, 8, 2, 5, DE_BEST, False),
                                                   (70, 117, 2, 3, DE_RANDOM, True), (70, 117, 2, 3, DE_BEST, True),
                                                   (8400, 2, 1, 1, DE_RANDOM, True)):
        shape_case(oracle, np.random.default_rng(pop * 10007 + D), "rosenbrock", pop, D, gens, strategy, minimize,
                   batch=batch, log=True)


def family_batches(m, oracle):
    """the resident batch engines: batch 3, per-solve seeds (and bounds, PSO), pop 5 and 40, D 2 and 17"""
    from tests import test_batch_params_gpu as BP
    from tests import test_de_batch_gpu as DB
    from tests import test_pso_batch_gpu as PB
    for strategy in (0, 1):
        kw = dict(strategy=strategy, CR=0.2, F=0.5, eps=0.0, max_iter=1000, best_val_no_change=1000)
        for pop, D in ((5, 2), (40, 17), (5, 17), (40, 2)):
            DB.follow_restatement(m, oracle, "rosenbrock", pop, D, 3, 4, x0=DB.x0_for(D), kw=kw,
                                  label=f"pop {pop} D {D}")
    for type_ in PB.TYPES:
        for n, D in ((5, 2), (40, 17), (5, 17), (40, 2)):
            PB.test_turns_follow_the_restatement(m, oracle, n, D, type_)
    with BP.engines(m) as get:
        BP.assert_matches_baked(get, "de", "terms", 8, 2, (), BP.rows_for("terms", 2))
        BP.assert_matches_baked(get, "pso", "terms", 12, 9, (("type", 1), ("bounded", True)),
                                BP.rows_for("terms", 9))


def family_nm(m, oracle):
    """n 2; 128: the largest simplex in LDS; 130: the global workspace. Tree and reference order."""
    from tests import test_nm_params_gpu as NP
    from tests.test_nm_gpu import nm_bit_exact_case
    from tests.test_reference_order_gpu import test_nm_reference_order_batches_equal_the_serial_oracle as ref_order
    for n, batch in ((2, 3), (128, 2), (130, 2)):
        nm_bit_exact_case(m, oracle, n, batch, dict(max_iter=60, eps=0.0, no_change_best_tol=100000))
        nm_bit_exact_case(m, oracle, n, batch, dict(max_iter=40, eps=1e-6, no_change_best_tol=20, step=0.4,
                                                    restarts=1))
        ref_order(m, oracle, "rosenbrock", n, batch)
    with NP.engines(m) as get:
        NP.assert_matches_baked(get, "nm", "chain", 9, NP.nm_extra(NP.TREE, 40), NP.rows_for("chain", 9))


def family_nmpso(m, oracle):
    from tests import test_nm_params_gpu as NP
    from tests.test_nmpso_gpu import check, starts
    check(m, oracle, "rosenbrock", 2, 3, starts(3, 2, 0.5, 1.0), max_iter=1000, eps=1e-6, no_change_best_iter=20)
    check(m, oracle, "rosenbrock", 32, 2, starts(2, 32, 0.5, 1.0), bounds=(np.full(32, -1.5), np.full(32, 2.5)),
          max_iter=30, eps=0.0, no_change_best_iter=1000)
    check(m, oracle, "rosenbrock", 130, 2, starts(2, 130, 0.5, 1.0), max_iter=8, eps=0.0, no_change_best_iter=1000)
    check(m, oracle, "sphere", 130, 2, starts(2, 130, 0.5, 1.0), bounds=(np.full(130, -1.5), np.full(130, 2.5)),
          max_iter=8, eps=0.0, no_change_best_iter=1000)
    with NP.engines(m) as get:
        NP.assert_matches_baked(get, "hyb", "chain", 9, NP.hyb_extra(30, bounded=True), NP.rows_for("chain", 9))


def family_sann(m, oracle):
    from tests.test_sann_gpu import test_sann_chains_bit_exact_vs_sync_oracle as chains
    for n, iters in ((1, 10), (8, 60), (127, 20), (130, 20), (1026, 6)):
        chains(m, oracle, "rosenbrock", n, dict(max_iter=iters, temperature_iter=5, temperature_max=10.0), True)
    chains(m, oracle, "rosenbrock", 8, dict(max_iter=60, temperature_iter=5, temperature_max=10.0), False)


def family_bfgs(m, oracle):
    """each order once with the inverse Hessian downloaded and compared; reference order at n = 130
    (rows n apart) and n = 512 (rows n + 16 apart)"""
    from tests import test_bfgs_gpu as T
    from tests import test_lm_bfgs_params_gpu as LP
    from tests import test_reference_order_gpu as R
    T.test_bfgs_batch_bit_exact_vs_tree_oracle(m, oracle, 96, 3, dict(max_iter=7, grad_eps=0.0, alpha=0.5))
    T.test_bfgs_inverse_hessian_and_gradient_after_k_iterations(m, oracle)  # tree order, n = 96
    T.test_bfgs_symmetric_bit_exact_vs_oracle(m, oracle, 130, 3, dict(max_iter=7, grad_eps=0.0, alpha=0.5))
    T.test_bfgs_symmetric_inverse_hessian_bit_exact_and_symmetric(m, oracle, 130)
    R.test_bfgs_reference_order_inverse_hessian_bit_exact(m, oracle, 130)
    R.test_bfgs_reference_order_inverse_hessian_bit_exact(m, oracle, 512)
    kw = dict(max_iter=6, grad_eps=0.0, alpha=1.0)
    T.test_bfgs_default_finite_difference_gradient_bit_exact(m, oracle, "rosenbrock", 8, 3, kw)
    T.test_bfgs_finite_difference_gradient_past_256_dimensions(m, oracle, "rosenbrock", 257, 2)
    R.test_bfgs_reference_order_batches_equal_the_serial_oracle(m, oracle, "rosenbrock", 8, 3)
    R.test_bfgs_reference_order_batches_equal_the_serial_oracle(m, oracle, "rosenbrock", 257, 2)
    with LP.engines(m) as get:
        LP.assert_matches_baked(get, "bfgs", "chain", 9, 6, LP.extra_of(max_iter=20, ref=False),
                                LP.rows_for("chain", 9, 6), which=[1])


def family_lm_narrow(m, oracle):
    """(40, 9): padded rows and columns of the repacked A; (64, 64): none. Both solvers; the default
    functors in both orders."""
    from tests import test_lm_gpu as T
    from tests import test_reference_order_gpu as R
    kw = dict(lam=10.0, max_iter=12, f_delta=0.0)
    for mm, n in ((40, 9), (64, 64)):
        T.test_lm_batch_bit_exact_vs_kernel_order_oracle(m, oracle, mm, n, 3, kw)
        T.test_lm_qr_solver_bit_exact_vs_kernel_order_oracle(m, oracle, mm, n, 3, kw)
    fd = dict(lam=1.0, up=4.0, down=3.0, max_iter=5, f_delta=0.0)
    T.test_lm_default_functors_bit_exact_vs_oracle(m, oracle, "rosenbrock", 2, 2.0, fd)
    T.test_lm_default_functors_bit_exact_vs_oracle(m, oracle, "rosenbrock", 16, 1.0, fd)
    R.test_lm_reference_order_batches_equal_the_serial_oracle(m, oracle, "rosenbrock", 2, 3)
    R.test_lm_reference_order_batches_equal_the_serial_oracle(m, oracle, "rosenbrock", 16, 3)


def family_lm_wide(m, oracle):
    """(80, 65) and (150, 129): the one-pass kernels up to 128 and 256 parameters; (130, 257): the
    128 x 128 super-blocks, the smallest n > 256 that tests/test_lm_wide_gpu.py reaches. The default
    functors at 65 and 130 in both orders (max_iter 2)."""
    from tests import test_lm_bfgs_params_gpu as LP
    from tests import test_lm_wide_gpu as T
    from tests import test_reference_order_gpu as R
    kw = dict(lam=10.0, max_iter=8, f_delta=0.0)
    for mm, n, batch in ((80, 65, 3), (150, 129, 2), (130, 257, 2)):
        T.test_lm_wide_tanh_bit_exact_vs_kernel_order_oracle(m, oracle, mm, n, batch, kw)
    for n in (65, 130):
        T.test_lm_wide_default_functors_bit_exact_vs_oracle(m, oracle, "rosenbrock", n, 1.0)
        R.test_lm_reference_order_batches_equal_the_serial_oracle(m, oracle, "rosenbrock", n, 2)
    with LP.engines(m) as get:
        LP.assert_matches_baked(get, "lm", "chain", 65, LP.LM_B, LP.extra_of(max_iter=8, ref=False),
                                LP.rows_for("chain", 65, LP.LM_B), which=[1])


def family_tinyqr(m, oracle):
    from tests import test_tinyqr_gpu as T
    tq = m.tinyqr
    for n, p in ((1, 1), (7, 7), (65, 64), (130, 63)):
        T.test_random_batches_bit_exact(tq, oracle, n, p, 3)
    # qr_decomposition with its work / Q / R buffers, and (p <= 64) lm(reference_order=True)
    for n, p in ((64, 64), (100, 70), (40, 9)):
        T.test_reference_order_batches_vs_literal_oracle(tq, oracle, n, p, 3)


# ---- a second solve on a used engine -------------------------------------------------------------------
def _second_equals_fresh(make, solve, A, B):
    """solve(engine, inputs) -> list of arrays, None and lists of status tuples: everything the solve
    hands back. A to its stop, then B on the same engine; a fresh engine solves only B."""
    with make() as eng:
        first = solve(eng, A)
        got = solve(eng, B)
    with make() as fresh:
        want = solve(fresh, B)
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert (g == w) if isinstance(g, list) else _same(g, w), f"result {k} of the second solve"
    assert not _same(first[0], got[0])  # (A was another problem)


def _stopped(sts):
    """every solve of the call ran to its stop (the engines' minimize returns only then and says so in
    Status.done) and did iterate"""
    assert all(s.done == 1 for s in sts), [s.done for s in sts]
    return [_status(s) for s in sts]


def reuse_de(m):
    def solve(eng, x0):
        x = np.array(x0, dtype=np.float64)
        st = eng.minimize(x, poll_every=5)
        assert st.done == 1
        P, S = eng.download()
        bx, bf, bi = eng.best()
        return [x, [_status(st)], P, S, bx, np.float64(bf), np.int64(bi)]
    for strategy in (0, 1):
        _second_equals_fresh(lambda: m.DEEngine("rosenbrock", 40, 2, strategy=strategy, eps=10e-4, max_iter=1000,
                                                best_val_no_change=50), solve, [5.0, 7.0], [-3.0, 2.5])


def reuse_pso(m):
    def solve(eng, bounds):
        x = np.zeros(2)
        st = eng.minimize(x, *bounds, poll_every=7)
        assert st.done == 1
        bx, bf, bi = eng.best()
        return [x, [_status(st)], *eng.download(), bx, np.float64(bf), np.int64(bi)]
    for type_ in (O.PSO_ACCELERATED, O.PSO_VANILLA):
        _second_equals_fresh(lambda: m.PSOEngine("rosenbrock", 10, 2, type=type_, eps=10e-4, max_iter=300,
                                                 best_val_no_change=50), solve, (-3.0, 3.0), (-2.0, 4.5))


def reuse_de_ref(m):
    def solve(eng, inputs):
        x, sts, states = eng.minimize(*inputs)
        assert all(s.done == 1 for s in sts)
        out = [x, [_status(s) for s in sts], np.asarray(states)]
        for b in range(2):
            lx, lf, n = eng.log(b)
            out += [lx, lf, np.int64(n)]
        return out
    A = (np.array([[5.0, 7.0], [2.0, 7.0]]), [(11, 22), (33, 44)])
    B = (np.array([[-3.0, 2.5], [4.0, -1.0]]), [(55, 66), (77, 88)])
    _second_equals_fresh(lambda: m.DERefEngine("rosenbrock", 2, 40, 2, log_capacity=100), solve, A, B)


def reuse_de_batch(m):
    from tests.test_de_batch_gpu import seeds_for

    def solve(eng, inputs):
        x, sts = eng.minimize(*inputs)
        assert all(s.done == 1 for s in sts)
        out = [x, [_status(s) for s in sts], *eng.best()]
        for b in range(3):
            out += list(eng.download(b))
        return out
    A = (np.tile([5.0, 7.0], (3, 1)), seeds_for(3))
    B = (np.array([[-3.0, 2.5], [4.0, -1.0], [0.5, 0.5]]), [s + 1 for s in seeds_for(3)])
    _second_equals_fresh(lambda: m.DEBatchEngine("rosenbrock", 3, 40, 2, eps=10e-4), solve, A, B)


def reuse_pso_batch(m):
    from tests.test_pso_batch_gpu import TYPES, bounds_for, seeds_for

    def solve(eng, inputs):
        x, sts = eng.minimize(*inputs)
        assert all(s.done == 1 for s in sts)
        out = [x, [_status(s) for s in sts], *eng.best()]
        for b in range(3):
            out += list(eng.download(b))
        return out
    lo, hi = bounds_for(3, 2)
    A = (lo, hi, seeds_for(3))
    B = (1.5 * lo, 0.75 * hi, [s + 1 for s in seeds_for(3)])
    for type_ in TYPES:
        _second_equals_fresh(lambda: m.PSOBatchEngine("rosenbrock", 3, 10, 2, type=type_, bounded=True, eps=10e-4,
                                                      max_iter=300, best_val_no_change=50), solve, A, B)


def reuse_batch_params(m):
    """the two batch engines with parameter rows: B brings other rows as well"""
    from tests import test_batch_params_gpu as BP

    def solve(eng, inputs):
        *args, rows = inputs
        x, sts = eng.minimize(*args, params=rows)
        return [x, _stopped(sts), *eng.best()]
    for kind, cls, args in (("de", m.DEBatchEngine, BP.DE_ARGS), ("pso", m.PSOBatchEngine, BP.PSO_ARGS)):
        A = (*BP.inputs(kind, 9, 0), BP.rows_for("chain", 9, 0))
        B = (*BP.inputs(kind, 9, 1), BP.rows_for("chain", 9, 1))
        B = (0.75 * B[0], *B[1:])
        _second_equals_fresh(lambda: cls(BP.objective(m, "chain", 9), BP.B, 12, 9, **args), solve, A, B)


def reuse_nm(m):
    from tests.test_nm_gpu import starts

    def solve(eng, x0):
        x, sts, eps = eng.minimize(x0.copy())
        assert all(0 < s.iteration <= 60 for s in sts) or eng.cfg.restarts
        return [x, _stopped(sts), eps]
    for kw in (dict(), dict(reference_order=True), dict(step=0.4, restarts=1)):
        for n in (4, 130):
            _second_equals_fresh(lambda: m.NMEngine("rosenbrock", 3, n, max_iter=60, eps=1e-6, no_change_best_tol=20,
                                                    **kw), solve, starts(3, n, seed=n), starts(3, n, seed=n + 1) * 0.9)


def reuse_nmpso(m):
    from tests.test_nmpso_gpu import starts

    def solve(eng, x0):
        x, sts = eng.minimize(x0)
        assert all(s.iteration > 0 for s in sts)
        return [x, _stopped(sts)]
    for n in (4, 130):
        _second_equals_fresh(lambda: m.NMPSOEngine("rosenbrock", 3, n, seed=SEED, max_iter=30, eps=1e-6,
                                                   no_change_best_iter=20), solve,
                             starts(3, n, 0.5, 1.0), starts(3, n, 0.3, 1.5, seed=1))


def reuse_nm_params(m):
    """Nelder-Mead and the hybrid with parameter rows: B brings other rows as well"""
    from tests import test_nm_params_gpu as NP

    def solve(eng, inputs):
        x0, rows = inputs
        out = eng.minimize(x0.copy(), None, None, params=rows)
        assert all(s.iteration > 0 for s in out[1])
        return [out[0], _stopped(out[1])]
    A = (NP.x0_for(9), NP.rows_for("chain", 9, 0))
    B = (0.75 * NP.x0_for(9), NP.rows_for("chain", 9, 1))
    _second_equals_fresh(lambda: m.NMEngine(NP.objective(m, "chain", 9), NP.B, 9, max_iter=40), solve, A, B)
    _second_equals_fresh(lambda: m.NMPSOEngine(NP.objective(m, "chain", 9), NP.B, 9, seed=SEED, max_iter=30),
                         solve, A, B)


def reuse_sann(m):
    from tests.test_sann_gpu import starts

    def solve(eng, x0):
        x, sts = eng.minimize(x0)
        assert all(s.iteration == eng.cfg.max_iter for s in sts)  # (the schedule ran out: SANN's only stop)
        return [x, _stopped(sts)]
    for n in (8, 1026):
        _second_equals_fresh(lambda: m.SANNEngine("rosenbrock", 3, n, max_iter=40 if n == 8 else 6,
                                                  temperature_iter=5, seed=SEED), solve,
                             starts(3, n, 0.5, 1.0), starts(3, n, 0.3, 1.5, seed=1))


def reuse_bfgs(m):
    from tests.test_bfgs_gpu import starts

    def solve(eng, x0):
        x, sts = eng.minimize(x0.copy())
        assert all(s.done == 1 for s in sts)
        g, H = eng.download_state()
        return [x, [_status(s) for s in sts], g, H]
    n = 96
    d, b, c = O.quad_problem(n)
    for kw in (dict(), dict(symmetric=True), dict(reference_order=True)):
        _second_equals_fresh(lambda: m.BFGSEngine(m.QuadDiagRank1(d, b, c), 3, max_iter=100, grad_eps=1e-8, **kw),
                             solve, starts(3, n, seed=1), 1.5 * starts(3, n, seed=2))
    rng = np.random.default_rng(8)
    for ref in (False, True):  # the default finite-difference gradient
        _second_equals_fresh(lambda: m.BFGSEngine("rosenbrock", 3, dim=8, max_iter=40, grad_eps=5e-3,
                                                  reference_order=ref), solve,
                             0.8 + 0.4 * (rng.random((3, 8)) - 0.5), 0.5 + 0.4 * (rng.random((3, 8)) - 0.5))


def reuse_lm(m):
    from nlsolver_amd import _capi
    from tests.test_lm_gpu import problems
    oracle = O.load()

    def solve(eng, t0):
        th, sts, lam = eng.minimize(t0.copy())
        assert all(s.done == 1 for s in sts)
        return [th, [_status(s) for s in sts], lam]
    for mm, n, solver in ((40, 9, _capi.LM_CHOLESKY), (40, 9, _capi.LM_QR), (80, 65, _capi.LM_CHOLESKY)):
        A, y, t0 = problems(oracle, 0, 3, mm, n)
        _second_equals_fresh(lambda: m.LMEngine(m.TanhRegression(A, y), solver=solver, lam=10.0, max_iter=100,
                                                f_delta=1e-12), solve, t0, 0.5 * t0 + 0.05)
    for n, solver in ((9, _capi.LM_CHOLESKY), (9, _capi.LM_CHOLESKY_REFERENCE_ORDER), (65, _capi.LM_CHOLESKY)):
        rng = np.random.default_rng(500 + n)  # (starts near the minimum: further out these short runs end in NaN)
        A, B = 0.9 + 0.2 * (rng.random((2, n)) - 0.5), 1.0 + 0.3 * (rng.random((2, n)) - 0.5)
        _second_equals_fresh(lambda: m.LMEngine("rosenbrock", batch=2, n=n, solver=solver, lam=10.0,
                                                   max_iter=3 if n < 64 else 2, f_delta=0.0), solve, A, B)


def _reuse_lm_or_bfgs_params(m, kind, batch, extra):
    """B brings other parameter rows as well as other starts"""
    from tests import test_lm_bfgs_params_gpu as LP

    def solve(eng, inputs):
        x0, rows = inputs
        x, sts, lam = LP.solve(eng, kind, x0, rows)
        return [x, _stopped(sts), lam]
    A = (LP.x0_for(9, batch), LP.rows_for("chain", 9, batch, 0))
    B = (0.75 * LP.x0_for(9, batch), LP.rows_for("chain", 9, batch, 1))
    _second_equals_fresh(lambda: LP.make_engine(m, kind, LP.objective(m, "chain", 9), batch, 9, extra), solve, A, B)


def reuse_lm_params(m):
    from tests import test_lm_bfgs_params_gpu as LP
    _reuse_lm_or_bfgs_params(m, "lm", LP.LM_B, LP.extra_of(max_iter=8, ref=False))


def reuse_bfgs_params(m):
    from tests import test_lm_bfgs_params_gpu as LP
    _reuse_lm_or_bfgs_params(m, "bfgs", 6, LP.extra_of(max_iter=20, ref=False))


FAMILIES = {
    "de_turns": family_de_turns, "pso_turns": family_pso_turns, "de_ref": family_de_ref,
    "batches": family_batches, "nm": family_nm, "nmpso": family_nmpso, "sann": family_sann,
    "bfgs": family_bfgs, "lm_narrow": family_lm_narrow, "lm_wide": family_lm_wide, "tinyqr": family_tinyqr,
}
REUSE = {
    "de": reuse_de, "pso": reuse_pso, "de_ref": reuse_de_ref, "de_batch": reuse_de_batch,
    "pso_batch": reuse_pso_batch, "batch_params": reuse_batch_params, "nm": reuse_nm, "nmpso": reuse_nmpso,
    "nm_params": reuse_nm_params, "sann": reuse_sann, "bfgs": reuse_bfgs, "lm": reuse_lm,
    "lm_params": reuse_lm_params, "bfgs_params": reuse_bfgs_params,
}


def family_reuse(m, oracle):
    for name in REUSE:
        REUSE[name](m)


# ---- the tests ---------------------------------------------------------------------------------------
# (torch first where a case borrows torch's stream: loaded after this library it finds no device)
TORCH_FIRST = {"family_de_turns", "family_pso_turns"}
CHILD_SCRIPT = r"""
import sys
sys.path.insert(0, %(root)r)
%(prelude)s
from nlsolver_amd import _capi
assert _capi.lib().nlsg_pool_poison() == %(byte)d, ("poison byte in force", _capi.lib().nlsg_pool_poison())
import nlsolver_amd
from tests import _oracle as O
from tests import test_poison_gpu as T
T.%(function)s(nlsolver_amd, O.load())
print("poison-ok %(function)s %(byte)d")
"""


def child_script(function, byte):
    prelude = "import torch\nassert torch.cuda.is_available()" if function in TORCH_FIRST else ""
    return CHILD_SCRIPT % dict(root=ROOT, byte=byte, function=function, prelude=prelude)


def run_child(function, pattern):
    byte = PATTERNS[pattern]
    env = dict(os.environ, NLSG_POOL_POISON=pattern)
    script = child_script(function, byte)
    r = subprocess.run([sys.executable, "-c", script], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and f"poison-ok {function} {byte}" in r.stdout, r.stderr[-3000:]


@pytest.mark.parametrize("pattern", sorted(PATTERNS))
@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_family_equals_its_oracle_on_poisoned_blocks(family, pattern):
    run_child(FAMILIES[family].__name__, pattern)


@pytest.mark.parametrize("engine", sorted(REUSE))
def test_second_solve_equals_a_fresh_engines(engine):
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    import nlsolver_amd
    REUSE[engine](nlsolver_amd)


@pytest.mark.parametrize("pattern", sorted(PATTERNS))
def test_second_solve_equals_a_fresh_engines_on_poisoned_blocks(pattern):
    run_child("family_reuse", pattern)
