"""Launch routes no other test runs against the oracle.

A route is what the host picks a kernel instantiation by (nlsg_dispatch.h): engine x objective x
width class x PSO type, or BFGS model. COVERED lists, per engine and objective, the widths at which
the engine's own test files compare a run with the oracle bit for bit (the parametrisations of
test_generations_bit_exact, test_randomised_configuration_sweep_bit_exact,
test_rows_longer_than_1024_coordinates_bit_exact, test_packing_does_not_change_the_history and their
PSO, SANN, NM, hybrid, BFGS, LM and resident-batch counterparts, read off their ids). The cases below
are the cells of objective x widths whose route none of those widths takes: one engine each at its
smallest population or batch, two turns, rows and scores bit for bit.

What a route reaches, engine by engine (engines are made with their defaults, no A/B switch set):

* DE, PSO, SANN (packed_route). D <= 64: the *_groups_kernel<O, G> (PSO: <O, G, T>) with G = 4, 8, 16, 32
  lanes per row. 65 .. 1024: de_generation_kernel / de_turn_kernel<O, C, V, B, S>, pso_move_kernel<O, C,
  V, T>, sann_anneal_kernel<O, C, V> by chunks C and alignment V (B and S follow from O and C). Past
  1024: the *_long_kernel<O, V>. DE runs both strategies: `best` the generation family, `random` the
  fused-turn family.
* NM (chunk_route). Class 1 (D <= 128) is nm_solve_driver_kernel<O> (the driver serves these widths
  unless NLSG_NM_DRIVER=0; nm_solve_kernel<O, 1> is reached only with that switch and has its own test,
  test_nm_phase_per_barrier_kernel_bit_exact). Classes 2, 4, 8 are nm_solve_kernel<O, C>. Reference
  order (flag NLSG_NM_REFERENCE_ORDER) is a second dimension at D <= 128 only, driver<O, true> for the
  three objectives that admit it: test_nm_reference_order_batches_equal_the_serial_oracle runs all
  three (Rosenbrock 3 and 100, sphere 17, Styblinski-Tang 64), so that dimension has no empty cell;
  past 128 the order is a run-time field of the same instantiation.
* Hybrid (chunk_route). Class 1 is nmpso_solve_kernel<O>, classes 2, 4, 8 nmpso_solve_wide_kernel<O, C>.
* BFGS (aligned_route). BFGSEngine takes the resident kernel only when asked (resident=True), so these
  cases run bfgs_init_kernel / bfgs_search_kernel<C, V, M> and bfgs_hy_kernel / bfgs_update_kernel<C, V>.
  Reference order is a run-time field of the same instantiations. The resident kernel
  bfgs_resident_kernel<1, V, M> has its own table (bfgs_resident).
* LM past 64 parameters (chunk_route): lm_wide_fd_eval_kernel<O, C>. Up to 64 parameters the kernel
  depends on the objective only, and test_lm_default_functors_bit_exact_vs_oracle runs all four. The
  reference-order kernels depend on the objective only as well (lm_fd_iter_kernel<O, true>,
  lm_wide_fd_lanes_kernel<O>), and test_lm_reference_order_batches_equal_the_serial_oracle runs each of
  the three admitted objectives on both sides of 64 parameters: no empty cell.
* Resident batch engines (batch_route): de_batch_kernel<O, G>, pso_batch_kernel<O, G, T>, G = 64 past 64
  coordinates.
* nlsg_de_ref picks by objective only; test_shape_matrix_against_oracle and test_reference_traces run all
  three admitted ones."""
import numpy as np
import pytest

from tests import _oracle as O

pytestmark = pytest.mark.gpu

OBJECTIVES = ("rosenbrock", "sphere", "styblinski_tang", "rastrigin")
# one width per dispatch value: lane groups 4, 8, 16, 32; one chunk odd and even; two, four (odd),
# eight chunks; streamed rows odd and even
WIDTHS = (8, 16, 32, 64, 65, 128, 130, 257, 600, 1025, 1026)


def packed_route(D):
    """DE, PSO, SANN: lanes per row, or chunks and alignment, or streamed and alignment."""
    if D <= 64:
        return "group", 4 if D <= 8 else 8 if D <= 16 else 16 if D <= 32 else 32
    if D > 1024:
        return "long", D % 2
    return chunks(D), D % 2


def chunks(D):
    return 1 if D <= 128 else 2 if D <= 256 else 4 if D <= 512 else 8


def chunk_route(D):
    """NM (driver kernel up to 128), the hybrid (narrow kernel up to 128), LM past 64: chunks only."""
    return chunks(D)


def batch_route(D):
    """The resident batch engines: lanes per row, a whole wave past 64 coordinates."""
    return 4 if D <= 8 else 8 if D <= 16 else 16 if D <= 32 else 32 if D <= 64 else 64


def aligned_route(D):
    """BFGS: chunks and alignment at every width."""
    return chunks(D), D % 2


COVERED = {
    "de": {"rosenbrock": [1, 2, 3, 4, 5, 8, 16, 17, 33, 64, 127, 128, 129, 130, 257, 300, 600, 1024, 1025, 1026,
                          2048, 3001],
           "sphere": [1, 2, 17, 48, 127, 128, 129, 255], "styblinski_tang": [1, 3, 48, 64, 127, 129, 300],
           "rastrigin": [32]},
    ("pso", O.PSO_ACCELERATED): {"rosenbrock": [1, 2, 3, 5, 8, 16, 31, 33, 64, 128, 130, 256, 300, 1024, 1025,
                                                1026, 2048, 3001],
                                 "sphere": [3, 20, 300], "styblinski_tang": [1, 2, 20, 31, 127, 256]},
    ("pso", O.PSO_VANILLA): {"rosenbrock": [2, 3, 5, 8, 16, 31, 33, 64, 128, 130, 256, 300, 1024, 1025, 1026,
                                            2048, 3001],
                             "sphere": [128, 129], "styblinski_tang": [1, 129, 256]},
    "sann": {"rosenbrock": [1, 2, 8, 127, 128, 130, 1025, 1026], "sphere": [16, 300, 2048],
             "styblinski_tang": [6, 1000, 3001], "rastrigin": [2049]},
    "nm": {"rosenbrock": [1, 2, 4, 7, 16, 33, 128, 129, 200, 256, 257, 600, 1024], "sphere": [10],
           "styblinski_tang": [10]},
    "nmpso": {"rosenbrock": [2, 3, 4, 8, 16, 33, 64, 127, 129, 513], "sphere": [6, 128, 200, 1024],
              "styblinski_tang": [5, 257], "rastrigin": [300]},
    "bfgs": {"quad": [8, 64, 100, 130, 257, 1024], "rosenbrock": [2, 5, 16, 128, 130, 256, 257, 300, 1024],
             "sphere": [7, 600], "styblinski_tang": [64], "rastrigin": [2, 48]},
    "de_batch": {"rosenbrock": [1, 2, 3, 4, 5, 8, 16, 64, 65, 128], "sphere": [48], "styblinski_tang": [48],
                 "rastrigin": [48]},
    ("pso_batch", O.PSO_ACCELERATED): {"rosenbrock": [1, 2, 5, 9, 17, 33, 64, 65, 128], "sphere": [20],
                                       "styblinski_tang": [20], "rastrigin": [20]},
    ("pso_batch", O.PSO_VANILLA): {"rosenbrock": [1, 2, 5, 9, 17, 33, 64, 65, 128]},
    "bfgs_resident": {"quad": [1, 2, 3, 31, 33, 63, 64], "rosenbrock": [2, 3, 17, 64], "sphere": [1]},
    "lm_wide": {"rosenbrock": [65, 130], "sphere": [100, 300], "styblinski_tang": [129], "rastrigin": [70]},
}


def empty_cells(engine, route, widths, objectives=OBJECTIVES):
    cells = []
    for obj in objectives:
        taken = {route(D) for D in COVERED[engine].get(obj, [])}
        seen = set()
        for D in widths:
            if route(D) not in taken and route(D) not in seen:
                seen.add(route(D))
                cells.append((obj, D))
    return cells


@pytest.fixture(scope="module")
def mod():
    import torch
    assert torch.cuda.is_available()
    import nlsolver_amd
    return nlsolver_amd


def starts(batch, n, base=0.5, spread=1.0):
    return base + spread * (np.random.default_rng(n).random((batch, n)) - 0.5)


@pytest.mark.parametrize("obj,D", empty_cells("de", packed_route, WIDTHS))
def test_de_route(mod, oracle, obj, D):
    """Both strategies: `best` launches the generation kernels, `random` the fused turn kernels."""
    pop, x0 = 8, 1.5 * (1.0 + 0.001 * np.arange(D))
    for strategy in (0, 1):
        kw = dict(strategy=strategy, CR=0.5, F=0.6, eps=0.0, max_iter=1000, best_val_no_change=1000)
        ref = O.DESyncRun(oracle, obj, pop, D, x0, **kw)
        with mod.DEEngine(obj, pop, D, **kw) as eng:
            eng.init(x0)
            eng.step(2)
            ref.step(2)
            P, S = eng.download()
            st = eng.status()
        assert np.array_equal(P, ref.population) and np.array_equal(S, ref.scores), strategy
        assert (st.iteration, st.function_calls_used, st.best_index) == (ref.s.iter, ref.s.fcalls, ref.s.best_id)


@pytest.mark.parametrize("type_,obj,D", [(t, obj, D) for t in (O.PSO_ACCELERATED, O.PSO_VANILLA)
                                         for obj, D in empty_cells(("pso", t), packed_route, WIDTHS)])
def test_pso_route(mod, oracle, type_, obj, D):
    n, kw = 8, dict(type=type_, bounded=True, eps=0.0, max_iter=1000, best_val_no_change=1000)
    ref = O.PSOSyncRun(oracle, obj, n, D, -1.5, 2.5, **kw)
    with mod.PSOEngine(obj, n, D, **kw) as eng:
        eng.init(-1.5, 2.5)
        eng.step(2)
        ref.step(2)
        pos, vel, pbest, cur = eng.download()
        st = eng.status()
    assert np.array_equal(pos, ref.pos) and np.array_equal(cur, ref.cur_val) and np.array_equal(pbest, ref.pbest_val)
    if vel is not None:
        assert np.array_equal(vel, ref.vel)
    assert (st.iteration, st.function_calls_used, st.f_value, st.best_index) == \
        (ref.s.iter, ref.s.fevals, ref.s.gbest_val, ref.s.gbest_idx)


@pytest.mark.parametrize("obj,D", empty_cells("sann", packed_route, WIDTHS))
def test_sann_route(mod, oracle, obj, D):
    batch, seed, kw = 2, 12374563468, dict(max_iter=2, temperature_iter=2, temperature_max=10.0)
    x0 = starts(batch, D)
    with mod.SANNEngine(obj, batch, D, seed=seed, **kw) as eng:
        x, st = eng.minimize(x0)
    for b in range(batch):
        ref, xr, _ = O.sann_sync(oracle, obj, x0[b], seed, b, max_iter=2, temp_iter=2, temp_max=10.0)
        assert np.array_equal(x[b], xr) and st[b].f_value == ref.f_value, b
        assert (st[b].iteration, st[b].function_calls_used) == (ref.iteration, ref.function_calls_used)


@pytest.mark.parametrize("obj,D", empty_cells("nm", chunk_route, (128, 130, 257, 600)))
def test_nm_route(mod, oracle, obj, D):
    batch, x0 = 2, starts(2, D)
    with mod.NMEngine(obj, batch, D, max_iter=2, eps=0.0, no_change_best_tol=100000) as eng:
        x, st, eps = eng.minimize(x0.copy())
    for b in range(batch):
        ref, xr, eps_r, _ = O.nm_run(oracle, x0[b], obj=obj, order=1, max_iter=2, eps=0.0, no_change=100000)
        assert st[b].f_value == ref.f_value and np.array_equal(x[b], xr) and eps[b] == eps_r, b
        assert (st[b].iteration, st[b].function_calls_used) == (ref.iteration, ref.function_calls_used)


@pytest.mark.parametrize("obj,D", empty_cells("nmpso", chunk_route, (128, 130, 257, 600)))
def test_hybrid_route(mod, oracle, obj, D):
    batch, seed, x0 = 2, 99, starts(2, D)
    with mod.NMPSOEngine(obj, batch, D, seed=seed, max_iter=2, eps=0.0, no_change_best_iter=1000) as eng:
        x, st = eng.minimize(x0, None, None)
    for b in range(batch):
        ref, xr, _ = O.nmpso_sync(oracle, obj, x0[b], seed, b, eps=0.0, max_iter=2, no_change=1000)
        assert np.array_equal(x[b], xr) and st[b].f_value == ref.f_value, b
        assert (st[b].iteration, st[b].function_calls_used) == (ref.iteration, ref.function_calls_used)


BATCH_WIDTHS, BATCH_SEEDS = (8, 16, 32, 64, 65), [20260101, 20268020]


@pytest.mark.parametrize("obj,D", empty_cells("de_batch", batch_route, BATCH_WIDTHS))
def test_de_batch_route(mod, oracle, obj, D):
    pop, x0 = 8, 1.5 * (1.0 + 0.001 * np.arange(D))
    kw = dict(strategy=1, CR=0.5, F=0.6, eps=0.0, max_iter=1000, best_val_no_change=1000)
    with mod.DEBatchEngine(obj, len(BATCH_SEEDS), pop, D, **kw) as eng:
        eng.init(np.tile(x0, (len(BATCH_SEEDS), 1)), BATCH_SEEDS)
        eng.step(2)
        for b, seed in enumerate(BATCH_SEEDS):
            ref = O.DESyncRun(oracle, obj, pop, D, x0, seed=seed, **kw)
            ref.step(2)
            P, S = eng.download(b)
            assert np.array_equal(P, ref.population) and np.array_equal(S, ref.scores), b


@pytest.mark.parametrize("type_,obj,D", [(t, obj, D) for t in (O.PSO_ACCELERATED, O.PSO_VANILLA)
                                         for obj, D in empty_cells(("pso_batch", t), batch_route, BATCH_WIDTHS)])
def test_pso_batch_route(mod, oracle, type_, obj, D):
    n, kw = 8, dict(type=type_, eps=0.0, max_iter=100, best_val_no_change=1000)
    with mod.PSOBatchEngine(obj, len(BATCH_SEEDS), n, D, **kw) as eng:
        eng.init(-2.0, 3.0, BATCH_SEEDS)
        eng.step(2)
        sts = eng.status()
        for b, seed in enumerate(BATCH_SEEDS):
            ref = O.PSOSyncRun(oracle, obj, n, D, -2.0, 3.0, seed=seed, **kw)
            ref.step(2)
            pos, _, pbest, cur = eng.download(b)
            assert np.array_equal(pos, ref.pos) and np.array_equal(cur, ref.cur_val), b
            assert np.array_equal(pbest, ref.pbest_val), b
            assert sts[b].f_value == ref.s.gbest_val and sts[b].best_index == ref.s.gbest_idx, b


BFGS_WIDTHS = (65, 128, 130, 257, 600)


@pytest.mark.parametrize("obj,D", empty_cells("bfgs", aligned_route, BFGS_WIDTHS, ("quad",) + OBJECTIVES))
def test_bfgs_route(mod, oracle, obj, D):
    batch, kw = 2, dict(max_iter=2, grad_eps=0.0, alpha=1.0)
    x0 = 0.8 + 0.4 * (np.random.default_rng(D).random((batch, D)) - 0.5)
    if obj == "quad":
        d, b, c = O.quad_problem(D)
        with mod.BFGSEngine(mod.QuadDiagRank1(d, b, c), batch, **kw) as eng:
            x, st = eng.minimize(x0.copy())
        refs = [O.bfgs_quad(oracle, x0[p], tree=1, **kw)[:2] for p in range(batch)]
    else:
        with mod.BFGSEngine(obj, batch, dim=D, **kw) as eng:
            x, st = eng.minimize(x0.copy())
        refs = [O.bfgs_fd(oracle, obj, x0[p], tree=1, **kw)[:2] for p in range(batch)]
    for p, (ref, xr) in enumerate(refs):
        assert st[p].f_value == ref.f_value and np.array_equal(x[p], xr), p
        assert (st[p].iteration, st[p].function_calls_used, st[p].gradient_evals_used) == \
            (ref.iteration, ref.function_calls_used, ref.gradient_evals_used)


# Resident BFGS kernel (resident=True, n <= 64): alignment x model. The existing cases
# (test_state_after_k_turns_equals_the_lock_step_engines) compare it with the lock-step engine, which
# the tests above pin to the oracle; here the resident run itself meets the oracle.
@pytest.mark.parametrize("obj,D", empty_cells("bfgs_resident", lambda D: D % 2, (64, 63), ("quad",) + OBJECTIVES))
def test_bfgs_resident_route(mod, oracle, obj, D):
    batch, kw = 2, dict(max_iter=2, grad_eps=0.0, alpha=1.0)
    x0 = 0.8 + 0.4 * (np.random.default_rng(D).random((batch, D)) - 0.5)
    with mod.BFGSEngine(obj, batch, dim=D, resident=True, **kw) as eng:
        assert eng.resident
        x, st = eng.minimize(x0.copy())
    for p in range(batch):
        ref, xr = O.bfgs_fd(oracle, obj, x0[p], tree=1, **kw)[:2]
        assert st[p].f_value == ref.f_value and np.array_equal(x[p], xr), p
        assert (st[p].iteration, st[p].function_calls_used, st[p].gradient_evals_used) == \
            (ref.iteration, ref.function_calls_used, ref.gradient_evals_used)


# LM past 64 parameters, finite-difference objectives: lm_wide_fd_eval_kernel<O, chunks>. One problem
# per case, because the finite-difference Hessian costs the oracle 16 n^2 evaluations of an
# n-coordinate objective on the CPU side: about 1 s per evaluation of f, g, H at n = 257 (Rastrigin,
# whose cosine is the deterministic one: 9 s) and 8 s at n = 600 for the sphere. Where that is about a
# second, a case makes one iteration (evaluation, step, evaluation: the step consumes g and H, so every
# output of the kernel is checked); Rastrigin at 257 and the eight-chunk class make the first
# evaluation only (max_iter = 0: f and the counters are checked, g and H are not). Eight chunks are run
# for the sphere alone: the other three objectives cost the oracle 9 s and more per evaluation there.
LM_EVALUATION_ONLY = {("rastrigin", 257), ("sphere", 600)}
LM_CELLS = [(obj, D) for obj, D in empty_cells("lm_wide", chunk_route, (65, 130, 257, 600))
            if D < 600 or obj == "sphere"]


@pytest.mark.parametrize("obj,D", LM_CELLS)
def test_lm_wide_route(mod, oracle, obj, D):
    batch = 1
    kw = dict(lam=1.0, up=4.0, down=3.0, max_iter=0 if (obj, D) in LM_EVALUATION_ONLY else 1, f_delta=0.0)
    x0 = starts(batch, D, 0.8, 0.2)
    with mod.lm.LMEngine(obj, batch=batch, n=D, **kw) as eng:
        x, st, lam = eng.minimize(x0.copy())
    for b in range(batch):
        ref, xr, lam_r, _ = O.lm_fd(oracle, obj, x0[b], order=1, **kw)
        assert st[b].f_value == ref.f_value and np.array_equal(x[b], xr) and lam[b] == lam_r, b
        assert (st[b].iteration, st[b].function_calls_used) == (ref.iteration, ref.function_calls_used)
