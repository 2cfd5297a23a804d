"""Wall and event times of reference-order DE (nlsg_de_ref_*) on one MI355X — the cases of
DESIGN.md §3 "Reference-order generation". One JSON line per case. Kernel times: run under
`rocprofv3 --kernel-trace --stats -- python scripts/de_ref_time.py` (a run of its own)."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nlsolver_amd  # noqa: E402
from nlsolver_amd import DE_BEST, DE_RANDOM  # noqa: E402


def states(n, seed=1):
    rs = np.random.default_rng(seed)
    return rs.integers(1, 2**64, size=(n, 2), dtype=np.uint64)


def case(name, B, pop, D, x0, st, repeats, **kw):
    with nlsolver_amd.DERefEngine("rosenbrock", B, pop, D, **kw) as eng:
        x0s = np.broadcast_to(np.asarray(x0, dtype=np.float64), (B, D)).copy()
        eng.minimize(x0s, st)  # warm-up
        t0 = time.perf_counter()
        for _ in range(repeats):
            _, status, _ = eng.minimize(x0s, st)
        wall = (time.perf_counter() - t0) * 1e3 / repeats
        ev = eng.time_solve(x0s, st, repeats) / repeats
    print(json.dumps({"case": name, "batch": B, "pop": pop, "D": D, "iters": int(status[0].iteration),
                      "fcalls": int(status[0].function_calls_used), "wall_ms": round(wall, 4),
                      "event_ms": round(ev, 4)}), flush=True)


def main():
    c1 = [nlsolver_amd.XorShift().state]
    case("c1_one_solve", 1, 40, 2, [5, 7], c1, 20, CR=0.9, F=0.8, eps=10e-4)
    case("c1_4096_solves", 4096, 40, 2, [5, 7], states(4096), 5, CR=0.9, F=0.8, eps=10e-4)
    case("pop4096_D128_50gen", 1, 4096, 128, np.full(128, 4.096), states(1), 1, CR=0.9, F=0.8, eps=0.0,
         max_iter=50, best_val_no_change=1000, strategy=DE_RANDOM)
    case("pop4096_D128_50gen_cr01_best", 1, 4096, 128, np.full(128, 4.096), states(1), 1, CR=0.1, F=0.8,
         eps=0.0, max_iter=50, best_val_no_change=1000, strategy=DE_BEST)


if __name__ == "__main__":
    main()
