"""numpy restatement of the DE generation's half-row reject screen (kDeBoundScreen,
nlsolver_amd/csrc/nlsg_de_kernels.h: de_generation_pair), for tests/test_de_screen_cpu.py and
tests/test_de_screen_gpu.py: the screen value in the kernel's tree order, the donor candidates a
half-wave sees, who tries the screen, and the miss count in bits 2-3 of the selector byte. The bound's
hint (bit 1) is restated beside it the way tests/_de_bound.py does, per shard."""
import numpy as np

from tests._de_bound import cross_masks, ctr_key, lane_tree, u01

HALF = 64          # coordinates a half-wave holds
CANDIDATES = 31    # donor candidates a half-wave draws (half-lanes 1..31)
SELECTORS = 7      # candidates whose selector byte the half-wave loaded (half-lanes 1..7)

# what an agent did in a generation (ScreenModel.generation returns one per agent)
DECIDED, MISS_BOUND, MISS_ACCEPT, MISS_REJECT, FEW_DONORS, PAST_SIX, BACKED_OFF, NOT_BOUND = range(8)
NAMES = ["screen decided", "missed, bound decided", "missed, accepted", "missed, rejected",
         "declined: donors", "declined: pick past candidate 6", "skipped by back-off",
         "no bound try this generation"]


def screen_value(obj, mutant, cross):
    """The lane tree over the terms that touch coordinates 0..63 alone, +0.0 for every other one
    (term 63 included: its neighbour x64 is not loaded, and the kernel drops it for every
    objective). Lanes 32..63 then hold +0.0 and level 32 of the butterfly adds +0.0 to a value
    >= +0: the half-wave's tree."""
    known = np.array(cross, dtype=bool, copy=True)
    known[:, HALF - 1 if obj != "rosenbrock" else HALF:] = False
    return lane_tree(obj, mutant, known)


def candidates(seed, generation, agents_global, D, shard_n):
    """[n, 31] shard-local donor candidates 0..30 of each agent: draw D + 1 + k of its stream"""
    kg = ctr_key(np.uint64(seed), np.uint64(generation))
    ka = ctr_key(kg, np.asarray(agents_global, dtype=np.uint64))
    z = ctr_key(ka[:, None], np.uint64(D + 1) + np.arange(CANDIDATES, dtype=np.uint64)[None, :])
    idx = (u01(z) * float(shard_n)).astype(np.uint64)
    return np.minimum(idx, np.uint64(shard_n - 1)).astype(np.int64)


def pick_three(cand, agents_local):
    """The first three candidates in order that differ from the agent and from each other.
    -> picks [n, 3] (-1 where missing), position of the third [n] (CANDIDATES where missing)"""
    n = cand.shape[0]
    picks = np.full((n, 3), -1, dtype=np.int64)
    third = np.full(n, CANDIDATES, dtype=np.int64)
    for i in range(n):
        have = []
        for k in range(CANDIDATES):
            c = cand[i, k]
            if c != agents_local[i] and c not in have:
                have.append(c)
                if len(have) == 3:
                    third[i] = k
                    break
        picks[i, :len(have)] = have
    return picks, third


def tries_screen(sel, generation, a, bound_retry, screen_retry):
    """the back-off rule on a selector byte: (tries the bound, tries the screen)"""
    ga = (generation + a) & 0xFFFFFFFF
    bound_tries = ((sel & 2) == 0) | ((ga & (bound_retry - 1)) == 0)
    cnt = (sel >> 2) & 3
    return bound_tries, bound_tries & ((cnt < 2) | ((ga & (screen_retry - 1)) == 0))


def count_after(cnt, outcome):
    """outcome 0 decided, 1 tried and missed, 2 not tried or declined"""
    return np.where(outcome == 0, 0, np.where(outcome == 1, np.minimum(cnt + 1, 3), cnt))


class ScreenModel:
    """Selector bits 1-3, paths and counters of one shard's engine, fed with the oracle's generations."""

    def __init__(self, obj, pop, D, CR, F, seed, bound_retry, screen_retry, *, shard_lo=0, shard_n=None,
                 bound=True, screen=True):
        self.obj, self.D, self.CR, self.F, self.seed = obj, D, CR, F, seed
        self.lo, self.n = shard_lo, pop if shard_n is None else shard_n
        self.bound_retry, self.screen_retry = bound_retry, screen_retry
        self.bound, self.screen = bound, screen and bound
        self.reset()

    def reset(self):
        self.bound_counts = [0, 0, 0]
        self.screen_counts = [0, 0]
        self.seen = np.zeros(len(NAMES), dtype=np.int64)
        self.clear_bits()

    def clear_bits(self):  # init and upload
        self.sel = np.zeros(self.n, dtype=np.int64)  # bits 1-3 of the selector byte

    def generation(self, generation, P, S, trace):
        """P, S: the whole population and scores the generation read; trace: the oracle's [pop, 5]
        of it. Returns the [shard_n] array of what each agent of the shard did."""
        what = np.full(self.n, NOT_BOUND)
        if not self.bound:
            return what
        lo, n = self.lo, self.n
        a = np.arange(n)
        T = trace[lo:lo + n]
        r = T[:, :3].astype(np.int64)
        accept = T[:, 4] != 0
        old = S[lo:lo + n]
        bound_tries, screen_tries = tries_screen(self.sel, generation, a, self.bound_retry, self.screen_retry)
        if not self.screen:
            screen_tries = np.zeros(n, dtype=bool)
        cross = cross_masks(self.seed, generation, lo + a, self.D, self.CR, T[:, 3])
        with np.errstate(all="ignore"):
            mutant = P[r[:, 0]] + self.F * (P[r[:, 1]] - P[r[:, 2]])
            bound = lane_tree(self.obj, mutant, cross)
            screen = screen_value(self.obj, mutant, cross)
            bound_dec = bound >= old
            screen_ge = screen >= old
        # the chain the kernel rests on: screen-decided implies bound-decided implies rejected
        assert not np.any(screen_ge & ~bound_dec & ~np.isnan(bound))
        assert not np.any(bound_dec & accept)
        assert not np.any(screen_ge & accept)
        cand = candidates(self.seed, generation, lo + a, self.D, n)
        picks, third = pick_three(cand, a)
        ok3 = third < CANDIDATES
        ok = ok3 & (third < SELECTORS)
        # a half-wave's picks are the one-agent path's (the oracle's) whenever it has three
        assert np.array_equal(picks[ok3] + lo, r[ok3])
        run = screen_tries & ok
        dec = run & screen_ge
        miss = run & ~dec
        cnt = (self.sel >> 2) & 3
        backed = bound_tries & ~screen_tries & self.screen
        what[dec] = DECIDED
        rest = bound_tries & ~dec
        label = np.where(bound_dec, MISS_BOUND, np.where(accept, MISS_ACCEPT, MISS_REJECT))
        what[miss] = label[miss]
        what[screen_tries & ~ok3] = FEW_DONORS
        what[screen_tries & ok3 & ~ok] = PAST_SIX
        what[backed] = BACKED_OFF
        self.retried = int(np.sum(screen_tries & (cnt >= 2)))
        # counters: the screen's decisions count as the bound's
        all_known = cross.all(axis=1)
        self.bound_counts[0] += int(np.sum(dec | (rest & bound_dec)))
        self.bound_counts[1] += int(np.sum(rest & ~bound_dec & ~accept))
        self.bound_counts[2] += int(np.sum(rest & ~bound_dec & accept))
        self.screen_counts[0] += int(np.sum(dec))
        self.screen_counts[1] += int(np.sum(miss))
        for k in range(len(NAMES)):
            self.seen[k] += int(np.sum(what == k))
        # selector bits: the hint as the one-agent path leaves it, the miss count
        hint = np.where(bound_tries, np.where(dec, False, rest & ~bound_dec & ~all_known), (self.sel & 2) != 0)
        cnt = count_after(cnt, np.where(dec, 0, np.where(miss, 1, 2)))
        self.sel = (hint.astype(np.int64) << 1) | (cnt << 2)
        return what


# ---- the case list of tests/test_de_screen_gpu.py, checked on the CPU first (test_de_screen_cpu.py) ----
SEED = 12374563468
# (obj, pop, D, CR, F, x0, generations, seed, screen retry period or None for the built-in one)
#   x0 4.096 F 0.8: the screen decides;  x0 1.2 F 0.5: mixed, with acceptances;
#   x0 1e-3: never decides, the counts saturate and retry;  pop 4..9: declines (tiny shards)
CASES = [
    ("rosenbrock", 5, 128, 0.9, 0.8, 4.096, 12, SEED, None),
    ("rosenbrock", 8, 65, 0.9, 0.5, 1.2, 20, SEED, 4),
    ("rosenbrock", 9, 66, 0.9, 0.8, 4.096, 12, SEED, None),
    ("rosenbrock", 33, 127, 0.9, 0.5, 1.2, 30, SEED, 8),
    ("rosenbrock", 40, 128, 0.9, 0.5, 1e-3, 40, SEED, 8),
    ("rosenbrock", 40, 66, 0.9, 0.5, 1.2, 24, SEED, 16),
    ("rosenbrock", 1000, 128, 0.9, 0.8, 4.096, 8, SEED, None),
    ("rosenbrock", 1000, 65, 0.9, 0.5, 1.2, 10, SEED, 4),
    ("sphere", 33, 128, 0.9, 0.3, 1.2, 12, SEED, 4),
    # pop 4: seeds at which 31 candidates leave an agent short of three donors
    ("rosenbrock", 4, 128, 0.9, 0.8, 4.096, 40, 17, None),
    ("rosenbrock", 4, 128, 0.9, 0.8, 4.096, 40, 28, None),
    ("rosenbrock", 4, 128, 0.9, 0.8, 4.096, 40, 39, None),
]
BOUND_RETRY, SCREEN_RETRY = 256, 16  # kDeBoundRetry, kDeScreenRetry


def case_id(c):
    return f"{c[0]}-pop{c[1]}-D{c[2]}-F{c[4]}-x0_{c[5]}-seed{c[7]}-R{c[8]}"


def case_kw(c):
    return dict(strategy=1, CR=c[3], F=c[4], eps=0.0, best_val_no_change=10**6, minimize=True, seed=c[7])


def run_model(O, oracle, c):
    """the oracle and the model over one case -> (model, retried-after-back-off count)"""
    obj, pop, D, CR, F, x0v, gens, seed, sr = c
    ref = O.DESyncRun(oracle, obj, pop, D, np.full(D, x0v), trace=True, **case_kw(c))
    model = ScreenModel(obj, pop, D, CR, F, seed, BOUND_RETRY, sr or SCREEN_RETRY)
    retried = 0
    for g in range(1, gens + 1):
        P, S = ref.population.copy(), ref.scores.copy()
        ref.step(1)
        model.generation(g, P, S, ref.trace)
        retried += model.retried
    return model, retried
