"""The donor picks of the screening wave (kDeBoundScreen, nlsolver_amd/csrc/nlsg_de_kernels.h:
de_generation_screen), which plans its agents eight lanes each, restated in numpy for
tests/test_de_picks_cpu.py and tests/test_de_octet_gpu.py, and the case list the two share.

The wave looks at donor candidates 0..6 only, eight lanes per agent: a candidate is kept when it
differs from the agent and from every candidate before it (first occurrences), the picks are the
first three kept ones in order, and the agent runs the screen when there are three. This is
tests/_de_screen.py's pick_three with "third pick at candidate <= 6": candidates 7..30 of the
rule's definition can only turn one kind of "declined" into the other."""
import numpy as np

from tests import _de_screen as M

SEEN = M.SELECTORS  # candidates the wave looks at


def first_occurrence_picks(cand, agents_local):
    """cand [n, >= 7] -> (picks [n, 3], -1 where missing; ok [n]; position of the third [n], 7 where missing)"""
    cand = np.asarray(cand)[:, :SEEN]
    a = np.asarray(agents_local)
    n = cand.shape[0]
    keep = cand != a[:, None]
    for k in range(1, SEEN):
        keep[:, k] &= ~(cand[:, :k] == cand[:, k:k + 1]).any(axis=1)
    rank = np.cumsum(keep, axis=1) - 1  # the lane's rank among the kept ones
    picks = np.full((n, 3), -1, dtype=np.int64)
    third = np.full(n, SEEN, dtype=np.int64)
    for r in range(3):
        hit = keep & (rank == r)
        has = hit.any(axis=1)
        pos = hit.argmax(axis=1)
        picks[has, r] = cand[has, pos[has]]
        if r == 2:
            third[has] = pos[has]
    return picks, keep.sum(axis=1) >= 3, third


def compare_with_pick_three(cand, agents_local):
    """-> (mismatches in ok, mismatches in the picks where the rule runs, positions of the third pick)"""
    want, third = M.pick_three(cand, agents_local)
    want_ok = third < M.SELECTORS
    got, ok, pos = first_occurrence_picks(cand, agents_local)
    bad_ok = int(np.sum(ok != want_ok))
    bad_picks = int(np.sum((got[want_ok] != want[want_ok]).any(axis=1))) + int(np.sum(pos[want_ok] != third[want_ok]))
    return bad_ok, bad_picks, third


SEED = M.SEED
# (obj, pop, D, CR, F, x0, generations, seed, screen retry period or None): the boundaries of a wave
# of four agents (of eight, as the wave was first built) and of a block of four waves
CASES = [
    ("rosenbrock", 7, 128, 0.9, 0.8, 4.096, 16, SEED, None),   # a wave and three agents
    ("rosenbrock", 12, 127, 0.9, 0.8, 4.096, 24, SEED, None),  # odd D, non-VEC loads, three full waves
    ("rosenbrock", 15, 65, 0.9, 0.5, 1.2, 24, SEED, 4),        # one agent short of a block, accepting
    ("rosenbrock", 17, 128, 0.9, 0.8, 4.096, 16, SEED, None),  # a block and a lone agent
    ("rosenbrock", 31, 66, 0.9, 0.5, 1.2, 24, SEED, 8),        # two blocks less one agent
    ("rosenbrock", 63, 128, 0.9, 0.8, 4.096, 12, SEED, None),  # four blocks less one agent
]
# what the oracle and the model find in the list (agent-generations); declines: fewer than three
# donors or a third pick past candidate 6; late third: the third pick lies at candidates 3..6 (a
# duplicate or a self-draw among the first candidates, and the screen must still run)
WANT = {"decided": 1699, "missed, bound": 38, "missed, accepted": 12, "missed, rejected": 32,
        "declined": 8, "backed off": 6, "retried": 1, "late third": 601}


def coverage(O, oracle):
    """The model and the oracle over the list -> the counts named in WANT, and the pick rule's
    mismatches summed over every generation's candidates()."""
    seen = np.zeros(len(M.NAMES), dtype=np.int64)
    retried = late = bad_ok = bad_picks = 0
    for c in CASES:
        obj, pop, D, CR, F, x0v, gens, seed, sr = c
        ref = O.DESyncRun(oracle, obj, pop, D, np.full(D, x0v), trace=True, **M.case_kw(c))
        model = M.ScreenModel(obj, pop, D, CR, F, seed, M.BOUND_RETRY, sr or M.SCREEN_RETRY)
        a = np.arange(pop)
        for g in range(1, gens + 1):
            P, S = ref.population.copy(), ref.scores.copy()
            ref.step(1)
            model.generation(g, P, S, ref.trace)
            retried += model.retried
            cand = M.candidates(seed, g, a, D, pop)
            b0, b1, third = compare_with_pick_three(cand, a)
            bad_ok += b0
            bad_picks += b1
            late += int(np.sum((third >= 3) & (third < M.SELECTORS)))
        seen += model.seen
    got = {"decided": int(seen[M.DECIDED]), "missed, bound": int(seen[M.MISS_BOUND]),
           "missed, accepted": int(seen[M.MISS_ACCEPT]), "missed, rejected": int(seen[M.MISS_REJECT]),
           "declined": int(seen[M.FEW_DONORS] + seen[M.PAST_SIX]), "backed off": int(seen[M.BACKED_OFF]),
           "retried": int(retried), "late third": int(late)}
    return got, bad_ok, bad_picks
