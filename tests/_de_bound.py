"""numpy restatement of what the DE generation's lower-bound rejection computes (DeParams.bound,
nlsolver_amd/csrc/nlsg_de_kernels.h), for tests/test_de_bound_cpu.py and tests/test_de_bound_gpu.py:
the lane tree of wave_objective / wave_objective_masked, the keyed crossover mask, and the path each
agent of a generation takes (bound decided / fell through / no kept coordinate) with its hint."""
import numpy as np

M64 = np.uint64(0xFFFFFFFFFFFFFFFF)
GOLDEN = np.uint64(0x9E3779B97F4A7C15)


def mix64(z):
    z = np.asarray(z, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def ctr_key(parent, index):
    with np.errstate(over="ignore"):
        return mix64(np.asarray(parent, dtype=np.uint64) +
                     GOLDEN * (np.asarray(index, dtype=np.uint64) + np.uint64(1)))


def u01(bits):
    return np.asarray(bits, dtype=np.uint64).astype(np.float64) * 2.0 ** -64


def chunks_of(D):
    return 1 if D <= 128 else 2 if D <= 256 else 4 if D <= 512 else 8


def _term(obj, xi, xn):
    if obj == "rosenbrock":
        t1 = 1 - xi
        t2 = xn - xi * xi
        return t1 * t1 + (100 * t2) * t2
    if obj == "sphere":
        return xi * xi
    raise ValueError(obj)


def lane_tree(obj, x, known=None):
    """x [N, D] (or [D]), known [N, D] bool or None (every coordinate known) -> [N] values of the
    wave's tree: 64 lanes x CHUNKS x 2 coordinates, each lane adds its terms in order (+0.0 in place
    of a term that reads an unknown coordinate), then the xor butterfly 32 .. 1."""
    x = np.atleast_2d(np.asarray(x, dtype=np.float64))
    N, D = x.shape
    C = chunks_of(D)
    W = 128 * C
    chain = obj == "rosenbrock"
    nt = D - 1 if chain else D
    xp = np.zeros((N, W + 2))
    xp[:, :D] = x
    kp = np.ones((N, W + 2), dtype=bool)
    if known is not None:
        kp[:, :D] = np.atleast_2d(known)
    lanes = np.arange(64)
    acc = np.zeros((N, 64))
    with np.errstate(all="ignore"):
        for c in range(C):
            e0 = c * 128 + 2 * lanes
            for k in range(2):
                e = e0 + k
                t = _term(obj, xp[:, e], xp[:, e + 1])
                ok = kp[:, e] & (kp[:, e + 1] if chain else True)
                add = np.where(ok, t, 0.0)
                acc = np.where((e < nt)[None, :], acc + add, acc)
        for off in (32, 16, 8, 4, 2, 1):
            acc = acc + acc[:, lanes ^ off]
    assert all(np.array_equal(acc[:, 0], acc[:, l], equal_nan=True) for l in (1, 31, 63))
    return acc[:, 0]


def cross_masks(seed, generation, agents, D, CR, jrand):
    """[len(agents), D] bool: the trial of agent a takes the mutant at e --
    u01(ctr_key(ctr_key(ctr_key(seed, generation), a), e)) < CR or e == jrand[a]"""
    kg = ctr_key(np.uint64(seed), np.uint64(generation))
    ka = ctr_key(kg, np.asarray(agents, dtype=np.uint64))
    z = ctr_key(ka[:, None], np.arange(D, dtype=np.uint64)[None, :])
    return (u01(z) < CR) | (np.arange(D)[None, :] == np.asarray(jrand).astype(np.int64)[:, None])


class BoundModel:
    """Paths and counters of an engine that uses the bound, fed with the oracle's generations."""

    def __init__(self, obj, pop, D, CR, F, seed, retry, enabled=True):
        self.obj, self.pop, self.D, self.CR, self.F, self.seed = obj, pop, D, CR, F, seed
        self.retry, self.enabled = retry, enabled
        self.reset()

    def reset(self):
        self.counts = [0, 0, 0]
        self.clear_hints()

    def clear_hints(self):  # init and upload
        self.hint = np.zeros(self.pop, dtype=bool)

    def generation(self, generation, P, S, trace):
        """P, S: population and scores the generation read; trace: the oracle's [pop, 5] of it
        (r1, r2, r3, jrand, accept). Returns the [pop] array of paths: -1 plain, 0 decided,
        1 not decided and rejected, 2 accepted."""
        a = np.arange(self.pop)
        path = np.full(self.pop, -1)
        if not self.enabled:
            return path
        r = trace[:, :3].astype(np.int64)
        accept = trace[:, 4] != 0
        tries = ~self.hint | (((generation + a) & (self.retry - 1)) == 0)
        cross = cross_masks(self.seed, generation, a, self.D, self.CR, trace[:, 3])
        with np.errstate(all="ignore"):
            mutant = P[r[:, 0]] + self.F * (P[r[:, 1]] - P[r[:, 2]])
            bound = lane_tree(self.obj, mutant, cross)
            decided = bound >= S
        all_known = cross.all(axis=1)
        # the bound is a bound: what it rejects, selection rejects
        assert not np.any(decided & accept)
        path[tries & decided] = 0
        rest = tries & ~decided
        path[rest & ~accept] = 1
        path[rest & accept] = 2
        self.hint = np.where(tries, rest & ~all_known, self.hint)
        for k in range(3):
            self.counts[k] += int(np.sum(path == k))
        return path
