"""The kernels' wave sum (wave_sum in nlsg_common.h) restated in numpy, and the inputs its tests
share. The restatement is the definition: six levels of an xor butterfly, offsets 32 .. 1, lane l
taking v[l] + v[l ^ off] — own operand first — so all 64 lanes end with the same value."""
import numpy as np

LANES = 64
OFFSETS = (32, 16, 8, 4, 2, 1)


def butterfly(v):
    """v: [waves, 64] float64 -> [waves, 64], every lane's value after the six levels."""
    v = np.array(v, dtype=np.float64, copy=True)
    assert v.ndim == 2 and v.shape[1] == LANES
    lane = np.arange(LANES)
    with np.errstate(all="ignore"):
        for off in OFFSETS:
            v = v + v[:, lane ^ off]
    return v


def normals(rng, waves):
    return rng.standard_normal((waves, LANES))


def wide(rng, waves):
    """Magnitudes spread over 600 binades; half of a wave's lanes hold the negation of another
    lane's value times (1 + a few ulps .. 1e-3), shuffled: the sum cancels to far below its terms."""
    e = rng.integers(-300, 301, size=(waves, LANES // 2))
    m = rng.uniform(1.0, 2.0, size=(waves, LANES // 2)) * rng.choice([-1.0, 1.0], size=(waves, LANES // 2))
    a = np.ldexp(m, e)
    near = 1.0 + rng.choice([0.0, 2.0 ** -52, 2.0 ** -40, 1e-9, 1e-3], size=a.shape)
    v = np.concatenate([a, -a * near], axis=1)
    return rng.permuted(v, axis=1)


def specials(rng, waves):
    """+-0, subnormals, normals and infinities. A wave holds infinities of ONE sign (its sum is
    that infinity): inf - inf makes a NaN whose sign IEEE 754 leaves to the implementation, and
    the restatement runs on another one than the kernel."""
    tiny = np.float64(5e-324)
    pool = np.array([0.0, -0.0, tiny, -tiny, 1000 * tiny, -(2.0 ** -1023), 2.0 ** -1022, 2.0 ** -1030,
                     1.0, -1.0, 2.0 ** -1074 * 3, 1e-310, -1e-310])
    v = rng.choice(pool, size=(waves, LANES))
    v[: waves // 8] = rng.choice(np.array([0.0, -0.0]), size=(waves // 8, LANES))  # zeros of both signs only
    v[waves // 8] = -0.0                                                           # all -0: the sum is -0
    v[waves // 8 + 1] = 0.0
    sub = slice(waves // 4, waves // 2)                                            # subnormals only
    v[sub] = rng.integers(-2 ** 40, 2 ** 40, size=v[sub].shape).astype(np.float64) * tiny
    w = np.arange(waves // 2, waves)                                               # with infinities
    sign = np.where(rng.random(w.size) < 0.5, -np.inf, np.inf)
    hit = rng.random((w.size, LANES)) < 0.1
    hit[np.arange(w.size), rng.integers(0, LANES, size=w.size)] = True
    v[w] = np.where(hit, sign[:, None], v[w])
    return v


def one_nan(rng, waves):
    v = rng.standard_normal((waves, LANES))
    v[np.arange(waves), rng.integers(0, LANES, size=waves)] = np.nan
    return v


def all_inputs(seed=20260101, waves_each=1024):
    """4 x waves_each waves: [normals | wide | specials | one NaN per wave]."""
    rng = np.random.default_rng(seed)
    return np.concatenate([normals(rng, waves_each), wide(rng, waves_each), specials(rng, waves_each),
                           one_nan(rng, waves_each)], axis=0)
