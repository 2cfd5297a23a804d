"""Pure-Python rng::xorshift<double> (nlsolver.h:1344-1378): the generator the reference's DE,
PSO and SANN take by reference. `DE(..., generation="reference")` advances one of these in place
exactly as the reference's DE advances its generator."""

_MASK = 2**64 - 1
SPLITMIX_SEED = 12374563468  # rng::splitmix's seed, nlsolver.h:1265
_GOLDEN = 0x9E3779B97F4A7C15


def splitmix_yield_init(state):
    """rng::splitmix::yield_init (nlsolver.h:1273-1278) on a u64 state: (next state, output)."""
    state = (state + _GOLDEN) & _MASK
    z = state
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _MASK
    return state, z ^ (z >> 31)


class XorShift:
    """xorshift128+ with the reference's default seeding (x[0] = splitmix's first output,
    x[1] = x[0] >> 32) and its [0, 1] scaling: (t + s) / (double)UINT64_MAX, where
    (double)UINT64_MAX == 2^64, so a draw of exactly 1.0 is possible."""

    def __init__(self, state=None):
        if state is None:
            _, x0 = splitmix_yield_init(SPLITMIX_SEED)
            state = (x0, x0 >> 32)
        self.state = state

    @property
    def state(self):
        """the raw state (x[0], x[1]) as two u64"""
        return (self._x0, self._x1)

    @state.setter
    def state(self, value):
        x0, x1 = value
        self._x0, self._x1 = int(x0) & _MASK, int(x1) & _MASK

    def next_u64(self):
        """one step; the 64-bit sum the draw scales"""
        t, s = self._x0, self._x1
        self._x0 = s
        t ^= (t << 23) & _MASK
        t ^= t >> 18
        t ^= s ^ (s >> 5)
        self._x1 = t
        return (t + s) & _MASK

    def __call__(self):
        return float(self.next_u64()) * 2.0**-64  # int -> double rounds to nearest, as the cast does

    yield_ = __call__
