"""What the CPU and the GPU leg of the head-rule tests share (TEST INFRASTRUCTURE): the sizes,
the rounding counts of the std_err bound, and the oracle's head driven on given scores.
tests/_head_ref.py stays free of the oracle; this module is where the two meet."""
import math

import numpy as np

from tests import _oracle as O

SIZES = [4, 5, 255, 256, 257, 1023, 1024, 1025, 2049, 263169]
SHARD_SIZES = [4, 257, 1024, 1025]
WORLDS = [2, 4, 8]

# Roundings on the longest path of the one-pass std_err through the two-level block tree
# (block_tree_256, nlsg_common.h): per level 4 sequential adds of a thread's strided partial,
# 6 butterfly adds inside a wave and 3 adds of the 4 wave sums = 13, twice (inside a tile, over
# the tiles) = 26; on the M2 path also the deviation, its square, the add of the merge term, the
# division by n - 1 and the square root = 31 (the path of a mean is shorter: 26 and 2 divisions);
# one spare for the subtraction of the two rounded means.
L_UNSHARDED = 32


def L_sharded(world):
    """shards merge serially in rank order: `world` more adds, and the merge term's 3 operations"""
    return L_UNSHARDED + world + 3


def make_run(lib, n, shards):
    return O.DESyncRun(lib, "sphere", n, 2, np.ones(2), n_shards=shards, eps=0.0,
                       max_iter=1000, best_val_no_change=10 ** 6)


def oracle_head(run):
    """The head of one oracle turn without its generation (whose scores the next vector
    overwrites anyway): what `sync_step` in oracle/oracle_de.c does before it calls
    orc_de_shard_generation -- one orc_de_shard_record per shard, orc_de_apply_records, and
    orc_de_commit unless a stop test fired. test_oracle_head_is_sync_steps_head holds it to
    orc_de_sync_step, so that it cannot drift from it. Returns the finaliser's best value: that
    of the winning record (the record that names the new best_id), NaN if none is valid."""
    s, lib = run.s, run.lib
    if s.done:
        return math.nan
    world, m = int(s.n_shards), int(s.pop // s.n_shards)
    recs = np.zeros((world, 5 + run.D))
    for r in range(world):
        lib.orc_de_shard_record(O.C.byref(s), r * m, m, O._ptr(recs[r]))
    if not lib.orc_de_apply_records(O.C.byref(s), O._ptr(recs), world, None):
        lib.orc_de_commit(O.C.byref(s))
    for r in range(world):
        if recs[r, 4] == 1.0 and int(recs[r, 1:2].view(np.uint64)[0]) == int(s.best_id):
            return float(recs[r, 0])
    return math.nan


def oracle_turns(run, vectors, *, eps=0.0, best_val_no_change=10 ** 6, max_iter=1000):
    """Resets the run's head state and feeds it one score vector per turn. Returns (best_id,
    val_no_change, iter, done, std_err, the last finaliser's best value)."""
    s = run.s
    s.best_id, s.iter, s.val_no_change, s.done, s.std_err = 0, 0, 0, 0, math.nan
    s.eps, s.best_val_no_change, s.max_iter = eps, best_val_no_change, max_iter
    f_value = math.nan
    for v in vectors:
        run.scores[:] = v
        if not s.done:
            f_value = oracle_head(run)
    return (int(s.best_id), int(s.val_no_change), int(s.iter), bool(s.done), float(s.std_err),
            f_value)
