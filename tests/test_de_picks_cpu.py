"""The screening wave's donor picks without a device: first occurrences among candidates 0..6
(tests/_de_octet.py) against the rule's definition over 31 candidates (tests/_de_screen.py:
pick_three) -- exhaustively over every sequence of seven candidates from five values, the agent's own
index among them, and on the candidates of the case list of tests/test_de_octet_gpu.py."""
import itertools

import numpy as np

from tests import _oracle as O
from tests import _de_screen as M
from tests import _de_octet as X


def test_first_occurrences_are_the_rule_on_every_sequence():
    values, agent = 5, 2
    head = np.array(list(itertools.product(range(values), repeat=X.SEEN)), dtype=np.int64)
    assert head.shape == (values ** X.SEEN, X.SEEN)
    # candidates 7..30: every value again and again, so that the definition finds its three donors
    # past candidate 6 wherever it has not found them before
    tail = np.resize(np.arange(values, dtype=np.int64), M.CANDIDATES - X.SEEN)
    cand = np.concatenate([head, np.broadcast_to(tail, (head.shape[0], tail.size))], axis=1)
    agents = np.full(head.shape[0], agent, dtype=np.int64)
    bad_ok, bad_picks, third = X.compare_with_pick_three(cand, agents)
    assert (bad_ok, bad_picks) == (0, 0)
    # both outcomes and every position of the third pick occur
    assert set(np.unique(third).tolist()) >= set(range(2, X.SEEN)) and (third >= X.SEEN).any()
    # candidates 7..30 never matter: another tail, the same picks and the same `ok`
    other = np.concatenate([head, np.full((head.shape[0], tail.size), agent, dtype=np.int64)], axis=1)
    p0, ok0, t0 = X.first_occurrence_picks(cand, agents)
    p1, ok1, t1 = X.first_occurrence_picks(other, agents)
    assert np.array_equal(p0, p1) and np.array_equal(ok0, ok1) and np.array_equal(t0, t1)
    want, pos = M.pick_three(other, agents)
    assert np.array_equal(pos < M.SELECTORS, ok1) and np.array_equal(want[ok1], p1[ok1])


def test_case_list_of_the_device_test(oracle):
    """the same comparison on candidates() of every generation of the case list, and what the list
    reaches"""
    got, bad_ok, bad_picks = X.coverage(O, oracle)
    print(got)
    assert (bad_ok, bad_picks) == (0, 0)
    assert got == X.WANT
