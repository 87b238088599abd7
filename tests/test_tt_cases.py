"""The biased TaintToleration clusters of tests/_tt_cases.py, without a GPU: the
Python model equals the C oracle on every one of them (the literal loop up to
40 rows, the closed form above), and every winner category is populated, counted
on the model alone: each count class 0..8 with and without a NodeNumber match,
each explicit entry (feasible ranks 0, 1, 2 and the last row), and lists of
2, 3 and 4 rows.

Parity. A middle row j of an F-row list is flipped F - 2 - j times between its
own step and the last one; it keeps a high score only when that number is odd.
So in a five-row list the one middle row (rank 3, flipped zero times) never
wins: it ends at most at 8 (+10 with a NodeNumber match) while the last row ends
at 92 or more. test_rank_3_of_five_rows_never_wins checks all 9^5 count lists
in the oracle's literal loop; the smallest list in which a middle row wins has
six rows (rank 3), and the clusters must show that case.
"""
import itertools

import numpy as np
import pytest

import _tt_cases as tc

MIDS = [("mid", c, m) for c in range(9) for m in (0, 1)]
EXPLICIT = ("first0", "first1", "first2", "last")


def _same(model, o, tag):
    for k in ("node", "code", "score", "mask"):
        a, b = np.asarray(model[k]).astype(np.int64), np.asarray(o[k]).astype(np.int64)
        assert np.array_equal(a, b), (tag, k, np.nonzero(a != b)[0][:8].tolist())


@pytest.mark.parametrize("n", tc.SMALL_SIZES + tc.LARGE_SIZES)
def test_model_equals_the_oracle(oracle, n):
    for _, v in tc.clusters((n,)):
        nr, pr = tc.cluster(n, v)
        _same(tc.modelled(n, v), oracle.schedule_tt(nr, pr, literal=n <= 40, seed=tc.SEED), f"{n} rows, variant {v}")


def test_small_lists_fill_every_category():
    cats, _ = tc.tally(tc.SMALL_SIZES)
    for c in MIDS:
        assert cats.get(c, 0) >= 10, (c, cats.get(c, 0))
    for c in EXPLICIT:
        assert cats.get(c, 0) >= 100, (c, cats.get(c, 0))
    for F in (2, 3, 4):
        assert cats.get(("small", F), 0) >= 20, (F, cats.get(("small", F), 0))
    runs = [tc.modelled(n, v) for n, v in tc.clusters(tc.SMALL_SIZES)]
    # a middle row wins in the smallest list where one can: rank 3 of six rows
    assert sum(int(((o["F"] == 6) & (o["rank"] == 3)).sum()) for o in runs) >= 10
    # five-row lists are there, and (see the module docstring) rank 3 never wins them
    assert sum(int(((o["F"] == 5) & (o["rank"] >= 0)).sum()) for o in runs) >= 100
    assert sum(int(((o["F"] == 5) & (o["rank"] == 3)).sum()) for o in runs) == 0


def test_large_lists_fill_every_category():
    cats, _ = tc.tally(tc.LARGE_SIZES)
    for c in MIDS + list(EXPLICIT):
        assert cats.get(c, 0) >= 20, (c, cats.get(c, 0))


def test_rank_3_of_five_rows_never_wins(oracle):
    for c in itertools.product(range(9), repeat=5):
        s = oracle.tt_inloop(np.asarray(c), literal=True)
        assert s[3] + 10 < s[4], c  # (even with the NodeNumber match on rank 3 alone)
