"""CPU: the restatement of the batched LSA kernel's algorithm (tests/lsap_ref.py, the parallel column-selection rule) is
exactly scipy's linear_sum_assignment on tie-heavy matrices of both orientations, and fails with scipy's errors."""
import numpy as np
import pytest
from scipy.optimize import linear_sum_assignment

from tests.lsap_ref import INFEASIBLE, INVALID, lsap, select


def _same(c):
    try:
        want = linear_sum_assignment(c)
    except ValueError as e:
        with pytest.raises(ValueError) as got:
            lsap(c)
        assert str(got.value) == str(e)
        return False
    got = lsap(c)
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(got[1], want[1])
    return True


def _matrix(r, kind, nr, nc):
    if kind == "uniform":
        return r.random((nr, nc)).astype(np.float32)
    if kind == "integer":
        return r.integers(0, 4, (nr, nc)).astype(np.float32)
    if kind == "quantized":
        return (np.round(r.random((nr, nc)) * 10) / 10).astype(np.float32)
    if kind == "constant":
        return np.full((nr, nc), 0.5, np.float32)
    c = r.integers(0, 3, (nr, nc)).astype(np.float32)       # with +inf entries: feasible or not
    c[r.random((nr, nc)) < 0.25] = np.inf
    return c


@pytest.mark.parametrize("kind", ["uniform", "integer", "quantized", "constant", "inf"])
def test_matches_scipy_on_small_tie_heavy_matrices(kind):
    r = np.random.default_rng({"uniform": 1, "integer": 2, "quantized": 3, "constant": 4, "inf": 5}[kind])
    solved = 0
    for _ in range(800):
        nr, nc = (int(x) for x in r.integers(1, 14, 2))
        solved += _same(_matrix(r, kind, nr, nc))
    assert solved >= (300 if kind == "inf" else 800)


@pytest.mark.parametrize("shape", [(200, 60), (60, 200), (100, 130), (64, 64)])
@pytest.mark.parametrize("kind", ["uniform", "quantized"])
def test_matches_scipy_at_criterion_sizes(shape, kind):
    r = np.random.default_rng(shape[0] * 1000 + shape[1])
    assert _same(_matrix(r, kind, *shape))


def test_constant_costs_give_the_identity():
    for nr, nc in [(5, 5), (3, 7), (7, 3)]:
        rows, cols = lsap(np.zeros((nr, nc), np.float32))
        np.testing.assert_array_equal(rows, np.arange(min(nr, nc)))
        np.testing.assert_array_equal(cols, np.arange(min(nr, nc)))


def test_empty_and_single_line_matrices():
    for shape in [(0, 0), (0, 5), (5, 0)]:
        rows, cols = lsap(np.zeros(shape, np.float32))
        assert rows.size == 0 and cols.size == 0
    r = np.random.default_rng(7)
    for n in (1, 2, 9, 64):
        assert _same(r.random((1, n)).astype(np.float32))
        assert _same(r.random((n, 1)).astype(np.float32))


def test_invalid_and_infeasible_raise_scipys_errors():
    c = np.ones((3, 4), np.float32)
    c[1, 2] = np.nan
    with pytest.raises(ValueError, match=INVALID):
        lsap(c)
    c[1, 2] = -np.inf
    with pytest.raises(ValueError, match=INVALID):
        lsap(c)
    c = np.ones((3, 4), np.float32)
    c[:, 1:] = np.inf                      # three rows share one finite column
    with pytest.raises(ValueError, match=INFEASIBLE):
        lsap(c)
    for bad in (c, c.T):
        _same(bad)


def test_selection_rule_equals_scipys_sequential_scan():
    """The order-independent rule picks the position scipy's `<, or == and unassigned` scan picks."""
    r = np.random.default_rng(11)
    for _ in range(3000):
        n = int(r.integers(1, 20))
        spc = r.integers(0, 3, n).astype(np.float64)
        spc[r.random(n) < 0.2] = np.inf
        un = r.random(n) < 0.5
        lowest, index = np.inf, -1
        for it in range(n):
            if spc[it] < lowest or (spc[it] == lowest and un[it]):
                lowest, index = spc[it], it
        if lowest == np.inf:
            continue                       # scipy reports the matrix infeasible whichever column it holds
        assert select(spc, un) == index
