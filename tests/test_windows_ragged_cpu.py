"""Host side of the ragged window batching (windows.ragged_batches): how fit_windows_batched groups windows whose
inducing-point counts differ, and its refusal of a window without inducing points — no GPU needed."""
import numpy as np
import pytest

from gpitch_amd.windows import fit_windows_batched, ragged_batches


def _flat(groups, single):
    return [i for _, ids in groups for i in ids] + list(single)


@pytest.mark.parametrize("batch", [1, 3, 4, 64])
def test_every_window_once_in_batches_of_neighbouring_counts(batch):
    rng = np.random.RandomState(batch)
    counts = list(rng.randint(1, 300, size=57)) + [256, 257, 16, 17]
    groups, single = ragged_batches(counts, batch)
    order = _flat(groups, single)
    assert sorted(order) == list(range(len(counts)))                   # every window exactly once
    inv = np.argsort(order)
    np.testing.assert_array_equal(np.asarray(order)[inv], np.arange(len(counts)))   # the inverse permutation restores order
    assert sorted(single) == [i for i, c in enumerate(counts) if c > 256]
    prev = 0
    for m, ids in groups:
        assert 1 <= len(ids) <= batch
        assert m % 16 == 0 and m <= 256
        cs = [counts[i] for i in ids]
        assert max(cs) <= m < max(cs) + 16
        assert cs == sorted(cs) and cs[0] >= prev                       # sorted by count: neighbours share a batch
        prev = cs[-1]
    # stable: equal counts keep their input order
    flat = [i for _, ids in groups for i in ids]
    for a, b in zip(flat, flat[1:]):
        if counts[a] == counts[b]:
            assert a < b


def test_equal_counts_are_todays_batches():
    groups, single = ragged_batches([37] * 10, 4)
    assert single == []
    assert groups == [(37, [0, 1, 2, 3]), (37, [4, 5, 6, 7]), (37, [8, 9])]
    groups, single = ragged_batches([64] * 3, 64)
    assert groups == [(64, [0, 1, 2])] and single == []
    # equal counts beside windows beyond the cap: one plan at exactly that count
    groups, single = ragged_batches([300, 50, 50, 400], 8)
    assert groups == [(50, [1, 2])] and single == [0, 3]


def test_plan_sizes_round_up_to_the_granule():
    groups, single = ragged_batches([1, 15, 16, 17, 40, 64, 100, 130, 250], 3)
    assert [(m, ids) for m, ids in groups] == [(16, [0, 1, 2]), (64, [3, 4, 5]), (256, [6, 7, 8])]
    assert single == []
    assert ragged_batches([5, 300], 4) == ([(5, [0])], [1])
    assert ragged_batches([300, 301], 4) == ([], [0, 1])


def test_a_window_without_inducing_points_is_refused():
    with pytest.raises(ValueError, match="window 1"):
        ragged_batches([3, 0, 5], 4)
    x = np.linspace(0, 1, 50).reshape(-1, 1)
    wins = [(x, np.sin(x), x[::5]), (x, np.sin(x), x[::7]), (x, np.cos(x), np.zeros((0, 1)))]

    def make(h):                  # never reached: the shapes are checked before any device work
        raise AssertionError("make_model called")
    with pytest.raises(ValueError, match="window 2 has no inducing point"):
        fit_windows_batched(make, wins, maxiter=2, batch=2)
    with pytest.raises(ValueError, match="same number of frames"):
        fit_windows_batched(make, [wins[0], (x[:40], np.sin(x[:40]), x[:4])], maxiter=2, batch=2)
