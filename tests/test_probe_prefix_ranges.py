"""IdCells.prefix_ranges, the batched form of IdCells.prefix_range, on a hand-built index (no GPU: both are torch
arithmetic on the index's tensors)."""
import itertools

import numpy as np
import pytest
import torch

from generative_ranking_recommender_amd import ops

SIZES = (3, 4, 5)


@pytest.fixture(scope="module")
def index():
    rng = np.random.default_rng(4)
    every = list(itertools.product(*[range(s) for s in SIZES]))
    # 17 of the 60 IDs, none under first value 1 with second value 2, and none at all under (2, 3)
    allowed = [i for i in every if i[:2] not in ((1, 2), (2, 3))]
    pick = sorted(allowed[j] for j in rng.choice(len(allowed), 17, replace=False))
    count = rng.integers(1, 5, 17)
    n = int(count.sum())
    i32 = lambda a: torch.tensor(np.asarray(a), dtype=torch.int32)  # noqa: E731
    off = np.concatenate([[0], np.cumsum(count)])
    cap = 20  # (the index's arrays are larger than the cells they hold)
    group = np.zeros(cap, np.int64)
    fine = np.zeros(cap, np.int64)
    group[:17] = [a * SIZES[1] + b for a, b, _ in pick]
    fine[:17] = [c for _, _, c in pick]
    offs = np.zeros(cap + 1, np.int64)
    offs[:18] = off
    counters = np.zeros(ops.CELLS_COUNTERS, np.int64)
    counters[0] = 17
    cells = np.repeat(np.arange(17), count)
    return ops.IdCells(i32(rng.permutation(n)), i32(np.zeros(n)), i32(count[cells]), i32(cells), i32(offs), i32(group),
                       i32(fine), i32(counters), SIZES, torch.zeros((), dtype=torch.int64)), pick


def test_equals_prefix_range_for_every_prefix(index):
    idx, pick = index
    assert idx.n_cells == 17
    for depth in (1, 2, 3):
        # every prefix of the depth, and values one below and one above each level's range
        values = [range(-1, s + 1) for s in SIZES[:depth]]
        prefixes = list(itertools.product(*values))
        lo, hi = idx.prefix_ranges(torch.tensor(prefixes, dtype=torch.int32))
        assert lo.dtype == torch.int32 and hi.dtype == torch.int32 and lo.shape == (len(prefixes),)
        present = 0
        for j, pre in enumerate(prefixes):
            _, _, p0, p1 = idx.prefix_range(pre)
            assert (int(lo[j]), int(hi[j])) == (p0, p1), pre
            rows = sum(int(idx.cell_off[c + 1] - idx.cell_off[c]) for c, i in enumerate(pick) if i[:depth] == pre)
            assert p1 - p0 == rows, pre
            present += rows > 0
        assert present > 0 and any(int(lo[j]) == int(hi[j]) for j in range(len(prefixes)))
    # absent but in range: empty; out of range: (0, 0)
    lo, hi = idx.prefix_ranges(torch.tensor([[2, 3], [1, 2], [3, 0], [0, -1]]))
    assert (lo == hi).all() and lo[2:].tolist() == [0, 0] and hi[2:].tolist() == [0, 0]


def test_batch_shapes_and_refusals(index):
    idx, _ = index
    pre = torch.tensor([[[0, 1], [2, 2], [1, 3]], [[2, 0], [0, 0], [9, 9]]], dtype=torch.int64)
    lo, hi = idx.prefix_ranges(pre)
    assert lo.shape == (2, 3) and hi.shape == (2, 3)
    for a in range(2):
        for b in range(3):
            assert (int(lo[a, b]), int(hi[a, b])) == idx.prefix_range(pre[a, b].tolist())[2:]
    with pytest.raises(ValueError):
        idx.prefix_ranges(torch.zeros((4, 4), dtype=torch.int32))
    with pytest.raises(ValueError):
        idx.prefix_ranges(torch.zeros((4, 0), dtype=torch.int32))
    with pytest.raises(ValueError):
        idx.prefix_ranges(torch.zeros((4, 2)))
