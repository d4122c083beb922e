"""rqsid_id_trie on the GPU against ``numpy.unique`` over prefixes (tests/_trie_model.tables): every table for
equality, over one and several levels, one cell, dropped cells, a node that vanishes at every depth, and enough cells
to cross the scans' tile boundary; byte-equal repeats; the error word."""
import numpy as np
import pytest
import torch

from generative_ranking_recommender_amd import ops
from tests import _trie_model as M

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


def cells_of(rows, sizes, seed):
    """Distinct random IDs over ``sizes``, lexicographically ascending."""
    rng = np.random.default_rng(seed)
    return np.unique(np.stack([rng.integers(0, s, rows) for s in sizes], 1), axis=0)


def group_fine(cells, sizes):
    """The cells as rqsid_id_cells writes them: the mixed-radix group of every level but the last, and the last."""
    cells = np.asarray(cells, dtype=np.int64)
    if len(sizes) == 1:
        return cells[:, 0].astype(np.int32), np.zeros(len(cells), dtype=np.int32)
    g = np.zeros(len(cells), dtype=np.int64)
    for l, s in enumerate(sizes[:-1]):
        g = g * s + cells[:, l]
    return g.astype(np.int32), cells[:, -1].astype(np.int32)


def build(cells, sizes, keep=None, check=True):
    g, f = group_fine(cells, sizes)
    k = None if keep is None else torch.from_numpy(np.asarray(keep, dtype=np.uint8)).to(DEV)
    return ops.id_trie_tables(torch.from_numpy(g).to(DEV), torch.from_numpy(f).to(DEV), sizes, k, check=check)


def assert_tables(trie, want):
    got = trie.to_arrays()
    assert got["count"].tolist() == want["count"].tolist()
    for d in range(len(trie.sizes)):
        assert np.array_equal(got[f"value{d}"], want["value"][d]), d
        assert np.array_equal(got[f"child_off{d}"], want["child_off"][d]), d
    assert np.array_equal(got["leaf_cell"], want["leaf_cell"])
    return got


@pytest.mark.parametrize("sizes, rows", [((5, 4, 7), 60), ((50,), 40), ((3, 4, 2, 6), 90), ((2, 2, 2, 2, 2, 2, 2, 2), 200),
                                         ((128, 128, 256), 300_000)])
def test_tables_equal_numpy_unique(sizes, rows):
    cells = cells_of(rows, sizes, seed=len(sizes) * 1000 + rows)
    want = M.tables(cells, len(sizes))
    a = assert_tables(build(cells, sizes), want)
    b = build(cells, sizes).to_arrays()
    assert all(a[k].tobytes() == b[k].tobytes() for k in a)  # two calls give identical bytes
    rng = np.random.default_rng(3)
    keep = rng.random(len(cells)) < 0.6
    assert_tables(build(cells, sizes, keep), M.tables(cells, len(sizes), keep))


def test_one_cell_and_no_cells():
    assert_tables(build([[3, 1, 6]], (5, 4, 7)), M.tables([[3, 1, 6]], 3))
    assert_tables(build([[7]], (9,)), M.tables([[7]], 1))
    empty = build(np.zeros((0, 3), dtype=np.int64), (5, 4, 7))
    assert empty.counts() == (1, 0, 0, 0) and int(empty.child_off.abs().sum()) == 0


def test_keep_drops_every_cell():
    cells = cells_of(60, (5, 4, 7), seed=1)
    trie = build(cells, (5, 4, 7), np.zeros(len(cells), dtype=np.uint8))
    assert trie.counts() == (1, 0, 0, 0)
    assert trie.child_off[:, 0].tolist() == [0, 0, 0] and int(trie.child_off[0, 1]) == 0


def test_a_node_without_kept_children_vanishes_at_every_depth():
    cells = cells_of(60, (5, 4, 7), seed=2)
    first = cells[len(cells) // 2, 0]
    keep = cells[:, 0] != first  # every cell under one level-0 value
    want = M.tables(cells, 3, keep)
    got = assert_tables(build(cells, (5, 4, 7), keep), want)
    assert first not in got["value0"] and len(got["value0"]) == len(np.unique(cells[:, 0])) - 1
    pair = cells[3, :2]
    keep = ~(cells[:, :2] == pair).all(1)  # every child of one depth-2 node
    assert_tables(build(cells, (5, 4, 7), keep), M.tables(cells, 3, keep))


def test_error_word_and_dropped_cells():
    sizes = (5, 4, 7)
    cells = cells_of(60, sizes, seed=4)
    i = 17
    bad = np.concatenate([cells[:i + 1], cells[i:i + 1], cells[i + 1:]])  # cell i twice: the second is not above it
    with pytest.raises(RuntimeError, match="error word"):
        build(bad, sizes)
    trie = build(bad, sizes, check=False)
    assert int(trie.error.item()) == 1
    keep = np.ones(len(bad), dtype=bool)
    keep[i + 1] = False
    assert_tables(trie, M.tables(bad, 3, keep))
    # a value outside its level's size: dropped as well (the fine ID, then the group)
    for cell in ([4, 3, 7], [5, 0, 0]):
        out = np.concatenate([cells, [cell]])
        trie = build(out, sizes, check=False)
        assert int(trie.error.item()) == 1
        keep = np.ones(len(out), dtype=bool)
        keep[-1] = False
        assert_tables(trie, M.tables(out, 3, keep))
    clean = build(cells, sizes, check=False)
    assert int(clean.error.item()) == 0


def test_trie_of_a_cell_index_and_npz_round_trip(tmp_path):
    sizes = (6, 5, 9)
    rng = np.random.default_rng(8)
    ids = np.stack([rng.integers(0, s, 500) for s in sizes], 1).astype(np.int32)
    index = ops.id_cells(torch.from_numpy(ids).to(DEV), sizes)
    cells = np.unique(ids, axis=0)
    trie = ops.id_trie(index)
    got = assert_tables(trie, M.tables(cells, 3))
    # a leaf leads to its rows through the index
    order, off = index.order.cpu().numpy(), index.cell_off.cpu().numpy()
    for j in (0, len(cells) // 2, len(cells) - 1):
        c = got["leaf_cell"][j]
        assert (ids[order[off[c]:off[c + 1]]] == cells[j]).all() and off[c + 1] > off[c]
    np.savez(tmp_path / "trie.npz", **got)
    with np.load(tmp_path / "trie.npz") as z:
        back = ops.IdTrie.from_arrays({k: z[k] for k in z.files}, DEV)
    assert back.sizes == sizes and back.counts() == trie.counts()
    assert all(np.array_equal(v, got[k]) for k, v in back.to_arrays().items())
