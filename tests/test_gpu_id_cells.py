"""rqsid_id_cells on the GPU against ``np.lexsort((row, keybits, fine, group))``: every output array and counter for
equality, over the shapes where the kernel takes another path (one-wave and 256-thread groups, counted / sorted /
run-merged cells, several windows per group), every kind of key, skipped groups and the error word; then the layers
above it (ops.id_cells, RQEncoder.unique_ids, collision_report, prefix ranges, the trainer's two files)."""
import collections
import json
import math
import os
import types

import numpy as np
import pytest
import torch

from generative_ranking_recommender_amd import io as rq_io
from generative_ranking_recommender_amd import ops, synth
from generative_ranking_recommender_amd.collision_report import collision_report
from generative_ranking_recommender_amd.encode import (HIERARCHICAL_PREDICT_REFERENCE, HIERARCHICAL_TRAIN, RQEncoder)
from generative_ranking_recommender_amd.hierarchical_rq_kmeans import HierarchicalRQKMeansConfig
from generative_ranking_recommender_amd.quant_report import quantization_report

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
FINE_MAX = 8192
SKIP = 1


# ------------------------------------------------------------------------------------------------ the yardstick
def key_bits(key):
    """The float's place in a total order: -0 taken as +0, every NaN after +inf."""
    u = np.ascontiguousarray(key, dtype=np.float32).view(np.uint32).copy()
    u[u == 0x80000000] = 0
    out = np.where(u & 0x80000000, ~u, u | np.uint32(0x80000000)).astype(np.uint32)
    out[np.isnan(key)] = 0xFFFFFFFF
    return out


def model(n, row_index, seg_off, flags, fine, n_fine, key):
    """Every output of rqsid_id_cells for valid tables (fine may hold values outside [0, n_fine))."""
    n_groups = len(seg_off) - 1
    idx = np.arange(n) if row_index is None else row_index
    group_at = np.repeat(np.arange(n_groups), np.diff(seg_off))
    group = np.empty(n, np.int64)
    group[idx] = group_at
    f = np.zeros(n, np.int64) if fine is None else fine.astype(np.int64)
    kb = np.zeros(n, np.uint32) if key is None else key_bits(key)
    skipped = np.zeros(n, bool) if flags is None else (flags[group] & SKIP) != 0
    counted = ~skipped & (f >= 0) & (f < n_fine)
    rows = np.flatnonzero(counted)
    srt = rows[np.lexsort((rows, kb[rows], f[rows], group[rows]))]
    cell_key = group[srt] * n_fine + f[srt]
    uniq, start, count = np.unique(cell_key, return_index=True, return_counts=True)
    n_cells = len(uniq)
    cell_of = np.repeat(np.arange(n_cells), count)
    rank = np.full(n, -1, np.int32)
    size = np.full(n, -1, np.int32)
    cell = np.full(n, -1, np.int32)
    rank[srt] = np.arange(len(srt)) - start[cell_of]
    size[srt] = count[cell_of]
    cell[srt] = cell_of
    # positions: per group its cells, then the rows of the extra bin by row number; a skipped group as it came
    order = np.empty(n, np.int32)
    pos_of_sorted = np.empty(len(srt), np.int64)
    for g in range(n_groups):
        a, b = seg_off[g], seg_off[g + 1]
        members = idx[a:b]
        if flags is not None and flags[g] & SKIP:
            order[a:b] = members
            continue
        mine = np.flatnonzero(group[srt] == g) if b > a else np.zeros(0, np.int64)
        order[a:a + len(mine)] = srt[mine]
        pos_of_sorted[mine] = a + np.arange(len(mine))
        extra = np.sort(members[~counted[members]])
        order[a + len(mine):b] = extra
    cell_off = pos_of_sorted[start].astype(np.int32) if n_cells else np.zeros(0, np.int32)
    end = int(cell_off[-1] + count[-1]) if n_cells else 0
    ctr = np.zeros(37, np.int64)
    ctr[0] = n_cells
    ctr[1] = (count >= 2).sum()
    ctr[2] = count[count >= 2].sum()
    ctr[3] = (count == 1).sum()
    ctr[4] = count.max() if n_cells else 0
    for c in count:
        ctr[5 + int(c).bit_length() - 1] += 1
    return dict(order=order, rank=rank, size=size, cell=cell, cell_off=np.append(cell_off, end).astype(np.int32),
                cell_group=(uniq // n_fine).astype(np.int32), cell_fine=(uniq % n_fine).astype(np.int32), counters=ctr)


# ------------------------------------------------------------------------------------------------ the raw call
def t32(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(DEV)


class Call:
    """Device tensors of one rqsid_id_cells call; ``run`` enqueues it, ``read`` copies everything back."""

    def __init__(self, n, row_index, seg_off, flags, fine, n_fine, key):
        self.n, self.n_groups, self.n_fine = n, len(seg_off) - 1, n_fine
        self.idx, self.off, self.fine = t32(row_index), t32(seg_off), t32(fine)
        self.flags = None if flags is None else torch.from_numpy(np.ascontiguousarray(flags, np.uint8)).to(DEV)
        self.key = None if key is None else torch.from_numpy(np.ascontiguousarray(key, np.float32)).to(DEV)
        self.cap = min(n, self.n_groups * n_fine)
        self.out = {k: torch.full((m,), -7, dtype=torch.int32, device=DEV) for k, m in (
            ("order", n), ("rank", n), ("size", n), ("cell", n), ("cell_off", self.cap + 1), ("cell_group", self.cap),
            ("cell_fine", self.cap))}
        self.ws = ops.IdCellsWorkspace(n, self.n_groups, n_fine, DEV)

    def run(self):
        o = self.out
        rc = ops.lib().rqsid_id_cells(self.n, ops._ptr(self.idx), self.n_groups, ops._ptr(self.off),
                                      ops._ptr(self.flags), ops._ptr(self.fine), self.n_fine, ops._ptr(self.key),
                                      ops._ptr(o["order"]), ops._ptr(o["rank"]), ops._ptr(o["size"]),
                                      ops._ptr(o["cell"]), ops._ptr(o["cell_off"]), ops._ptr(o["cell_group"]),
                                      ops._ptr(o["cell_fine"]),
                                      ops._ptr(self.ws.buf), self.ws.bytes, ops._stream())
        assert rc == 0, ops.lib().rqsid_last_error().decode()
        return self

    def read(self):
        got = {k: v.cpu().numpy() for k, v in self.out.items()}
        got["counters"] = self.ws.counters().cpu().numpy().astype(np.int64)
        got["error"] = int(self.ws.error_word().item())
        return got


def compare(got, want, n_cells_written=True):
    n_cells = int(want["counters"][0])
    assert got["counters"].tolist() == want["counters"].tolist()
    for k in ("order", "rank", "size", "cell"):
        assert np.array_equal(got[k], want[k]), k
    assert np.array_equal(got["cell_off"][:n_cells + 1], want["cell_off"])
    assert np.array_equal(got["cell_group"][:n_cells], want["cell_group"])
    assert np.array_equal(got["cell_fine"][:n_cells], want["cell_fine"])
    # entries past n_cells are not written
    assert (got["cell_off"][n_cells + 1:] == -7).all() and (got["cell_group"][n_cells:] == -7).all()
    assert (got["cell_fine"][n_cells:] == -7).all()


def layout(group, n_groups, rng):
    """row_index / seg_row_off of rows with the given group keys, in a random order inside every segment."""
    n = len(group)
    shuffled = rng.permutation(n)
    row_index = shuffled[np.argsort(group[shuffled], kind="stable")]
    seg_off = np.concatenate([[0], np.cumsum(np.bincount(group, minlength=n_groups))])
    return row_index.astype(np.int32), seg_off.astype(np.int32)


def check(group, n_groups, fine, n_fine, key, flags=None, seed=0, error=0):
    rng = np.random.default_rng(seed)
    n = len(group)
    row_index, seg_off = layout(group, n_groups, rng)
    got = Call(n, row_index, seg_off, flags, fine, n_fine, key).run().read()
    assert got["error"] == error
    want = model(n, row_index, seg_off, flags, fine, n_fine, key)
    compare(got, want)
    return row_index, seg_off, got


SPECIAL = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1e-40, -1e-40, 1.0, -1.0, 1.0, 3.0e38, 1.4e-45],
                   dtype=np.float32)


def special_keys(n, rng):
    key = SPECIAL[rng.integers(0, len(SPECIAL), n)].copy()
    neg_nan = np.array([0xFFC00001], dtype=np.uint32).view(np.float32)[0]  # a NaN with the sign bit and a payload
    key[rng.random(n) < 0.05] = neg_nan
    return key


KEYS = {
    "null": lambda n, rng: None,
    "equal": lambda n, rng: np.full(n, 2.5, np.float32),
    "special": special_keys,
    "duplicated": lambda n, rng: rng.integers(0, 7, n).astype(np.float32) * 0.25,
    "random": lambda n, rng: rng.standard_normal(n).astype(np.float32),
}


# ------------------------------------------------------------------------------------------------ shapes and keys
@pytest.mark.parametrize("n", [1, 2, 257])
@pytest.mark.parametrize("keys", ["null", "special"])
def test_small_shapes(n, keys):
    rng = np.random.default_rng(n)
    group = rng.integers(0, 3, n)
    fine = rng.integers(0, 5, n).astype(np.int32)
    check(group, 3, fine, 5, KEYS[keys](n, rng))
    check(np.zeros(n, np.int64), 1, fine, 5, KEYS[keys](n, rng))  # one group


def test_zero_rows_touch_nothing():
    c = Call(0, None, np.zeros(4, np.int32), None, None, 3, None)
    c.ws.buf[4:152].fill_(9)
    got = c.run().read()
    assert (got["cell_off"] == -7).all() and (got["counters"] == 0x09090909).all() and got["error"] == 0
    ix = ops.id_cells(torch.zeros((0, 3), dtype=torch.int32, device=DEV))
    assert ix.n_cells == 0 and ix.order.numel() == 0 and ix.prefix_range([0]) == (0, 0, 0, 0)


@pytest.mark.parametrize("keys", sorted(KEYS))
def test_empty_groups_at_the_start_in_the_middle_and_at_the_end(keys):
    rng = np.random.default_rng(11)
    n = 900
    group = rng.choice([2, 3, 6, 7, 8], n)  # of 12 groups: 0, 1, 4, 5, 9, 10, 11 stay empty
    fine = rng.integers(0, 40, n).astype(np.int32)
    check(group, 12, fine, 40, KEYS[keys](n, rng))


@pytest.mark.parametrize("keys", ["null", "duplicated"])
def test_one_cell_per_group_with_null_fine_id(keys):
    rng = np.random.default_rng(12)
    n = 5000
    group = np.minimum(rng.geometric(0.02, n), 299)  # sizes from 0 to a few hundred: counted and sorted cells
    group[:2100] = 299                               # one cell beyond the LDS buffer, in a 256-thread group
    check(group, 300, None, 1, KEYS[keys](n, rng))


def test_the_widest_fine_level_with_three_occupied_values():
    rng = np.random.default_rng(13)
    n = 700
    group = rng.integers(0, 2, n)
    fine = rng.choice([0, 4097, FINE_MAX - 1], n).astype(np.int32)
    check(group, 2, fine, FINE_MAX, KEYS["random"](n, rng))


@pytest.mark.parametrize("keys", ["null", "equal", "special", "duplicated"])
def test_cell_sizes_around_every_threshold(keys):
    """1, 2, 63, 64, 65, C - 1, C, C + 1 and 2C + 3 in one call (C = rqsid_id_cells_lds_rows()): counting, the sort in
    one piece and the run merge, in one-wave and in 256-thread groups."""
    C = ops.id_cells_lds_rows()
    cells = [(0, 0, 1), (0, 1, 2), (0, 2, 63), (0, 3, 64), (0, 5, 65),  # a one-wave group
             (1, 1, C - 1), (1, 2, C),                                  # 256 threads, two windows
             (2, 0, C + 1), (2, 7, 2 * C + 3),                          # run merges
             (4, 3, C + 5), (4, 4, 2)]                                  # a run merge on one wave
    group = np.concatenate([np.full(s, g) for g, f, s in cells])
    fine = np.concatenate([np.full(s, f) for g, f, s in cells]).astype(np.int32)
    rng = np.random.default_rng(14)
    _, _, got = check(group, 5, fine, 8, KEYS[keys](len(group), rng))
    assert sorted(np.diff(got["cell_off"][:12]).tolist()) == sorted(s for _, _, s in cells)


@pytest.mark.parametrize("keys", ["null", "random"])
def test_a_large_group_beside_many_small_ones(keys):
    rng = np.random.default_rng(15)
    small = np.repeat(np.arange(1, 501), rng.integers(0, 4, 500))
    group = np.concatenate([np.full(70_000, 0), small])
    fine = np.concatenate([rng.integers(0, 3, 70_000), rng.integers(0, 200, len(small))]).astype(np.int32)
    check(group, 501, fine, 200, KEYS[keys](len(group), rng))


@pytest.mark.parametrize("rows, n_fine", [(1500, 64), (3000, 256), (5000, 2)])
def test_several_windows_per_group(rows, n_fine):
    """Groups whose cells fill the LDS buffer more than once (and, with 2 fine values, cells beyond it)."""
    rng = np.random.default_rng(rows)
    group = np.concatenate([np.zeros(rows, np.int64), np.ones(rows // 3, np.int64)])
    fine = rng.integers(0, n_fine, len(group)).astype(np.int32)
    check(group, 2, fine, n_fine, KEYS["duplicated"](len(group), rng))


# ------------------------------------------------------------------------------------------------ invariance
@pytest.fixture(scope="module")
def mixed():
    rng = np.random.default_rng(21)
    n = 6000
    group = np.minimum(rng.geometric(0.01, n), 63)
    group[:1700] = 40
    fine = rng.integers(0, 6, n).astype(np.int32)
    key = special_keys(n, rng)
    return n, group, fine, key


def test_a_permutation_inside_segments_and_a_second_call_change_no_byte(mixed):
    n, group, fine, key = mixed
    results = []
    for seed in (1, 1, 2, 3):
        row_index, seg_off = layout(group, 64, np.random.default_rng(seed))
        results.append(Call(n, row_index, seg_off, None, fine, 6, key).run().read())
    n_cells = int(results[0]["counters"][0])
    for other in results[1:]:
        for k, v in results[0].items():
            m = {"cell_off": n_cells + 1, "cell_group": n_cells, "cell_fine": n_cells}.get(k)
            assert np.array_equal(v[:m], other[k][:m]) if m is not None else np.array_equal(v, other[k]), k


def test_identity_row_index_and_the_output_of_rqsid_bucket(mixed):
    n, group, fine, key = mixed
    seg_off = np.concatenate([[0], np.cumsum(np.bincount(np.sort(group), minlength=64))]).astype(np.int32)
    order = np.argsort(group, kind="stable")
    got = Call(n, None, seg_off, None, fine[order], 6, key[order]).run().read()  # rows already grouped
    compare(got, model(n, None, seg_off, None, fine[order], 6, key[order]))
    b = ops.bucket(t32(group), 64)
    c = Call(n, None, seg_off, None, fine, 6, key)
    c.idx, c.off = b.row_index, b.seg_row_off
    compare(c.run().read(), model(n, b.row_index.cpu().numpy(), seg_off, None, fine, 6, key))


def test_one_graph_replay_equals_the_eager_call(mixed):
    n, group, fine, key = mixed
    row_index, seg_off = layout(group, 64, np.random.default_rng(5))
    eager = Call(n, row_index, seg_off, None, fine, 6, key).run().read()
    c = Call(n, row_index, seg_off, None, fine, 6, key)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        c.run()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for v in c.out.values():
        v.fill_(-7)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):  # one stream, no parallel branches
        c.run()
    g.replay()
    torch.cuda.synchronize()
    got = c.read()
    for k, v in eager.items():
        assert np.array_equal(v, got[k]), k
    del g


# --------------------------------------------------------------------------------------- skipped groups, errors
def test_skipped_groups_get_minus_one_keep_their_order_and_are_not_counted(mixed):
    n, group, fine, key = mixed
    flags = np.zeros(64, np.uint8)
    flags[[0, 7, 40, 63]] = SKIP  # empty, small, the 256-thread group, the last
    row_index, seg_off, got = check(group, 64, fine, 6, key, flags=flags)
    for g in (7, 40, 63):
        a, b = seg_off[g], seg_off[g + 1]
        assert b > a and np.array_equal(got["order"][a:b], row_index[a:b])
        assert (got["rank"][row_index[a:b]] == -1).all() and (got["cell"][row_index[a:b]] == -1).all()
    assert not np.isin(got["cell_group"][:got["counters"][0]], [7, 40, 63]).any()
    assert got["counters"][2] + got["counters"][3] == (~np.isin(group, [7, 40, 63])).sum()


def test_an_out_of_range_fine_id_sets_bit_4_and_spares_the_other_rows(mixed):
    n, group, fine, key = mixed
    bad = fine.copy()
    bad[[5, 1701, 3000, 5999]] = [6, -1, 2**31 - 1, -2**31]
    check(group, 64, bad, 6, key, error=4)
    # through the wrapper: a negative ID parks its row, one at or above the level's size raises under check
    ids = torch.from_numpy(np.stack([group, fine], 1).astype(np.int32)).to(DEV)
    ids[5, 1] = -1
    ix = ops.id_cells(ids, sizes=[64, 6])
    assert ix.n_invalid == 1 and int(ix.rank[5].item()) == -1 and int(ix.order[-1].item()) == 5
    ids[6, 1] = 6
    with pytest.raises(RuntimeError, match="rqsid_id_cells"):
        ops.id_cells(ids, sizes=[64, 6])
    ix = ops.id_cells(ids, sizes=[64, 6], check=False)
    keep = np.ones(n, bool)
    keep[[5, 6]] = False
    # the other rows are what they are without rows 5 and 6 (no key: the order inside a cell is the rows')
    part = model(keep.sum(), *layout(group[keep], 64, np.random.default_rng(0)), None, fine[keep], 6, None)
    assert ix.n_cells == part["counters"][0]
    assert ix.counters.cpu().numpy().tolist() == part["counters"].tolist()
    for k in ("rank", "size", "cell"):
        assert np.array_equal(getattr(ix, k).cpu().numpy()[keep], part[k]), k
        assert (getattr(ix, k).cpu().numpy()[~keep] == -1).all()
    with pytest.raises(ValueError):
        ops.id_cells(ids, sizes=[64, FINE_MAX + 1])
    with pytest.raises(ValueError):
        ops.id_cells(torch.zeros((4, 3), dtype=torch.int32, device=DEV), sizes=[4097, 4097, 2])


# ------------------------------------------------------------------------------------------------ encoder level
NEED = [16, 16, 32]


@pytest.fixture(scope="module")
def encoded():
    cb = synth.encode_codebooks(seed=5, need=tuple(NEED), n_cand=320, pool_rows=8192)
    x = torch.from_numpy(synth.mixture_rows(0, 3000)).to(DEV)
    enc = RQEncoder([torch.from_numpy(cb[k]) for k in ("c0", "c1", "c2")], NEED, match=torch.from_numpy(cb["match"]),
                    semantics=HIERARCHICAL_TRAIN, device=DEV)
    enc1 = RQEncoder([torch.from_numpy(cb["c0"])], NEED[:1], semantics=HIERARCHICAL_TRAIN, device=DEV)
    return cb, x, enc, enc1


def _check_unique(enc, x):
    qe = enc.quant_error(x)
    uniq = enc.unique_ids(x).cpu().numpy()
    ids, rec = qe.ids.cpu().numpy(), qe.recon_err.cpu().numpy()
    L = ids.shape[1]
    assert uniq.dtype == np.int32 and uniq.shape == (len(ids), L + 1) and np.array_equal(uniq[:, :L], ids)
    assert len({tuple(r) for r in uniq.tolist()}) == len(uniq)  # pairwise distinct
    members = collections.defaultdict(list)
    for i, t in enumerate(map(tuple, ids.tolist())):
        members[t].append(i)
    assert max(map(len, members.values())) >= 2  # (the data do collide)
    for rows in members.values():
        assert sorted(uniq[rows, L].tolist()) == list(range(len(rows)))  # every token below its cell's size
        best = rows[int(np.argmin(uniq[rows, L]))]
        assert rec[best] == rec[rows].min()  # token 0: the smallest recon
        by_rank = [rows[j] for j in np.argsort(uniq[rows, L])]
        assert by_rank == sorted(rows, key=lambda r: (rec[r], r))
    return ids, members


def test_unique_ids(encoded):
    cb, x, enc, enc1 = encoded
    _check_unique(enc, x)
    _check_unique(enc1, x)
    quirks = RQEncoder([torch.from_numpy(cb[k]) for k in ("c0", "c1", "c2")], NEED,
                       semantics=HIERARCHICAL_PREDICT_REFERENCE, device=DEV)
    with pytest.raises(ValueError):
        quirks.unique_ids(x)


def _five(v):
    v = np.asarray(v, dtype=np.float64)
    return {"mean": float(v.mean()), "min": float(v.min()), "max": float(v.max()), "median": float(np.median(v)),
            "std": float(v.std())}


def _approx_five(got, want):
    assert set(got) == set(want)
    for k in want:
        assert got[k] == pytest.approx(want[k], rel=1e-12, abs=1e-12), k


@pytest.mark.parametrize("which", ["three_levels", "one_level"])
def test_collision_report_against_a_counter_restatement(encoded, which):
    cb, x, enc, enc1 = encoded
    enc = enc if which == "three_levels" else enc1
    ids, members = _check_unique(enc, x)
    rec = enc.quant_error(x).recon_err.cpu().numpy()
    rep = collision_report(enc, x, top=5, members=10)
    q = quantization_report(enc, x)
    L = ids.shape[1]
    tuples = list(map(tuple, ids.tolist()))
    counts = collections.Counter(tuples)
    assert rep["rows"] == len(ids) == q["rows"] and rep["rows_without_id"] == 0
    assert rep["unique_semantic_ids"] == q["unique_semantic_ids"] == len(counts)
    assert rep["coverage"] == q["coverage"]
    shared = {t: c for t, c in counts.items() if c >= 2}
    assert rep["colliding_ids"] == len(shared)
    assert rep["rows_in_collisions"] == sum(shared.values())
    assert rep["max_collision"] == max(shared.values())
    once = sum(1 for c in counts.values() if c == 1)
    assert rep["ids_used_once"] == once and rep["ids_used_once_share"] == once / len(counts)
    assert rep["rows_per_id"] == len(ids) / len(counts)
    hist = collections.Counter(1 << (c.bit_length() - 1) for c in counts.values())
    assert rep["size_histogram"] == {str(k): v for k, v in sorted(hist.items())}
    assert rep["dedup_token_bits"] == math.ceil(math.log2(max(counts.values())))
    ranked = sorted(counts.items(), key=lambda kv: (-kv[1], kv[0]))
    assert rep["most_common"] == [{"semantic_id": list(t), "size": c} for t, c in ranked[:10]]
    assert rep["worst"] == [{"semantic_id": list(t), "size": c,
                             "rows": sorted(members[t], key=lambda r: (rec[r], r))[:10]} for t, c in ranked[:5]]
    assert rep["level_unique_ids"] == [len(set(ids[:, l].tolist())) for l in range(L)]
    if L == 1:
        assert "prefixes" not in rep
        return
    last = collections.defaultdict(set)
    prows = collections.Counter()
    for t in tuples:
        last[t[:-1]].add(t[-1])
        prows[t[:-1]] += 1
    p = rep["prefixes"]
    assert p["depth"] == L - 1 and p["used"] == len(last) and p["possible"] == NEED[0] * NEED[1]
    assert p["share"] == len(last) / (NEED[0] * NEED[1])
    _approx_five(p["last_level_ids"], _five([len(v) for v in last.values()]))
    _approx_five(p["rows"], _five(list(prows.values())))
    fewest = sorted(prows.items(), key=lambda kv: (kv[1], kv[0]))[:10]
    assert p["fewest_rows"] == [{"prefix": list(t), "rows": c, "last_level_ids": len(last[t])} for t, c in fewest]


def test_prefix_range_against_a_mask(encoded):
    cb, x, enc, enc1 = encoded
    ids_d = enc.encode(x)
    ids = ids_d.cpu().numpy()
    ix = enc.id_index(ids_d)
    order = ix.order.cpu().numpy()
    cells = ix.ids_of(torch.arange(ix.n_cells, device=DEV)).cpu().numpy()
    assert np.array_equal(cells, np.unique(ids, axis=0))  # the cells in lexicographic ID order
    own = (ids[:, :2] == ids[0, :2]).all(1)
    absent = next(v for v in range(ix.sizes[2]) if not (own & (ids[:, 2] == v)).any())
    prefixes = [tuple(ids[i, :d]) for i in (0, 1234, 2999) for d in (1, 2, 3)] + [
        (int(ids[0, 0]), int(ids[0, 1]), absent), (99,)]
    for prefix in prefixes:
        c0, c1, p0, p1 = ix.prefix_range(prefix)
        mask = (ids[:, :len(prefix)] == np.array(prefix)).all(1) if max(prefix) < 99 else np.zeros(len(ids), bool)
        assert p1 - p0 == mask.sum() and sorted(order[p0:p1].tolist()) == np.flatnonzero(mask).tolist()
        assert c1 - c0 == len(np.unique(ids[mask], axis=0)) if mask.any() else c1 == c0
        assert (cells[c0:c1, :len(prefix)] == np.array(prefix)).all()
    with pytest.raises(ValueError):
        ix.prefix_range(())


TRAIN_CFG = dict(layer_clusters=[4, 8, 8], need_clusters=[4, 4, 4], embedding_dim=64, iter_limit=3)


def _trainer_cfg(root, csv_path):
    return types.SimpleNamespace(
        output_dir=os.path.join(root, "outputs"), model_dir=os.path.join(root, "models"),
        h_rqkmeans_test=HierarchicalRQKMeansConfig(**TRAIN_CFG), h_rqkmeans=None,
        data=types.SimpleNamespace(song_vectors_file=csv_path,
                                   semantic_ids_file=os.path.join(root, "outputs", "semantic_id",
                                                                  "song_semantic_ids.jsonl")))


def test_trainer_writes_the_collision_report_and_the_unique_ids(tmp_path):
    from generative_ranking_recommender_amd.train_semantic_ids import SemanticIDTrainer
    x = synth.small_mixture(600, d=64, m=16, seed=5)
    csv_path = str(tmp_path / "vec.csv")
    rq_io.write_song_vectors(csv_path, [f"song{i}" for i in range(len(x))], x)
    written = {}
    for name, kw in (("plain", {}), ("cells", dict(report_collisions=True, dedup_token=True))):
        np.random.seed(7)
        torch.manual_seed(7)
        root = str(tmp_path / name)
        result = SemanticIDTrainer(_trainer_cfg(root, csv_path), use_test_config=True, device=DEV, **kw).train(
            resume=False)
        with open(os.path.join(root, "outputs", "semantic_id", "song_semantic_ids.jsonl"), "rb") as f:
            written[name] = f.read()
    assert written["plain"] == written["cells"] and len(written["plain"]) > 0
    out = os.path.join(str(tmp_path / "cells"), "outputs", "semantic_id")
    assert not os.path.exists(os.path.join(str(tmp_path / "plain"), "outputs", "semantic_id", "collision_report.json"))
    with open(os.path.join(out, "collision_report.json")) as f:
        rep = json.load(f)
    assert rep == result["collision_report"] and rep["rows"] == len(x)
    assert rep["unique_semantic_ids"] + rep["rows_in_collisions"] - rep["colliding_ids"] == len(x)
    with open(os.path.join(out, "song_semantic_ids_unique.jsonl")) as f:
        lines = [json.loads(l) for l in f]
    assert len(lines) == len(x)
    tuples = [tuple(l["semantic_ids"]) for l in lines]
    assert [l["song_id"] for l in lines] == [f"song{i}" for i in range(len(x))]
    assert all(len(t) == 4 for t in tuples) and len(set(tuples)) == len(x)
    assert [list(t[:3]) for t in tuples] == [json.loads(l)["semantic_ids"] for l in written["cells"].splitlines()]
    model_ = result["model"]
    count, rows = model_.find_rows_by_prefix(tuples[0][:2], limit=3)
    pred = model_.predict(x, reference_quirks=False)
    assert count == (pred[:, :2] == np.array(tuples[0][:2])).all(1).sum() and len(rows) == min(3, count)
    assert (pred[rows, :2] == np.array(tuples[0][:2])).all()
    # the multi-GPU form is refused in the constructor, before any training (the group is never touched)
    for kw in (dict(report_collisions=True), dict(dedup_token=True)):
        with pytest.raises(NotImplementedError):
            SemanticIDTrainer(_trainer_cfg(str(tmp_path / "g"), csv_path), use_test_config=True, device=DEV,
                              group=object(), **kw)
