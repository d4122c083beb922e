"""rqsid_probe_knn's method against its specification on the CPU (tests/_probe_model.py): per-item lists, one U per
query over all of them, the certificate; and why a query's ranges have to be disjoint."""
import numpy as np
import pytest

from tests import _knn_model as M
from tests import _probe_model as PM

N_Q = 200


@pytest.fixture(scope="module")
def fix():
    x = M.fixture_t()
    q = x[:N_Q]
    s, e = M.screen(q, x, "l2")
    xi = x.astype(np.int64)
    keys = ((xi[:N_Q, None, :] - xi[None, :, :]) ** 2).sum(-1).astype(np.float64)  # exact
    lo, hi = PM.t_ranges(N_Q)
    qself = np.arange(N_Q)
    want, _, scanned = PM.brute_force(q, x, 16, "l2", lo, hi, query_self=qself, keys=keys)
    assert (scanned == 900).all()
    return dict(x=x, q=q, s=s, e=e, keys=keys, lo=lo, hi=hi, qself=qself, want=want)


@pytest.mark.parametrize("slack", (0, 2, 8))
def test_method_equals_specification(fix, slack):
    f = fix
    for k in (1, 10, 16):
        got, all_rows = PM.lists_fold_certify(f["s"], f["e"], f["keys"], f["lo"], f["hi"], k, slack,
                                              query_self=f["qself"])
        assert (got == f["want"][:, :k]).all(), (k, slack)
        if k == 10:
            assert all_rows > 0  # the copies of row 7: no list of k + slack certifies


def test_the_fixture_ties_across_place_ten(fix):
    f = fix
    ok, _ = PM.eligible(f["lo"], f["hi"], len(f["x"]))  # (the self row included: a query may be a copy of row 7)
    srt = np.sort(np.where(ok, f["keys"], np.inf), axis=1)
    tied = srt[:, 9] == srt[:, 10]
    assert tied.sum() == 88
    assert max((srt[i] == srt[i, 9]).sum() for i in np.flatnonzero(tied)) == 41
    # the copies of row 7 lie in two ranges
    lo, hi = f["lo"][0], f["hi"][0]
    assert lo[0] <= 7 and 100 < hi[0] == lo[1] <= 139 < hi[1]


def test_a_row_listed_twice_breaks_the_bound(fix):
    """Each query's nearest row entered into a second list as well: U, the k-th smallest upper bound over the kept
    entries, then counts that row twice and falls below the true k-th key on some query, which loses a neighbour.
    This is why rqsid_probe_knn drops a range that overlaps an earlier one."""
    f = fix
    k = 10
    nearest = f["want"][:, 0]
    own = np.array([[c for c, (a, b) in enumerate(PM.T_RANGES) if a <= r < b][0] for r in nearest])
    twice = {i: ((own[i] + 1) % 3, int(nearest[i])) for i in range(N_Q)}
    got, _ = PM.lists_fold_certify(f["s"], f["e"], f["keys"], f["lo"], f["hi"], k, 8, query_self=f["qself"],
                                   also_listed=twice)
    differs = (got != f["want"][:, :k]).any(1)
    assert differs.any()
    # every query that differs lost a neighbour; none gained a wrong one
    for i in np.flatnonzero(differs):
        assert set(got[i][got[i] >= 0]) < set(f["want"][i, :k])


def test_clean_ranges():
    lo = np.array([[0, 50, 200, 10, 400]])
    hi = np.array([[100, 150, 190, 10, 2000]])
    clo, chi, word = PM.clean_ranges(lo, hi, 1000)
    assert word == PM.ERR_RANGE | PM.ERR_OVERLAP
    assert clo.tolist() == [[0, 50, 200, 10, 400]] and chi.tolist() == [[100, 50, 200, 10, 1000]]
    _, _, word = PM.clean_ranges([[0, 100, 100]], [[100, 100, 300]], 1000)
    assert word == 0  # adjacent ranges and an empty one on the seam do not overlap


def test_block_runs():
    """The blocks' runs as the GPU tests count them: G items per block by first tile, touching intervals merged."""
    assert [PM.items_per_block(v) for v in (1, 1023, 1024, 2047, 2048, 8192, 131071, 131072, 10**6)] == \
        [1, 1, 1, 1, 2, 8, 127, 128, 128]
    lo = np.array([[0, 300, 5000], [130, 5130, 9000]] * 1025)  # 6,150 items, 6 per block, 1,025 per range
    hi = np.array([[100, 400, 5050], [250, 5300, 9000]] * 1025)
    blocks = PM.block_runs(lo, hi, 10000)
    assert len(blocks) == 1025 and blocks[0] == [(0, 0)] and blocks[-1] == []  # (the empty items come last)
    assert blocks[170] == [(0, 1)] and blocks[341] == [(1, 3)]     # tiles 0 | 1 | 2-3 are adjacent and merge
    assert blocks[512] == [(2, 3), (39, 39)]                       # 35 tiles between: two runs
    assert blocks[683] == [(39, 41)]                               # 39 and 40-41 are adjacent
