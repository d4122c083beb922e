"""rqsid_silhouette on the GPU against the fp64 oracle (tests/_cluster_oracle.py), within the DERIVED bound of
DESIGN.md 3.3b (never a tuned one): per pair e = 1.01 u [(2 dim + 6)|q||x| + 3(|q|^2 + |x|^2)] >= |d2^ - d2|,
|d^ - d| <= min(sqrt e, e / d) + 2 u d, plus tile_rows u sum d for the fp32 sum inside a tile, 2^-24 relative for
the store of a and b, and the propagated bound for s."""
import numpy as np
import pytest
import torch

from generative_ranking_recommender_amd import ops
from tests import _cluster_oracle as CO

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
N_QUERIES = 257


def _fixture(seed, n, dim, blobs, spread, small):
    """Blobs plus, in this cluster order: the blobs, one EMPTY cluster, a singleton, a two-row cluster of bitwise
    duplicates, then `small` clusters of 1-3 rows; blob 0 also holds a bitwise duplicate pair."""
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((blobs, dim))
    lab = rng.integers(0, blobs, n)
    x = (centres[lab] + spread * rng.standard_normal((n, dim))).astype(np.float32)
    lab = lab.astype(np.int64)
    nxt = blobs + 1  # cluster `blobs` stays empty
    single = n - 1
    lab[single] = nxt
    pair = (n - 3, n - 2)
    x[pair[1]] = x[pair[0]]
    lab[list(pair)] = nxt + 1
    nxt += 2
    row = n - 4
    for c in range(small):
        for _ in range(1 + c % 3):
            lab[row] = nxt
            row -= 1
        nxt += 1
    in0 = np.nonzero(lab[:row] == 0)[0][:2]
    x[in0[1]] = x[in0[0]]
    return dict(x=x, lab=lab, n_clusters=nxt, single=single, pair=pair, in0=tuple(int(v) for v in in0), dim=dim,
                first_small=row + 1)


def _queries(fx, seed):
    rng = np.random.default_rng(seed)
    n = len(fx["x"])
    special = list(dict.fromkeys([fx["single"], *fx["pair"], *fx["in0"], fx["first_small"], fx["first_small"] + 1]))
    rest = rng.choice(np.setdiff1d(np.arange(n), special), N_QUERIES - len(special), replace=False)
    rows = np.concatenate([special, rest]).astype(np.int64)
    qself = rows.copy()
    qself[-40:] = -1  # scored like foreign rows: no self row, the own cluster divides by n_o
    return rows, qself.astype(np.int32), fx["lab"][rows].astype(np.int32)


class Case:
    def __init__(self, seed, n, dim, blobs, spread, small):
        fx = _fixture(seed, n, dim, blobs, spread, small)
        self.fx = fx
        dev = torch.device("cuda", 0)
        self.x = torch.from_numpy(fx["x"]).to(dev)
        b = ops.bucket(torch.from_numpy(fx["lab"]).to(dev).to(torch.int32), fx["n_clusters"])
        ops.check_error_words([b.error_word()], "rqsid_bucket")
        self.order, self.off = b.row_index, b.seg_row_off
        self.rows, qself, qseg = _queries(fx, seed + 1)
        self.q = self.x[torch.from_numpy(self.rows).to(dev)].contiguous()
        self.qself, self.qseg = torch.from_numpy(qself).to(dev), torch.from_numpy(qseg).to(dev)
        self.ref = CO.silhouette(fx["x"], self.order.cpu().numpy(), self.off.cpu().numpy(), fx["x"][self.rows], qself,
                                 qseg, dim_bound=dim, tile_rows=ops.silhouette_tile_rows())
        self.ws = ops.SilhouetteWorkspace(n, N_QUERIES, dev, 0)

    def run(self, x=None, q=None, qself="own", chunk_rows=0, ws=None):
        x = self.x if x is None else x
        q = self.q if q is None else q
        qself = self.qself if isinstance(qself, str) else qself
        ws = ws or (self.ws if chunk_rows == 0 else ops.SilhouetteWorkspace(len(x), len(q), x.device, chunk_rows))
        out = ops.silhouette(x, self.order, self.off, q, qself, self.qseg, chunk_rows=chunk_rows, workspace=ws,
                             check=False)
        assert int(ws.error_word().item()) == 0
        return [t.cpu().numpy() for t in out]


@pytest.fixture(scope="module")
def case_a():
    return Case(11, 3001, 64, 7, 0.7, 0)


@pytest.fixture(scope="module")
def case_b():
    return Case(23, 2500, 512, 12, 1.0, 500)


@pytest.fixture(scope="module", params=["a", "b"])
def case(request, case_a, case_b):
    return case_a if request.param == "a" else case_b


def test_fixture_has_the_shapes_that_matter(case):
    off = case.off.cpu().numpy()
    sizes = off[1:] - off[:-1]
    assert (sizes == 0).sum() >= 1 and (sizes == 1).sum() >= 1 and sizes.max() > ops.silhouette_tile_rows()
    assert off[-1] == len(case.fx["x"]) and N_QUERIES % ops.silhouette_tile_rows() != 0
    assert np.array_equal(case.fx["x"][case.fx["pair"][0]], case.fx["x"][case.fx["pair"][1]])
    if case.fx["dim"] == 512:  # tiles that straddle many clusters
        assert ((sizes >= 1) & (sizes <= 3)).sum() >= 500


def test_sums_within_the_derived_bound(case):
    a, b, b_seg, s = case.run()
    ref = case.ref
    qseg, qself = case.qseg.cpu().numpy(), case.qself.cpu().numpy()
    n_c, S, SB = ref["n_c"], ref["S"], ref["S_bound"]
    idx = np.arange(N_QUERIES)
    den_a = np.where(qself >= 0, n_c[qseg] - 1, n_c[qseg])
    da = np.where(den_a > 0, SB[idx, qseg] / np.maximum(den_a, 1), 0.0)
    err_a = np.abs(a.astype(np.float64) - ref["a"])
    print("a: max err / bound", float((err_a / np.maximum(da + U * ref["a"], 1e-300)).max()))
    assert (err_a <= da + U * (ref["a"] + da)).all()
    # the winning b against the oracle's mean of the cluster the kernel chose
    assert (b_seg >= 0).all() and (b_seg != qseg).all() and (n_c[b_seg] > 0).all()
    mean_hat = S[idx, b_seg] / n_c[b_seg]
    db_win = SB[idx, b_seg] / n_c[b_seg]
    err_b = np.abs(b.astype(np.float64) - mean_hat)
    print("b: max err / bound", float((err_b / (db_win + U * mean_hat)).max()))
    assert (err_b <= db_win + U * (mean_hat + db_win)).all()
    # b_seg: the oracle's wherever no other cluster's mean comes within the two bounds of the winner's
    clear = ref["b_clear"]
    print("b_seg: excluded as near ties", int((~clear).sum()), "of", N_QUERIES)
    assert (~clear).sum() <= 0.02 * N_QUERIES
    assert np.array_equal(b_seg[clear], ref["b_seg"][clear])
    # s: |s^ - s| <= (da + db + max(da, db)) / max(a^, b^) + 2^-24, db = how far the min of the means can move
    db = ref["b_err"]
    m_hat = np.maximum(a, b).astype(np.float64)
    ds = (da + db + np.maximum(da, db)) / m_hat + 2 * U
    err_s = np.abs(s.astype(np.float64) - ref["s"])
    print("s: max err", float(err_s.max()), "max err / bound", float((err_s / ds).max()))
    assert (err_s <= ds).all()


def test_self_row_is_excluded_by_index(case):
    fx, ref = case.fx, case.ref
    a, b, b_seg, s = case.run()
    # the singleton (query 0) scores 0, sklearn's rule
    assert case.rows[0] == fx["single"] and a[0] == 0 and s[0] == 0
    # without self rows the duplicate queries count their own row like any other: n_o instead of n_o - 1, and one
    # more distance (their own, equal to the duplicate's bit for bit, and NOT 0 in the expanded form in general)
    none = torch.full_like(case.qself, -1)
    a2, b2, b_seg2, s2 = case.run(qself=none)
    assert np.array_equal(b, b2) and np.array_equal(b_seg, b_seg2)
    qseg = case.qseg.cpu().numpy()
    x64 = fx["x"].astype(np.float64)
    for i in (1, 2, 3, 4):  # both rows of the two-row cluster, both duplicates inside blob 0
        n_o = ref["n_c"][qseg[i]]
        qn2 = float((x64[case.rows[i]] ** 2).sum())
        e = 1.01 * U * ((2 * fx["dim"] + 6) * qn2 + 6 * qn2)
        # with a self row the sum holds the duplicate's distance once, without it twice: d^(i, i) <= sqrt(e) each
        with_self, without = float(a[i]) * (n_o - 1), float(a2[i]) * n_o
        assert abs(without - with_self) <= np.sqrt(e) + 4 * U * (without + with_self)
        if n_o == 2:
            assert a[i] <= np.sqrt(e) and np.isfinite(s[i])
    assert np.array_equal(np.isnan(s2), np.isnan(s))


def test_chunking_moves_only_fp64_roundings(case):
    tile = ops.silhouette_tile_rows()
    base = case.run(chunk_rows=0)
    again = case.run(chunk_rows=0)
    for u, v in zip(base, again):
        assert u.tobytes() == v.tobytes()
    for cr in (tile, 2 * tile, 8 * tile):
        a, b, b_seg, s = case.run(chunk_rows=cr)
        np.testing.assert_allclose(a, base[0], rtol=1e-12, atol=0)
        np.testing.assert_allclose(b, base[1], rtol=1e-12, atol=0)
        assert np.array_equal(b_seg, base[2])
    sizes = np.diff(case.off.cpu().numpy())
    if case.fx["dim"] == 64:  # a cluster larger than several chunks; chunks then start mid-cluster
        assert sizes.max() > 3 * tile


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_16bit_rows_equal_the_widened_rows(case, dtype):
    x16, q16 = case.x.to(dtype), case.q.to(dtype)
    # binary16 subnormals and the edge of its normal range must be widened exactly too
    edge = torch.tensor([6e-8, 3e-6, -6.1e-5, 1000.0], device=x16.device).to(dtype)
    x16[5, :4] = edge
    q16[9, 4:8] = edge
    got = case.run(x=x16, q=q16)
    want = case.run(x=x16.float(), q=q16.float())
    for u, v in zip(got, want):
        assert u.tobytes() == v.tobytes()


def test_bad_query_seg_sets_bit_2_and_nothing_else(case_a):
    c = case_a
    qseg = c.qseg.clone()
    qseg[5] = c.fx["n_clusters"]  # one past the last cluster: a bounded index, taken as -1
    ws = ops.SilhouetteWorkspace(len(c.x), N_QUERIES, c.x.device, 0)
    a, b, b_seg, s = ops.silhouette(c.x, c.order, c.off, c.q, c.qself, qseg, workspace=ws, check=False)
    assert int(ws.error_word().item()) == 2
    assert float(a[5]) == 0.0 and int(b_seg[5]) >= 0
    with pytest.raises(RuntimeError):
        ops.silhouette(c.x, c.order, c.off, c.q, c.qself, qseg, workspace=ws)


def test_wrapper_checks_shapes_before_the_call(case_a):
    c = case_a
    with pytest.raises(ValueError):
        ops.silhouette(c.x, c.order, c.off, c.q.half(), c.qself, c.qseg)
    with pytest.raises(ValueError):
        ops.silhouette(c.x, c.order.long(), c.off, c.q, c.qself, c.qseg)
    with pytest.raises(ValueError):
        ops.silhouette(c.x, c.order, c.off, c.q, c.qself[:-1], c.qseg)
    with pytest.raises(ValueError):
        ops.silhouette(c.x.double(), c.order, c.off, c.q.double(), c.qself, c.qseg)
