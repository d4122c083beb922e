"""The kernels of one Lloyd iteration (csrc/rqsid.hip) against fp64 references at tile, dim and segment edges.

Bars (tests/_lloyd_model.py; tests/test_lloyd_model.py shows on the CPU that the numpy references meet them and
that an fp32-accumulating centroid does not): centroid means within 0.5 ulp32 + count 2^-52 mean|x| of the exact
mean, fp64 sums within count 2^-52 sum|x|; plain residuals and group weights bit-equal to the oracle, normalised
residuals within 1 ulp on fewer than 1e-3 of the elements; fp32 distances inside ``dist_interval32``, cosine
distances inside ``cosine_interval``, fp16 scores equal to the oracle's or both inside the any-summation-order
interval (``O.uncertified`` empty); candidate lists and greedy matches equal to numpy's.

Kernel branch -> the case that runs it
  centroid_accumulate  d0 loop's break (dim <= 256, dim % 256 != 0)   test_centroid_update_edges[dim 1/255/257-*]
                       4-row unroll tail (1..5 rows), one-row tile     sizes "edges": 1, 2, 3, 4, 5 and 513
                       tile edges 255 / 256 / 257 / 513                sizes "edges"
                       tile_off search over equal entries              sizes "edges" (leading, trailing, runs of
                                                                       empties), "all_in_last"; k = 1: "k1"
                       rows outside [0, k) dropped                     test_centroid_keys_outside_the_clusters
  centroid_finalize    count <= 0 keeps prev                           test_centroid_update_edges (bit-equal prev)
  centroid_sums        the fp64 sums themselves                        test_centroid_update_edges
  residual             grid-stride loop (n > 32768)                    test_residual_rows[32773]
                       one lane active (dim 4); partial second pass    test_residual_dims[4-*], [260-*], [36-*]
                       group edges inside a float4; 16 groups          kinds "5_7_rest", "1_rest", "16_uneven"
                       den = 1e-8 (zero group)                         rows 0 and 1 of every residual case
  scale_groups         tail block, 1 / 3 / 16 groups                   test_scale_groups
  pairwise_distance    row / centre tiles of 1, 63, 64, 65, 2 tiles+   test_distances[*] (distance_shapes)
                       dim 32 (one pass) .. 1024                       test_distances[65x65x32 .. 1024]
                       d^2 <= 0 clamp; mode 2's 1e-5 clamp             rows equal to a centre (distance_case)
                       worker-major layout, nothing past k n           test_score_layout_and_bounds
  SEG form             leading / trailing / runs of empty segments,    test_segmented_scores[*]
                       partial tiles, centres s k .. s k + k - 1
  match_to_candidates  bucket_scan run length 1 -> 2 -> 3 (1024 /      test_match_lists[1023/1024/1025/2049-*]
                       1025 / 2049 groups); n_cand < 64, = 64, > 64    n_cand 1, 63, 64, 65, 130
                       bytes other than 0 / 1, all-ones, empty rows    match_case; bool input: test_match_lists_bool
  greedy_match         equal minima across lanes and waves; C < 256;   test_greedy_match_edges[3/255/257]
                       +inf columns; more sub-centres than columns;
                       max_take 0
  wrappers             dtype, group_dims, dim and group-count checks   test_wrappers_refuse_*"""
import numpy as np
import pytest
import torch

from generative_ranking_recommender_amd import ops
from oracle import rq_oracle as O
from tests import _lloyd_model as M

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
F32 = np.float32
POISON16 = 0x7B5A  # an fp16 bit pattern (a finite 60224) no score takes


def gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _ids(shapes):
    return ["x".join(map(str, s)) for s in shapes]


# ---------------------------------------------------------------------------
# centroid update / sums
# ---------------------------------------------------------------------------
def _check_centroids(x, a, k, prev):
    """ops.centroid_update and ops.centroid_sums of rows x with keys a against ``M.centroid_ref``."""
    sums, counts, mean, tol, sum_tol = M.centroid_ref(x, a, k)
    cen, cnt = ops.centroid_update(gpu(x), gpu(a.astype(np.int32)), k, gpu(prev.copy()))
    cen, cnt = cen.cpu().numpy(), cnt.cpu().numpy()
    assert np.array_equal(cnt, counts)
    full = counts > 0
    err = np.abs(cen.astype(np.float64) - mean)
    print(f"centroid: worst error / bound = {(err[full] / tol[full]).max() if full.any() else 0:.4f}")
    assert (err[full] <= tol[full]).all(), f"{int((err[full] > tol[full]).sum())} means outside the bound"
    assert np.array_equal(cen[~full].view(np.int32), prev[~full].view(np.int32))  # empty clusters keep prev's bits
    s, cnt2 = ops.centroid_sums(gpu(x), gpu(a), k)
    s = s.cpu().numpy()
    assert s.dtype == np.float64 and np.array_equal(cnt2.cpu().numpy(), counts)
    serr = np.abs(s.astype(np.longdouble) - sums).astype(np.float64)
    assert (serr <= sum_tol).all(), f"{int((serr > sum_tol).sum())} sums outside the bound"
    return cen


@pytest.mark.parametrize("case", list(M.CLUSTER_SIZES))
@pytest.mark.parametrize("dim", [1, 255, 256, 257, 512, 1024])
def test_centroid_update_edges(dim, case):
    sizes = M.CLUSTER_SIZES[case]
    k = len(sizes)
    x = M.mixed_magnitude_rows(int(np.sum(sizes)), dim, seed=dim)
    a = M.shuffled_assignment(sizes, seed=dim + 1)
    prev = np.random.default_rng(dim + 2).standard_normal((k, dim)).astype(F32)
    _check_centroids(x, a, k, prev)


def test_centroid_keys_outside_the_clusters():
    """Rows whose key lies outside [0, k) belong to no cluster (include/rqsid.h rqsid_centroid_accumulate): they
    enter no sum and no count, and the other clusters' means are those of the same rows without them."""
    sizes = [3, 0, 257, 40]
    k, dim = len(sizes), 260
    x = M.mixed_magnitude_rows(int(np.sum(sizes)) + 64, dim, seed=11)
    a = np.concatenate([M.shuffled_assignment(sizes, seed=12),
                        np.tile(np.array([-1, k, k + 3, 2 ** 31 - 1, -2 ** 31, 1000, -7, 65536]), 8)])
    perm = np.random.default_rng(13).permutation(len(a))
    x, a = x[perm], a[perm]
    prev = np.random.default_rng(14).standard_normal((k, dim)).astype(F32)
    cen = _check_centroids(x, a, k, prev)
    keep = (a >= 0) & (a < k)
    alone = ops.centroid_update(gpu(x[keep]), gpu(a[keep].astype(np.int32)), k, gpu(prev.copy()))[0].cpu().numpy()
    assert np.array_equal(cen[[1]], prev[[1]])
    # the same rows in the same relative order; fp64 tile sums may combine in another order: the derived bound twice
    _, counts, _, tol, _ = M.centroid_ref(x, a, k)
    assert (np.abs(cen.astype(np.float64) - alone)[counts > 0] <= 2 * tol[counts > 0]).all()


# ---------------------------------------------------------------------------
# residual / scale_groups
# ---------------------------------------------------------------------------
def _check_residual(n, dim):
    for kind, gd in M.group_kinds(dim).items():
        x, c, ids = M.residual_case(n, dim, 7, seed=M.residual_seed(n, dim), zero_groups=[(0, gd[0])])
        xg, cg, ig = gpu(x), gpu(c), gpu(ids.astype(np.int32))
        plain = ops.residual(xg, cg, ig, gd, False).cpu().numpy()
        assert np.array_equal(plain.view(np.int32), O.residual(x, c, ids, gd, False).view(np.int32)), kind
        got = ops.residual(xg, cg, ig, gd, True).cpu().numpy()
        mx, frac, ok = M.residual_close(got, O.residual(x, c, ids, gd, True))
        print(f"residual n={n} dim={dim} {kind}: max {mx} ulp, differing fraction {frac:.2e}")
        assert ok, f"{kind}: max {mx} ulp, {frac:.2e} of the elements differ"
        assert (got[0] == 0).all(), kind                # every group zero: exactly 0.0
        if n > 1:
            assert (got[1, :gd[0]] == 0).all(), kind    # one zero group beside non-zero ones


@pytest.mark.parametrize("n", [1, 3, 4, 5, M.GRID_STRIDE_ROWS])
def test_residual_rows(n):
    _check_residual(n, 32)


@pytest.mark.parametrize("dim", [4, 36, 256, 260, 512, 1024])
def test_residual_dims(dim):
    _check_residual(257, dim)


def test_residual_writes_into_out():
    x, c, ids = M.residual_case(5, 36, 3, seed=1)
    out = torch.full((5, 36), 7.0, device=DEV)
    ret = ops.residual(gpu(x), gpu(c), gpu(ids.astype(np.int32)), [36], False, out=out)
    assert ret is out and np.array_equal(out.cpu().numpy(), O.residual(x, c, ids, [36], False))


@pytest.mark.parametrize("n,dim,n_groups", [(7, 1, 1), (7, 33, 1), (7, 33, 3), (7, 33, 16), (7, 512, 1), (7, 512, 3),
                                            (7, 512, 16), (300, 33, 16)])
def test_scale_groups(n, dim, n_groups):
    """n dim is no multiple of the 256-thread block wherever dim allows it (7 x 512 cannot be)."""
    gd = M.uneven_groups(dim, n_groups)
    w = [float(F32(0.3 + 0.17 * i)) for i in range(n_groups)]
    x = M.mixed_magnitude_rows(n, dim, seed=dim + n_groups)
    got = ops.scale_groups(gpu(x), gd, w).cpu().numpy()
    assert np.array_equal(got.view(np.int32), O.apply_weights(x, gd, w).view(np.int32))


# ---------------------------------------------------------------------------
# distances
# ---------------------------------------------------------------------------
SHAPES = M.distance_shapes()


def _inside(got, lo, hi, what):
    got = np.asarray(got, np.float64)
    out = (got < lo) | (got > hi) | np.isnan(got)
    assert not out.any(), f"{what}: {int(out.sum())} of {out.size} outside the interval, first at {np.argwhere(out)[0]}"


@pytest.mark.parametrize("n,k,dim", SHAPES, ids=_ids(SHAPES))
def test_distances(n, k, dim):
    x, c = M.distance_case(n, k, dim, seed=n + k + dim)
    xg, cg = gpu(x), gpu(c)
    # mode 0
    _inside(ops.pairwise_distance(xg, cg).cpu().numpy(), *M.dist_interval32(x, c), "pairwise_distance")
    # mode 3, fp32 and worker-major fp16 scores
    _inside(ops.pairwise_cosine(xg, cg).cpu().numpy(), *M.cosine_interval(x, c), "pairwise_cosine")
    w = ops.pairwise_cosine(xg, cg, scores=True).cpu().numpy()
    assert w.shape == (k, n) and w.dtype == np.float16
    _inside(w, *M.cosine_score_interval(x, c), "pairwise_cosine scores")
    # modes 1 and 2: the oracle's value, or both inside what any summation order can give
    for half, ref_fn in ((False, M.full_scores_ref), (True, M.half_scores_ref)):
        w = ops.auction_scores(xg, cg, half=half).cpu().numpy()
        assert w.shape == (k, n) and w.dtype == np.float16
        ref, lo, hi = ref_fn(x, c)
        got = -w.T.astype(np.float64)
        bad = O.uncertified(got, ref, lo, hi)
        print(f"{n}x{k}x{dim} half={half}: {int((got != ref).sum())} entries differ from the oracle, {int(bad.sum())} uncertified")
        assert not bad.any(), f"half={half}: {int(bad.sum())} uncertified entries, first at {np.argwhere(bad)[0]}"
        if half:
            assert (got >= float(np.float16(1e-5))).all()  # the clamp: no score of -0


def _poisoned(n_values, extra=257):
    return torch.full((n_values + extra,), POISON16, dtype=torch.int16, device=DEV)


LAYOUT_SHAPES = [(65, 65, 96), (130, 3, 32), (1, 129, 32)]


@pytest.mark.parametrize("n,k,dim", LAYOUT_SHAPES, ids=_ids(LAYOUT_SHAPES))
def test_score_layout_and_bounds(n, k, dim):
    """w[c][r] is row r's score for centre c for every r < n, and an oversize poison-filled buffer keeps its
    bytes past k n (the C ABI called on a buffer of our own)."""
    x, c = M.distance_case(n, k, dim, seed=n + k)
    xg, cg = gpu(x), gpu(c)
    lib, st = ops.lib(), torch.cuda.current_stream().cuda_stream
    calls = {
        "full": lambda p: lib.rqsid_auction_scores(xg.data_ptr(), n, dim, cg.data_ptr(), k, 0, p, st),
        "half": lambda p: lib.rqsid_auction_scores(xg.data_ptr(), n, dim, cg.data_ptr(), k, 1, p, st),
        "cosine": lambda p: lib.rqsid_pairwise_cosine(xg.data_ptr(), n, dim, cg.data_ptr(), k, None, p, st),
    }
    wrappers = {"full": lambda: ops.auction_scores(xg, cg), "half": lambda: ops.auction_scores(xg, cg, half=True),
                "cosine": lambda: ops.pairwise_cosine(xg, cg, scores=True)}
    slo, shi = M.cosine_score_interval(x, c)
    for name, call in calls.items():
        buf = _poisoned(k * n)
        assert call(buf.data_ptr()) == 0, name
        out = buf.cpu().numpy()
        assert (out[k * n:] == np.int16(POISON16)).all(), f"{name}: wrote past k n"
        w = out[:k * n].view(np.float16).reshape(k, n)
        assert not (out[:k * n] == np.int16(POISON16)).any(), f"{name}: left a score unwritten"
        assert np.array_equal(w.view(np.int16), wrappers[name]().cpu().numpy().view(np.int16)), name
        # every entry sits where its (centre, row) pair belongs: w[c][r] is certified as the score of row r and
        # centre c (a transposed or strided layout would be off by whole distances)
        if name == "cosine":
            _inside(w, slo, shi, name)
        else:
            ref, lo, hi = (M.half_scores_ref if name == "half" else M.full_scores_ref)(x, c)
            assert not O.uncertified(-w.T.astype(np.float64), ref, lo, hi).any(), name


# ---------------------------------------------------------------------------
# segmented scores
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("k", [3, 65])
@pytest.mark.parametrize("sizes", M.SEGMENT_SIZES, ids=lambda s: "-".join(map(str, s)))
def test_segmented_scores(sizes, k, half):
    dim = 96
    x, c, off = M.segment_case(sizes, k, dim, seed=len(sizes) + k)
    n = int(off[-1])
    xg, cg = gpu(x), gpu(c)
    lay = ops.SegmentLayout(sizes, DEV)
    assert lay.n == n and lay.n_tiles == sum((m + 63) // 64 for m in sizes)
    buf = _poisoned(k * n)
    rc = ops.lib().rqsid_seg_auction_scores(xg.data_ptr(), n, dim, cg.data_ptr(), k, lay.n_seg, lay.seg_off.data_ptr(),
                                           lay.tile_off.data_ptr(), lay.n_tiles, int(half), buf.data_ptr(),
                                           torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    out = buf.cpu().numpy()
    assert (out[k * n:] == np.int16(POISON16)).all(), "wrote outside the k N values"
    assert not (out[:k * n] == np.int16(POISON16)).any(), "left a score unwritten"
    flat = ops.seg_auction_scores(xg, cg, k, lay, half=half).cpu().numpy()
    assert np.array_equal(flat[:k * n].view(np.int16), out[:k * n])
    ref_fn = M.half_scores_ref if half else M.full_scores_ref
    for s, m in enumerate(sizes):
        if not m:
            continue
        blk = out[k * off[s]:k * off[s + 1]].view(np.float16).reshape(k, m)
        xs, cs = x[off[s]:off[s + 1]], c[s * k:(s + 1) * k]
        ref, lo, hi = ref_fn(xs, cs)
        bad = O.uncertified(-blk.T.astype(np.float64), ref, lo, hi)
        assert not bad.any(), f"segment {s}: {int(bad.sum())} uncertified entries"
        alone = ops.auction_scores(gpu(xs), gpu(cs), half=half).cpu().numpy()
        assert np.array_equal(blk.view(np.int16), alone.view(np.int16)), f"segment {s} differs from its own call"


# ---------------------------------------------------------------------------
# match lists
# ---------------------------------------------------------------------------
def _check_match_lists(m_host, m_dev):
    cand = ops.match_to_candidates(m_dev)
    base, count, flags, idx = M.match_lists_ref(m_host)
    assert np.array_equal(cand.count.cpu().numpy(), count)
    assert np.array_equal(cand.base.cpu().numpy(), base)
    assert np.array_equal(cand.flags.cpu().numpy() != 0, flags)
    assert np.array_equal(cand.idx.cpu().numpy()[:int(count.sum())], idx)
    assert cand.count_max == int(count.max())


@pytest.mark.parametrize("n_cand", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("groups", [1, 3, 5, 1023, 1024, 1025, 2049])
def test_match_lists(groups, n_cand):
    m = M.match_case(groups, n_cand, seed=groups + n_cand)
    _check_match_lists(m, gpu(m))


def test_match_lists_prod_width_and_bool():
    m = M.match_case(64, 1280, seed=5)
    _check_match_lists(m, gpu(m))
    b = M.match_case(37, 70, seed=6) != 0
    _check_match_lists(b, gpu(b))
    ones = np.full((3, 65), 255, np.uint8)
    _check_match_lists(ones, gpu(ones))


# ---------------------------------------------------------------------------
# greedy match
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n_cand,inf_cols", [(3, 0), (255, 0), (255, 17), (257, 0), (257, 40)])
def test_greedy_match_edges(n_cand, inf_cols):
    dist, sub_off = M.greedy_case(n_cand, seed=n_cand + inf_cols, inf_cols=inf_cols)
    dg, og = gpu(dist), gpu(sub_off)
    for max_take in (n_cand + 5, 4, 0):
        got, nsel = ops.greedy_match(dg, og, max_take)
        want = M.greedy_ref(dist, sub_off, max_take)
        assert np.array_equal(got.cpu().numpy(), want), max_take
        assert np.array_equal(nsel.cpu().numpy(), want.sum(1)), max_take


# ---------------------------------------------------------------------------
# wrappers
# ---------------------------------------------------------------------------
def _wrapper_calls(x):
    """The eight wrappers that read x through a raw fp32 pointer, on rows x [8, 32]."""
    c = torch.zeros((4, 32), device=DEV)
    ids = torch.zeros(8, dtype=torch.int32, device=DEV)
    lay = ops.SegmentLayout([8], DEV)
    return {
        "residual": lambda: ops.residual(x, c, ids, [32], True),
        "residual_plain": lambda: ops.residual(x, c, ids, normalize=False),
        "scale_groups": lambda: ops.scale_groups(x, [32], [0.5]),
        "centroid_update": lambda: ops.centroid_update(x, ids, 4, c.clone()),
        "centroid_sums": lambda: ops.centroid_sums(x, ids, 4),
        "pairwise_distance": lambda: ops.pairwise_distance(x, c),
        "pairwise_cosine": lambda: ops.pairwise_cosine(x, c),
        "pairwise_cosine_scores": lambda: ops.pairwise_cosine(x, c, scores=True),
        "auction_scores": lambda: ops.auction_scores(x, c),
        "seg_auction_scores": lambda: ops.seg_auction_scores(x, c, 4, lay),
    }


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float64, torch.int32])
def test_wrappers_refuse_rows_that_are_not_fp32(dtype, monkeypatch):
    """The check comes before any library call: the library handle is replaced by one that fails the test."""
    x = torch.ones((8, 32), device=DEV).to(dtype)
    calls = _wrapper_calls(x)

    def no_library():
        raise AssertionError("the wrapper reached the library")
    monkeypatch.setattr(ops, "lib", no_library)
    for name, call in calls.items():
        with pytest.raises(TypeError):
            call()
    out16 = torch.empty((8, 32), dtype=torch.float16, device=DEV)
    with pytest.raises(TypeError):
        ops.residual(torch.ones((8, 32), device=DEV), torch.zeros((4, 32), device=DEV),
                     torch.zeros(8, dtype=torch.int32, device=DEV), normalize=False, out=out16)


def test_wrappers_accept_fp32_rows():
    for name, call in _wrapper_calls(torch.ones((8, 32), device=DEV)).items():
        call()
    torch.cuda.synchronize()


def test_wrappers_refuse_bad_groups_and_dims(monkeypatch):
    x = torch.ones((8, 32), device=DEV)
    c = torch.zeros((4, 32), device=DEV)
    ids = torch.zeros(8, dtype=torch.int32, device=DEV)
    seventeen = [1] * 16 + [16]
    real_lib = ops.lib

    def no_library():
        raise AssertionError("the wrapper reached the library")
    monkeypatch.setattr(ops, "lib", no_library)
    for gd in ([16, 8], [16, 17], [32, 0], [40, -8], seventeen):
        with pytest.raises(ValueError):
            ops.residual(x, c, ids, gd, True)
        with pytest.raises(ValueError):
            ops.scale_groups(x, gd, [1.0] * len(gd))
    monkeypatch.setattr(ops, "lib", real_lib)
    # the library's own refusals (RQSID_E_ARG before any launch)
    x33, c33 = torch.ones((8, 33), device=DEV), torch.zeros((4, 33), device=DEV)
    lay = ops.SegmentLayout([8], DEV)
    for call in (lambda: ops.pairwise_distance(x33, c33), lambda: ops.pairwise_cosine(x33, c33),
                 lambda: ops.auction_scores(x33, c33), lambda: ops.seg_auction_scores(x33, c33, 4, lay)):
        with pytest.raises(ValueError):
            call()
    x6, c6 = torch.ones((8, 6), device=DEV), torch.zeros((4, 6), device=DEV)
    with pytest.raises(ValueError):
        ops.residual(x6, c6, ids, [6], True)
    with pytest.raises(ValueError):
        ops.residual(x6, c6, ids, normalize=False)
    lib, st = real_lib(), torch.cuda.current_stream().cuda_stream
    g17 = torch.tensor(seventeen, dtype=torch.int32, device=DEV)
    out = torch.empty_like(x)
    assert lib.rqsid_residual(x.data_ptr(), 8, 32, c.data_ptr(), 4, ids.data_ptr(), g17.data_ptr(), 17, 1,
                              out.data_ptr(), st) == -1
