"""The bars of tests/test_gpu_lloyd_kernels.py are fair and sharp before a GPU is involved (tests/_lloyd_model.py).

Fair: the oracle's own numpy restatements (O.cdist_f32, O.pairwise_cosine, O.cdist_half, O.residual) lie inside
the derived intervals at every shape the GPU tests use, and an fp64 centroid in the kernel's 4-partial, any-tile-
order scheme meets the centroid bound bit for bit.  Sharp: a centroid that sums a 256-row tile in fp32 misses that
bound on the mixed-magnitude rows, by tens to thousands of ulps."""
import numpy as np
import pytest

from oracle import rq_oracle as O
from tests import _lloyd_model as M

F32 = np.float32
SHAPES = M.distance_shapes()


def _ids(shapes):
    return ["x".join(map(str, s)) for s in shapes]


@pytest.mark.parametrize("n,k,dim", SHAPES, ids=_ids(SHAPES))
def test_oracle_distances_lie_inside_their_intervals(n, k, dim):
    x, c = M.distance_case(n, k, dim, seed=n + k + dim)
    d = O.cdist_f32(x, c).astype(np.float64)
    lo, hi = M.dist_interval32(x, c)
    assert ((d >= lo) & (d <= hi)).all(), f"cdist_f32 outside dist_interval32 at {int(((d < lo) | (d > hi)).sum())} entries"
    assert (lo[::7] == 0).any() or n * k == 0  # the rows equal to a centre reach the clamp's side of the interval
    q = O.pairwise_cosine(x, c).astype(np.float64)
    lo, hi = M.cosine_interval(x, c)
    assert ((q >= lo) & (q <= hi)).all(), f"pairwise_cosine outside cosine_interval at {int(((q < lo) | (q > hi)).sum())}"
    # the interval is no wider than the derivation says: (2 G + 5 u) at most, G = 2 (dim - 1) u
    assert (hi - lo).max() <= 2 * (4 * (dim - 1) + 5) * M.U32 * M.SLACK * 1.000001
    h = O.cdist_half(x, c).astype(np.float64)
    lo, hi = O.half_dist_interval(x, c)
    assert ((h >= lo) & (h <= hi)).all()
    ref, lo, hi = M.full_scores_ref(x, c)
    assert ((ref >= lo) & (ref <= hi)).all()
    # zero uncertified entries is a condition the references keep against themselves
    assert not O.uncertified(ref, ref, lo, hi).any()


@pytest.mark.parametrize("sizes", M.SEGMENT_SIZES, ids=lambda s: "-".join(map(str, s)))
@pytest.mark.parametrize("k", [3, 65])
def test_oracle_segment_blocks_lie_inside_their_intervals(sizes, k):
    x, c, off = M.segment_case(sizes, k, 96, seed=len(sizes) + k)
    for s, m in enumerate(sizes):
        if not m:
            continue
        xs, cs = x[off[s]:off[s + 1]], c[s * k:(s + 1) * k]
        ref, lo, hi = M.full_scores_ref(xs, cs)
        assert ((ref >= lo) & (ref <= hi)).all()
        ref, lo, hi = M.half_scores_ref(xs, cs)
        assert ((ref >= lo) & (ref <= hi)).all()


@pytest.mark.parametrize("dim", [1, 255, 256, 257, 512, 1024])
def test_fp64_partials_meet_the_centroid_bound_and_fp32_tiles_miss_it(dim):
    sizes = M.CLUSTER_SIZES["edges"]
    k = len(sizes)
    x = M.mixed_magnitude_rows(int(np.sum(sizes)), dim, seed=dim)
    a = M.shuffled_assignment(sizes, seed=dim + 1)
    sums, counts, mean, tol, _ = M.centroid_ref(x, a, k)
    assert np.array_equal(counts, sizes)
    full = counts > 0
    good = M.centroid_fp64_partials(x, a, k, seed=dim + 2)
    assert (np.abs(good.astype(np.float64) - mean)[full] <= tol[full]).all()
    assert np.array_equal(good[full], mean.astype(F32)[full])  # zero bit differences from fl32(fp64 mean)
    assert np.array_equal(good[full], O.centroid_update(x, a, good, lambda n: 0)[full])
    bad = M.centroid_fp32_tiles(x, a, k)
    big = counts >= 255  # clusters long enough for the fp32 accumulator to lose bits
    miss = np.abs(bad.astype(np.float64) - mean)[big] > tol[big]
    assert miss.mean() > 0.5, f"only {miss.mean():.3f} of the fp32-accumulated means miss the bound"
    worst = (np.abs(bad.astype(np.float64) - mean)[big] / M.ulp32(mean[big])).max()
    assert worst > 8  # far outside, not marginally: the old test's rtol of 1e-6 (~8 ulps) sat inside this
    # and the bound is tight: half an ulp and a sliver (more only where a mean cancels to far below its rows)
    assert np.median(tol[full] / M.ulp32(mean[full])) < 0.5001


def test_centroid_ref_drops_keys_outside_the_clusters():
    x = M.mixed_magnitude_rows(40, 8, seed=3)
    a = np.arange(40) % 5
    base = M.centroid_ref(x[a < 4], a[a < 4], 4)
    a2 = a.copy()
    a2[a == 4] = np.array([-1, 4, 7, 2 ** 31 - 1, -2 ** 31, 100, -7, 4])
    got = M.centroid_ref(x, a2, 4)
    assert np.array_equal(got[1], base[1]) and np.array_equal(got[0], base[0])


@pytest.mark.parametrize("n,dim", M.RESIDUAL_SHAPES, ids=_ids(M.RESIDUAL_SHAPES))
def test_oracle_residual_norm_is_order_stable_on_the_chosen_seeds(n, dim):
    """O.residual takes each norm in numpy's pairwise fp64 order; the exactly summed restatement rounds to the same
    fp32 on these seeds, so the 1-ulp / 1e-3 cap of the GPU test is a condition a correct kernel can keep."""
    for kind, gd in M.group_kinds(dim).items():
        x, c, ids = M.residual_case(n, dim, 7, seed=M.residual_seed(n, dim), zero_groups=[(0, gd[0])])
        ref = O.residual(x, c, ids, gd, True)
        mx, frac, ok = M.residual_close(M.residual_ref64(x, c, ids, gd), ref)
        assert ok, f"{kind}: max {mx} ulp, {frac:.2e} differing"
        assert (ref[0] == 0).all()                      # every group zero: exactly 0.0, not NaN
        if n > 1:
            assert (ref[1, :gd[0]] == 0).all() and (len(gd) == 1 or (ref[1, gd[0]:] != 0).any())


def test_ulp_helpers():
    one = F32(1.0)
    assert M.ulp32(1.0) == 2.0 ** -23 and M.ulp32(0.999) == 2.0 ** -24 and M.ulp32(0.0) == 2.0 ** -149
    assert M.ulp_diff(np.array([one]), np.array([np.nextafter(one, F32(2))]))[0] == 1
    assert M.ulp_diff(np.array([F32(0.0)]), np.array([F32(-0.0)]))[0] == 0
    assert M.uneven_groups(36, 16) == [1, 2, 3] * 5 + [6]
    with pytest.raises(ValueError):
        M.uneven_groups(20, 16)


def test_match_and_greedy_references():
    m = M.match_case(11, 9, seed=1)
    base, count, flags, idx = M.match_lists_ref(m)
    assert (m[::5] == 0).all() and (m[2] == 1).all() and (m == 255).any() and (m == 2).any()
    assert count[0] == 0 and flags[0] and count[2] == 9 and base[-1] + count[-1] == len(idx)
    for C, inf_cols in ((3, 0), (255, 17), (257, 0)):
        dist, sub_off = M.greedy_case(C, seed=C, inf_cols=inf_cols)
        want = M.greedy_ref(dist, sub_off, max_take=C + 5)
        sizes = np.diff(sub_off)
        assert np.array_equal(want.sum(1), np.minimum(sizes, C))
        assert not want[:, np.isinf(dist[0])].any()  # a +inf column is never taken while finite ones are left
        assert M.greedy_ref(dist, sub_off, 0).sum() == 0
        # equal minima: the lowest column wins
        assert want[4].argmax() == int(np.argmin(dist[sub_off[4]]))
