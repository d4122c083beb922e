"""Numpy references and derived error bounds for the kernels of one Lloyd iteration (csrc/rqsid.hip: residual,
scale_groups, centroid_accumulate / centroid_finalize, pairwise_distance_kernel<MODE, SEG>, match_to_candidates,
greedy_match), shared by tests/test_lloyd_model.py (CPU: the oracle's own restatements meet every bar, a subtly
wrong centroid misses it) and tests/test_gpu_lloyd_kernels.py (the HIP kernels against the same bars).

Every tolerance here is derived, none is measured.  u = 2^-24 is the fp32 unit roundoff (half an ulp of 1),
``O._fp32_sum_bound(n)`` = (n - 1) u the first-order bound of an fp32 sum of n terms in any order, relative to
the sum of the terms' magnitudes."""
import numpy as np

from oracle import rq_oracle as O

F32 = np.float32
U32 = 2.0 ** -24
SLACK = 1.0001  # second-order terms of the first-order bounds below


# ---------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------
def ulp32(v):
    """The spacing of fp32 numbers in the binade of |v| (float64 in, float64 out; 2^-149 at and below the
    subnormals).  A value just under a power of two gets the smaller binade's spacing: the tighter choice."""
    v = np.abs(np.asarray(v, np.float64))
    _, e = np.frexp(v)  # |v| = m 2^e, m in [0.5, 1)
    return np.where(v == 0, 2.0 ** -149, np.ldexp(1.0, np.maximum(e - 24, -149)))


def ulp_diff(a, b):
    """Distance in representable fp32 values between two fp32 arrays (sign-magnitude order, -0 == +0)."""
    def key(v):
        i = np.ascontiguousarray(v, F32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(a) - key(b))


def uneven_groups(dim, n_groups):
    """n_groups widths summing to dim: 1, 2, 3, 1, 2, 3, ... and the rest in the last group (edges that are no
    multiples of 4, one-element groups included)."""
    head = [(i % 3) + 1 for i in range(n_groups - 1)]
    last = dim - sum(head)
    if last < 1:
        raise ValueError(f"{n_groups} uneven groups do not fit {dim} dimensions")
    return head + [last]


# ---------------------------------------------------------------------------
# case builders (seeded)
# ---------------------------------------------------------------------------
def mixed_magnitude_rows(n, dim, seed):
    """Rows N(0, 1) x (1e3 or 1, drawn per row) + 0.37: a column of a cluster then sums values of magnitude 1e3
    and of magnitude 1, which an fp32 accumulator cannot hold together (the small rows' low bits are lost at
    every step) while the mean stays O(10)."""
    rng = np.random.default_rng(seed)
    scale = np.where(rng.random(n) < 0.5, 1e3, 1.0)[:, None]
    return (rng.standard_normal((n, dim)) * scale + 0.37).astype(F32)


CLUSTER_SIZES = {
    # leading, trailing and runs of empty clusters; the 4-row unroll's tails (1..5 rows); the 256-row tile's
    # edges (255, 256, 257) and a third tile of one row (513)
    "edges": [0, 0, 1, 2, 3, 4, 5, 0, 255, 256, 257, 513, 0, 0],
    "k1": [300],
    "all_in_last": [0, 0, 0, 0, 0, 0, 261],
}


def shuffled_assignment(sizes, seed):
    """A cluster id per row with exactly sizes[j] rows in cluster j, in shuffled row order (so the bucketing's
    row_index is a true permutation, not the identity)."""
    a = np.repeat(np.arange(len(sizes)), sizes)
    np.random.default_rng(seed).shuffle(a)
    return a.astype(np.int64)


def distance_case(n, k, dim, seed):
    """Rows and centres N(0, 1); every 7th row (and always row 0) is bitwise equal to a centre, every 7th + 1
    sits 1e-3 away from one (d^2 is then all cancellation)."""
    rng = np.random.default_rng(seed)
    c = rng.standard_normal((k, dim)).astype(F32)
    x = rng.standard_normal((n, dim)).astype(F32)
    for r in range(0, n, 7):
        x[r] = c[(3 * r) % k]
        if r + 1 < n:
            x[r + 1] = c[(5 * r + 1) % k] + F32(1e-3) * rng.standard_normal(dim).astype(F32)
    return x, c


CENTRE_SHAPE = (65, 65, 96)


def distance_shapes():
    """(n, k, dim): each axis varied around CENTRE_SHAPE, and the two corners."""
    n0, k0, d0 = CENTRE_SHAPE
    shapes = [(n, k0, d0) for n in (1, 63, 64, 65, 130)]
    shapes += [(n0, k, d0) for k in (1, 63, 64, 129)]
    shapes += [(n0, k0, d) for d in (32, 512, 1024)]
    shapes += [(1, 1, 32), (130, 129, 1024)]
    return shapes


SEGMENT_SIZES = [[0, 0, 1, 63, 64, 65, 0, 129, 0, 0], [5], [0, 7], [7, 0]]


def segment_case(sizes, k, dim, seed):
    """Rows grouped by segment and k centres per segment (segment s owns centres s*k .. s*k+k-1); the first row of
    every non-empty segment equals one of that segment's centres."""
    rng = np.random.default_rng(seed)
    n = int(np.sum(sizes))
    x = rng.standard_normal((n, dim)).astype(F32)
    c = rng.standard_normal((len(sizes) * k, dim)).astype(F32)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    for s, m in enumerate(sizes):
        if m:
            x[off[s]] = c[s * k + (s % k)]
    return x, c, off


def residual_case(n, dim, n_centers, seed, zero_groups=()):
    """Rows, centres and ids for the residual kernel.  Row 0 equals its centre in every dimension (all groups
    zero); row 1 (if any) equals its centre inside the dimension ranges ``zero_groups`` [(lo, hi), ...] only."""
    rng = np.random.default_rng(seed)
    c = rng.standard_normal((n_centers, dim)).astype(F32)
    ids = rng.integers(0, n_centers, n).astype(np.int64)
    x = (c[ids] + 0.5 * rng.standard_normal((n, dim))).astype(F32)
    x[0] = c[ids[0]]
    if n > 1:
        for lo, hi in zero_groups:
            x[1, lo:hi] = c[ids[1], lo:hi]
    return x, c, ids


GRID_STRIDE_ROWS = 32768 + 5  # residual_kernel runs at most 8192 blocks of 4 rows: its grid-stride loop starts here
RESIDUAL_SHAPES = [(n, 32) for n in (1, 3, 4, 5, GRID_STRIDE_ROWS)] + \
                  [(257, d) for d in (4, 36, 256, 260, 512, 1024)]
# seeds for which no fp64 summation order moves an fp32 norm (tests/test_lloyd_model.py checks it); a shape
# whose default seed did not qualify gets another one here
RESIDUAL_SEEDS = {}


def residual_seed(n, dim):
    return RESIDUAL_SEEDS.get((n, dim), 100 * n + dim)


def group_kinds(dim):
    """The group layouts of a residual test at this dim: one group; edges 5 | 12 (no multiples of 4); a one-element
    first group; 16 uneven groups (kMaxGroups) -- each where dim has room for it."""
    kinds = {"one": [dim]}
    if dim > 12:
        kinds["5_7_rest"] = [5, 7, dim - 12]
    if dim > 1:
        kinds["1_rest"] = [1, dim - 1]
    if dim >= 34:
        kinds["16_uneven"] = uneven_groups(dim, 16)
    return kinds


# ---------------------------------------------------------------------------
# residual
# ---------------------------------------------------------------------------
def residual_ref64(x, c, ids, group_dims=()):
    """The normalised residual with each group's sum of squares taken exactly (long double, not numpy's pairwise
    fp64 order) and rounded once: r = fl32(x - c[id]); n_g = fl32(sqrt(sum r_g^2)); out = fl32(r / fl32(n_g + 1e-8)).
    Where O.residual agrees with this bit for bit, no fp64 summation order moves the fp32 norm, so a correct
    kernel must agree too (its fp32 steps are the same single roundings)."""
    r = (x.astype(F32) - c.astype(F32)[ids]).astype(F32)
    gd = list(group_dims) or [x.shape[1]]
    s = 0
    for g in gd:
        blk = r[:, s:s + g]
        t = (blk.astype(np.longdouble) ** 2).sum(1, keepdims=True)
        nrm = np.sqrt(t).astype(np.float64).astype(F32)
        r[:, s:s + g] = blk / (nrm + F32(1e-8))
        s += g
    return r


def residual_close(got, ref):
    """The bar of test_residual: at most 1 ulp anywhere and fewer than 1e-3 of the elements differing.
    Returns (max ulp, differing fraction, ok)."""
    d = ulp_diff(got, ref)
    return int(d.max()), float((d > 0).mean()), bool(d.max() <= 1 and (d > 0).mean() < 1e-3)


# ---------------------------------------------------------------------------
# centroid update
# ---------------------------------------------------------------------------
def centroid_ref(x, assign, k):
    """Exact per-cluster sums, counts and the allowed error of the fp32 mean.

    Returns (sums long double [k, D], counts int64 [k], mean float64 [k, D], tol float64 [k, D], sum_tol [k, D]).
    The sums are taken in long double (64-bit significand: 2^-11 of an fp64 ulp per step, nothing beside the
    bounds below).  Rows whose key lies outside [0, k) belong to no cluster.

    tol = 0.5 ulp32(mean) + count 2^-52 mean|x|:
      * an fp64 sum of `count` terms in ANY order (4 partials per thread, tiles added by atomics in any order)
        errs by at most (count - 1) 2^-53 sum|x| to first order; divided by count that is below
        count 2^-53 mean|x|.  The division sums / count adds 2^-53 |mean| <= 2^-53 mean|x|.  Together they stay
        below count 2^-52 mean|x| (the factor 2 pays for the second-order terms).
      * rounding that fp64 mean to fp32 adds half an fp32 ulp of the mean.
    sum_tol = count 2^-52 sum|x| bounds the fp64 sums themselves (rqsid_centroid_accumulate / ops.centroid_sums)
    the same way."""
    x = np.asarray(x, F32)
    assign = np.asarray(assign)
    d = x.shape[1]
    sums = np.zeros((k, d), np.longdouble)
    sabs = np.zeros((k, d), np.float64)
    counts = np.zeros(k, np.int64)
    order = np.argsort(assign, kind="stable")
    keys = assign[order]
    lo = np.searchsorted(keys, np.arange(k), "left")
    hi = np.searchsorted(keys, np.arange(k), "right")
    for j in range(k):
        rows = x[order[lo[j]:hi[j]]]
        counts[j] = len(rows)
        if len(rows):
            sums[j] = rows.astype(np.longdouble).sum(0)
            sabs[j] = np.abs(rows).astype(np.float64).sum(0)
    cnt = np.maximum(counts, 1)[:, None]
    mean = (sums / cnt).astype(np.float64)
    sum_tol = counts[:, None] * 2.0 ** -52 * sabs
    tol = 0.5 * ulp32(mean) + sum_tol / cnt
    return sums, counts, mean, tol, sum_tol


def centroid_fp32_tiles(x, assign, k, tile=256):
    """A subtly wrong centroid: every 256-row tile summed sequentially in fp32, the tiles then combined and
    divided in fp64 (what the kernel would compute with float accumulators)."""
    x = np.asarray(x, F32)
    out = np.zeros((k, x.shape[1]), F32)
    for j in range(k):
        rows = x[np.asarray(assign) == j]
        if len(rows) == 0:
            continue
        tot = np.zeros(x.shape[1], np.float64)
        for t in range(0, len(rows), tile):
            tot += np.cumsum(rows[t:t + tile], axis=0, dtype=F32)[-1].astype(np.float64)
        out[j] = (tot / len(rows)).astype(F32)
    return out


def centroid_fp64_partials(x, assign, k, seed, tile=256):
    """The kernel's own scheme: per tile four fp64 partials over rows i, i+1, i+2, i+3 (mod 4) combined as
    (a0 + a1) + (a2 + a3), the tiles added in a permuted order, one fp64 division, one rounding to fp32.  The rows
    of a cluster are taken in a permuted order too (the bucketing's scatter order is not fixed)."""
    rng = np.random.default_rng(seed)
    x = np.asarray(x, F32)
    out = np.zeros((k, x.shape[1]), F32)
    for j in range(k):
        rows = x[rng.permutation(np.nonzero(np.asarray(assign) == j)[0])].astype(np.float64)
        if len(rows) == 0:
            continue
        parts = []
        for t in range(0, len(rows), tile):
            blk = rows[t:t + tile]
            full = len(blk) // 4 * 4
            a = [np.cumsum(blk[q:full:4], axis=0)[-1] if full else np.zeros(x.shape[1]) for q in range(4)]
            for r in blk[full:]:
                a[0] = a[0] + r
            parts.append((a[0] + a[1]) + (a[2] + a[3]))
        tot = np.zeros(x.shape[1], np.float64)
        for p in rng.permutation(len(parts)):
            tot = tot + parts[p]
        out[j] = (tot / len(rows)).astype(F32)
    return out


# ---------------------------------------------------------------------------
# distances
# ---------------------------------------------------------------------------
def _d2_error(x, c):
    """2 _fp32_sum_bound(dim + 2) (2|x|.|c| + |x|^2 + |c|^2): any fp32 evaluation of the expansion |x|^2 + |c|^2
    - 2 x.c (three sums of dim terms and two additions, fused or not, in any order) stays within it; the factor 2
    is the one ``O.full_dist_interval`` uses (product roundings of an unfused sum, second-order terms)."""
    xd = np.asarray(x, F32).astype(np.float64)
    cd = np.asarray(c, F32).astype(np.float64)
    xn, cn = (xd * xd).sum(1), (cd * cd).sum(1)
    mag = 2.0 * (np.abs(xd) @ np.abs(cd).T) + xn[:, None] + cn[None, :]
    return 2.0 * O._fp32_sum_bound(xd.shape[1] + 2) * mag


def dist_interval32(x, c):
    """[lo, hi] (fp32 values as float64) of every fp32 distance sqrt(max(|x|^2 + |c|^2 - 2 x.c, 0)) that
    torch.cdist's expansion can give under any fp32 summation order: the pre-fp16 form of
    ``O.full_dist_interval``.  The exact d^2 (fp64) moves by at most ``_d2_error``; the square root is monotone
    and correctly rounded, so the fp32 result lies between the fp32 roundings of the two ends' roots; one more
    fp32 ulp each way pays for a square root that is only faithfully rounded and for the fp64 arithmetic here."""
    exact = O.exact_d2(np.asarray(x, F32), np.asarray(c, F32))
    e = _d2_error(x, c)
    lo = np.sqrt(np.maximum(exact - e, 0.0)).astype(F32)
    hi = np.sqrt(np.maximum(exact + e, 0.0)).astype(F32)
    lo = np.maximum(np.nextafter(lo, F32(-np.inf)), F32(0.0))
    hi = np.nextafter(hi, F32(np.inf))
    return lo.astype(np.float64), hi.astype(np.float64)


def cosine_interval(x, c):
    """[lo, hi] (float64) of every fp32 evaluation of the cosine distance 1 - x.c / (|x| |c|).

    Centre: the exact q = x.c / (|x| |c|) in fp64, distance 1 - q.  Let r = sum|x_i c_i| / (|x| |c|)
    (|q| <= r <= 1 by Cauchy-Schwarz) and G = 2 _fp32_sum_bound(dim) (an fp32 sum of dim terms in any order,
    products rounded or fused; the factor 2 as in ``_d2_error``).

    The kernel's order (rqsid_pairwise_cosine: three fp32 sums, two square roots, their product, one quotient, one
    subtraction):
      * the dot product errs by at most G sum|x_i c_i|: G r in q;
      * each squared norm carries a relative error <= G, its square root half of that plus one rounding u; the
        product of the roots one more u, the quotient one more u: the denominator and the division together
        move q by at most |q| (G + 4u);
      * the subtraction 1 - q rounds once: u |1 - q|.
    The reference's order (pairwise_cosine, balancekmeans/__init__.py:625-655: each operand divided by its fp32
    norm, then an fp32 matrix product) puts the same roundings elsewhere: every element x_i / |x| carries 2u (the
    norm's rounding and the division's), likewise c_i / |c|, so each product term errs by 4u and the sum by
    G: (G + 4u) r in all.  Since |q| <= r, one width covers both orders:

        W = ((G + 4u) r + G |q| + u |1 - q|) (1 + 1e-4)."""
    xd = np.asarray(x, F32).astype(np.float64)
    cd = np.asarray(c, F32).astype(np.float64)
    nx = np.sqrt((xd * xd).sum(1))[:, None]
    nc = np.sqrt((cd * cd).sum(1))[None, :]
    q = (xd @ cd.T) / (nx * nc)
    r = (np.abs(xd) @ np.abs(cd).T) / (nx * nc)
    g = 2.0 * O._fp32_sum_bound(xd.shape[1])
    w = ((g + 4.0 * U32) * r + g * np.abs(q) + U32 * np.abs(1.0 - q)) * SLACK
    return (1.0 - q) - w, (1.0 - q) + w


def cosine_score_interval(x, c):
    """[lo, hi] of the worker-major fp16 scores -distance (rounding to fp16 is monotone)."""
    lo, hi = cosine_interval(x, c)
    f16 = np.float16
    return (-hi).astype(f16).astype(np.float64).T, (-lo).astype(f16).astype(np.float64).T


def full_scores_ref(x, c):
    """(ref, lo, hi), all [n, k] float64: fp16(O.cdist_f32) and ``O.full_dist_interval`` (mode 1's distances)."""
    lo, hi = O.full_dist_interval(x, c)
    return O.cdist_f32(x, c).astype(np.float16).astype(np.float64), lo, hi


def half_scores_ref(x, c):
    """(ref, lo, hi), all [n, k] float64: O.cdist_half and ``O.half_dist_interval`` (mode 2's distances)."""
    lo, hi = O.half_dist_interval(x, c)
    return O.cdist_half(x, c).astype(np.float64), lo, hi


# ---------------------------------------------------------------------------
# match lists / greedy match
# ---------------------------------------------------------------------------
def match_case(groups, n_cand, seed):
    """A uint8 match matrix with empty rows, all-ones rows and bytes of 2 and 255 among the ones."""
    rng = np.random.default_rng(seed)
    m = (rng.random((groups, n_cand)) < 0.3).astype(np.uint8)
    m[rng.random((groups, n_cand)) < 0.05] = 2
    m[rng.random((groups, n_cand)) < 0.05] = 255
    m[::5] = 0
    m[2::7] = 1
    if groups > 1:
        m[-1] = 0
    return m


def match_lists_ref(m):
    """(base, count, flags, idx) of rqsid_match_to_candidates: row popcounts of the non-zero bytes, their
    exclusive scan, the penalty flag of empty rows, the non-zero columns in row-major order."""
    on = np.asarray(m) != 0
    count = on.sum(1).astype(np.int64)
    base = np.concatenate([[0], np.cumsum(count)[:-1]])
    return base, count, (count == 0), np.nonzero(on)[1]


def greedy_ref(dist, sub_off, max_take):
    """_assign_last_match_matrix :1022-1038 as tests/test_gpu_training.py restates it: sub-centre by sub-centre
    the first index of the smallest distance among the unused columns (used ones set to +inf).  Once every column
    is used the argmin falls on a used one and nothing more is taken.  (A sub-centre whose unused columns are all
    +inf is not defined by this loop; ``greedy_case`` never builds one.)"""
    groups, n_cand = len(sub_off) - 1, dist.shape[1]
    want = np.zeros((groups, n_cand), np.uint8)
    for g in range(groups):
        used = np.zeros(n_cand, bool)
        for r in range(sub_off[g], sub_off[g] + min(sub_off[g + 1] - sub_off[g], max_take)):
            d = np.where(used, np.inf, dist[r])
            col = int(np.argmin(d))
            used[col] = True
            want[g, col] = 1
    return want


def greedy_case(n_cand, seed, levels=5, inf_cols=0):
    """(dist f32 [total_sub, n_cand], sub_off): distances quantised to ``levels`` values, so the minimum of a row
    is shared by many columns, in different lanes and (n_cand > 64) different waves; ``inf_cols`` whole columns
    are +inf.  Group sizes: 5, 0, n_cand + 2 (more sub-centres than columns; without +inf columns only), 3, 1."""
    rng = np.random.default_rng(seed)
    sizes = [5, 0, 0 if inf_cols else n_cand + 2, 3, 1]
    sub_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    dist = (rng.integers(1, levels + 1, (int(sub_off[-1]), n_cand)) * 0.25).astype(F32)
    dist[2] = dist[1]  # duplicate rows: the second takes the next free column
    if inf_cols:
        assert n_cand - inf_cols >= max(sizes)  # a finite unused column is left at every step
        dist[:, rng.choice(n_cand, inf_cols, replace=False)] = np.inf
    return dist, sub_off
