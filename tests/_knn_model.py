"""numpy restatement of rqsid_row_knn (csrc/row_knn.hip): the fp32 screen value as the k-ordered
fmaf chain the MFMA computes, the interval e, the fp64 keys, and the keep / fold / certify / exact-pass logic.  Also
the fixtures test_knn_bound.py and test_gpu_knn.py share.  Test support, not product code."""
import numpy as np

F32 = np.float32
U32 = 2.0 ** -24
SLACK = 8
TILE = 128
# the dims of a 32-dim chunk in the order they enter an accumulator: lane half h feeds dims 8 qd + 4 h + j to the
# j-th MFMA of quarter qd, and an MFMA adds its h = 0 product before its h = 1 product
K_ORDER = np.array([8 * qd + 4 * h + j for qd in range(4) for j in range(4) for h in range(2)])


def fmaf(a, b, c):
    """fl32(a b + c) for fp32 arrays with ONE rounding: the product is exact in fp64, the sum is rounded to odd in
    fp64 (TwoSum gives the rounding's sign) and then to nearest in fp32."""
    p = a.astype(np.float64) * b.astype(np.float64)
    c = c.astype(np.float64)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    even = (s.view(np.int64) & 1) == 0
    fix = (err != 0) & even & np.isfinite(s)
    toward = np.where(err > 0, np.inf, -np.inf)
    s = np.where(fix, np.nextafter(s, toward), s)
    return s.astype(F32)


def chain_dot(q, x):
    """D[i, j]: the dot product of q[i] and x[j] as the screen's accumulator holds it (fp32 fmaf chain from 0)."""
    q, x = np.asarray(q, F32), np.asarray(x, F32)
    acc = np.zeros((q.shape[0], x.shape[0]), F32)
    for c0 in range(0, q.shape[1], 32):
        for d in c0 + K_ORDER:
            acc = fmaf(np.broadcast_to(x[None, :, d], acc.shape), np.broadcast_to(q[:, None, d], acc.shape), acc)
    return acc


def sumsq(a):
    return (np.asarray(a, F32).astype(np.float64) ** 2).sum(-1)


def rel(dim):
    return 1.01 * (dim + 8) * U32


def screen(q, x, metric):
    """(s, e): the fp32 screen values [m, n] and the interval the kernel attaches to each (fp64)."""
    q, x = np.asarray(q, F32), np.asarray(x, F32)
    dim = q.shape[1]
    d = chain_dot(q, x)
    with np.errstate(over="ignore", invalid="ignore"):
        if metric == "l2":
            qn, xn = sumsq(q).astype(F32), sumsq(x).astype(F32)
            s = fmaf(np.full(d.shape, -2.0, F32), d, (qn[:, None] + xn[None, :]).astype(F32))
            e = (qn[:, None].astype(np.float64) + xn[None, :].astype(np.float64)) * rel(dim) + dim * 2.0 ** -120
        else:
            qi, xi = (1.0 / np.sqrt(sumsq(q))).astype(F32), (1.0 / np.sqrt(sumsq(x))).astype(F32)
            s = -((d * qi[:, None]).astype(F32) * xi[None, :]).astype(F32)
            e = np.full(d.shape, rel(dim) + 2.0 ** -50)
    return s, e


def exact_keys(q, x, metric):
    """The ascending fp64 key [m, n]: d2 for l2, -sim for cosine (numpy's summation order, not the kernel's)."""
    qd, xd = np.asarray(q, F32).astype(np.float64), np.asarray(x, F32).astype(np.float64)
    if metric == "l2":  # (sixteen queries at a time: the differences of all pairs at once would take gigabytes)
        return np.concatenate([((qd[i:i + 16, None, :] - xd[None, :, :]) ** 2).sum(-1) for i in range(0, len(qd), 16)])
    with np.errstate(invalid="ignore", divide="ignore"):
        return -((qd @ xd.T) / (np.sqrt((qd * qd).sum(1))[:, None] * np.sqrt((xd * xd).sum(1))[None, :]))


def rank(keys, eligible, k):
    """rows [m, k] (-1 past the end) and keys [m, k] (+inf) of the k smallest (key, row) among the eligible."""
    m, n = keys.shape
    out_r = np.full((m, k), -1, np.int32)
    out_k = np.full((m, k), np.inf)
    for i in range(m):
        ok = np.flatnonzero(eligible[i] & np.isfinite(keys[i]))
        o = ok[np.lexsort((ok, keys[i, ok]))][:k]
        out_r[i, :len(o)] = o
        out_k[i, :len(o)] = keys[i, o]
    return out_r, out_k


def values(keys, metric):
    """out_val of ascending keys: fl32(sqrt(d2)) / fl32(sim); +inf stays +inf."""
    with np.errstate(invalid="ignore"):
        v = np.sqrt(keys) if metric == "l2" else np.where(np.isinf(keys), np.inf, -keys)
    return v.astype(F32)


def brute_force(q, x, k, metric, query_self=None, order=None, seg_row_off=None, query_seg=None):
    """The specification: fp64 keys of every eligible row, ranked by (key, row)."""
    keys = exact_keys(q, x, metric)
    eligible = np.ones(keys.shape, bool)
    n = len(x)
    if query_seg is not None:
        order = np.arange(n) if order is None else np.asarray(order)
        for i, s in enumerate(query_seg):
            if s >= 0:
                eligible[i] = False
                eligible[i, order[seg_row_off[s]:seg_row_off[s + 1]]] = True
    if query_self is not None:
        for i, r in enumerate(query_self):
            if r >= 0:
                eligible[i, r] = False
    bad_q = ~np.isfinite(np.asarray(q, F32)).all(1)
    if metric == "cosine":
        bad_q |= sumsq(q) == 0
    rows, kk = rank(keys, eligible, k)
    val = values(kk, metric)
    rows[bad_q] = -1
    val[bad_q] = np.nan
    return rows, val


def keep_fold_certify(s, e, keys, eligible, k, slack, chunk_rows, order=None):
    """The kernel's method on given screen values s [m, n], intervals e [m, n] (by row) and exact keys: per chunk of
    the order keep the k + slack smallest s, U = k-th smallest s + e of the kept, certify, rank the candidates and
    every eligible row of an uncertified chunk.  Returns (rows [m, k], all-rows pairs)."""
    m, n = s.shape
    order = np.arange(n) if order is None else np.asarray(order)
    C = k + slack
    out = np.full((m, k), -1, np.int32)
    pairs = 0
    for i in range(m):
        lists = []
        for c0 in range(0, n, chunk_rows):
            rows = order[c0:c0 + chunk_rows]
            rows = rows[eligible[i, rows]]
            kept = rows[np.argsort(s[i, rows], kind="stable")[:C]]
            lists.append((rows, kept, len(kept) == C))
        merged = np.concatenate([kept for _, kept, _ in lists])
        upper = np.sort(s[i, merged].astype(np.float64) + e[i, merged])
        U = upper[k - 1] if len(upper) >= k else np.inf
        cand = []
        for rows, kept, full in lists:
            worst_e = e[i, rows].max() if len(rows) else 0.0
            if full and not s[i, kept].astype(np.float64).max() - worst_e > U:
                cand.append(rows)
                pairs += 1
            else:
                cand.append(kept[s[i, kept].astype(np.float64) - e[i, kept] <= U])
        cand = np.concatenate(cand).astype(np.int64)
        o = cand[np.lexsort((cand, keys[i, cand]))][:k]
        out[i, :len(o)] = o
    return out, pairs


def blobs(n, dim, centres, spread, seed):
    """n fp32 rows around `centres` Gaussian centres, and their blob labels."""
    rng = np.random.default_rng(seed)
    mu = rng.normal(size=(centres, dim))
    lab = rng.integers(0, centres, n)
    return (mu[lab] + spread * rng.normal(size=(n, dim))).astype(F32), lab


def fixture_t(seed=5):
    """1500 x 64 rows of integers in [-2, 2], rows 100..139 copies of row 7: every key is exact in fp32 and fp64, and
    ties abound."""
    x = np.random.default_rng(seed).integers(-2, 3, (1500, 64)).astype(F32)
    x[100:140] = x[7]
    return x


def auto_chunk_rows(n, m, target_blocks=2048):
    """What chunk_rows = 0 stands for: the fewest chunks of whole tiles that give target_blocks blocks."""
    tiles, qtiles = -(-n // TILE), -(-m // TILE)
    want = max(1, min(-(-target_blocks // qtiles), tiles))
    return -(-tiles // want) * TILE


def block_tile_ranges(n, seg_row_off, query_seg, chunk_rows):
    """(tile0, tile1, ntile) of every (query tile, chunk) block of the screen: a block runs the tiles of its chunk
    that the union of its queries' position ranges touches (finite queries; -1 searches every position)."""
    query_seg = np.asarray(query_seg)
    chunk_rows = chunk_rows or auto_chunk_rows(n, len(query_seg))
    lo = np.where(query_seg >= 0, seg_row_off[np.maximum(query_seg, 0)], 0).astype(np.int64)
    hi = np.where(query_seg >= 0, seg_row_off[np.maximum(query_seg, 0) + 1], n).astype(np.int64)
    out = []
    for q0 in range(0, len(query_seg), TILE):
        some = lo[q0:q0 + TILE] < hi[q0:q0 + TILE]
        ulo = lo[q0:q0 + TILE][some].min() if some.any() else 2 ** 31 - 1
        uhi = hi[q0:q0 + TILE][some].max() if some.any() else 0
        for c0 in range(0, n, chunk_rows):
            ntile = -(-(min(c0 + chunk_rows, n) - c0) // TILE)
            tile0 = min((ulo - c0) // TILE, ntile) if ulo > c0 else 0
            tile1 = min(-(-(uhi - c0) // TILE), ntile) if uhi > c0 else 0
            out.append((int(tile0), int(tile1), ntile))
    return np.array(out)
