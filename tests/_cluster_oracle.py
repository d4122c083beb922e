"""fp64 numpy restatement of the cluster-quality scores (no GPU, no torch): direct differences sum (x - y)^2, no
expansion.  tests/test_cluster_oracle.py pins it to sklearn's silhouette_samples / calinski_harabasz_score /
davies_bouldin_score, the functions the reference's calculate_metrics.py calls; the GPU tests compare
rqsid_silhouette and cluster_report against it.

Clusters are given as the kernels take them: ``order`` (rows grouped by cluster) and ``off`` ([C + 1] offsets)."""
import numpy as np

U = 2.0 ** -24


def group(labels, n_clusters=None):
    """(order, off) of a label vector: a stable sort, clusters 0 .. n_clusters - 1 (empty ones allowed)."""
    labels = np.asarray(labels, dtype=np.int64)
    k = int(labels.max()) + 1 if n_clusters is None else n_clusters
    order = np.argsort(labels, kind="stable").astype(np.int32)
    off = np.zeros(k + 1, dtype=np.int64)
    np.cumsum(np.bincount(labels, minlength=k), out=off[1:])
    return order, off.astype(np.int32)


def pair_dist(q, x):
    """d[i, j] = sqrt(sum_k (q_ik - x_jk)^2) in fp64."""
    q = np.asarray(q, dtype=np.float64)
    x = np.asarray(x, dtype=np.float64)
    out = np.empty((len(q), len(x)))
    block = max(1, 2 ** 24 // max(1, x.size))  # <= 128 MiB of differences at a time
    for i0 in range(0, len(q), block):
        diff = q[i0:i0 + block, None, :] - x[None, :, :]
        out[i0:i0 + block] = np.sqrt(np.einsum("ijk,ijk->ij", diff, diff))
    return out


def _segment_sums(vals, off):
    """sum of vals[:, off[c]:off[c+1]] per cluster c (0 for an empty one), each added on its own."""
    off = np.asarray(off, dtype=np.int64)
    out = np.zeros((vals.shape[0], len(off) - 1))
    full = np.nonzero(off[1:] > off[:-1])[0]
    if len(full):
        red = np.add.reduceat(vals, off[full], axis=1)
        # reduceat runs each piece to the next listed start: the non-empty clusters tile the positions, so exact
        out[:, full] = red
    return out


def silhouette(x, order, off, q, query_self, query_seg, dim_bound=None, tile_rows=128):
    """S(i, c), a, b, b_seg, s as include/rqsid.h defines them, and (dim_bound = the dim) the derived bound on the
    kernel's error of S(i, c): per pair e = 1.01 u [(2 dim + 6)|q||x| + 3(|q|^2 + |x|^2)] >= |d2^ - d2|, so
    |d^ - d| <= min(sqrt e, e / d) + 2 u d, plus tile_rows u sum d for the fp32 sum inside a tile."""
    x = np.asarray(x, dtype=np.float64)
    q = np.asarray(q, dtype=np.float64)
    order = np.arange(len(x)) if order is None else np.asarray(order, dtype=np.int64)
    off = np.asarray(off, dtype=np.int64)
    m, C = len(q), len(off) - 1
    query_self = np.full(m, -1) if query_self is None else np.asarray(query_self, dtype=np.int64)
    query_seg = np.full(m, -1) if query_seg is None else np.asarray(query_seg, dtype=np.int64)
    xs = x[order]
    d = pair_dist(q, xs)
    pos_of = np.empty(len(x), dtype=np.int64)
    pos_of[order] = np.arange(len(x))
    has_self = query_self >= 0
    keep = np.ones_like(d)
    keep[np.nonzero(has_self)[0], pos_of[query_self[has_self]]] = 0.0
    d = d * keep
    S = _segment_sums(d, off)
    n_c = (off[1:] - off[:-1]).astype(np.float64)
    res = {"S": S, "n_c": n_c}
    if dim_bound is not None:
        qn = np.sqrt((q * q).sum(1))[:, None]
        xn = np.sqrt((xs * xs).sum(1))[None, :]
        e = 1.01 * U * ((2 * dim_bound + 6) * qn * xn + 3 * (qn * qn + xn * xn))
        with np.errstate(divide="ignore", invalid="ignore"):
            per = np.minimum(np.sqrt(e), np.where(d > 0, e / d, np.inf)) + 2 * U * d
        res["S_bound"] = _segment_sums(per * keep, off) + tile_rows * U * S
    a = np.zeros(m)
    b = np.full(m, np.inf)
    b_seg = np.full(m, -1, dtype=np.int64)
    b_err = np.zeros(m)             # with the bound: how far the kernel's b may lie from b
    b_clear = np.ones(m, dtype=bool)  # with the bound: no other cluster's interval reaches the winner's
    s = np.zeros(m)
    for i in range(m):
        o = int(query_seg[i])
        if o >= 0:
            den = n_c[o] - 1 if has_self[i] else n_c[o]
            a[i] = S[i, o] / den if den > 0 else 0.0
        with np.errstate(divide="ignore", invalid="ignore"):
            means = np.where(n_c > 0, S[i] / n_c, np.inf)
        if o >= 0:
            means[o] = np.inf
        c = int(np.argmin(means))  # the first minimum: the lowest c on a tie
        if np.isfinite(means[c]):
            b[i], b_seg[i] = means[c], c
            if dim_bound is not None:
                with np.errstate(divide="ignore", invalid="ignore"):
                    dlt = np.where(n_c > 0, res["S_bound"][i] / n_c, 0.0)
                low = means - dlt  # (inf for the clusters that do not compete)
                b_err[i] = max(dlt[c], means[c] - low.min())
                low[c] = np.inf
                b_clear[i] = low.min() > means[c] + dlt[c]
        if has_self[i] and o >= 0 and n_c[o] <= 1:
            s[i] = 0.0
        elif not np.isfinite(b[i]):
            s[i] = np.nan
        else:
            mx = max(a[i], b[i])
            s[i] = 0.0 if mx == 0 else (b[i] - a[i]) / mx
    res.update(a=a, b=b, b_seg=b_seg, b_err=b_err, b_clear=b_clear, s=s)
    return res


def centroid_scores(x, labels):
    """(K, CH, DB) of sklearn's calinski_harabasz_score / davies_bouldin_score over the non-empty labels; a score
    that is undefined (K < 2, or n <= K for CH) is None."""
    x = np.asarray(x, dtype=np.float64)
    _, inv = np.unique(np.asarray(labels), return_inverse=True)
    K, n = int(inv.max()) + 1, len(x)
    cnt = np.bincount(inv, minlength=K).astype(np.float64)
    mu = np.zeros((K, x.shape[1]))
    np.add.at(mu, inv, x)
    mu /= cnt[:, None]
    dist = np.sqrt(((x - mu[inv]) ** 2).sum(1))
    if K < 2:
        return K, None, None
    W = float((dist ** 2).sum())
    B = float((cnt * ((mu - x.mean(0)) ** 2).sum(1)).sum())
    ch = None if n <= K else (1.0 if W == 0 else (B / (K - 1)) / (W / (n - K)))
    intra = np.bincount(inv, weights=dist, minlength=K) / cnt
    M = pair_dist(mu, mu)
    if np.allclose(intra, 0) or np.allclose(M, 0):
        return K, ch, 0.0
    M[M == 0] = np.inf  # (the diagonal too: a cluster is not its own neighbour)
    R = (intra[:, None] + intra[None, :]) / M
    return K, ch, float(R.max(1).mean())
