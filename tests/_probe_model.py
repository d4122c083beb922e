"""numpy restatement of rqsid_probe_knn (csrc/probe_knn.hip) on top of tests/_knn_model.py: the
specification (eligible = the union of a query's cleaned ranges minus its self row, ranked by the fp64 key and the row
number) and the method as code (one list of k + slack screen values per (query, probe) item, U over every kept entry
of a query, the certificate per item, the candidates).  Test support, not product code."""
import numpy as np

from tests import _knn_model as M

ERR_RANGE, ERR_OVERLAP = 4, 8


def clean_ranges(lo, hi, n):
    """The ranges as the kernel takes them: ends clamped into [0, n], lo > hi empty, and a range that overlaps an
    earlier kept range of its query dropped whole.  Returns (lo, hi, error word)."""
    lo, hi = np.array(lo, np.int64), np.array(hi, np.int64)
    word = 0
    if ((lo < 0) | (lo > n) | (hi < 0) | (hi > n) | (lo > hi)).any():
        word |= ERR_RANGE
    lo, hi = np.clip(lo, 0, n), np.clip(hi, 0, n)
    hi = np.maximum(hi, lo)
    for i in range(lo.shape[0]):
        for c in range(lo.shape[1]):
            for b in range(c):
                if lo[i, c] < hi[i, c] and lo[i, b] < hi[i, b] and lo[i, c] < hi[i, b] and lo[i, b] < hi[i, c]:
                    word |= ERR_OVERLAP
                    hi[i, c] = lo[i, c]
    return lo, hi, word


def item_rows(lo, hi, order, query_self, i, c):
    """The eligible rows of item (i, c) of cleaned ranges, in position order."""
    rows = order[lo[i, c]:hi[i, c]]
    if query_self is not None and query_self[i] >= 0:
        rows = rows[rows != query_self[i]]
    return rows


def eligible(lo, hi, n, order=None, query_self=None):
    """[M, n] bool and scanned [M] of raw ranges."""
    order = np.arange(n) if order is None else np.asarray(order)
    lo, hi, _ = clean_ranges(lo, hi, n)
    ok = np.zeros((lo.shape[0], n), bool)
    for i in range(lo.shape[0]):
        for c in range(lo.shape[1]):
            ok[i, item_rows(lo, hi, order, query_self, i, c)] = True
    return ok, (hi - lo).sum(1).astype(np.int32)


def brute_force(q, x, k, metric, lo, hi, order=None, query_self=None, keys=None):
    """The specification: (rows [M, k], val [M, k], scanned [M])."""
    keys = M.exact_keys(q, x, metric) if keys is None else keys
    ok, scanned = eligible(lo, hi, len(x), order, query_self)
    bad_q = ~np.isfinite(np.asarray(q, M.F32)).all(1)
    if metric == "cosine":
        bad_q |= M.sumsq(q) == 0
    rows, kk = M.rank(keys, ok, k)
    val = M.values(kk, metric)
    rows[bad_q] = -1
    val[bad_q] = np.nan
    return rows, val, scanned


def lists_fold_certify(s, e, keys, lo, hi, k, slack, order=None, query_self=None, also_listed=None):
    """The kernel's method on given screen values s [M, n], intervals e [M, n] (by row) and exact keys: per item keep
    the k + slack smallest s of its range, U = the k-th smallest s + e over EVERY kept entry of the query, certify
    each item, rank the candidates and every eligible row of an uncertified item.  ``also_listed``: {query: (probe,
    row)} enters that row into that item's list as well, which the disjoint ranges of the kernel rule out.  Returns
    (rows [M, k], items that took the all-rows pass)."""
    m, n = s.shape
    order = np.arange(n) if order is None else np.asarray(order)
    lo, hi, _ = clean_ranges(lo, hi, n)
    C = k + slack
    out = np.full((m, k), -1, np.int32)
    all_rows = 0
    for i in range(m):
        lists = []
        for c in range(lo.shape[1]):
            rows = item_rows(lo, hi, order, query_self, i, c)
            kept = rows[np.argsort(s[i, rows], kind="stable")[:C]]
            full = len(kept) == C
            if also_listed is not None and i in also_listed and also_listed[i][0] == c:
                kept = np.append(kept, also_listed[i][1])
            lists.append((rows, kept, full))
        merged = np.concatenate([kept for _, kept, _ in lists]).astype(np.int64)
        upper = np.sort(s[i, merged].astype(np.float64) + e[i, merged])
        U = upper[k - 1] if len(upper) >= k else np.inf
        cand = []
        for rows, kept, full in lists:
            worst_e = e[i, rows].max() if len(rows) else 0.0
            if full and not s[i, kept].astype(np.float64).max() - worst_e > U:
                cand.append(rows)
                all_rows += 1
            else:
                cand.append(kept[s[i, kept].astype(np.float64) - e[i, kept] <= U])
        cand = np.unique(np.concatenate(cand).astype(np.int64))
        o = cand[np.lexsort((cand, keys[i, cand]))][:k]
        out[i, :len(o)] = o
    return out, all_rows


T_RANGES = ((0, 128), (128, 300), (900, 1500))  # of fixture_t: the 41 copies of row 7 split across the first two


def t_ranges(m):
    lo = np.tile(np.array([r[0] for r in T_RANGES], np.int32), (m, 1))
    hi = np.tile(np.array([r[1] for r in T_RANGES], np.int32), (m, 1))
    return lo, hi


TILE = 128
TARGET_BLOCKS = 1024  # kProbeTargetBlocks


def items_per_block(n_items):
    """G: 128 once that gives TARGET_BLOCKS blocks, else n_items / TARGET_BLOCKS, at least 1."""
    return max(1, min(128, n_items // TARGET_BLOCKS))


def block_runs(lo, hi, n, clean=True):
    """What the screen's blocks sweep for raw ranges [M, P]: the non-empty cleaned items ordered by their first tile
    (empty ones last), G consecutive ones per block, each block's (first tile, last tile) intervals merged into runs
    where they share a tile or are adjacent.  Returns a list, per block, of its runs [(first, last), ...].  Which of
    several items with the same first tile comes first is not defined by the kernel: the caller's ranges must not
    let that matter (equal first tile, equal last tile) if it compares counts.  ``clean=False``: the ranges are
    clean already (the check is quadratic in P)."""
    if clean:
        lo, hi, _ = clean_ranges(lo, hi, n)
    lo, hi = np.asarray(lo, np.int64).reshape(-1), np.asarray(hi, np.int64).reshape(-1)
    G = items_per_block(len(lo))
    live = np.flatnonzero(lo < hi)
    live = live[np.argsort(lo[live] // TILE, kind="stable")]
    order = np.concatenate([live, np.setdiff1d(np.arange(len(lo)), live)])
    blocks = []
    for b0 in range(0, len(order), G):
        items = [i for i in order[b0:b0 + G] if lo[i] < hi[i]]
        runs = []
        for f, l in sorted((int(lo[i] // TILE), int((hi[i] - 1) // TILE)) for i in items):
            if runs and f <= runs[-1][1] + 1:
                runs[-1][1] = max(runs[-1][1], l)
            else:
                runs.append([f, l])
        blocks.append([tuple(r) for r in runs])
    return blocks
