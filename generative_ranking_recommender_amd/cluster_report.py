"""Cluster quality of a set of semantic IDs: the three scores of the reference's own check.

The reference's src/semantic_id_generator/calculate_metrics.py draws 50,000 songs, labels each by its semantic-ID
tuple and prints sklearn's ``silhouette_score``, ``calinski_harabasz_score`` and ``davies_bouldin_score`` on the raw
vectors.  ``cluster_report`` computes the same three numbers on the GPU, for every prefix depth of the IDs (depth p
labels a row by its first p IDs), in the ORIGINAL vector space:

* the silhouette is exact and pairwise (``ops.silhouette``, rqsid_silhouette: every scored row against every row,
  no distance matrix), unlike ``margin_report``'s simplified, centre-based one;
* Calinski-Harabasz and Davies-Bouldin are centroid-based and come from entry points that existed already:
  rqsid_centroid_accumulate / rqsid_centroid_finalize for the centroids, rqsid_quant_error with one level for the
  per-row distance to the own centroid, fp64 cumulative sums over the sorted order for the per-cluster totals.

``against="all"`` scores the sampled rows against every row; ``against="sample"`` first restricts rows and labels to
the sample, which is calculate_metrics.py's own computation (its numbers compare one to one).

Per depth: ``clusters`` (non-empty), ``silhouette`` (mean of the finite s; None without one), ``silhouette_scored``
(how many were finite), ``share_negative`` (share of those below 0), ``calinski_harabasz`` (None when K < 2 or
n <= K), ``davies_bouldin`` (None when K < 2 or K > ``db_max_clusters``: K x K centroid distances).  Top level:
``rows``, ``sample``, ``seed``, ``against``, ``depths``.  Single process only: the multi-GPU form (each rank scoring
foreign queries against the clusters it owns, then a MIN-reduce of b) is not built; a process group raises.
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence

import numpy as np
import torch

BUCKET_MAX_LABELS = 65536     # up to here rqsid_bucket groups the rows; beyond, torch.unique + a stable sort
WIDEN_CHUNK_ROWS = 1 << 20    # 16-bit rows are widened this many at a time for the centroid sums only


def prefix_keys(ids: torch.Tensor, radices: Sequence[int], depth: int) -> torch.Tensor:
    """int64 mixed-radix key of the first ``depth`` IDs of every row (ids [N, L], 0 <= ids[:, l] < radices[l])."""
    key = torch.zeros(ids.shape[0], dtype=torch.int64, device=ids.device)
    for l in range(depth):
        key = key * int(radices[l]) + ids[:, l].long()
    return key


def sample_rows(n: int, sample: int, seed: int) -> np.ndarray:
    """The scored rows: ``min(sample, n)`` distinct rows, sorted."""
    return np.sort(np.random.default_rng(seed).choice(n, min(int(sample), n), replace=False))


def centroid_scores(k: int, n: int, between: float, within: float, db: Optional[float], db_max_clusters: int):
    """(calinski_harabasz, davies_bouldin) with their None rules (sklearn's formulas otherwise)."""
    ch = None
    if k >= 2 and n > k:
        ch = 1.0 if within == 0.0 else (between / (k - 1)) / (within / (n - k))
    return ch, (db if 2 <= k <= db_max_clusters else None)


def silhouette_summary(s: np.ndarray) -> Dict:
    fin = s[np.isfinite(s)].astype(np.float64)
    return {"silhouette": float(fin.mean()) if fin.size else None, "silhouette_scored": int(fin.size),
            "share_negative": float((fin < 0).mean()) if fin.size else None}


def _group(labels: torch.Tensor, k: int, tile_rows: int):
    """Rows grouped by compact label 0 .. k-1: (order i32 [N], off i32 [k + 1], tile_off i32 [k + 1], max_tiles)."""
    from . import ops
    if k <= BUCKET_MAX_LABELS:
        b = ops.bucket(labels.to(torch.int32), k, rows_per_tile=tile_rows)
        ops.check_error_words([b.error_word()], "rqsid_bucket")
        return b.row_index, b.seg_row_off, b.seg_tile_off, b.max_tiles
    order = torch.sort(labels, stable=True).indices.to(torch.int32)
    cnt = torch.bincount(labels, minlength=k)
    zero = torch.zeros(1, dtype=torch.int64, device=labels.device)
    off = torch.cat([zero, torch.cumsum(cnt, 0)])
    toff = torch.cat([zero, torch.cumsum((cnt + tile_rows - 1) // tile_rows, 0)])
    return order, off.to(torch.int32), toff.to(torch.int32), int(toff[-1].item())


def _davies_bouldin(mu: torch.Tensor, intra: torch.Tensor) -> float:
    """sklearn's davies_bouldin_score from fp64 centroids [K, D] and mean intra-cluster distances [K]."""
    if float(intra.max()) <= 1e-8:
        return 0.0
    k = mu.shape[0]
    worst = torch.empty(k, dtype=torch.float64, device=mu.device)
    step = max(1, (1 << 24) // k)
    for i0 in range(0, k, step):
        m = torch.cdist(mu[i0:i0 + step], mu, compute_mode="donot_use_mm_for_euclid_dist")
        m[m == 0] = float("inf")  # (the diagonal too)
        worst[i0:i0 + step] = ((intra[i0:i0 + step, None] + intra[None, :]) / m).amax(1)
    return float(worst.mean())


def _depth_report(x: torch.Tensor, key: torch.Tensor, q_rows: torch.Tensor, db_max_clusters: int) -> Dict:
    """One depth: x [n, D] (f32 / f16 / bf16), key int64 [n], q_rows int64 [m] = the scored rows of x."""
    from . import _lib, ops
    n, d = x.shape
    dev = x.device
    uniq, inv = torch.unique(key, return_inverse=True)
    k = int(uniq.numel())
    order, off, toff, max_tiles = _group(inv, k, ops.centroid_tile_rows())
    inv32 = inv.to(torch.int32)
    # ---- silhouette: the scored rows against every row ----
    a, b, b_seg, s = ops.silhouette(x, order, off, x[q_rows].contiguous(), q_rows.to(torch.int32).contiguous(),
                                    inv32[q_rows].contiguous())
    out = {"clusters": k}
    out.update(silhouette_summary(s.cpu().numpy()))
    # ---- centroids (fp64 sums), per-row distance to the own centroid, per-cluster totals in the sorted order ----
    sums = torch.zeros((k, d), dtype=torch.float64, device=dev)
    lib = ops.lib()
    if x.dtype == torch.float32:
        _lib.check(lib.rqsid_centroid_accumulate(x.data_ptr(), d, order.data_ptr(), k, off.data_ptr(), toff.data_ptr(),
                                                 max_tiles, sums.data_ptr(), ops._stream()), "rqsid_centroid_accumulate")
    else:
        for r0 in range(0, n, WIDEN_CHUNK_ROWS):
            xc = x[r0:r0 + WIDEN_CHUNK_ROWS].float()
            o, f, t, mt = _group(inv[r0:r0 + WIDEN_CHUNK_ROWS], k, ops.centroid_tile_rows())
            _lib.check(lib.rqsid_centroid_accumulate(xc.data_ptr(), d, o.data_ptr(), k, f.data_ptr(), t.data_ptr(), mt,
                                                     sums.data_ptr(), ops._stream()), "rqsid_centroid_accumulate")
            torch.cuda.current_stream().synchronize()  # xc and the chunk's tables die with this iteration
    centres = torch.empty((k, d), dtype=torch.float32, device=dev)
    _lib.check(lib.rqsid_centroid_finalize(sums.data_ptr(), off.data_ptr(), k, d, centres.data_ptr(), ops._stream()),
               "rqsid_centroid_finalize")
    err, _, _ = ops.quant_error(x, [centres], [inv32.contiguous()], normalize=False, row_order=order,
                                want_x_norm=False, want_sums=False)
    dist = err[:, 0].double()
    cnt = (off[1:] - off[:-1]).double()
    mean = sums.sum(0) / n
    del sums
    mu = centres.double()
    between = float((cnt * (mu - mean).pow(2).sum(1)).sum())
    within = float(dist.pow(2).sum())
    db = None
    if 2 <= k <= db_max_clusters:
        run = torch.cat([torch.zeros(1, dtype=torch.float64, device=dev), torch.cumsum(dist[order.long()], 0)])
        intra = (run[off[1:].long()] - run[off[:-1].long()]) / cnt
        db = _davies_bouldin(mu, intra)
    ch, db = centroid_scores(k, n, between, within, db, db_max_clusters)
    out.update(calinski_harabasz=ch, davies_bouldin=db)
    return out


def cluster_report(enc, x: torch.Tensor, ids: Optional[torch.Tensor] = None, sample: int = 50000, seed: int = 0,
                   against: str = "all", depths: Optional[Sequence[int]] = None, db_max_clusters: int = 32768,
                   comm=None) -> Dict:
    """``enc``: an ``RQEncoder``; ``x``: the rows on the device (f32, f16 or bf16 [N, D]); ``ids``: their IDs
    (int [N, L]; default ``enc.encode(x)``); ``depths``: the prefix depths to report (default 1 .. L)."""
    if comm is not None:
        raise NotImplementedError("cluster_report: the multi-GPU form is not built (single process only)")
    if against not in ("all", "sample"):
        raise ValueError(f"cluster_report: against must be 'all' or 'sample', not {against!r}")
    n = x.shape[0]
    if n == 0:
        raise ValueError("cluster_report: no rows")
    if ids is None:
        ids = enc.encode(x)
    L = ids.shape[1]
    depths = list(range(1, L + 1)) if depths is None else [int(p) for p in depths]
    if any(not 1 <= p <= L for p in depths):
        raise ValueError(f"cluster_report: depths must lie in 1..{L}")
    radices = [pc.k for pc in enc.pcs]
    rows = sample_rows(n, sample, seed)
    q_rows = torch.from_numpy(rows).to(x.device)
    if against == "sample":
        x = x[q_rows].contiguous()
        ids = ids[q_rows]
        q_rows = torch.arange(len(rows), dtype=torch.int64, device=x.device)
    report = {"rows": int(n), "sample": int(len(rows)), "seed": int(seed), "against": against, "depths": []}
    for p in depths:
        entry = {"depth": p}
        entry.update(_depth_report(x, prefix_keys(ids, radices, p), q_rows, db_max_clusters))
        report["depths"].append(entry)
    return report
