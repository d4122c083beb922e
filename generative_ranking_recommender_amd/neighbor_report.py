"""Neighbourhood preservation of a set of semantic IDs, and the nearest rows inside an ID cluster.

The reference's src/semantic_id_generator/evaluate_semantic_ids.py checks an ID set by hand: ``Evaluator.find_neighbors``
takes one song and ranks the other songs of its level-1 cluster by cosine similarity of the raw vectors, one Python
loop per song.  Both functions here rest on ``ops.row_knn`` (rqsid_row_knn: the EXACT k nearest rows, fp64 keys, ties
to the lowest row number, no distance matrix):

* ``neighbor_report``: of a sampled row's ``k`` true nearest rows in the raw space (the row itself excluded), how many
  share its first p IDs.  One unrestricted search serves every depth.  Per depth: ``recall`` (shared slots / filled
  slots over all sampled rows), ``all_shared`` and ``none_shared`` (shares of the sampled rows that have a neighbour
  at all), ``clusters`` (distinct prefixes among all rows).  Top level: ``rows``, ``sample``, ``seed``, ``k``,
  ``metric``, ``mean_neighbor_value`` (per slot: the mean distance / similarity of the filled slots; None for a slot
  nobody fills), ``counters`` (the kernel's: queries ranked from their lists, (query, chunk) pairs that took the
  all-rows pass, queries without an answer) and ``depths``.
* ``index_recall``: what a search THROUGH the IDs finds (``RQEncoder.search``: the query's ``P`` nearest ID prefixes of
  a depth, the rows under them, ``ops.probe_knn``): one exact unrestricted search is the truth, then one probe search
  per (depth, P).  Per pair, in ``searches``: ``depth``, ``probes``, ``recall`` (the truth's filled slots the search
  also returned / all filled slots), ``all_found`` (share of the sampled rows with a neighbour whose every true
  neighbour was returned), ``mean_scanned_share`` (catalogue positions read per query / rows) and ``counters`` (the
  probe kernel's: queries ranked from their lists, (query, probe) items that took the all-rows pass, queries without
  an answer, tile visits).  Top level: ``rows``, ``sample``, ``seed``, ``k``, ``metric``.
* ``neighbors_in_cluster``: ``find_neighbors`` for many rows at once: the ``top_n`` nearest rows among those that share
  the row's first ``depth`` IDs, the row itself excluded.

Single process only: the multi-GPU form is not built; a process group raises.
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence

import numpy as np
import torch

from .cluster_report import _group, prefix_keys, sample_rows


def neighbor_report(enc, x: torch.Tensor, ids: Optional[torch.Tensor] = None, sample: int = 50000, seed: int = 0,
                    k: int = 10, metric: str = "cosine", depths: Optional[Sequence[int]] = None, comm=None) -> Dict:
    """``enc``: an ``RQEncoder``; ``x``: the rows on the device (f32, f16 or bf16 [N, D]); ``ids``: their IDs
    (int [N, L]; default ``enc.encode(x)``); ``depths``: the prefix depths to report (default 1 .. L)."""
    from . import ops
    if comm is not None:
        raise NotImplementedError("neighbor_report: the multi-GPU form is not built (single process only)")
    n = x.shape[0]
    if n == 0:
        raise ValueError("neighbor_report: no rows")
    if ids is None:
        ids = enc.encode(x)
    L = ids.shape[1]
    depths = list(range(1, L + 1)) if depths is None else [int(p) for p in depths]
    if any(not 1 <= p <= L for p in depths):
        raise ValueError(f"neighbor_report: depths must lie in 1..{L}")
    radices = [pc.k for pc in enc.pcs]
    rows = sample_rows(n, sample, seed)
    q_rows = torch.from_numpy(rows).to(x.device)
    ws = ops.RowKnnWorkspace(n, len(rows), k, x.device)
    nbr, val = ops.row_knn(x, x[q_rows].contiguous(), k, metric, query_self=q_rows.to(torch.int32).contiguous(),
                           workspace=ws)
    filled = nbr >= 0
    slots = filled.sum(0)
    sums = torch.where(filled, val.double(), torch.zeros((), dtype=torch.float64, device=x.device)).sum(0)
    report = {"rows": int(n), "sample": int(len(rows)), "seed": int(seed), "k": int(k), "metric": metric,
              "mean_neighbor_value": [float(s / c) if c else None for s, c in zip(sums.tolist(), slots.tolist())],
              "counters": ws.counters(), "depths": []}
    per_query = filled.sum(1)
    answered = int((per_query > 0).sum())
    total = int(per_query.sum())
    for p in depths:
        key = prefix_keys(ids, radices, p)
        shared = (filled & (key[nbr.clamp(min=0).long()] == key[q_rows][:, None])).sum(1)
        report["depths"].append({
            "depth": p, "clusters": int(torch.unique(key).numel()),
            "recall": float(shared.sum()) / total if total else None,
            "all_shared": float(((shared == per_query) & (per_query > 0)).sum()) / answered if answered else None,
            "none_shared": float(((shared == 0) & (per_query > 0)).sum()) / answered if answered else None})
    return report


def _found(truth: torch.Tensor, got: torch.Tensor) -> torch.Tensor:
    """bool [M, k]: the truth's filled slots whose row the search returned as well."""
    return (truth >= 0) & (truth[:, :, None] == got[:, None, :]).any(-1)


def index_recall(enc, x: torch.Tensor, ids: Optional[torch.Tensor] = None, sample: int = 50000, seed: int = 0,
                 k: int = 10, metric: str = "cosine", depths: Optional[Sequence[int]] = None,
                 probes: Sequence[int] = (1, 2, 4, 8), comm=None) -> Dict:
    """``enc``: an ``RQEncoder`` in ``encode_beam``'s domain; ``x``: the catalogue on the device; ``ids``: its IDs
    (default ``enc.encode(x)``); ``depths``: the prefix depths to probe (default 1 .. L); ``probes``: the numbers of
    prefixes per query.  The sampled rows are the queries, each excluded from its own answer."""
    from . import ops
    if comm is not None:
        raise NotImplementedError("index_recall: the multi-GPU form is not built (single process only)")
    n = x.shape[0]
    if n == 0:
        raise ValueError("index_recall: no rows")
    if ids is None:
        ids = enc.encode(x)
    L = ids.shape[1]
    depths = list(range(1, L + 1)) if depths is None else [int(p) for p in depths]
    if any(not 1 <= p <= L for p in depths):
        raise ValueError(f"index_recall: depths must lie in 1..{L}")
    probes = [int(p) for p in probes]
    rows = sample_rows(n, sample, seed)
    q_rows = torch.from_numpy(rows).to(x.device)
    q = x[q_rows].contiguous()
    q_self = q_rows.to(torch.int32).contiguous()
    truth, _ = ops.row_knn(x, q, k, metric, query_self=q_self)
    per_query = (truth >= 0).sum(1)
    answered = int((per_query > 0).sum())
    total = int(per_query.sum())
    index = enc.id_index(ids.to(torch.int32).contiguous())
    report = {"rows": int(n), "sample": int(len(rows)), "seed": int(seed), "k": int(k), "metric": metric,
              "searches": []}
    for depth in depths:
        for P in probes:
            ws = ops.ProbeKnnWorkspace(n, len(rows), P, k, x.device)
            got = enc.search(x, index, q, k=k, probes=P, depth=depth, metric=metric, query_self=q_self, workspace=ws)
            found = _found(truth, got.rows).sum(1)
            report["searches"].append({
                "depth": depth, "probes": P,
                "recall": float(found.sum()) / total if total else None,
                "all_found": float(((found == per_query) & (per_query > 0)).sum()) / answered if answered else None,
                "mean_scanned_share": float(got.scanned.double().mean()) / n,
                "counters": ws.counters()})
    return report


def neighbors_in_cluster(x: torch.Tensor, ids: torch.Tensor, radices: Sequence[int], rows, top_n: int = 10,
                         depth: int = 1, metric: str = "cosine"):
    """For every row in ``rows`` (row numbers of ``x``): its ``top_n`` nearest rows among those with the same first
    ``depth`` IDs, itself excluded.  Returns ``(neighbors i32 [M, top_n], values f32 [M, top_n])`` in the order of
    ``rows``; -1 / +inf where the cluster has fewer other rows."""
    from . import ops
    if not 1 <= depth <= ids.shape[1]:
        raise ValueError(f"neighbors_in_cluster: depth must lie in 1..{ids.shape[1]}")
    q_rows = torch.as_tensor(np.asarray(rows), dtype=torch.int64, device=x.device)
    uniq, inv = torch.unique(prefix_keys(ids, radices, depth), return_inverse=True)
    order, off, _, _ = _group(inv, int(uniq.numel()), ops.centroid_tile_rows())
    # the kernel skips the tiles outside the union of a block's ranges: queries sorted by segment keep it narrow
    by_seg = torch.sort(inv[q_rows], stable=True)
    q_sorted = q_rows[by_seg.indices]
    nbr, val = ops.row_knn(x, x[q_sorted].contiguous(), top_n, metric, order=order, seg_row_off=off,
                           query_self=q_sorted.to(torch.int32).contiguous(),
                           query_seg=by_seg.values.to(torch.int32).contiguous())
    back = torch.empty_like(by_seg.indices)
    back[by_seg.indices] = torch.arange(len(q_rows), device=x.device)
    return nbr[back], val[back]
