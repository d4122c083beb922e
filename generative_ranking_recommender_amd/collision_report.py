"""Collision report of semantic IDs: which IDs are shared, by how many rows, and how the ID space is used.

The reference diagnoses low coverage with two stand-alone scripts over ``song_semantic_ids.jsonl``
(src/semantic_id_generator/debug_collisions.py and analyze_semantic_ids.py: Python dicts and Counters over every
row).  The report below holds the same quantities, computed from the cell index of the IDs (``RQEncoder.id_index``,
one pass of rqsid_id_cells) and its per-cell arrays on the device:

* ``rows``, ``unique_semantic_ids``, ``coverage``: ``quantization_report``'s figures;
* ``colliding_ids`` (IDs shared by two or more rows), ``rows_in_collisions`` (the rows of those IDs),
  ``max_collision`` (the rows of the most shared ID; 0 without a collision): debug_collisions.py's three figures;
* ``ids_used_once`` and ``ids_used_once_share`` (of the unique IDs), ``rows_per_id`` (rows / unique IDs);
* ``size_histogram``: ``{str(2^b): IDs shared by 2^b .. 2^(b+1) - 1 rows}``, occupied bins only;
* ``dedup_token_bits``: ceil(log2(rows of the most shared ID)), the width of a disambiguating last token;
* ``worst``: the ``top`` most shared IDs, each ``{"semantic_id", "size", "rows"}`` with its first ``members`` rows in
  rank order (by original-space reconstruction error, the order of ``RQEncoder.unique_ids``; by row number where the
  encoder's semantics leave that error undefined); ``most_common``: the 10 most shared IDs, ``{"semantic_id",
  "size"}``.  Equal sizes come in ascending ID order;
* ``level_unique_ids``: per level the number of distinct IDs;
* ``prefixes`` (L >= 2), over the used prefixes of depth L - 1: ``depth``, ``used``, ``possible``, ``share``,
  ``last_level_ids`` and ``rows`` (per prefix: ``mean``, ``min``, ``max``, ``median``, ``std``) and ``fewest_rows``,
  the 10 prefixes with the fewest rows, ``{"prefix", "rows", "last_level_ids"}`` (ties in ascending prefix order).

Single process only.  Rows whose ID names no cell (a -1 of a penalty segment) are reported as ``rows_without_id``
and take no part in any other figure but ``rows``.
"""
from __future__ import annotations

from typing import Dict, Optional

import torch


def _five(v: torch.Tensor) -> Dict:
    """mean, min, max, median and (population) standard deviation of a non-empty device vector, numpy's definitions."""
    s = torch.sort(v.double()).values
    n = s.numel()
    return {"mean": float(s.mean().item()), "min": float(s[0].item()), "max": float(s[-1].item()),
            "median": float(((s[(n - 1) // 2] + s[n // 2]) / 2).item()),
            "std": float(s.std(unbiased=False).item()) if n > 1 else 0.0}


def _largest(sizes: torch.Tensor, count: int):
    """Cell numbers of the ``count`` largest cells, equal sizes in ascending cell order."""
    order = torch.sort(sizes, descending=True, stable=True).indices
    return order[:count]


def collision_report(enc, x: torch.Tensor, ids: Optional[torch.Tensor] = None, top: int = 5, members: int = 10,
                     comm=None, return_index: bool = False):
    """``enc``: an ``RQEncoder``; ``x``: the rows on the device; ``ids``: their IDs (default ``enc.encode(x)``).
    ``return_index`` also returns the ``ops.IdCells`` the figures came from."""
    if comm is not None:
        raise NotImplementedError("collision_report: the multi-GPU form is not built (single process only)")
    if enc.sem.residual_global_id:
        qe = enc.quant_error(x, ids)
        ids, key = qe.ids, qe.recon_err.contiguous()
    else:  # the reconstruction error of such IDs is undefined (RQEncoder.quant_error): rank by row number
        ids = enc.encode(x) if ids is None else ids
        key = None
    rows = int(ids.shape[0])
    if rows == 0:
        raise ValueError("collision_report: no rows")
    index = enc.id_index(ids, key)
    n = index.n_cells
    ctr = index.counters.tolist()
    sizes = (index.cell_off[1:n + 1] - index.cell_off[:n]).long()
    largest = ctr[4]
    out = {
        "rows": rows,
        "rows_without_id": index.n_invalid,
        "unique_semantic_ids": n,
        "coverage": n / rows,
        "colliding_ids": ctr[1],
        "rows_in_collisions": ctr[2],
        "max_collision": largest if ctr[1] else 0,
        "ids_used_once": ctr[3],
        "ids_used_once_share": ctr[3] / n if n else 0.0,
        "rows_per_id": rows / n if n else 0.0,
        "size_histogram": {str(1 << b): c for b, c in enumerate(ctr[5:37]) if c},
        "dedup_token_bits": (largest - 1).bit_length() if largest > 1 else 0,
    }
    big = _largest(sizes, max(int(top), 10))
    big_ids = index.ids_of(big).tolist()
    big_sizes = sizes[big].tolist()
    big_off = index.cell_off[big].tolist()
    out["worst"] = [{"semantic_id": big_ids[i], "size": big_sizes[i],
                     "rows": index.order[big_off[i]:big_off[i] + min(big_sizes[i], int(members))].tolist()}
                    for i in range(min(int(top), len(big_ids)))]
    out["most_common"] = [{"semantic_id": big_ids[i], "size": big_sizes[i]} for i in range(min(10, len(big_ids)))]
    all_ids = index.ids_of(torch.arange(n, device=sizes.device))
    out["level_unique_ids"] = [int(torch.unique(all_ids[:, l]).numel()) for l in range(all_ids.shape[1])]
    L = len(index.sizes)
    if L >= 2 and n:
        # a prefix of depth L - 1 is a group: its cells are consecutive
        grp, per = torch.unique_consecutive(index.cell_group[:n], return_counts=True)
        start = torch.cumsum(per, 0) - per
        csum = torch.cat([sizes.new_zeros(1), torch.cumsum(sizes, 0)])
        prows = csum[start + per] - csum[start]
        possible = 1
        for s in index.sizes[:-1]:
            possible *= s
        few = torch.sort(prows, stable=True).indices[:10]
        few_prefix = []
        g = grp[few].long()
        for s in reversed(index.sizes[:-1]):
            few_prefix.append(g % s)
            g = g // s
        few_prefix = torch.stack(few_prefix[::-1], 1).tolist()
        out["prefixes"] = {
            "depth": L - 1, "used": int(grp.numel()), "possible": possible, "share": grp.numel() / possible,
            "last_level_ids": _five(per), "rows": _five(prows),
            "fewest_rows": [{"prefix": p, "rows": r, "last_level_ids": c}
                            for p, r, c in zip(few_prefix, prows[few].tolist(), per[few].tolist())],
        }
    return (out, index) if return_index else out
