"""Assignment margins of a trained residual quantiser: how far the runner-up centre is behind the chosen one.

Built on ``RQEncoder.encode_topk(x, 2)`` (one rqsid_assign_topk pass per level over all rows).  With d1 <= d2 the
distances of a row's nearest and second-nearest allowed centre at a level:

* ``rows_ranked``: rows with two finite places (a segment with one allowed centre, a penalty segment or a
  non-finite row has none);
* ``mean_margin`` / ``min_margin``: mean and minimum of ``d2 - d1`` over the ranked rows (a row with a small margin
  flips its ID when the embeddings move);
* ``mean_silhouette``: mean of the simplified silhouette ``(d2 - d1) / d2`` (0 where d2 == 0), the cluster score
  the reference's QA (calculate_metrics.py) takes from sklearn on a 50k sample, here over every row (centre-based:
  the exact, pairwise score and the other two sklearn scores are ``cluster_report.py``'s);
* ``share_below``: per threshold, the share of ranked rows whose silhouette is below it.

Means of an empty set and the minimum of one are ``None``.  With a process group every rank passes its own shard;
the fp64 sums are all-reduced, so every rank returns the same dict.
"""
from __future__ import annotations

from typing import Dict, Sequence

import torch


def margin_report(enc, x: torch.Tensor, comm=None, thresholds: Sequence[float] = (1e-3, 1e-2, 1e-1)) -> Dict:
    """``enc``: an ``RQEncoder``; ``x``: this rank's rows on the device (f32, f16 or bf16); ``comm``:
    ``distributed.Comm`` or None."""
    import torch.distributed as dist
    L = enc.L
    dev = x.device
    th = [float(t) for t in thresholds]
    T = len(th)
    n_local = x.shape[0]
    if n_local:
        d = enc.encode_topk(x, 2).dist.double()
    else:  # a rank without rows still takes part in the collectives
        if L == 2:
            raise IndexError("list index out of range")  # as encode
        d = torch.zeros((0, L, 2), dtype=torch.float64, device=dev)
    d1, d2 = d[:, :, 0], d[:, :, 1]
    ranked = torch.isfinite(d1) & torch.isfinite(d2)
    zero = torch.zeros((), dtype=torch.float64, device=dev)
    margin = torch.where(ranked, d2 - d1, zero)
    sil = torch.where(ranked & (d2 > 0), (d2 - d1) / torch.where(d2 > 0, d2, 1.0), zero)
    # one fp64 vector to sum over ranks: rows, then per level {ranked rows, sum margin, sum silhouette, rows below t}
    parts = [torch.tensor([float(n_local)], dtype=torch.float64, device=dev), ranked.sum(0).double(), margin.sum(0),
             sil.sum(0)]
    parts += [(ranked & (sil < t)).sum(0).double() for t in th]
    tot = torch.cat(parts)
    inf = torch.full((), float("inf"), dtype=torch.float64, device=dev)
    mn = torch.where(ranked, d2 - d1, inf).amin(0) if n_local else inf.expand(L).clone()
    if comm is not None:
        tot = comm.all_reduce(tot)
        mn = comm.all_reduce(mn.contiguous(), op=dist.ReduceOp.MIN)
    tot, mn = tot.cpu().numpy(), mn.cpu().numpy()
    rows = int(tot[0])
    if rows == 0:
        raise ValueError("margin_report: no rows")
    levels = []
    for l in range(L):
        r = int(tot[1 + l])
        levels.append({
            "level": l + 1,
            "rows_ranked": r,
            "mean_margin": float(tot[1 + L + l]) / r if r else None,
            "mean_silhouette": float(tot[1 + 2 * L + l]) / r if r else None,
            "min_margin": float(mn[l]) if r else None,
            "share_below": {f"{t:g}": (float(tot[1 + (3 + i) * L + l]) / r if r else None) for i, t in enumerate(th)},
        })
    return {"rows": rows, "thresholds": th, "levels": levels}
