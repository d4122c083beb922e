"""Quantisation report of a trained residual quantiser: how well the semantic IDs stand for the rows.

The reference has no direct measure of this: its QA is sklearn cluster scores on a 50k sample
(calculate_metrics.py) and ID-usage counts (train_semantic_ids.py:290-333 ``_generate_statistics``).  The
report below is built from ``RQEncoder.quant_error`` (one streaming HIP pass over the rows) and the IDs:

* ``rows``;
* ``levels[l]``: ``mse`` (mean squared distance from level l's input vector to its assigned centre, in the
  level's own space), ``rmse``, ``max``, ``recon_mse`` (mean squared error in the ORIGINAL space had the chain
  stopped at this level), ``relative`` (that error's share of the rows' energy, sum ||x - x_hat_l||^2 /
  sum ||x||^2), ``unique_clusters`` and the ``cluster_distribution`` quadruple of ``io.semantic_id_statistics``;
* ``unique_semantic_ids`` and ``coverage`` (unique IDs / rows, the figure train_semantic_ids.py:355 logs).

With a process group every rank passes its own shard; the fp64 sums, the maxima and the per-level ID counts are
all-reduced and the ranks' distinct IDs gathered, so every rank returns the same dict.
"""
from __future__ import annotations

import math
from typing import Dict, Optional

import numpy as np
import torch


def quantization_report(enc, x: torch.Tensor, comm=None, return_rows: bool = False) -> Dict:
    """``enc``: an ``RQEncoder`` with training-consistent semantics; ``x``: this rank's rows on the device (f32,
    f16 or bf16); ``comm``: ``distributed.Comm`` or None.  ``return_rows`` adds ``ids`` (int64 [N, L]), ``err``
    and ``recon_err`` as numpy arrays over ALL rows in rank order."""
    import torch.distributed as dist
    L = enc.L
    dev = x.device
    n_local = x.shape[0]
    if n_local:
        qe = enc.quant_error(x)
        ids, err, rec = qe.ids, qe.err, qe.recon_levels
        sums = qe.sums.clone()
    else:  # a rank without rows still takes part in the collectives
        ids = torch.zeros((0, L), dtype=torch.int32, device=dev)
        err = rec = torch.zeros((0, L), dtype=torch.float32, device=dev)
        sums = torch.zeros(L + 1, dtype=torch.float64, device=dev)
    # one fp64 vector to sum over ranks: rows, per level sum err^2 and sum recon^2, sum ||x||^2
    tot = torch.cat([torch.tensor([float(n_local)], dtype=torch.float64, device=dev), sums[:L],
                     rec.double().pow(2).sum(0), sums[L:]])
    mx = err.max(0).values.double() if n_local else torch.zeros(L, dtype=torch.float64, device=dev)
    kmax = [pc.k for pc in enc.pcs]  # every id of level l is below its codebook's size
    counts = [torch.bincount(ids[:, l].long(), minlength=kmax[l])[:kmax[l]] for l in range(L)]
    key = torch.zeros(n_local, dtype=torch.int64, device=dev)
    for l in range(L):
        key = key * kmax[l] + ids[:, l].long()
    uniq = torch.unique(key)
    if comm is not None:
        tot = comm.all_reduce(tot)
        mx = comm.all_reduce(mx, op=dist.ReduceOp.MAX)
        counts = [comm.all_reduce(c) for c in counts]
        uniq = torch.unique(comm.all_gather_rows(uniq))
    tot, mx = tot.cpu().numpy(), mx.cpu().numpy()
    rows = int(tot[0])
    if rows == 0:
        raise ValueError("quantization_error: no rows")
    energy = float(tot[2 * L + 1])
    levels = []
    for l in range(L):
        c = counts[l].cpu().numpy()
        c = c[:int(np.nonzero(c)[0].max()) + 1]  # np.bincount's length: the largest id seen + 1
        mse = float(tot[1 + l]) / rows
        levels.append({
            "level": l + 1,
            "mse": mse,
            "rmse": math.sqrt(mse),
            "max": float(mx[l]),
            "recon_mse": float(tot[1 + L + l]) / rows,
            "relative": float(tot[1 + L + l]) / energy if energy > 0 else float("nan"),
            "unique_clusters": int((c > 0).sum()),
            "cluster_distribution": {"min": int(c.min()), "max": int(c.max()), "mean": float(c.mean()),
                                     "std": float(c.std())},
        })
    n_unique = int(uniq.numel())
    out = {"rows": rows, "levels": levels, "unique_semantic_ids": n_unique, "coverage": n_unique / rows}
    if return_rows:
        gather = (lambda t: t) if comm is None else comm.all_gather_rows
        out["ids"] = gather(ids.contiguous()).cpu().numpy().astype(np.int64)
        out["err"] = gather(err.contiguous()).cpu().numpy()
        out["recon_err"] = gather(rec[:, L - 1].contiguous()).cpu().numpy()
    return out


def shard_rows(X: np.ndarray, device, group=None):
    """The rows of this rank on the device, as ``predict`` sends them (fp16 stays fp16), and the Comm (or None)."""
    row_dtype = np.float16 if X.dtype == np.float16 else np.float32
    comm: Optional[object] = None
    if group is not None:
        from .distributed import Comm, shard_bounds
        comm = Comm(group)
        s0, s1 = shard_bounds(len(X), comm.rank, comm.world)
        X = X[s0:s1]
    return torch.from_numpy(np.ascontiguousarray(X, dtype=row_dtype)).to(device), comm
