#!/usr/bin/env python3
"""rqsid_probe_knn at the bench shape (10M x 512 rows as bench.py makes them with the fitted codebooks, 50,000 sampled
query rows, self excluded, k = 10) in ONE process: per prefix depth 1 / 2 / 3 and P = 1 / 2 / 4 / 8 probed prefixes

  ours         ops.probe_knn alone between device events (cosine and l2, fp32 and fp16 rows), its four counters, the
               mean scanned share, the recall against the exact unrestricted ops.row_knn of the same rows, and the
               peak device memory above what is resident; probe selection (RQEncoder.probe_prefixes and
               IdCells.prefix_ranges) is timed separately;
  composition  the only way to the same answer without the entry: every query gathered P times, ops.row_knn with
               query_seg on the depth's bucketing (the copies sorted by segment, which is the order that kernel's
               tile skip likes best), and a torch merge of the P * k entries per query.  cosine, fp32 rows.

and once more with few queries (default 1,000), where the composition's blocks span most of the catalogue.  One
warm-up, then the variants alternating; median / min / max.  Writes one JSON document (default
profiles/probe_ab.json); DESIGN.md 3.3f quotes it.
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))

import bench  # noqa: E402  (codebooks and rows exactly as the benchmark builds them)
from generative_ranking_recommender_amd import cluster_report as CR  # noqa: E402
from generative_ranking_recommender_amd import ops  # noqa: E402
from generative_ranking_recommender_amd.encode import HIERARCHICAL_TRAIN, RQEncoder  # noqa: E402


def log(msg):
    print(f"[probe_bench] {msg}", file=sys.stderr, flush=True)


def stats(v):
    return {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "n": len(v)}


def timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    out = fn()
    e.record()
    torch.cuda.synchronize()
    return out, s.elapsed_time(e)


def peak_above(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    return out, torch.cuda.max_memory_allocated() - base


def recall(truth, got):
    filled = truth >= 0
    found = filled & (truth[:, :, None] == got[:, None, :]).any(-1)
    return float(found.sum()) / max(int(filled.sum()), 1)


class Depth:
    """The depth's bucketing for the composition: the rows grouped by prefix, and a query's segment per prefix."""

    def __init__(self, ids, radices, depth):
        self.radices, self.depth = radices, depth
        self.uniq, inv = torch.unique(CR.prefix_keys(ids, radices, depth), return_inverse=True)
        self.order, off, _, _ = CR._group(inv, int(self.uniq.numel()), ops.centroid_tile_rows())
        self.off = torch.cat([off, off[-1:]]).contiguous()  # one more, empty, segment for a dead or absent prefix
        self.empty = int(self.uniq.numel())

    def segments(self, prefixes):
        """i32 [M, P]: the segment of every prefix."""
        dead = (prefixes < 0).any(-1)
        key = CR.prefix_keys(prefixes.reshape(-1, self.depth).clamp(min=0), self.radices, self.depth)
        at = torch.searchsorted(self.uniq, key).clamp(max=self.empty - 1)
        seg = torch.where(self.uniq[at] == key, at, torch.full_like(at, self.empty)).reshape(dead.shape)
        return torch.where(dead, torch.full_like(seg, self.empty), seg).to(torch.int32)


def composition(x, q, qself, dp, seg, k, metric, ws=None):
    """(rows [M, k], val [M, k]) through ops.row_knn: gather, restricted search, merge."""
    m, P = seg.shape
    by_seg = torch.sort(seg.reshape(-1), stable=True)
    src = torch.div(by_seg.indices, P, rounding_mode="floor")
    qq = q[src].contiguous()                                     # the gather of M * P * D elements
    rows, val = ops.row_knn(x, qq, k, metric, order=dp.order, seg_row_off=dp.off, query_self=qself[src].contiguous(),
                            query_seg=by_seg.values.contiguous(), workspace=ws, check=False)
    back = torch.empty_like(by_seg.indices)
    back[by_seg.indices] = torch.arange(m * P, device=q.device)
    rows, val = rows[back].reshape(m, P * k), val[back].reshape(m, P * k)
    # the merge: distinct prefixes hold distinct rows, so de-duplication comes down to ordering the empty slots last
    score = torch.where(rows >= 0, val if metric == "cosine" else -val, torch.full_like(val, float("-inf")))
    pick = torch.topk(score, k, dim=1).indices
    return torch.gather(rows, 1, pick), torch.gather(val, 1, pick)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--sample", type=int, default=50_000)
    ap.add_argument("--few", type=int, default=1_000)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--alternations", type=int, default=3)
    ap.add_argument("--probes", type=int, nargs="+", default=[1, 2, 4, 8])
    ap.add_argument("--codebooks", choices=("fitted", "sampled"), default="fitted")
    ap.add_argument("--out", default=str(REPO / "profiles" / "probe_ab.json"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    cb = bench.codebooks(a.codebooks, dev)
    enc = RQEncoder([torch.from_numpy(cb[k]) for k in ("c0", "c1", "c2")], list(bench.NEED),
                    match=torch.from_numpy(cb["match"]), semantics=HIERARCHICAL_TRAIN, device=dev)
    x32 = bench.make_rows(a.rows, 0, dev)
    n, d = x32.shape
    ids = enc.encode(x32)
    index = enc.id_index(ids)
    radices = [pc.k for pc in enc.pcs]
    L, k = ids.shape[1], a.k
    xs = {"f32": x32, "f16": x32.to(torch.float16)}
    depths = {p: Depth(ids, radices, p) for p in range(1, L + 1)}
    torch.cuda.synchronize()
    log(f"{n} rows, their IDs, the cell index ({index.n_cells} cells) and the depths' bucketings ready")

    doc = {"what": "tools/probe_bench.py: rqsid_probe_knn through the ID index against gather + restricted "
                   "rqsid_row_knn + torch merge, one process (measured)",
           "rows": n, "dim": d, "k": k, "seed": a.seed, "need": list(bench.NEED), "codebooks": a.codebooks,
           "alternations": a.alternations, "warmup": 1, "device": torch.cuda.get_device_name(dev),
           "prefixes_per_depth": {str(p): int(dp.uniq.numel()) for p, dp in depths.items()}, "runs": []}

    for m_want, tag in ((a.sample, "sample"), (a.few, "few")):
        rows = torch.from_numpy(CR.sample_rows(n, m_want, a.seed)).to(dev)
        m = rows.numel()
        qself = rows.to(torch.int32).contiguous()
        qs = {f: v[rows].contiguous() for f, v in xs.items()}
        variants = [(metric, f) for metric in ("cosine", "l2") for f in ("f32", "f16")] if tag == "sample" \
            else [("cosine", "f32")]
        truth = {}
        for metric, f in variants:
            (truth[metric, f], _), ms = timed(lambda: ops.row_knn(xs[f], qs[f], k, metric, query_self=qself))
            log(f"{tag}: exact unrestricted {metric} {f}: {ms:.0f} ms")
        kws = None
        for depth, dp in depths.items():
            for P in a.probes:
                enc.probe_prefixes(qs["f32"], depth, P)  # warm
                prefixes, select_ms = timed(lambda: enc.probe_prefixes(qs["f32"], depth, P))
                (lo, hi), ranges_ms = timed(lambda: index.prefix_ranges(prefixes))
                seg = dp.segments(prefixes)
                ws = ops.ProbeKnnWorkspace(n, m, P, k, dev)
                need = int(ops.lib().rqsid_row_knn_workspace_bytes(n, m * P, k, 0))
                if kws is None or kws.bytes < need:
                    kws = None
                    kws = ops.RowKnnWorkspace(n, m * P, k, dev)
                fns = {f"{metric}_{f}": (lambda metric=metric, f=f: ops.probe_knn(
                    xs[f], qs[f], k, lo, hi, metric, order=index.order, query_self=qself, workspace=ws, check=False))
                    for metric, f in variants}
                fns["composition_cosine_f32"] = lambda: composition(x32, qs["f32"], qself, dp, seg, k, "cosine", kws)
                run = {"queries": m, "set": tag, "depth": depth, "probes": P, "select_ms": select_ms,
                       "prefix_ranges_ms": ranges_ms, "ours": {}, "probe_workspace_bytes": ws.bytes}
                outs, peak = {}, {}
                for name, fn in fns.items():
                    outs[name], peak[name] = peak_above(fn)  # the warm-up
                    if not name.startswith("composition"):
                        metric, f = name.split("_")
                        run["ours"][name] = {"counters": ws.counters(), "recall": recall(truth[metric, f], outs[name][0]),
                                             "mean_scanned_share": float(outs[name][2].double().mean()) / n,
                                             "peak_bytes_above_resident": peak[name]}
                ops.check_error_words([ws.error_word()], "rqsid_probe_knn", ops.PROBE_KNN_WORD)
                same = (outs["cosine_f32"][0] == outs["composition_cosine_f32"][0]).all(1).double().mean()
                res = {name: [] for name in fns}
                for _ in range(a.alternations):
                    for name, fn in fns.items():
                        res[name].append(timed(fn)[1])
                for name in fns:
                    if name.startswith("composition"):
                        run["composition"] = dict(stats(res[name]), peak_bytes_above_resident=peak[name],
                                                  row_knn_workspace_bytes=kws.bytes,
                                                  lists_equal_share=float(same))
                    else:
                        run["ours"][name].update(stats(res[name]))
                run["ratio_composition_over_ours"] = run["composition"]["median_ms"] / \
                    run["ours"]["cosine_f32"]["median_ms"]
                doc["runs"].append(run)
                log(f"{tag} depth {depth} P {P}: ours {run['ours']['cosine_f32']['median_ms']:.2f} ms, composition "
                    f"{run['composition']['median_ms']:.2f} ms, recall {run['ours']['cosine_f32']['recall']:.4f}, "
                    f"scanned {run['ours']['cosine_f32']['mean_scanned_share']:.2e}")
                del outs
    ratios = [r["ratio_composition_over_ours"] for r in doc["runs"]]
    doc["criterion"] = {"text": "ours at most half the composition's time at every (depth, P)",
                        "smallest_ratio_composition_over_ours": min(ratios), "met": min(ratios) >= 2.0}
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(doc, indent=1) + "\n")
    print(json.dumps({"criterion": doc["criterion"],
                      "runs": [[r["set"], r["depth"], r["probes"], round(r["ours"]["cosine_f32"]["median_ms"], 3),
                                round(r["composition"]["median_ms"], 3), round(r["ours"]["cosine_f32"]["recall"], 4)]
                               for r in doc["runs"]]}))


if __name__ == "__main__":
    main()
