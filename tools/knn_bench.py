#!/usr/bin/env python3
"""rqsid_row_knn at the bench shape (10M x 512 rows as bench.py makes them, 50,000 query rows, k = 10) in ONE process
against

  silhouette  ops.silhouette on the same rows, queries and depth-1 grouping: the same MFMA work with the walk this
              kernel replaces, so the ratio says what keeping the smallest values costs over summing them;
  torch       the only composition available without the kernel: per chunk of rows torch.cdist (l2) or a matmul of
              the normalised rows (cosine), the self entries masked by index, torch.topk, and a running merge of the
              best k.  fp32 rows only.  Its fp32 arithmetic is not exact: the share of queries on which its row lists
              equal the kernel's is recorded, not asserted.

ours: both metrics, fp32 and fp16 rows, unrestricted with the self row excluded, and one restricted run (cosine, fp32,
inside the depth-1 cluster, queries sorted by segment).  Per measurement: device events around the call alone, the
variants alternating, median / min / max over the timed repetitions after warm-up.  Also the kernel's three counters
and the peak device memory each side allocates above what is resident before it starts.  Writes one JSON document
(default profiles/knn_ab.json); DESIGN.md 3.3c quotes it.
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

PEAK_TF = 155.0


def log(msg):
    print(f"[knn_bench] {msg}", file=sys.stderr, flush=True)


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
    """(result, peak bytes allocated while fn ran above what was allocated before it)."""
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    return out, torch.cuda.max_memory_allocated() - base


def torch_knn(x, q, qself, k, metric, chunk):
    """The composition: (rows int64 [m, k], values [m, k]), ascending distance / descending similarity."""
    m, dev = q.shape[0], q.device
    largest = metric == "cosine"
    if largest:
        q = torch.nn.functional.normalize(q, dim=1)
    best_v = torch.full((m, k), float("-inf") if largest else float("inf"), dtype=torch.float32, device=dev)
    best_r = torch.full((m, k), -1, dtype=torch.int64, device=dev)
    qi = torch.arange(m, device=dev)
    for p0 in range(0, x.shape[0], chunk):
        xc = x[p0:p0 + chunk]
        v = q @ torch.nn.functional.normalize(xc, dim=1).T if largest else torch.cdist(q, xc)
        mine = (qself >= p0) & (qself < p0 + xc.shape[0])
        v[qi[mine], qself[mine] - p0] = float("-inf") if largest else float("inf")
        cv, cr = torch.topk(v, min(k, xc.shape[0]), dim=1, largest=largest)
        del v
        av, ar = torch.cat([best_v, cv], 1), torch.cat([best_r, cr + p0], 1)
        best_v, pick = torch.topk(av, k, dim=1, largest=largest)
        best_r = torch.gather(ar, 1, pick)
    return best_r, best_v


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--sample", type=int, default=50_000)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--alternations", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--chunk", type=int, default=1 << 16, help="rows per chunk of the torch composition")
    ap.add_argument("--chunk-rows", type=int, default=0, help="rqsid_row_knn's chunk_rows (0 = automatic)")
    ap.add_argument("--codebooks", choices=("fitted", "sampled"), default="fitted")
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--out", default=str(REPO / "profiles" / "knn_ab.json"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    cb = bench.codebooks(a.codebooks, dev)
    enc = RQEncoder([torch.from_numpy(cb[k]) for k in ("c0", "c1", "c2")], list(bench.NEED),
                    match=torch.from_numpy(cb["match"]), semantics=HIERARCHICAL_TRAIN, device=dev)
    x32 = bench.make_rows(a.rows, 0, dev)
    n, d = x32.shape
    ids = enc.encode(x32)
    radices = [pc.k for pc in enc.pcs]
    rows = torch.from_numpy(CR.sample_rows(n, a.sample, a.seed)).to(dev)
    m, k = rows.numel(), a.k
    xs = {"f32": x32, "f16": x32.to(torch.float16)}
    qs = {f: v[rows].contiguous() for f, v in xs.items()}
    qself = rows.to(torch.int32)
    # the depth-1 grouping: the silhouette's segments, and the restricted search's (its queries sorted by segment)
    uniq, inv = torch.unique(CR.prefix_keys(ids, radices, 1), return_inverse=True)
    order, off, _, _ = CR._group(inv, int(uniq.numel()), ops.centroid_tile_rows())
    qseg = inv[rows].to(torch.int32).contiguous()
    by_seg = torch.sort(qseg, stable=True)
    r_rows = rows[by_seg.indices]
    r_q, r_self, r_seg = x32[r_rows].contiguous(), r_rows.to(torch.int32), by_seg.values.contiguous()
    torch.cuda.synchronize()
    log(f"codebooks, {n} rows, their IDs, {m} queries and {uniq.numel()} depth-1 clusters ready")

    ws = ops.RowKnnWorkspace(n, m, k, dev, a.chunk_rows)
    sws = ops.SilhouetteWorkspace(n, m, dev, 0)

    def knn(metric, f):
        return ops.row_knn(xs[f], qs[f], k, metric, query_self=qself, chunk_rows=a.chunk_rows, workspace=ws,
                           check=False)

    def knn_restricted():
        return ops.row_knn(x32, r_q, k, "cosine", order=order, seg_row_off=off, query_self=r_self, query_seg=r_seg,
                           chunk_rows=a.chunk_rows, workspace=ws, check=False)

    def sil(f):
        return ops.silhouette(xs[f], order, off, qs[f], qself, qseg, workspace=sws, check=False)

    variants = {f"{metric}_{f}": (lambda metric=metric, f=f: knn(metric, f))
                for metric in ("l2", "cosine") for f in ("f32", "f16")}
    variants["cosine_f32_depth1"] = knn_restricted
    variants["silhouette_f32"] = lambda: sil("f32")
    variants["silhouette_f16"] = lambda: sil("f16")
    res = {name: [] for name in variants}
    counters, ours_rows, peak = {}, {}, {}
    for name, fn in variants.items():
        for _ in range(a.warmup):
            out, peak[name] = peak_above(fn)
        if not name.startswith("silhouette"):
            counters[name] = ws.counters()
            ours_rows[name] = out[0]
        log(f"{name}: warm" + (f", counters {counters[name]}" if name in counters else ""))
    ops.check_error_words([ws.error_word()], "rqsid_row_knn", ops.SILHOUETTE_WORD)
    peak_ws = {"row_knn_workspace_bytes": ws.bytes, "silhouette_workspace_bytes": sws.bytes}

    torch_res, agree, torch_peak = {}, {}, {}
    if not a.no_torch:
        for metric in ("l2", "cosine"):
            args = (x32, qs["f32"], rows, k, metric, a.chunk)
            for _ in range(a.warmup):
                (tr, _), torch_peak[metric] = peak_above(lambda: torch_knn(*args))
            agree[metric] = float((tr == ours_rows[f"{metric}_f32"].long()).all(1).double().mean().item())
            torch_res[metric] = [timed(lambda: torch_knn(*args))[1] for _ in range(a.alternations)]
            log(f"torch {metric}: {torch_res[metric]} ms, lists equal on {agree[metric]:.6f} of the queries")
            del tr

    for alt in range(a.alternations):
        log(f"alternation {alt}")
        for name, fn in variants.items():
            res[name].append(timed(fn)[1])
    ops.check_error_words([ws.error_word()], "rqsid_row_knn", ops.SILHOUETTE_WORD)

    flop = 2.0 * m * n * d
    doc = {"what": "tools/knn_bench.py: rqsid_row_knn against rqsid_silhouette (same MFMA work) and against chunked "
                   "torch.cdist / matmul + torch.topk + a running merge, one process (measured)",
           "rows": n, "dim": d, "queries": m, "k": k, "seed": a.seed, "need": list(bench.NEED),
           "codebooks": a.codebooks, "alternations": a.alternations, "warmup": a.warmup, "chunk_rows": a.chunk_rows,
           "torch_chunk_rows": a.chunk, "depth1_clusters": int(uniq.numel()),
           "device": torch.cuda.get_device_name(dev), "flop_per_unrestricted_call": flop,
           "peak_fp32_mfma_tflops": PEAK_TF, "ours": {}, "silhouette": {}, "torch": {}, **peak_ws}
    for name in variants:
        st = dict(stats(res[name]), peak_bytes_above_resident=peak[name])
        if name.startswith("silhouette"):
            doc["silhouette"][name[len("silhouette_"):]] = st
        else:
            if not name.endswith("depth1"):
                st["tflops"] = flop / st["median_ms"] / 1e9
                st["fraction_of_peak"] = st["tflops"] / PEAK_TF
            doc["ours"][name] = dict(st, counters=counters[name])
    for metric, v in torch_res.items():
        doc["torch"][f"{metric}_f32"] = dict(stats(v), peak_bytes_above_resident=torch_peak[metric],
                                             lists_equal_share=agree[metric])
    doc["ratio_ours_over_silhouette"] = {f"{metric}_{f}": doc["ours"][f"{metric}_{f}"]["median_ms"] /
                                         doc["silhouette"][f]["median_ms"]
                                         for metric in ("l2", "cosine") for f in ("f32", "f16")}
    doc["ratio_torch_over_ours"] = {metric: doc["torch"][f"{metric}_f32"]["median_ms"] /
                                    doc["ours"][f"{metric}_f32"]["median_ms"] for metric in torch_res}
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(doc, indent=1) + "\n")
    print(json.dumps({"ours_median_ms": {n_: v["median_ms"] for n_, v in doc["ours"].items()},
                      "silhouette_median_ms": {n_: v["median_ms"] for n_, v in doc["silhouette"].items()},
                      "torch_median_ms": {n_: v["median_ms"] for n_, v in doc["torch"].items()},
                      "ratio_ours_over_silhouette": doc["ratio_ours_over_silhouette"],
                      "ratio_torch_over_ours": doc["ratio_torch_over_ours"],
                      "torch_lists_equal_share": agree}))


if __name__ == "__main__":
    main()
