#!/usr/bin/env python3
"""rqsid_silhouette at the bench shape (10M x 512 rows, the PROD codebooks bench.py fits, 50,000 scored rows) against
the only composition available without it, in ONE process:

  ours   the rqsid_silhouette call alone (device events around it; grouping, gathers and the workspace are outside),
         for the ID prefixes of depth 1, 2 and 3 and fp32 and fp16 rows, the variants alternating;
  torch  torch.cdist of the scored rows against chunks of the rows in the sorted order (the chunk x sample distance
         matrix is materialised; chunks end on cluster boundaries), the self entries zeroed by index, a segmented sum
         (torch.segment_reduce, or index_add_ where that is unavailable: recorded), means, a running min.  fp32 rows
         only; the gather of the rows into the sorted order is outside the timed region.  Its fp32 mm-expansion is
         not the kernel's arithmetic: the mean silhouettes of the two are recorded side by side, not asserted.

Per measurement: median / min / max over every timed repetition after warm-up.  Achieved TFLOP/s counts
2 x sample x rows x dim against the 155-TF fp32-MFMA figure of the microarchitecture guide.  Writes one JSON document
(default profiles/silhouette_ab.json); DESIGN.md 3.3b quotes it.
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
    print(f"[silhouette_bench] {msg}", file=sys.stderr, flush=True)


def stats(v):
    return {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "n": len(v)}


def timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    out = fn()
    e.record()
    torch.cuda.synchronize()
    return out, s.elapsed_time(e)


def mean_finite(s):
    fin = torch.isfinite(s)
    return float(s[fin].double().mean().item()) if bool(fin.any()) else None


def torch_silhouette(xs, off, q, pos_self, qseg, chunk, how):
    """The composition.  xs: the rows in the sorted order; off: int64 [K + 1] on the host side as a tensor; pos_self:
    each query's position in the sorted order; qseg: its cluster.  Returns s [m]."""
    m, dev = q.shape[0], q.device
    n, k = xs.shape[0], off.numel() - 1
    cnt = (off[1:] - off[:-1])
    a_sum = torch.zeros(m, dtype=torch.float32, device=dev)
    best = torch.full((m,), float("inf"), dtype=torch.float32, device=dev)
    qi = torch.arange(m, device=dev)
    c0 = 0
    while c0 < k:
        # clusters c0 .. c1-1: as many whole clusters as fit in `chunk` rows (one at least)
        c1 = int(torch.searchsorted(off, off[c0] + chunk, right=True).item()) - 1
        c1 = min(max(c1, c0 + 1), k)
        p0, p1 = int(off[c0].item()), int(off[c1].item())
        if p1 > p0:
            d = torch.cdist(xs[p0:p1], q)  # [rows of the chunk, m]
            mine = (pos_self >= p0) & (pos_self < p1)
            d[pos_self[mine] - p0, qi[mine]] = 0.0
            lens = cnt[c0:c1]
            if how == "segment_reduce":
                sums = torch.segment_reduce(d, "sum", lengths=lens, axis=0)
            else:
                seg = torch.repeat_interleave(torch.arange(c1 - c0, device=dev), lens)
                sums = torch.zeros((c1 - c0, m), dtype=torch.float32, device=dev).index_add_(0, seg, d)
            del d
            means = sums / lens.clamp(min=1)[:, None].float()
            means[lens == 0] = float("inf")
            own = (qseg >= c0) & (qseg < c1)
            a_sum[own] = sums[qseg[own] - c0, qi[own]]
            means[qseg[own] - c0, qi[own]] = float("inf")
            best = torch.minimum(best, means.amin(0))
            del sums, means
        c0 = c1
    n_o = cnt[qseg].float()
    a = torch.where(n_o > 1, a_sum / (n_o - 1).clamp(min=1), torch.zeros_like(a_sum))
    s = (best - a) / torch.maximum(a, best)
    return torch.where(n_o > 1, s, torch.zeros_like(s))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--sample", type=int, default=50_000)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--alternations", type=int, default=3)
    ap.add_argument("--reps", type=int, default=1, help="timed repetitions per variant per alternation")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--chunk", type=int, default=1 << 16, help="rows per torch.cdist chunk")
    ap.add_argument("--chunk-rows", type=int, default=0, help="rqsid_silhouette's chunk_rows (0 = automatic)")
    ap.add_argument("--codebooks", choices=("fitted", "sampled"), default="fitted")
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--out", default=str(REPO / "profiles" / "silhouette_ab.json"))
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
    m = rows.numel()
    xs = {"f32": x32, "f16": x32.to(torch.float16)}
    qs = {k: v[rows].contiguous() for k, v in xs.items()}
    qself = rows.to(torch.int32)
    torch.cuda.synchronize()
    log(f"codebooks, {n} rows, their IDs and {m} scored rows ready")

    groups = {}
    for p in (1, 2, 3):
        uniq, inv = torch.unique(CR.prefix_keys(ids, radices, p), return_inverse=True)
        order, off, _, _ = CR._group(inv, int(uniq.numel()), ops.centroid_tile_rows())
        groups[p] = dict(k=int(uniq.numel()), order=order, off=off, qseg=inv[rows].to(torch.int32).contiguous(), inv=inv)
        log(f"depth {p}: {groups[p]['k']} clusters")
    ws = ops.SilhouetteWorkspace(n, m, dev, a.chunk_rows)
    variants = [(p, f) for p in (1, 2, 3) for f in ("f32", "f16")]

    def ours(p, f):
        g = groups[p]
        return ops.silhouette(xs[f], g["order"], g["off"], qs[f], qself, g["qseg"], chunk_rows=a.chunk_rows,
                              workspace=ws, check=False)

    res = {v: [] for v in variants}
    mean_s = {}
    for p, f in variants:
        for _ in range(a.warmup):
            out = ours(p, f)
        mean_s[(p, f)] = mean_finite(out[3])
        log(f"depth {p} {f}: mean silhouette {mean_s[(p, f)]}")
    ops.check_error_words([ws.error_word()], "rqsid_silhouette", ops.SILHOUETTE_WORD)

    torch_res, torch_mean, how = {}, {}, None
    if not a.no_torch:
        for p in (1, 2, 3):
            g = groups[p]
            srt = x32[g["order"].long()]
            pos = torch.empty(n, dtype=torch.int64, device=dev)
            pos[g["order"].long()] = torch.arange(n, device=dev)
            args = (srt, g["off"].long(), qs["f32"], pos[rows], g["qseg"].long(), a.chunk)
            if how is None:
                try:
                    torch_silhouette(*args, "segment_reduce")
                    how = "segment_reduce"
                except (RuntimeError, NotImplementedError) as exc:
                    log(f"torch.segment_reduce unavailable here ({str(exc)[:80]}): index_add_")
                    how = "index_add_"
            for _ in range(a.warmup):
                s = torch_silhouette(*args, how)
            torch_mean[p] = mean_finite(s)
            torch_res[p] = [timed(lambda: torch_silhouette(*args, how))[1] for _ in range(a.alternations * a.reps)]
            log(f"torch depth {p}: {torch_res[p]} ms, mean silhouette {torch_mean[p]}")
            del srt, pos, args, s

    for alt in range(a.alternations):
        log(f"alternation {alt}")
        for p, f in variants:
            for _ in range(a.reps):
                res[(p, f)].append(timed(lambda: ours(p, f))[1])
    ops.check_error_words([ws.error_word()], "rqsid_silhouette", ops.SILHOUETTE_WORD)

    flop = 2.0 * m * n * d
    doc = {"what": "tools/silhouette_bench.py: rqsid_silhouette against torch.cdist + a segmented sum, one process "
                   "(measured)",
           "rows": n, "dim": d, "sample": m, "seed": a.seed, "need": list(bench.NEED), "codebooks": a.codebooks,
           "alternations": a.alternations, "reps": a.reps, "warmup": a.warmup, "chunk_rows": a.chunk_rows,
           "torch_chunk_rows": a.chunk, "torch_segmented_sum": how, "device": torch.cuda.get_device_name(dev),
           "flop_per_call": flop, "peak_fp32_mfma_tflops": PEAK_TF, "ours": {}, "torch": {}}
    for p, f in variants:
        st = stats(res[(p, f)])
        tf = flop / st["median_ms"] / 1e9
        doc["ours"][f"depth{p}_{f}"] = dict(st, clusters=groups[p]["k"], tflops=tf, fraction_of_peak=tf / PEAK_TF,
                                            mean_silhouette=mean_s[(p, f)])
    for p, v in torch_res.items():
        doc["torch"][f"depth{p}_f32"] = dict(stats(v), mean_silhouette=torch_mean[p])
    doc["ratio_torch_over_ours"] = {f"depth{p}": doc["torch"][f"depth{p}_f32"]["median_ms"] /
                                    doc["ours"][f"depth{p}_f32"]["median_ms"] for p in torch_res}
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(doc, indent=1) + "\n")
    print(json.dumps({"ours_median_ms": {k: v["median_ms"] for k, v in doc["ours"].items()},
                      "ours_fraction_of_peak": {k: v["fraction_of_peak"] for k, v in doc["ours"].items()},
                      "torch_median_ms": {k: v["median_ms"] for k, v in doc["torch"].items()},
                      "ratio_torch_over_ours": doc["ratio_torch_over_ours"]}))


if __name__ == "__main__":
    main()
