#!/usr/bin/env python3
"""A/B of the quantisation-error pass at the bench shape (10M x 512, [128,128,256], the PROD codebooks bench.py
builds), alternating inside ONE process:

  kernel_f32 / kernel_f16   rqsid_quant_error (one streaming pass), rows processed in the order of the last level's
                            bucketing, as RQEncoder.quant_error calls it
  kernel_f32_unordered      the same without a row order (every row re-reads its c0 / c1 rows from L2)
  composition               what the library offered before the kernel: per level
                            torch.linalg.vector_norm(cur - c[g], dim=1) on the gathered centre rows, and
                            ops.residual for the next level's input (two fp32 residual matrices written and re-read)

Times are device events around each call (median, min, max over every timed repetition of every alternation, after
warm-up).  The kernel's share of the HBM peak bench.py uses is taken on the bytes the pass needs:
N * (row bytes + 4 L ids + 4 (L + 1) outputs).  The IDs come from one encode; the kernel's errors are compared
with the composition's (fp32 norms there, so they agree to fp32 rounding only).

Writes one JSON document (default profiles/quant_error_ab.json); DESIGN.md quotes it.  Gate: the ordered fp32 kernel
takes at most half the composition's time.
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
from generative_ranking_recommender_amd import ops  # noqa: E402
from generative_ranking_recommender_amd.encode import HIERARCHICAL_TRAIN, RQEncoder  # noqa: E402


def timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    out = fn()
    e.record()
    torch.cuda.synchronize()
    return out, s.elapsed_time(e)


def stats(v):
    return {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "n": len(v)}


def composition(x, cents, globs, normalize):
    cur, errs = x, []
    for l, (c, g) in enumerate(zip(cents, globs)):
        errs.append(torch.linalg.vector_norm(cur - c[g.long()], dim=1))
        if l < len(cents) - 1:
            cur = ops.residual(cur, c, g, normalize=normalize)
    return torch.stack(errs, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--alternations", type=int, default=4)
    ap.add_argument("--reps", type=int, default=3, help="timed calls per variant per alternation")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--codebooks", choices=("fitted", "sampled"), default="fitted")
    ap.add_argument("--out", default=str(REPO / "profiles" / "quant_error_ab.json"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    cb = bench.codebooks(a.codebooks, dev)
    enc = RQEncoder([torch.from_numpy(cb[k]) for k in ("c0", "c1", "c2")], list(bench.NEED),
                    match=torch.from_numpy(cb["match"]), semantics=HIERARCHICAL_TRAIN, device=dev)
    n, L = a.rows, 3
    x32 = bench.make_rows(n, 0, dev)
    ids = enc.encode(x32)
    globs = enc.global_rows(ids)
    cents = [pc.centers for pc in enc.pcs]
    grp = ids[:, 0] * bench.NEED[0] + ids[:, 1]
    order = ops.bucket(grp, bench.NEED[0] * bench.NEED[1]).row_index
    x16 = x32.to(torch.float16)
    ws = ops.QuantErrorWorkspace(n, dev)

    def kernel(x, ro):
        return lambda: ops.quant_error(x, cents, globs, True, row_order=ro, workspace=ws, check=False)

    variants = [("kernel_f32", kernel(x32, order), 4), ("kernel_f16", kernel(x16, order), 2),
                ("kernel_f32_unordered", kernel(x32, None), 4),
                ("composition", lambda: composition(x32, cents, globs, True), 4)]
    outs = {}
    for name, fn, _ in variants:
        for _ in range(a.warmup):
            outs[name] = fn()
        torch.cuda.synchronize()
    times = {name: [] for name, _, _ in variants}
    for _ in range(a.alternations):
        for name, fn, _ in variants:
            for _ in range(a.reps):
                times[name].append(timed(fn)[1])
    assert int(ws.error_word().item()) == 0
    err_k, err_c = outs["kernel_f32"][0], outs["composition"]
    rel = ((err_k - err_c).abs() / err_c.abs().clamp(min=1e-30)).max(0).values.cpu().tolist()
    same_order = bool(torch.equal(outs["kernel_f32"][0], outs["kernel_f32_unordered"][0]))
    # what the pass says about these codebooks: per level the mean squared distance in the level's own space and
    # the share of the rows' energy the chain leaves unexplained when it stops there
    qe = enc.quant_error(x32, ids=ids)
    sums = qe.sums.cpu().tolist()
    quality = {"mse": [s / n for s in sums[:L]],
               "relative": (qe.recon_levels.double().pow(2).sum(0) / sums[L]).cpu().tolist()}

    doc = {"what": "tools/quant_error_bench.py: rqsid_quant_error against the composition of ops.residual and "
                   "torch norms, alternating in one process (measured)",
           "rows": n, "dim": bench.D, "need": list(bench.NEED), "levels": L, "codebooks": a.codebooks,
           "alternations": a.alternations, "reps": a.reps, "device": torch.cuda.get_device_name(dev),
           "hbm_peak_GBs": bench.HBM_PEAK_GBS, "max_rel_diff_kernel_vs_composition_per_level": rel,
           "err_identical_with_and_without_row_order": same_order, "codebook_quality": quality, "variants": {}}
    for name, _, elem in variants:
        st = stats(times[name])
        if name.startswith("kernel"):
            nbytes = n * (bench.D * elem + 4 * L + 4 * (L + 1))
            gbs = nbytes / (st["median_ms"] * 1e-3) / 1e9
            st.update({"bytes_basis": nbytes, "GB/s": gbs, "hbm_frac": gbs / bench.HBM_PEAK_GBS})
        doc["variants"][name] = st
    k, c = doc["variants"]["kernel_f32"]["median_ms"], doc["variants"]["composition"]["median_ms"]
    doc["gate"] = {"kernel_f32_median_ms": k, "composition_median_ms": c, "kernel_over_composition": k / c,
                   "passed": k <= 0.5 * c}
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(doc, indent=1) + "\n")
    print(json.dumps({"gate": doc["gate"], "median_ms": {k: v["median_ms"] for k, v in doc["variants"].items()},
                      "hbm_frac": {k: v.get("hbm_frac") for k, v in doc["variants"].items()},
                      "max_rel_diff": rel, "codebook_quality": quality}))


if __name__ == "__main__":
    main()
