#!/usr/bin/env python3
"""A/B of the row formats of the fused 3-level encode at the bench shape (10M x 512, [128,128,256], the PROD
codebooks bench.py builds), fp32 and 16-bit rows alternating inside ONE process:

  f32_default   fp32 rows, default dispatch (what bench.py times)
  f32_per_tile  fp32 rows forced to the per-tile screen (RQSID_SCREEN_VARIANT=1): the form 16-bit rows take
  f16 / bf16    16-bit rows (rqsid_assign_x)

Per variant: per-level and per-step times from device events (median, min, max over every timed repetition of
every alternation, after warm-up), the rows each level re-scores, and a check that all four return identical
IDs.  The rows are the bench's mixture rounded to bfloat16 with elements below 2^-14 set to 0, so the same
real values are exact in fp32, fp16 and bf16 and the four variants must agree bit for bit.

Writes one JSON document (default profiles/rows16_ab.json); DESIGN.md quotes it.  The gate it evaluates: fp16
level 0 no slower than fp32 level 0 beyond the fp32 figure's own run-to-run spread in this process.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
from pathlib import Path

import torch

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))

import bench  # noqa: E402  (codebooks and rows exactly as the benchmark builds them)
import generative_ranking_recommender_amd.encode as encmod  # noqa: E402
from generative_ranking_recommender_amd import ops  # noqa: E402
from generative_ranking_recommender_amd.encode import HIERARCHICAL_TRAIN, RQEncoder  # noqa: E402

VARIANTS = [("f32_default", torch.float32, {}), ("f32_per_tile", torch.float32, {"RQSID_SCREEN_VARIANT": "1"}),
            ("f16", torch.float16, {}), ("bf16", torch.bfloat16, {})]
# level-0 bytes per row: the 512-d row + the int32 id (centre tables stay in L2)
L0_BYTE_RATIO = (512 * 2 + 4) / (512 * 4 + 4)


def common_rows(n, dev):
    """bench rows rounded so that fp32, fp16 and bf16 hold the same values (in place, 1M rows at a time)"""
    x = bench.make_rows(n, 0, dev)
    for i in range(0, n, 1 << 20):
        blk = x[i:i + (1 << 20)]
        q = blk.to(torch.bfloat16).float()
        q[q.abs() < 2.0 ** -14] = 0.0
        blk.copy_(q)
    assert bool(torch.isfinite(x).all()) and float(x.abs().max()) < 65504.0
    return x


class EnvSet:
    def __init__(self, env):
        self.env, self.old = env, {}

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.env}
        os.environ.update(self.env)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def timed_encode(enc, x):
    """One encode with device events around the step and around each level's rqsid_assign call."""
    marks, orig = [], ops.assign

    def hook(*a, **k):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        out = orig(*a, **k)
        e.record()
        marks.append((s, e))
        return out

    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    encmod.ops.assign = hook
    try:
        s.record()
        out = enc.encode(x, check=False)
        e.record()
    finally:
        encmod.ops.assign = orig
    torch.cuda.synchronize()
    return out, s.elapsed_time(e), [a.elapsed_time(b) for a, b in marks]


def stats(v):
    return {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "n": len(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--alternations", type=int, default=4)
    ap.add_argument("--reps", type=int, default=3, help="timed encodes per variant per alternation")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--codebooks", choices=("fitted", "sampled"), default="fitted")
    ap.add_argument("--out", default=str(REPO / "profiles" / "rows16_ab.json"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    cb = bench.codebooks(a.codebooks, dev)
    enc = RQEncoder([torch.from_numpy(cb[k]) for k in ("c0", "c1", "c2")], list(bench.NEED),
                    match=torch.from_numpy(cb["match"]), semantics=HIERARCHICAL_TRAIN, device=dev)
    assert enc.fused
    x32 = common_rows(a.rows, dev)
    xs = {torch.float32: x32, torch.float16: x32.to(torch.float16), torch.bfloat16: x32.to(torch.bfloat16)}
    for t in (torch.float16, torch.bfloat16):  # the same values in every format
        for i in range(0, a.rows, 1 << 20):
            assert torch.equal(xs[t][i:i + (1 << 20)].float(), x32[i:i + (1 << 20)])
    torch.cuda.synchronize()

    res = {name: {"step": [], "levels": [[], [], []]} for name, _, _ in VARIANTS}
    ids, rescored, fmt = {}, {}, {}
    for name, dt, env in VARIANTS:  # warm-up, the re-score counts and the IDs, outside the timed alternations
        with EnvSet(env):
            for _ in range(a.warmup):
                enc.encode(xs[dt], check=False)
            ids[name] = enc.encode(xs[dt], count_rescored=True).clone()
            rescored[name] = list(enc.last_rescored)
            fmt[name] = enc.last_row_format
    first = VARIANTS[0][0]
    same = {name: bool(torch.equal(ids[name], ids[first])) for name in ids}
    assert all(same.values()), f"IDs differ between the variants: {same}"
    for _ in range(a.alternations):
        for name, dt, env in VARIANTS:
            with EnvSet(env):
                for _ in range(a.reps):
                    out, step, lv = timed_encode(enc, xs[dt])
                    assert len(lv) == 3
                    res[name]["step"].append(step)
                    for l in range(3):
                        res[name]["levels"][l].append(lv[l])
        assert torch.equal(out, ids[first])
    enc.check_errors()

    doc = {"what": "tools/rows16_bench.py: row formats of the fused encode, alternating in one process (measured)",
           "rows": a.rows, "dim": bench.D, "need": list(bench.NEED), "codebooks": a.codebooks,
           "alternations": a.alternations, "reps": a.reps, "device": torch.cuda.get_device_name(dev),
           "ids_identical": same, "l0_byte_ratio_expected": L0_BYTE_RATIO, "variants": {}}
    for name, _, env in VARIANTS:
        doc["variants"][name] = {"row_format": fmt[name], "env": env, "rescored_rows": rescored[name],
                                 "step": stats(res[name]["step"]),
                                 "levels": [stats(v) for v in res[name]["levels"]]}
    f32, f16 = doc["variants"]["f32_default"]["levels"][0], doc["variants"]["f16"]["levels"][0]
    spread = f32["max_ms"] - f32["min_ms"]
    doc["gate_l0"] = {"f32_median_ms": f32["median_ms"], "f32_spread_ms": spread, "f16_median_ms": f16["median_ms"],
                      "f16_over_f32": f16["median_ms"] / f32["median_ms"],
                      "passed": f16["median_ms"] <= f32["median_ms"] + spread}
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(doc, indent=1) + "\n")
    print(json.dumps({"gate_l0": doc["gate_l0"],
                      "step_median_ms": {k: v["step"]["median_ms"] for k, v in doc["variants"].items()},
                      "level_median_ms": {k: [l["median_ms"] for l in v["levels"]] for k, v in doc["variants"].items()},
                      "rescored_rows": rescored}))


if __name__ == "__main__":
    main()
