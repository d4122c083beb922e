#!/usr/bin/env python3
"""rqsid_assign_topk at the bench shape (10M x 512, need [128,128,256], the PROD codebooks bench.py builds) against
the only composition available without it, torch.cdist in row chunks + torch.topk, in ONE process:

  ours   RQEncoder.encode_topk: per level the rqsid_assign_topk call alone (device events around it), on the
         encoder's own segments, for k = 2 and k = 8 and fp32 and fp16 rows, the variants alternating;
         nearest_topk against one unconstrained 1280-centre table (the arithmetic of a level-2 segment);
  torch  cdist + topk over the same rows in chunks (the N x K distance matrix of a chunk is materialised), at
         level 0 (K = 128) and against the same 1280-centre table.  It has no segmented form, so levels 1 and 2
         have no torch counterpart; its fp32 mm-expansion is also not exact (the agreement of its first place with
         ours is recorded, not asserted).

The fp16 rows are the fp32 rows rounded to fp16 (other values: ``ids_identical_across_variants``, which compares
every variant with the first, is expected to hold between k = 2 and k = 8 of one format only).

Per measurement: median / min / max over every timed repetition after warm-up.  Per level the three workspace
counters (rows ranked from their list, rows that took the all-candidate pass, non-finite rows) and the bytes the
call has to move (rows once + the three outputs; centre tables stay in cache).  Writes one JSON document (default
profiles/topk_ab.json); DESIGN.md 3.1g quotes it.
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
import generative_ranking_recommender_amd.encode as encmod  # noqa: E402
from generative_ranking_recommender_amd import ops  # noqa: E402
from generative_ranking_recommender_amd.encode import HIERARCHICAL_TRAIN, RQEncoder  # noqa: E402

VARIANTS = [("f32_k2", torch.float32, 2), ("f32_k8", torch.float32, 8), ("f16_k2", torch.float16, 2),
            ("f16_k8", torch.float16, 8)]
TABLE = 1280


def log(msg):
    print(f"[topk_bench] {msg}", file=sys.stderr, flush=True)


def stats(v):
    return {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "n": len(v)}


def event_pair():
    return torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)


def timed_encode_topk(enc, x, k, counters=None):
    """One encode_topk with device events around each level's rqsid_assign_topk call (``counters``: a list that
    receives each level's workspace counters; reading them synchronises, so not in a timed repetition)."""
    marks, orig = [], ops.assign_topk

    def hook(*a, **kw):
        s, e = event_pair()
        s.record()
        out = orig(*a, **kw)
        e.record()
        marks.append((s, e))
        if counters is not None:
            counters.append(kw["workspace"].counters())
        return out

    encmod.ops.assign_topk = hook
    try:
        out = enc.encode_topk(x, k, check=False)
    finally:
        encmod.ops.assign_topk = orig
    torch.cuda.synchronize()
    return out, [a.elapsed_time(b) for a, b in marks]


def timed(fn):
    s, e = event_pair()
    s.record()
    out = fn()
    e.record()
    torch.cuda.synchronize()
    return out, s.elapsed_time(e)


def torch_topk(x, c, k, chunk):
    """The composition: per row chunk the full distance matrix, then its k smallest per row."""
    idx = torch.empty((x.shape[0], k), dtype=torch.int64, device=x.device)
    dist = torch.empty((x.shape[0], k), dtype=torch.float32, device=x.device)
    for i in range(0, x.shape[0], chunk):
        d = torch.cdist(x[i:i + chunk], c)
        v, j = torch.topk(d, k, dim=1, largest=False)
        idx[i:i + chunk], dist[i:i + chunk] = j, v
    return idx, dist


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--alternations", type=int, default=3)
    ap.add_argument("--reps", type=int, default=2, help="timed repetitions per variant per alternation")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--chunk", type=int, default=1 << 18, help="rows per torch.cdist chunk")
    ap.add_argument("--codebooks", choices=("fitted", "sampled"), default="fitted")
    ap.add_argument("--out", default=str(REPO / "profiles" / "topk_ab.json"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    cb = bench.codebooks(a.codebooks, dev)
    enc = RQEncoder([torch.from_numpy(cb[k]) for k in ("c0", "c1", "c2")], list(bench.NEED),
                    match=torch.from_numpy(cb["match"]), semantics=HIERARCHICAL_TRAIN, device=dev)
    assert enc.fused
    x32 = bench.make_rows(a.rows, 0, dev)
    xs = {torch.float32: x32, torch.float16: x32.to(torch.float16)}
    n, d = x32.shape
    table = torch.from_numpy(cb["c2"][:TABLE]).to(dev).contiguous()
    pc_table = ops.prepare_centers(table)
    c0 = enc.pcs[0].centers
    torch.cuda.synchronize()
    log(f"codebooks and {n} rows ready")

    res = {name: [[], [], []] for name, _, _ in VARIANTS}
    counters, ids = {}, {}
    for name, dt, k in VARIANTS:  # warm-up, the counters and the IDs, outside the timed alternations
        for _ in range(a.warmup):
            enc.encode_topk(xs[dt], k, check=False)
        cnt = []
        out, _ = timed_encode_topk(enc, xs[dt], k, cnt)
        counters[name] = cnt
        ids[name] = out.ids.clone()
        del out
        log(f"{name}: counters {cnt}")
    enc.check_errors()
    table_ms = {2: [], 8: []}
    torch_ms = {"level0": {2: [], 8: []}, "table1280": {2: [], 8: []}}
    agree = {}
    for k in (2, 8):  # warm-up of the one-table forms; first-place agreement of the two methods
        ours = ops.nearest_topk(x32, pc_table, k)[1]
        theirs = torch_topk(x32, table, k, a.chunk)[0]
        agree[f"table1280_k{k}_first_place"] = float((ours[:, 0].long() == theirs[:, 0]).double().mean().item())
        agree[f"table1280_k{k}_all_places"] = float((ours.long() == theirs).all(1).double().mean().item())
        del ours, theirs
        torch_topk(x32, c0, k, a.chunk)
    log(f"torch agreement {agree}")
    for alt in range(a.alternations):
        log(f"alternation {alt}")
        for name, dt, k in VARIANTS:
            for _ in range(a.reps):
                out, lv = timed_encode_topk(enc, xs[dt], k)
                assert len(lv) == 3
                for l in range(3):
                    res[name][l].append(lv[l])
                del out
        for k in (2, 8):
            for _ in range(a.reps):
                table_ms[k].append(timed(lambda: ops.nearest_topk(x32, pc_table, k, check=False))[1])
                torch_ms["level0"][k].append(timed(lambda: torch_topk(x32, c0, k, a.chunk))[1])
                torch_ms["table1280"][k].append(timed(lambda: torch_topk(x32, table, k, a.chunk))[1])

    doc = {"what": "tools/topk_bench.py: rqsid_assign_topk against torch.cdist + torch.topk, one process (measured)",
           "rows": n, "dim": d, "need": list(bench.NEED), "codebooks": a.codebooks, "alternations": a.alternations,
           "reps": a.reps, "torch_chunk_rows": a.chunk, "device": torch.cuda.get_device_name(dev),
           "ids_identical_across_variants": {name: bool(torch.equal(ids[name], ids[VARIANTS[0][0]])) for name in ids},
           "torch_agreement": agree, "ours": {}, "torch": {}}
    for name, dt, k in VARIANTS:
        es = torch.empty((), dtype=dt).element_size()
        byts = n * d * es + n * k * 12
        levels = []
        for l in range(3):
            st = stats(res[name][l])
            c = counters[name][l]
            levels.append(dict(st, counters=c, all_candidate_share=c["all_candidate_rows"] / n, bytes_moved=byts,
                               gbytes_per_s=byts / st["median_ms"] / 1e6))
        doc["ours"][name] = {"k": k, "row_dtype": str(dt).replace("torch.", ""), "levels": levels}
    for k in (2, 8):
        doc["ours"][f"table1280_f32_k{k}"] = stats(table_ms[k])
        doc["torch"][f"level0_f32_k{k}"] = stats(torch_ms["level0"][k])
        doc["torch"][f"table1280_f32_k{k}"] = stats(torch_ms["table1280"][k])
    doc["ratio_torch_over_ours"] = {
        f"level0_k{k}": doc["torch"][f"level0_f32_k{k}"]["median_ms"] / doc["ours"][f"f32_k{k}"]["levels"][0]["median_ms"]
        for k in (2, 8)}
    doc["ratio_torch_over_ours"].update({
        f"table1280_k{k}": doc["torch"][f"table1280_f32_k{k}"]["median_ms"] /
        doc["ours"][f"table1280_f32_k{k}"]["median_ms"] for k in (2, 8)})
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(doc, indent=1) + "\n")
    print(json.dumps({"ours_level_median_ms": {k: [l["median_ms"] for l in v["levels"]] for k, v in doc["ours"].items()
                                               if "levels" in v},
                      "ours_table1280_ms": {k: doc["ours"][f"table1280_f32_k{k}"]["median_ms"] for k in (2, 8)},
                      "torch_ms": {k: v["median_ms"] for k, v in doc["torch"].items()},
                      "ratio_torch_over_ours": doc["ratio_torch_over_ours"],
                      "all_candidate_share": {k: [l["all_candidate_share"] for l in v["levels"]]
                                              for k, v in doc["ours"].items() if "levels" in v}}))


if __name__ == "__main__":
    main()
