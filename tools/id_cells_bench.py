#!/usr/bin/env python3
"""A/B of the ID cell index at the bench shape (10M rows, [128,128,256], the PROD codebooks and rows bench.py builds,
IDs from one encode, ranked by reconstruction error) and at the XL shape (65,536 groups x 512 fine IDs, 6.25M rows,
synthetic IDs: uniform groups, fine IDs skewed towards the low values, random keys), alternating inside ONE process:

  kernel        rqsid_bucket over the group key + rqsid_id_cells (outputs allocated inside the timed call)
  composition   what torch offers: the key-bit mapping, a stable sort of (cell key << 32 | key bits),
                unique_consecutive, then rank / size / cell arithmetic and the scatters back to row order

Both arms start from the same device tensors (group key i32, fine ID i32, rank key f32).  Times are device events
around each call (median, min, max over every timed repetition of every alternation, after warm-up).  The integer
outputs of both arms (order, rank, size, cell, the cells' keys and offsets) are asserted equal on all rows.

Writes one JSON document (default profiles/id_cells_ab.json); DESIGN.md quotes it.  Gate (PROD shape): the kernel arm
takes at most half the composition's median.  The XL figures are recorded without a gate.
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


def kernel_arm(group, n_groups, fine, n_fine, key, ws):
    n, dev = group.numel(), group.device
    b = ops.bucket(group, n_groups)
    cap = min(n, n_groups * n_fine)
    o = {k: torch.empty(m, dtype=torch.int32, device=dev) for k, m in (
        ("order", n), ("rank", n), ("size", n), ("cell", n), ("cell_off", cap + 1), ("cell_group", cap),
        ("cell_fine", cap))}
    rc = ops.lib().rqsid_id_cells(n, ops._ptr(b.row_index), n_groups, ops._ptr(b.seg_row_off), None, ops._ptr(fine),
                                  n_fine, ops._ptr(key), ops._ptr(o["order"]), ops._ptr(o["rank"]), ops._ptr(o["size"]),
                                  ops._ptr(o["cell"]), ops._ptr(o["cell_off"]), ops._ptr(o["cell_group"]),
                                  ops._ptr(o["cell_fine"]), ops._ptr(ws.buf), ws.bytes, ops._stream())
    assert rc == 0, ops.lib().rqsid_last_error().decode()
    o["bucket"] = b
    return o


def composition_arm(group, n_groups, fine, n_fine, key):
    n, dev = group.numel(), group.device
    u = key.view(torch.int32).long() & 0xFFFFFFFF
    u = torch.where(u == 0x80000000, torch.zeros_like(u), u)
    kb = torch.where((u & 0x80000000) != 0, ~u & 0xFFFFFFFF, u | 0x80000000)
    kb = torch.where(torch.isnan(key), torch.full_like(kb, 0xFFFFFFFF), kb)
    packed = ((group.long() * n_fine + fine.long()) << 32) | kb
    srt, perm = torch.sort(packed, stable=True)  # equal (cell, key): by row number
    keys, inverse, counts = torch.unique_consecutive(srt >> 32, return_inverse=True, return_counts=True)
    start = torch.cumsum(counts, 0) - counts
    pos = torch.arange(n, device=dev)
    rank = torch.empty(n, dtype=torch.int32, device=dev)
    size = torch.empty(n, dtype=torch.int32, device=dev)
    cell = torch.empty(n, dtype=torch.int32, device=dev)
    rank[perm] = (pos - start[inverse]).to(torch.int32)
    size[perm] = counts[inverse].to(torch.int32)
    cell[perm] = inverse.to(torch.int32)
    return {"order": perm.to(torch.int32), "rank": rank, "size": size, "cell": cell, "keys": keys,
            "cell_off": start.to(torch.int32)}


def run_shape(name, group, n_groups, fine, n_fine, key, a):
    n, dev = group.numel(), group.device
    ws = ops.IdCellsWorkspace(n, n_groups, n_fine, dev)
    arms = [("kernel", lambda: kernel_arm(group, n_groups, fine, n_fine, key, ws)),
            ("composition", lambda: composition_arm(group, n_groups, fine, n_fine, key))]
    outs = {}
    for arm, fn in arms:
        for _ in range(a.warmup):
            outs[arm] = fn()
        torch.cuda.synchronize()
    k, c = outs["kernel"], outs["composition"]
    ctr = ws.counters().tolist()
    n_cells = ctr[0]
    assert int(ws.error_word().item()) == 0 and int(k["bucket"].error_word().item()) == 0
    assert n_cells == c["keys"].numel()
    for f in ("order", "rank", "size", "cell"):
        assert torch.equal(k[f], c[f]), f
    assert torch.equal(k["cell_group"][:n_cells].long() * n_fine + k["cell_fine"][:n_cells].long(), c["keys"])
    assert torch.equal(k["cell_off"][:n_cells], c["cell_off"]) and int(k["cell_off"][n_cells].item()) == n
    del outs, k, c
    times = {arm: [] for arm, _ in arms}
    for _ in range(a.alternations):
        for arm, fn in arms:
            for _ in range(a.reps):
                times[arm].append(timed(fn)[1])
    doc = {"rows": n, "groups": n_groups, "n_fine": n_fine, "cells": n_cells, "cells_of_two_or_more": ctr[1],
           "rows_in_them": ctr[2], "cells_of_one": ctr[3], "largest_cell": ctr[4],
           "outputs_equal_on_all_rows": True, "arms": {arm: stats(times[arm]) for arm, _ in arms}}
    km, cm = doc["arms"]["kernel"]["median_ms"], doc["arms"]["composition"]["median_ms"]
    doc["kernel_over_composition"] = km / cm
    print(json.dumps({name: {"kernel_ms": km, "composition_ms": cm, "ratio": km / cm, "cells": n_cells}}), flush=True)
    return doc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--xl-rows", type=int, default=6_250_000)
    ap.add_argument("--alternations", type=int, default=4)
    ap.add_argument("--reps", type=int, default=3, help="timed calls per arm per alternation")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--codebooks", choices=("fitted", "sampled"), default="fitted")
    ap.add_argument("--out", default=str(REPO / "profiles" / "id_cells_ab.json"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    cb = bench.codebooks(a.codebooks, dev)
    enc = RQEncoder([torch.from_numpy(cb[k]) for k in ("c0", "c1", "c2")], list(bench.NEED),
                    match=torch.from_numpy(cb["match"]), semantics=HIERARCHICAL_TRAIN, device=dev)
    x = bench.make_rows(a.rows, 0, dev)
    qe = enc.quant_error(x)
    del x
    sizes = enc.id_sizes()
    ids = qe.ids
    group = (ids[:, 0] * sizes[1] + ids[:, 1]).contiguous()
    fine, key = ids[:, 2].contiguous(), qe.recon_err.contiguous()
    del qe
    doc = {"what": "tools/id_cells_bench.py: rqsid_bucket + rqsid_id_cells against a stable torch sort of (cell key, "
                   "key bits) with unique_consecutive and rank arithmetic, alternating in one process (measured)",
           "need": list(bench.NEED), "codebooks": a.codebooks, "alternations": a.alternations, "reps": a.reps,
           "device": torch.cuda.get_device_name(dev), "lds_rows": ops.id_cells_lds_rows()}
    doc["prod"] = run_shape("prod", group, sizes[0] * sizes[1], fine, sizes[2], key, a)
    del group, fine, key, ids
    gen = torch.Generator(device=dev)
    gen.manual_seed(1234)
    n = a.xl_rows
    group = torch.randint(0, 65536, (n,), generator=gen, device=dev, dtype=torch.int32)
    fine = (torch.rand(n, generator=gen, device=dev).pow(2) * 512).to(torch.int32).clamp_(0, 511)
    key = torch.rand(n, generator=gen, device=dev)
    doc["xl"] = run_shape("xl", group, 65536, fine, 512, key, a)
    km, cm = (doc["prod"]["arms"][k]["median_ms"] for k in ("kernel", "composition"))
    doc["gate"] = {"kernel_median_ms": km, "composition_median_ms": cm, "kernel_over_composition": km / cm,
                   "passed": km <= 0.5 * cm}
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(doc, indent=1) + "\n")
    print(json.dumps({"gate": doc["gate"]}))


if __name__ == "__main__":
    main()
