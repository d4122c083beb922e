#!/usr/bin/env python3
"""The beam-search encode at the bench shape (10M x 512, need [128,128,256], the PROD codebooks bench.py builds), in
ONE process, for beam widths 1, 2, 4 and 8:

  beam         RQEncoder.encode_beam with device events around every rqsid_beam_expand / rqsid_beam_merge call
               (and level 0's rqsid_assign_topk), summed per level over the row chunks; the whole call's time too;
  topk         rqsid_assign_topk at k = beam over the same rows on the greedy path's segments (encode_topk, events
               around each level's call): the expand does `beam` times its work, so expand / topk is expected near
               `beam` (reported, not asserted);
  composition  what the feature replaces, at --comp-rows rows (the residual matrices of `beam` hypotheses must fit):
               per hypothesis ops.residual matrices, ops.assign_topk on them, then torch.topk over the beam * beam
               scaled distances.  The hypotheses are the prefixes of encode_beam's own paths, so both do the same
               ranking work; the composition has no forced slot 0 (timing only);
  error        mean squared original-space reconstruction error of greedy (slot 0) and of the beam's answer, and the
               share of rows whose ids changed.

Per measurement: median / min / max over every timed repetition after warm-up, the beam widths alternating.  Writes
one JSON document (default profiles/beam_ab.json); DESIGN.md 3.1h quotes it.
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

BEAMS = (1, 2, 4, 8)


def log(msg):
    print(f"[beam_bench] {msg}", file=sys.stderr, flush=True)


def stats(v):
    return {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "n": len(v)}


def event_pair():
    return torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)


class Hooks:
    """Device events around the named ops functions while a call runs; ``marks[name]`` keeps them in call order."""

    def __init__(self, names):
        self.names, self.marks, self.orig = names, {n: [] for n in names}, {}

    def __enter__(self):
        for name in self.names:
            self.orig[name] = orig = getattr(ops, name)

            def hook(*a, _orig=orig, _name=name, **kw):
                s, e = event_pair()
                s.record()
                out = _orig(*a, **kw)
                e.record()
                self.marks[_name].append((s, e))
                return out
            setattr(encmod.ops, name, hook)
        return self

    def __exit__(self, *exc):
        for name, orig in self.orig.items():
            setattr(encmod.ops, name, orig)

    def times(self, name):
        return [s.elapsed_time(e) for s, e in self.marks[name]]


def timed_beam(enc, x, B, chunk_rows):
    """One encode_beam: (Beam, whole ms, expand ms per level [3], merge ms per level [3])."""
    s, e = event_pair()
    with Hooks(("assign_topk", "beam_expand", "beam_merge")) as h:
        s.record()
        bm = enc.encode_beam(x, B, chunk_rows=chunk_rows, check=False)
        e.record()
    torch.cuda.synchronize()
    ex, mg = h.times("beam_expand"), h.times("beam_merge")
    expand = [sum(h.times("assign_topk")), sum(ex[0::2]), sum(ex[1::2])]  # per chunk: level 1 then level 2
    merge = [sum(mg[0::3]), sum(mg[1::3]), sum(mg[2::3])]
    return bm, s.elapsed_time(e), expand, merge


def timed_topk(enc, x, k):
    with Hooks(("assign_topk",)) as h:
        out = enc.encode_topk(x, k, check=False)
    torch.cuda.synchronize()
    del out
    return h.times("assign_topk")


def composition(enc, x, paths, B):
    """Levels 1 and 2 of a beam step without rqsid_beam_expand: (ms level 1, ms level 2)."""
    n = x.shape[0]
    norm = enc.sem.normalize_residual
    c0, c1 = enc.pcs[0].centers, enc.pcs[1].centers
    p0 = [paths[:, h, 0].clamp(min=0).contiguous() for h in range(B)]
    g1 = [(p0[h] * enc.need[1] + paths[:, h, 1].clamp(min=0)).contiguous() for h in range(B)]
    grp = [(p0[h] * enc._last_mult() + paths[:, h, 1].clamp(min=0)).contiguous() for h in range(B)]
    out = []
    for level in (1, 2):
        s, e = event_pair()
        s.record()
        dists = []
        for h in range(B):
            r = ops.residual(x, c0, p0[h], normalize=norm)
            if level == 1:
                b = enc._bucket(p0[h], enc.need[0])
            else:
                r = ops.residual(r, c1, g1[h], normalize=norm)
                b = enc._bucket(grp[h], enc.n_groups)
            dists.append(ops.assign_topk(r, enc.pcs[level], b, enc.raw_cands[level], B, workspace=enc._tws,
                                         check=False)[2])
            del r
        torch.topk(torch.cat(dists, 1), B, dim=1, largest=False)
        e.record()
        torch.cuda.synchronize()
        out.append(s.elapsed_time(e))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--comp-rows", type=int, default=1_000_000, help="rows of the composition's measurement")
    ap.add_argument("--chunk-rows", type=int, default=0, help="encode_beam's chunk_rows (0: its default)")
    ap.add_argument("--alternations", type=int, default=3)
    ap.add_argument("--reps", type=int, default=1, help="timed repetitions per beam width per alternation")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--codebooks", choices=("fitted", "sampled"), default="fitted")
    ap.add_argument("--out", default=str(REPO / "profiles" / "beam_ab.json"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    cb = bench.codebooks(a.codebooks, dev)
    enc = RQEncoder([torch.from_numpy(cb[k]) for k in ("c0", "c1", "c2")], list(bench.NEED),
                    match=torch.from_numpy(cb["match"]), semantics=HIERARCHICAL_TRAIN, device=dev)
    assert enc.fused
    x = bench.make_rows(a.rows, 0, dev)
    n, d = x.shape
    xc = x[:min(a.comp_rows, n)]
    chunk = a.chunk_rows or None
    torch.cuda.synchronize()
    log(f"codebooks and {n} rows ready")

    res = {B: {"whole": [], "expand": [[], [], []], "merge": [[], [], []], "topk": [[], [], []],
               "comp": [[], []], "beam_comp_rows": [[], []]} for B in BEAMS}
    err = {}
    for B in BEAMS:  # warm-up and the error figures, outside the timed alternations
        for _ in range(a.warmup):
            bm = enc.encode_beam(x, B, chunk_rows=chunk, check=False)
            enc.encode_topk(x, B, check=False)
            composition(enc, xc, bm.paths[:len(xc)], B)
        g2 = bm.path_err[:, 0].double().pow(2)
        b2 = bm.recon_err.double().pow(2)
        ok = torch.isfinite(g2) & torch.isfinite(b2)
        err[B] = {"rows_scored": int(ok.sum().item()), "greedy_mse": float(g2[ok].mean().item()),
                  "beam_mse": float(b2[ok].mean().item()),
                  "changed_share": float((bm.slot != 0).double().mean().item()),
                  "greedy_equals_encode": bool(torch.equal(bm.paths[:, 0], enc.encode(x)))}
        del bm, g2, b2, ok
        log(f"beam {B}: {err[B]}")
    enc.check_errors()
    for alt in range(a.alternations):
        log(f"alternation {alt}")
        for B in BEAMS:
            for _ in range(a.reps):
                bm, whole, expand, merge = timed_beam(enc, x, B, chunk)
                res[B]["whole"].append(whole)
                topk = timed_topk(enc, x, B)
                for l in range(3):
                    res[B]["expand"][l].append(expand[l])
                    res[B]["merge"][l].append(merge[l])
                    res[B]["topk"][l].append(topk[l])
                comp = composition(enc, xc, bm.paths[:len(xc)], B)
                _, _, ex_c, mg_c = timed_beam(enc, xc, B, chunk)
                for i in range(2):
                    res[B]["comp"][i].append(comp[i])
                    res[B]["beam_comp_rows"][i].append(ex_c[i + 1] + mg_c[i + 1])
                del bm
    enc.check_errors()

    doc = {"what": "tools/beam_bench.py: encode_beam against rqsid_assign_topk at the same k and against the "
                   "composition it replaces, one process (measured)",
           "rows": n, "dim": d, "need": list(bench.NEED), "codebooks": a.codebooks, "alternations": a.alternations,
           "reps": a.reps, "composition_rows": len(xc), "chunk_rows": a.chunk_rows or "default",
           "device": torch.cuda.get_device_name(dev), "beams": {}}
    for B in BEAMS:
        r = res[B]
        levels = []
        for l in range(3):
            ex, mg, tk = stats(r["expand"][l]), stats(r["merge"][l]), stats(r["topk"][l])
            lv = {"level": l, "expand": ex, "merge": mg, "assign_topk_same_k": tk,
                  "expand_over_topk": ex["median_ms"] / tk["median_ms"]}
            if l:
                co, bc = stats(r["comp"][l - 1]), stats(r["beam_comp_rows"][l - 1])
                lv["composition"] = co
                lv["expand_plus_merge_at_composition_rows"] = bc
                lv["composition_over_ours"] = co["median_ms"] / bc["median_ms"]
            levels.append(lv)
        doc["beams"][str(B)] = dict(err[B], whole=stats(r["whole"]), levels=levels)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(doc, indent=1) + "\n")
    print(json.dumps({B: {"whole_ms": v["whole"]["median_ms"],
                          "expand_ms": [l["expand"]["median_ms"] for l in v["levels"]],
                          "merge_ms": [l["merge"]["median_ms"] for l in v["levels"]],
                          "expand_over_topk": [l["expand_over_topk"] for l in v["levels"]],
                          "composition_over_ours": [l.get("composition_over_ours") for l in v["levels"]],
                          "greedy_mse": v["greedy_mse"], "beam_mse": v["beam_mse"],
                          "changed_share": v["changed_share"]} for B, v in doc["beams"].items()}))


if __name__ == "__main__":
    main()
