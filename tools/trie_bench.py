#!/usr/bin/env python3
"""A/B of the constrained-decoding mask at a decoder's shape: B = 2048 rows (256 sequences x 8 beams) x V = 32,614
(a T5 vocabulary of 32,100 + 512 ID tokens + 2), fp32 and bf16 scores, over the trie of the IDs of the bench's encode
(--ids encode: the PROD codebooks and rows bench.py builds) or of synthetic IDs of the PROD sizes (--ids synth: uniform
level 1 and 2, skewed level 3); the document says which.  Alternating inside ONE process:

  kernel        rqsid_trie_mask (ops.trie_mask, check=False: no host read)
  composition   the same tables walked with torch ops: tok_code gather, last level-0 position, one searchsorted per
                level over (parent, value) keys, the children's tokens scattered into a [B, V] bool mask rebuilt per
                call, masked_fill
  python        for the record, at B = 64: a per-row Python loop in the reference's style (tolist, a backwards scan, a
                dict walk, one assignment per allowed token, masked_fill)

All three leave the same bytes (asserted).  Also timed: the trie build (rqsid_id_trie) beside rqsid_bucket +
rqsid_id_cells on the same IDs, and one beam step (beam_in = beam_out = 8, 256 rows, the last level).
Times are device events around each call (median, min, max over every timed repetition of every alternation, after
warm-up); the python arm is a host clock around a synchronised call.  Gate: the kernel takes at most half the
composition's median (fp32 and bf16).  Also printed: the fraction of the 8 TB/s peak that B x V x element bytes of
stores reach in the kernel's time (both of its launches included).

Writes one JSON document (default profiles/trie_ab.json); README.md and DESIGN.md quote it.
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))

from generative_ranking_recommender_amd import ops  # noqa: E402
from generative_ranking_recommender_amd.semantic_id_trie import SemanticIDTrie  # noqa: E402

NEED = (128, 128, 256)
BASE_VOCAB, VOCAB, EOS = 32100, 32614, 1
PEAK_BYTES_PER_S = 8e12


def timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    out = fn()
    e.record()
    torch.cuda.synchronize()
    return out, s.elapsed_time(e)


def stats(v):
    return {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "n": len(v)}


def alternate(arms, a):
    for _, fn in arms:
        for _ in range(a.warmup):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _ in arms}
    for _ in range(a.alternations):
        for name, fn in arms:
            for _ in range(a.reps):
                times[name].append(timed(fn)[1])
    return {name: stats(v) for name, v in times.items()}


def encode_ids(a, dev):
    import bench  # (codebooks and rows exactly as the benchmark builds them)
    from generative_ranking_recommender_amd.encode import HIERARCHICAL_TRAIN, RQEncoder
    cb = bench.codebooks(a.codebooks, dev)
    enc = RQEncoder([torch.from_numpy(cb[k]) for k in ("c0", "c1", "c2")], list(bench.NEED),
                    match=torch.from_numpy(cb["match"]), semantics=HIERARCHICAL_TRAIN, device=dev)
    ids = enc.encode(bench.make_rows(a.rows, 0, dev))
    return ids.contiguous(), tuple(enc.id_sizes())


def synth_ids(a, dev):
    gen = torch.Generator(device=dev)
    gen.manual_seed(1234)
    cols = [torch.randint(0, s, (a.rows,), generator=gen, device=dev, dtype=torch.int32) for s in NEED[:2]]
    cols.append((torch.rand(a.rows, generator=gen, device=dev).pow(2) * NEED[2]).to(torch.int32).clamp_(0, NEED[2] - 1))
    return torch.stack(cols, 1).contiguous(), NEED


class TorchTables:
    """What the composition walks: per level the (parent, value) keys of the nodes, ascending, and the fan-out bound."""

    def __init__(self, trie: ops.IdTrie, tokens: ops.TokenMap):
        self.L, self.sizes, self.tokens = trie.levels, trie.sizes, tokens
        cnt = trie.counts()
        dev = trie.count.device
        self.value, self.off, self.key, self.fan = [], [], [], []
        for d in range(self.L):
            off = trie.child_off[d, :cnt[d] + 1].long()
            val = trie.value[d, :cnt[d + 1]].long()
            parent = torch.repeat_interleave(torch.arange(cnt[d], device=dev), off[1:] - off[:-1])
            self.value.append(val)
            self.off.append(off)
            self.key.append(parent * self.sizes[d] + val)
            self.fan.append(int((off[1:] - off[:-1]).max().item()) if cnt[d] else 0)
        self.level_tok = [tokens.level_tok[tokens.level_off[l]:tokens.level_off[l + 1]].long() for l in range(self.L)]
        self.l0 = self.level_tok[0][self.level_tok[0] >= 0]

    def mask(self, input_ids, scores):
        """ConstrainedLogitsProcessor.__call__ with torch ops alone; no host read."""
        B, T = input_ids.shape
        V, L, dev = scores.shape[1], self.L, scores.device
        inside = (input_ids >= 0) & (input_ids < V)
        code = torch.where(inside, self.tokens.tok_code[input_ids.clamp(0, V - 1)].long(), -1)
        is0 = (code >= 0) & ((code >> 24) == 0)
        pos = torch.arange(T, device=dev)
        first = torch.where(is0, pos, -1).max(1).values                     # the last level-0 position, or -1
        plen = torch.where(first < 0, 0, (T - first).clamp_max(L))
        at = (first.clamp_min(0).unsqueeze(1) + torch.arange(L, device=dev)).clamp_max(T - 1)
        pcode = torch.gather(code, 1, at)                                    # the prefix's codes (beyond plen: unused)
        node = torch.zeros(B, dtype=torch.long, device=dev)
        ok = torch.ones(B, dtype=torch.bool, device=dev)
        allowed = torch.zeros(B, V + 1, dtype=torch.bool, device=dev)        # column V takes what is not allowed
        for d in range(L):
            here = ok & (plen == d)                                          # the rows whose walk ends at depth d
            lo, hi = self.off[d][node.clamp_max(len(self.off[d]) - 2)], self.off[d][node.clamp_max(len(self.off[d]) - 2) + 1]
            j = torch.arange(self.fan[d], device=dev).unsqueeze(0)
            child = (lo.unsqueeze(1) + j).clamp_max(max(len(self.value[d]) - 1, 0))
            tok = self.level_tok[d][self.value[d][child]]
            tok = torch.where(here.unsqueeze(1) & (j < (hi - lo).unsqueeze(1)) & (tok >= 0), tok, V)
            allowed.scatter_(1, tok, True)
            if d + 1 < L:                                                    # one more level for the longer prefixes
                c = pcode[:, d]
                good = (c >= 0) & ((c >> 24) == d)
                want = node * self.sizes[d] + (c & 0xFFFFFF)
                p = torch.searchsorted(self.key[d], want).clamp_max(max(len(self.key[d]) - 1, 0))
                ok = ok & ((plen <= d) | (good & (self.key[d][p] == want)))
                node = torch.where(plen > d, p, node)
        complete = plen == L
        allowed[:, :V] |= complete.unsqueeze(1) & torch.zeros(V, dtype=torch.bool, device=dev).index_fill_(
            0, self.l0, True).unsqueeze(0)
        allowed[:, self.tokens.eos_token_id] |= complete | ~allowed[:, :V].any(1)
        scores.masked_fill_(~allowed[:, :V], float("-inf"))
        return scores


class PythonLoop:
    """The per-row host loop a logits processor without the kernel runs (the reference's shape of work)."""

    def __init__(self, trie: SemanticIDTrie):
        self.L = trie.levels
        self.root = {}
        for seq in trie.get_all_valid_sequences():
            node = self.root
            for t in seq:
                node = node.setdefault(t, {})
        tok = trie.tokens
        self.l0 = {int(t) for t in tok.level_tok_host[:tok.sizes[0]] if t >= 0}
        self.eos = tok.eos_token_id

    def __call__(self, input_ids, scores):
        for b in range(input_ids.shape[0]):
            seq = input_ids[b].tolist()
            prefix = []
            for i in range(len(seq) - 1, -1, -1):
                if seq[i] in self.l0:
                    prefix = seq[i:i + self.L]
                    break
            node = self.root
            for t in prefix:
                node = node.get(t) if node is not None else None
            valid = set(node.keys()) if node else set()
            if len(prefix) == self.L:
                valid = self.l0 | {self.eos}
            if not valid:
                valid = {self.eos}
            mask = torch.ones_like(scores[b], dtype=torch.bool)
            for t in valid:
                mask[t] = False
            scores[b] = scores[b].masked_fill(mask, float("-inf"))
        return scores


def decoder_rows(trie: SemanticIDTrie, B, T, seed):
    """Token rows as a beam of decoders holds them: ordinary tokens, one complete ID, then 0 .. 3 tokens of the next
    (one row in 16 breaks off into a pair the trie does not hold)."""
    rng = np.random.default_rng(seed)
    seqs = np.asarray(trie.get_all_valid_sequences(), dtype=np.int64)
    rows = rng.integers(2, BASE_VOCAB, (B, T))
    done, cur = seqs[rng.integers(0, len(seqs), B)], seqs[rng.integers(0, len(seqs), B)]
    n = rng.integers(0, 4, B)
    for b in range(B):
        tail = list(done[b]) + list(cur[b][:n[b]])
        if b % 16 == 5 and n[b] == 2:
            tail[-1] = int(seqs[rng.integers(0, len(seqs)), 1])
        rows[b, T - len(tail):] = tail
    return torch.from_numpy(rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ids", choices=("encode", "synth"), default="encode")
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--codebooks", choices=("fitted", "sampled"), default="fitted")
    ap.add_argument("--batch", type=int, default=2048)
    ap.add_argument("--tokens", type=int, default=16, help="columns of input_ids")
    ap.add_argument("--alternations", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5, help="timed calls per arm per alternation")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=str(REPO / "profiles" / "trie_ab.json"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    ids, sizes = (encode_ids if a.ids == "encode" else synth_ids)(a, dev)
    level_tokens = [np.arange(BASE_VOCAB + sum(sizes[:l]), BASE_VOCAB + sum(sizes[:l + 1])) for l in range(len(sizes))]
    tokens = ops.TokenMap(VOCAB, level_tokens, EOS, device=dev)
    doc = {"what": "tools/trie_bench.py: rqsid_trie_mask against the same tables walked with torch ops and against a "
                   "per-row Python loop; the trie build beside rqsid_id_cells; one beam step (measured)",
           "ids": ("the bench's encode (%s codebooks)" % a.codebooks) if a.ids == "encode" else
                  "synthetic IDs of the PROD sizes (uniform level 1 and 2, level 3 skewed to low values)",
           "rows": int(ids.shape[0]), "sizes": list(sizes), "vocab": VOCAB, "batch": a.batch, "tokens": a.tokens,
           "alternations": a.alternations, "reps": a.reps, "device": torch.cuda.get_device_name(dev)}

    # ---- the builds
    n = ids.shape[0]
    group = (ids[:, 0] * sizes[1] + ids[:, 1]).contiguous()
    fine = ids[:, 2].contiguous()
    index = ops.id_cells(ids, sizes)
    n_cells = index.n_cells
    cg, cf = index.cell_group[:n_cells].contiguous(), index.cell_fine[:n_cells].contiguous()
    cells_ws = ops.IdCellsWorkspace(n, sizes[0] * sizes[1], sizes[2], dev)

    def cells_arm():
        b = ops.bucket(group, sizes[0] * sizes[1])
        cap = min(n, sizes[0] * sizes[1] * sizes[2])
        o = [torch.empty(m, dtype=torch.int32, device=dev) for m in (n, n, n, n, cap + 1, cap, cap)]
        rc = ops.lib().rqsid_id_cells(n, ops._ptr(b.row_index), sizes[0] * sizes[1], ops._ptr(b.seg_row_off), None,
                                      ops._ptr(fine), sizes[2], None, *(ops._ptr(t) for t in o), ops._ptr(cells_ws.buf),
                                      cells_ws.bytes, ops._stream())
        assert rc == 0, ops.lib().rqsid_last_error().decode()
        return o

    doc["build"] = {"cells": n_cells, "arms": alternate([
        ("id_cells", cells_arm), ("id_trie", lambda: ops.id_trie_tables(cg, cf, sizes, check=False))], a)}
    trie = SemanticIDTrie.from_index(index, tokens)
    assert int(trie.trie.error.item()) == 0
    doc["build"]["nodes_per_depth"] = list(trie.trie.counts())
    print(json.dumps({"build": {k: v["median_ms"] for k, v in doc["build"]["arms"].items()}, "cells": n_cells}),
          flush=True)

    # ---- the mask
    tt = TorchTables(trie.trie, tokens)
    input_ids = decoder_rows(trie, a.batch, a.tokens, seed=7).to(dev)
    ws = ops.TrieMaskWorkspace(a.batch, dev)
    loop = PythonLoop(trie)
    doc["mask"] = {}
    for name, dtype in (("f32", torch.float32), ("bf16", torch.bfloat16)):
        src = (torch.randn(a.batch, VOCAB, device=dev) * 3).to(dtype)
        bits = torch.int32 if dtype == torch.float32 else torch.int16
        k, c = src.clone(), src.clone()
        rows = ops.trie_mask(trie.trie, tokens, input_ids, k, ws, check=False)
        tt.mask(input_ids, c)
        assert int(ws.error_word().item()) == 0
        assert torch.equal(k.view(bits), c.view(bits)), "the composition and the kernel disagree"
        p64 = loop(input_ids[:64].cpu(), src[:64].clone())
        assert torch.equal(p64.view(bits), k[:64].view(bits)), "the python loop and the kernel disagree"
        buf = src.clone()
        arms = alternate([("kernel", lambda: ops.trie_mask(trie.trie, tokens, input_ids, buf, ws, check=False)),
                          ("composition", lambda: tt.mask(input_ids, buf))], a)
        small_ids, small = input_ids[:64].contiguous(), src[:64].clone()
        py = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            loop(small_ids, small)
            torch.cuda.synchronize()
            py.append((time.perf_counter() - t0) * 1e3)
        km, cm = arms["kernel"]["median_ms"], arms["composition"]["median_ms"]
        stored = a.batch * VOCAB * src.element_size()
        doc["mask"][name] = {
            "arms": arms, "python_loop_64_rows_device_tensors": stats(py), "kernel_over_composition": km / cm,
            "rows_by_kind": rows.kinds.tolist(), "outputs_equal": True, "bytes_stored_at_most": stored,
            "fraction_of_8TBps_peak": stored / (km * 1e-3) / PEAK_BYTES_PER_S, "gate_passed": km <= 0.5 * cm}
        print(json.dumps({name: {"kernel_ms": km, "composition_ms": cm, "ratio": km / cm,
                                 "python_loop_64_rows_ms": statistics.median(py),
                                 "fraction_of_peak": doc["mask"][name]["fraction_of_8TBps_peak"]}}), flush=True)

    # ---- one beam step on the last level
    cnt = trie.trie.counts()
    gen = torch.Generator(device=dev)
    gen.manual_seed(5)
    node_in = torch.randint(0, cnt[2], (256, 8), generator=gen, device=dev, dtype=torch.int32)
    score_in = -torch.rand(256, 8, generator=gen, device=dev)
    logp = torch.log_softmax(torch.randn(2048, VOCAB, generator=gen, device=dev), 1)
    doc["beam_step"] = {"rows": 256, "beam_in": 8, "beam_out": 8, "depth": 2, "arms": alternate(
        [("kernel", lambda: ops.trie_beam_step(trie.trie, tokens, 2, node_in, score_in, logp, 8))], a)}
    doc["gate"] = {"kernel_at_most_half_the_composition": all(m["gate_passed"] for m in doc["mask"].values()),
                   **{name: m["kernel_over_composition"] for name, m in doc["mask"].items()}}
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(doc, indent=1) + "\n")
    print(json.dumps({"beam_step_ms": doc["beam_step"]["arms"]["kernel"]["median_ms"], "gate": doc["gate"]}))


if __name__ == "__main__":
    main()
