"""Raw output bytes of everything the exact tail decides (csrc/exact_row.h: the re-score, the fp32 re-screen and the
top-k / beam exact pass), on small seeded inputs through the public API, as one .npz:

    RQSID_LIB=path/to/other/librqsid.so python tools/exact_tail_dump.py a.npz
    python tools/exact_tail_dump.py b.npz
    python tools/exact_tail_dump.py --compare a.npz b.npz     # every array byte for byte; exit status 1 if not

Two builds of the same ABI that agree here do the exact arithmetic the same way: the shapes are those of the tests
that pin it (near-isotropic rows that list and overflow, duplicated centres, penalty segments, the three residual
levels with and without normalisation, 16-bit rows).  Floats are stored as their bit patterns.
"""
import argparse
import json
import os
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from generative_ranking_recommender_amd import ops, synth  # noqa: E402
from generative_ranking_recommender_amd.encode import HIERARCHICAL_TRAIN, SIMPLIFIED, RQEncoder  # noqa: E402

NEED = [16, 16, 32]
ROWS = 4097


def raw(t):
    a = t.detach().contiguous().cpu()
    if a.dtype in (torch.float32, torch.int32):
        return a.view(torch.int32).numpy()
    return a.numpy()


def with_env(env, fn):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update({k: str(v) for k, v in env.items()})
    try:
        return fn()
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def dump(dev):
    out = {}
    gpu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731

    # re-score: near-isotropic rows against many close centres (most rows listed, many "every candidate")
    for k, dim in ((300, 512), (200, 1024), (64, 256)):
        rng = np.random.default_rng(k + dim)
        c = (rng.standard_normal((k, dim)) * 0.05 + 1.0).astype(np.float32)
        x = gpu((rng.standard_normal((ROWS, dim)) * 0.05 + 1.0).astype(np.float32))
        pc = ops.prepare_centers(gpu(c))
        ws = ops.AssignWorkspace(ROWS, dev)
        out[f"rescore_k{k}_d{dim}"] = raw(ops.nearest(x, pc, workspace=ws, screen_terms=1))
        out[f"rescore_k{k}_d{dim}_items"] = np.array([ws.rescored(), ws.error()], dtype=np.int64)
        if (k, dim) == (300, 512):
            out["rescore_k300_d512_full"] = raw(with_env({"RQSID_RESCORE_FULL": 1},
                                                         lambda: ops.nearest(x, pc, screen_terms=1)))

    # re-screen: diffuse unit rows, 12 exact duplicates of one centre keep a true > 8-way tie overflowing
    rng = np.random.default_rng(2560 + 12)
    x = rng.standard_normal((3000, 512), dtype=np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    c = rng.standard_normal((2560, 512), dtype=np.float32)
    c /= np.linalg.norm(c, axis=1, keepdims=True)
    c[100:112] = c[7]
    x[:500] = c[7] + np.float32(0.01) * rng.standard_normal((500, 512), dtype=np.float32)
    pc, xg = ops.prepare_centers(gpu(c)), gpu(x)
    for mode in (0, 1):
        ws = ops.AssignWorkspace(len(x), dev)
        out[f"rescreen_off{mode}"] = raw(with_env({"RQSID_NO_RESCREEN": mode}, lambda: ops.nearest(xg, pc, workspace=ws)))
        out[f"rescreen_off{mode}_items"] = np.array([ws.rescored(), ws.error()], dtype=np.int64)

    # penalty segments (empty groups: +10000 everywhere)
    rng = np.random.default_rng(2)
    x = synth.small_mixture(500, m=10, seed=1)
    c = synth.small_mixture(96, m=10, seed=2)
    match = np.zeros((4, 96), dtype=np.uint8)
    match[0, :32] = 1
    match[2, 40:80] = 1
    seg = rng.integers(0, 4, 500).astype(np.int32)
    loc, glob = ops.assign(gpu(x), ops.prepare_centers(gpu(c)), ops.bucket(gpu(seg), 4),
                           ops.match_to_candidates(gpu(match)))
    out["penalty_local"], out["penalty_global"] = raw(loc), raw(glob)

    # fused three-level encode, top-k and beam: residual levels 0 / 1 / 2, normalised (hier) and plain (simplified)
    cb = synth.encode_codebooks(seed=5, need=tuple(NEED), n_cand=320, pool_rows=8192)
    x32 = synth.mixture_rows(0, ROWS)
    rows = {"f32": gpu(x32), "f16": gpu(x32).to(torch.float16), "bf16": gpu(x32).to(torch.bfloat16)}
    for sem_name, sem in (("hier", HIERARCHICAL_TRAIN), ("simplified", SIMPLIFIED)):
        enc = RQEncoder([torch.from_numpy(cb[k]) for k in ("c0", "c1", "c2")], NEED, match=torch.from_numpy(cb["match"]),
                        semantics=sem, device=dev)
        for fmt, xr in rows.items():
            out[f"encode_{sem_name}_{fmt}"] = raw(enc.encode(xr))
            if sem_name == "hier":  # the level-1 divisor the screen or the re-score wrote
                b = ops.bucket(ops.nearest(rows["f32"], enc.pcs[0]), NEED[0])
                den = torch.zeros(ROWS, dtype=torch.float32, device=dev)
                fr = ops.FusedResidual(1, True, enc.pcs[0].centers, None, den_out=den)
                loc, _ = ops.assign(xr, enc.pcs[1], b, enc.cands[1], fused=fr)
                out[f"level1_{fmt}_local"], out[f"level1_{fmt}_den"] = raw(loc), raw(den)
        for k in (1, 3, 8):
            tk = enc.encode_topk(rows["f32"], k)
            for name in ("ids", "local", "glob", "dist"):
                out[f"topk{k}_{sem_name}_{name}"] = raw(getattr(tk, name))
        tk = enc.encode_topk(rows["bf16"], 3)
        for name in ("local", "glob", "dist"):
            out[f"topk3_{sem_name}_bf16_{name}"] = raw(getattr(tk, name))
        for beam in (1, 4):
            bm = enc.encode_beam(rows["f32"], beam)
            for name in ("ids", "recon_err", "paths", "path_err", "slot"):
                out[f"beam{beam}_{sem_name}_{name}"] = raw(getattr(bm, name))
        out[f"error_words_{sem_name}"] = np.array([int(w.item()) for w in enc.error_words()], dtype=np.int64)
    return out


def compare(a_path, b_path):
    a, b = np.load(a_path), np.load(b_path)
    res = {}
    for name in sorted(set(a.files) | set(b.files)):
        same = name in a.files and name in b.files and a[name].dtype == b[name].dtype and \
            a[name].shape == b[name].shape and a[name].tobytes() == b[name].tobytes()
        res[name] = "equal" if same else "DIFFERENT"
    print(json.dumps(res, indent=1))
    return all(v == "equal" for v in res.values())


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--compare", action="store_true", help="compare two dumps instead of writing one")
    ap.add_argument("paths", nargs="+")
    a = ap.parse_args()
    if a.compare:
        if len(a.paths) != 2:
            ap.error("--compare takes two .npz files")
        sys.exit(0 if compare(*a.paths) else 1)
    if len(a.paths) != 1:
        ap.error("one output .npz")
    out = dump(torch.device("cuda", 0))
    np.savez(a.paths[0], **out)
    print(f"{a.paths[0]}: {len(out)} arrays, library {os.environ.get('RQSID_LIB', 'of this tree')}")


if __name__ == "__main__":
    main()
