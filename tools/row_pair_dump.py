"""Raw output bytes of the two entries built on the row-against-row block (csrc/tile_rows.h): rqsid_silhouette and
rqsid_row_knn, with their error words and the k-NN counters, on small seeded inputs through the public API, as one
.npz:

    RQSID_LIB=path/to/other/librqsid.so python tools/row_pair_dump.py a.npz
    python tools/row_pair_dump.py b.npz
    python tools/row_pair_dump.py --compare a.npz b.npz     # every array byte for byte; exit status 1 if not

Both entries are pure functions of their arguments, so two builds of the same ABI agree here byte for byte or one of
them changed what the block computes.  The inputs take every path of the block: one ragged tile (100 rows), row
counts that are no multiple of the tile, a ragged query tile (300 queries), one chunk per tile (dim 32) and many,
chunk_rows 128 / 256 / 0, the three row formats, both metrics and k = 1 / 10 / 16, identity and bucketed order with
an empty segment and segments that span chunks, queries sorted by segment (tiles skipped at both ends of a chunk),
NaNs in a base row and in a query, and tables with one bad entry (check=False).  Floats are stored as bit patterns.
"""
import argparse
import json
import os
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from generative_ranking_recommender_amd import ops  # noqa: E402

N_QUERIES = 300
SHAPES = ((100, 32, 3), (3000, 64, 7), (2500, 512, 5))  # rows, dim, blobs
CHUNKS = (128, 256, 0)
FORMATS = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
KNN = tuple((metric, k) for metric in ("l2", "cosine") for k in (1, 10, 16))


def raw(t):
    a = t.detach().contiguous().cpu()
    if a.dtype in (torch.float32, torch.int32):
        return a.view(torch.int32).numpy()
    return a.numpy()


class Input:
    """Rows around `blobs` centres bucketed by blob; segment `blobs` is empty, segment `blobs + 1` holds five rows."""

    def __init__(self, n, dim, blobs, dev):
        rng = np.random.default_rng(1000 * n + dim)
        lab = rng.integers(0, blobs, n).astype(np.int32)
        lab[-5:] = blobs + 1
        x = (rng.normal(size=(blobs + 2, dim))[lab] + rng.normal(size=(n, dim))).astype(np.float32)
        self.n, self.dev = n, dev
        self.x = torch.from_numpy(x).to(dev)
        self.rows = np.concatenate([np.arange(n - 5, n), rng.choice(n - 5, N_QUERIES - 5, replace=n < N_QUERIES)])
        # grouped on the host: rqsid_bucket places rows by a device counter, so its order inside a segment differs
        # from run to run, and the silhouette's fp32 sums follow the order
        self.off_np = np.concatenate([[0], np.cumsum(np.bincount(lab, minlength=blobs + 2))]).astype(np.int32)
        self.order, self.off = self.gpu(np.argsort(lab, kind="stable").astype(np.int32)), self.gpu(self.off_np)
        self.qself = self.gpu(self.rows.astype(np.int32))
        # the query's segment under the bucketed order (its blob) and under the identity order (where its row lies)
        self.qseg = {"bucketed": lab[self.rows].copy(),
                     "identity": (np.searchsorted(self.off_np, self.rows, "right") - 1).astype(np.int32)}
        for v in self.qseg.values():
            v[5:25] = -1
            v[25:30] = blobs

    def gpu(self, a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)

    def both(self, out, tag, x, q, order, off, qself, qseg, chunk, knn=KNN):
        """One silhouette call and one row_knn call per (metric, k) on the same tables."""
        ws = ops.SilhouetteWorkspace(len(x), len(q), self.dev, chunk)
        res = ops.silhouette(x, order, off, q, qself, qseg, chunk, workspace=ws, check=False)
        for name, t in zip(("a", "b", "b_seg", "s"), res):
            out[f"sil_{tag}_{name}"] = raw(t)
        out[f"sil_{tag}_word"] = raw(ws.error_word())
        for metric, k in knn:
            ws = ops.RowKnnWorkspace(len(x), len(q), k, self.dev, chunk)
            rows, val = ops.row_knn(x, q, k, metric, order=order, seg_row_off=off, query_self=qself, query_seg=qseg,
                                    chunk_rows=chunk, workspace=ws, check=False)
            out[f"knn_{tag}_{metric}{k}_rows"], out[f"knn_{tag}_{metric}{k}_val"] = raw(rows), raw(val)
            out[f"knn_{tag}_{metric}{k}_word"] = raw(ws.error_word())
            out[f"knn_{tag}_{metric}{k}_counters"] = np.array(list(ws.counters().values()), dtype=np.int64)


def dump(dev):
    out = {}
    for n, dim, blobs in SHAPES:
        c = Input(n, dim, blobs, dev)
        for fmt, dtype in FORMATS.items():
            x = c.x.to(dtype)
            q = x[c.gpu(c.rows)].contiguous()
            for chunk in CHUNKS:
                for order_name, order in (("identity", None), ("bucketed", c.order)):
                    tag = f"n{n}_d{dim}_{fmt}_c{chunk}_{order_name}"
                    c.both(out, tag, x, q, order, c.off, c.qself, c.gpu(c.qseg[order_name]), chunk)
        if n != 3000:
            continue
        # the restricted queries sorted by segment: a block's union range leaves tiles out at both ends
        keep = np.flatnonzero(c.qseg["bucketed"] >= 0)
        pick = keep[np.argsort(c.qseg["bucketed"][keep], kind="stable")]
        for chunk in (128, 1024, 0):
            c.both(out, f"sorted_c{chunk}", c.x, c.x[c.gpu(c.rows[pick])].contiguous(), c.order, c.off,
                   c.gpu(c.rows[pick].astype(np.int32)), c.gpu(c.qseg["bucketed"][pick]), chunk)
        # without any table but the offsets the silhouette needs: every query searches every row
        for metric, k in KNN:
            rows, val = ops.row_knn(c.x, c.x[c.gpu(c.rows)].contiguous(), k, metric, check=False)
            out[f"knn_plain_{metric}{k}_rows"], out[f"knn_plain_{metric}{k}_val"] = raw(rows), raw(val)
        # a NaN in a base row, a NaN in a query
        q = c.x[c.gpu(c.rows)].contiguous()
        qseg = c.gpu(c.qseg["bucketed"])
        x = c.x.clone()
        x[int(c.rows[40]), 5] = float("nan")
        c.both(out, "nan_row", x, q, c.order, c.off, c.qself, qseg, 256)
        qn = q.clone()
        qn[33, 2] = float("nan")
        c.both(out, "nan_query", c.x, qn, c.order, c.off, c.qself, qseg, 256)
        # tables with one bad entry: clamped, and the word says which
        order = c.order.clone()
        order[1234] = n + 3
        c.both(out, "bad_row_index", c.x, q, order, c.off, c.qself, qseg, 256)
        bad = c.qseg["bucketed"].copy()
        bad[10] = blobs + 2
        c.both(out, "bad_query_seg", c.x, q, c.order, c.off, c.qself, c.gpu(bad), 256)
        off = c.off.clone()
        off[3] = off[2] - 7
        c.both(out, "bad_seg_row_off", c.x, q, c.order, off, c.qself, qseg, 256)
    return out


def compare(a_path, b_path):
    a, b = np.load(a_path), np.load(b_path)
    res = {}
    for name in sorted(set(a.files) | set(b.files)):
        same = name in a.files and name in b.files and a[name].dtype == b[name].dtype and \
            a[name].shape == b[name].shape and a[name].tobytes() == b[name].tobytes()
        res[name] = "equal" if same else "DIFFERENT"
    diff = [k for k, v in res.items() if v != "equal"]
    print(json.dumps({"arrays": len(res), "different": diff}, indent=1))
    return not diff


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
    words = {k: int(v[0]) for k, v in out.items() if k.endswith("_word") and int(v[0])}
    print(f"{a.paths[0]}: {len(out)} arrays, library {os.environ.get('RQSID_LIB', 'of this tree')}; "
          f"non-zero error words: {json.dumps(words)}")


if __name__ == "__main__":
    main()
