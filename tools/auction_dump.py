"""Assignments and round counts of the segmented auction (csrc/auction_seg.hip) in every form of its rounds, on small
seeded inputs through the public API, as one .npz:

    RQSID_LIB=path/to/other/librqsid.so python tools/auction_dump.py a.npz
    python tools/auction_dump.py b.npz
    python tools/auction_dump.py --compare a.npz b.npz     # every array byte for byte; exit status 1 if not

The auction is a pure function of its scores, so two builds of the same ABI agree here byte for byte or one of them
changed what a round computes.  The scores are made on the host (synth.auction_scores): -distance of unit rows to
0.9-scaled sampled rows, or the tied form -(integers in 1..L) * 0.37.  Cases: the single auction at K = 16 with
N % K != 0 (1002 rounds, lists from round 32) in the one-block form with 256 and 1024 threads, lists in registers and
from memory, 2-byte and 8-byte loads, the multi-block form by switch and by default, with thousands of ties, the
two-array gather and the sweep alone; three segmented layouts (ops.seg_auction) mixing multi-chunk, one-chunk and
smaller-than-K segments; the row-sharded protocol over a world-1 group with its lists on and off.  Every case runs with
RQSID_LIST_STATS=1 and keeps the library's verdict line (stderr) beside its arrays.
"""
import argparse
import json
import os
import sys
import tempfile
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from generative_ranking_recommender_amd import ops, synth  # noqa: E402

# (N, tied levels, switches) of the single auction, K = 16
SINGLE = [(1603, 0, {}), (1604, 0, {}), (8003, 0, {}), (16003, 0, {}), (16003, 0, {"RQSID_LIST_MB_JPW": "64"}),
          (16003, 3, {"RQSID_LIST_MB_JPW": "64"}), (131203, 0, {}), (8003, 0, {"RQSID_LIST_JS": "0"}),
          (8003, 0, {"RQSID_AUCTION_LIST": "0"})]
SEGMENTED = [([2051, 700, 1500, 5, 1027], 8), ([1100, 1280, 1300], 16), ([8003, 1100], 8)]
SHARDED = [(3002, 0), (16006, 7)]  # (N, tied levels), K = 16, each with RQSID_DAUCTION_LIST 1 and 0
K = 16


class Env:
    """Switches for one case (the library reads them on every call) and the library's stderr of the case."""

    def __init__(self, switches):
        self.switches = {"RQSID_LIST_STATS": "1", **switches}

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.switches}
        os.environ.update(self.switches)
        sys.stderr.flush()
        self.tmp = tempfile.TemporaryFile()
        self.saved = os.dup(2)
        os.dup2(self.tmp.fileno(), 2)
        return self

    def __exit__(self, *exc):
        torch.cuda.synchronize()
        os.dup2(self.saved, 2)
        os.close(self.saved)
        self.tmp.seek(0)
        self.text = self.tmp.read().decode(errors="replace").strip()
        self.tmp.close()
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def tag(switches):
    return "".join(f"_{k[6:].lower()}{v}" for k, v in switches.items())


def seg_scores(sizes, k, seed=0):
    """Each segment's [k][N_s] block, concatenated (the layout of rqsid_seg_auction_lap_half)."""
    return np.concatenate([synth.auction_scores(n, k, seed=seed + s).ravel() for s, n in enumerate(sizes)])


def dump(dev):
    out, stats = {}, {}
    for n, levels, sw in SINGLE:
        name = f"single_n{n}_l{levels}{tag(sw)}"
        w = torch.from_numpy(synth.auction_scores(n, K, levels)).to(dev)
        with Env(sw) as e:
            a, rounds = ops.auction(w)
            out[name + "_assign"], out[name + "_rounds"] = a.cpu().numpy(), np.array([rounds], dtype=np.int32)
        stats[name] = e.text
    for sizes, k in SEGMENTED:
        name = "seg_" + "_".join(map(str, sizes)) + f"_k{k}"
        lay = ops.SegmentLayout(sizes, dev)
        w = torch.from_numpy(seg_scores(sizes, k)).to(dev)
        with Env({}) as e:
            a, rounds = ops.seg_auction(w, k, lay)
            out[name + "_assign"], out[name + "_rounds"] = a.cpu().numpy(), rounds.cpu().numpy()
        stats[name] = e.text
    import torch.distributed as dist
    from generative_ranking_recommender_amd.distributed import GpuAuctionPasses, ShardedAuction
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29534")
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    try:
        for n, levels in SHARDED:
            w = torch.from_numpy(synth.auction_scores(n, K, levels)).to(dev)
            for dlist in ("1", "0"):
                name = f"sharded_n{n}_l{levels}_dlist{dlist}"
                with Env({"RQSID_DAUCTION_LIST": dlist}) as e:
                    a, rounds = ShardedAuction().run(GpuAuctionPasses(w, n), n, K)
                    out[name + "_assign"] = a.cpu().numpy()
                    out[name + "_rounds"] = np.array([rounds], dtype=np.int32)
                stats[name] = e.text
    finally:
        dist.destroy_process_group()
    for name, text in stats.items():
        out["stats_" + name] = np.frombuffer(text.encode(), dtype=np.uint8)
    return out, stats


def compare(a_path, b_path):
    a, b = np.load(a_path), np.load(b_path)
    diff, notes = [], []
    for name in sorted(set(a.files) | set(b.files)):
        same = name in a.files and name in b.files and a[name].dtype == b[name].dtype and \
            a[name].shape == b[name].shape and a[name].tobytes() == b[name].tobytes()
        if not same:
            (notes if name.startswith("stats_") else diff).append(name)
    n_arrays = sum(not f.startswith("stats_") for f in set(a.files) | set(b.files))
    print(json.dumps({"arrays": n_arrays, "different": diff, "verdict_lines_different": notes}, indent=1))
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
    out, stats = dump(torch.device("cuda", 0))
    np.savez(a.paths[0], **out)
    print(f"{a.paths[0]}: {len(out) - len(stats)} arrays, library {os.environ.get('RQSID_LIB', 'of this tree')}")
    for name, text in stats.items():
        print(f"{name}: rounds {out[name + '_rounds'].tolist()} | {text or '(no verdict line)'}")


if __name__ == "__main__":
    main()
