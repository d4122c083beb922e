"""Tensor-level wrappers over the C ABI (include/rqsid.h).

Every function takes/returns DEVICE tensors on the current HIP device and
enqueues on torch's current stream; nothing here synchronises with the host.
There is deliberately no CPU implementation: a CPU tensor or a missing
``librqsid.so`` raises.
"""
from __future__ import annotations

import copy
import ctypes
from dataclasses import dataclass
from typing import Optional, Sequence

import torch

from . import _lib

_ALIGN = 256


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _require_device(*ts: Optional[torch.Tensor]) -> None:
    for t in ts:
        if t is not None and t.device.type != "cuda":
            raise RuntimeError("rqsid kernels run on the GPU only: got a %s tensor" % t.device.type)
        if t is not None and not t.is_contiguous():
            raise ValueError("rqsid kernels need contiguous tensors")


def _require_f32(who: str, *ts: Optional[torch.Tensor]) -> None:
    """The kernels behind these wrappers read their rows as fp32 through a raw pointer: any other dtype would be
    read (and, for an output, written) past its end.  A host-side check of metadata: no device sync."""
    for t in ts:
        if t is not None and t.dtype != torch.float32:
            raise TypeError("%s: rows must be float32, got %s (convert with .float() at the caller)" % (who, t.dtype))


def lib():
    return _lib.load()


def tile_rows() -> int:
    return int(lib().rqsid_assign_tile_rows())


def centroid_tile_rows() -> int:
    return int(lib().rqsid_centroid_tile_rows())


kMaxList = 8  # candidates a screen can list per row (assign_common.h)
# row dtypes rqsid_assign reads -> RQSID_X_* (include/rqsid.h) and the name RQEncoder.last_row_format reports
ROW_FORMATS = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}
ROW_FORMAT_NAMES = {torch.float32: "f32", torch.float16: "f16", torch.bfloat16: "bf16"}
# the 1-term streamed screens gather centre pieces from a hi-only copy of the table (RQSID_HI_TABLE=0: from the
# interleaved table, for A/B); read once at import
HI_TABLE = __import__("os").environ.get("RQSID_HI_TABLE", "1") != "0"


@dataclass
class PreparedCenters:
    """Centres + the derived data rqsid_assign reads (fp16 copy and screening-bound norms)."""
    centers: torch.Tensor      # f32 [K, D]
    c16: torch.Tensor          # int16 [K, D/32, 2, 32]: per 32-dim chunk the hi then lo fp16 terms of c 2^s
    meta: torch.Tensor         # f32 [K+1, 4]: |c|^2, |c|, |2-term residual|, |1-term residual|; row K: 2^-s
    nearest_cand: Optional["Candidates"] = None  # nearest()'s candidate list (duplicates dropped), built once
    c16h: Optional[torch.Tensor] = None  # int16 [K, D]: the hi terms alone (the 1-term streamed screens' source)

    @property
    def k(self) -> int:
        return self.centers.shape[0]

    @property
    def sqnorm(self) -> torch.Tensor:
        return self.meta[:-1, 0]


def prepare_centers(c: torch.Tensor) -> PreparedCenters:
    c = c.float().contiguous()
    _require_device(c)
    k, d = c.shape
    c16 = torch.empty((k, d // 32, 2, 32), dtype=torch.int16, device=c.device)
    meta = torch.empty((k + 1, 4), dtype=torch.float32, device=c.device)
    _lib.check(lib().rqsid_prepare_centers(_ptr(c), k, d, _ptr(c16), _ptr(meta), _stream()),
               "rqsid_prepare_centers")
    c16h = None
    if HI_TABLE and k > 0:
        c16h = torch.empty((k, d), dtype=torch.int16, device=c.device)
        _lib.check(lib().rqsid_prepare_centers_hi(_ptr(c16), k, d, _ptr(c16h), _stream()), "rqsid_prepare_centers_hi")
    return PreparedCenters(c, c16, meta, c16h=c16h)


@dataclass
class Buckets:
    """Rows grouped by segment key (counting sort), as consumed by rqsid_assign."""
    seg_row_off: torch.Tensor   # i32 [S+1]
    seg_tile_off: torch.Tensor  # i32 [S+1]
    row_index: Optional[torch.Tensor]  # i32 [N] or None (identity)
    n_segments: int
    max_tiles: int
    workspace: Optional[torch.Tensor] = None  # rqsid_bucket's workspace (its sticky error word: error_word())

    def error_word(self) -> Optional[torch.Tensor]:
        """Device view of the workspace's sticky error word (include/rqsid.h rqsid_bucket), or None."""
        return None if self.workspace is None else bucket_error_word(self.workspace, self.n_segments)


def bucket_workspace(n_segments: int, device) -> torch.Tensor:
    """A reusable rqsid_bucket workspace with its sticky error word zeroed (the caller's duty)."""
    wsb = int(lib().rqsid_bucket_workspace_bytes(0, n_segments))
    ws = torch.empty(wsb, dtype=torch.uint8, device=device)
    bucket_error_word(ws, n_segments).zero_()
    return ws


def bucket_error_word(ws: torch.Tensor, n_segments: int) -> torch.Tensor:
    return ws[8 * n_segments:8 * n_segments + 4].view(torch.int32)


def single_segment(n: int, device, rows_per_tile: Optional[int] = None) -> Buckets:
    """All n rows in one segment, identity order (layer 0 / dense prediction)."""
    tr = rows_per_tile or tile_rows()
    # built by device fills, not host copies: the encode can be captured in a HIP graph
    off = torch.arange(2, dtype=torch.int32, device=device) * n
    toff = torch.arange(2, dtype=torch.int32, device=device) * ((n + tr - 1) // tr)
    return Buckets(off, toff, None, 1, (n + tr - 1) // tr)


def bucket(keys: torch.Tensor, n_segments: int, rows_per_tile: Optional[int] = None,
           workspace: Optional[torch.Tensor] = None) -> Buckets:
    """Counting sort of rows by key.  ``workspace``: a reusable ``bucket_workspace(n_segments)`` whose sticky
    error word accumulates over calls (default: a fresh one per call)."""
    keys = keys.to(torch.int32).contiguous()
    _require_device(keys)
    n = keys.numel()
    tr = rows_per_tile or tile_rows()
    off = torch.empty(n_segments + 1, dtype=torch.int32, device=keys.device)
    toff = torch.empty(n_segments + 1, dtype=torch.int32, device=keys.device)
    idx = torch.empty(max(n, 1), dtype=torch.int32, device=keys.device)
    wsb = int(lib().rqsid_bucket_workspace_bytes(n, n_segments))
    ws = workspace if workspace is not None and workspace.numel() >= wsb else bucket_workspace(n_segments, keys.device)
    _lib.check(lib().rqsid_bucket(_ptr(keys), n, n_segments, tr, _ptr(off), _ptr(toff), _ptr(idx), _ptr(ws), wsb,
                                  _stream()), "rqsid_bucket")
    return Buckets(off, toff, idx[:n], n_segments, (n + tr - 1) // tr + n_segments, ws)


@dataclass
class Candidates:
    """Per-segment allowed centres: global index of local j = idx[base[s]+j] (idx None: base[s]+j)."""
    base: torch.Tensor          # i32 [S]
    count: torch.Tensor         # i32 [S]
    count_max: int
    idx: Optional[torch.Tensor] = None   # i32
    flags: Optional[torch.Tensor] = None  # u8 [S]
    lid: Optional[torch.Tensor] = None   # i32: local id reported for list position (None: the position)


def contiguous_candidates(n_segments: int, per_segment: int, device) -> Candidates:
    base = torch.arange(n_segments, dtype=torch.int32, device=device) * per_segment
    cnt = torch.full((n_segments,), per_segment, dtype=torch.int32, device=device)
    return Candidates(base, cnt, per_segment)


def match_to_candidates(match: torch.Tensor) -> Candidates:
    """uint8 [groups, n_cand] match matrix -> ascending allowed-column lists (+ penalty flags)."""
    match = match.to(torch.uint8).contiguous()
    _require_device(match)
    g, nc = match.shape
    base = torch.empty(g, dtype=torch.int32, device=match.device)
    cnt = torch.empty(g, dtype=torch.int32, device=match.device)
    flags = torch.empty(g, dtype=torch.uint8, device=match.device)
    idx = torch.empty(g * nc, dtype=torch.int32, device=match.device)
    wsb = int(lib().rqsid_match_workspace_bytes(g))
    ws = torch.empty(wsb, dtype=torch.uint8, device=match.device)
    _lib.check(lib().rqsid_match_to_candidates(_ptr(match), g, nc, _ptr(base), _ptr(cnt), _ptr(idx), _ptr(flags),
                                               _ptr(ws), wsb, _stream()), "rqsid_match_to_candidates")
    # the maximum allowed count decides the kernel variant; match rows are host-known data
    cmax = int((match != 0).sum(1).max().item()) if g else 0
    return Candidates(base, cnt, cmax, idx, flags)


def dedup_candidates(cand: Candidates, centers: torch.Tensor) -> Candidates:
    """Drop every list entry whose centre is bitwise identical to an EARLIER entry of the same list.

    Exact: identical centres have identical distances, and the reference's argmin returns the first
    of equal minima, so a later duplicate can never be the answer.  The kept entries report their
    original local ids through ``lid``.  Without duplicates the input is returned unchanged."""
    dev = centers.device
    canon = torch.unique(centers.float().contiguous().view(torch.int32), dim=0, return_inverse=True)[1]
    n_unique = int(canon.max().item()) + 1 if centers.shape[0] else 0
    if n_unique == centers.shape[0]:
        return cand  # no duplicate rows at all
    S = cand.base.numel()
    cnt = cand.count.long()
    total = int(cnt.sum().item())
    seg = torch.repeat_interleave(torch.arange(S, device=dev), cnt)
    off = torch.zeros(S + 1, dtype=torch.long, device=dev)
    off[1:] = torch.cumsum(cnt, 0)
    pos = torch.arange(total, device=dev) - off[seg]
    if cand.idx is None:
        glob = cand.base.long()[seg] + pos
    else:
        glob = cand.idx.long()[cand.base.long()[seg] + pos]
    lid_in = pos if cand.lid is None else cand.lid.long()[cand.base.long()[seg] + pos]
    key = seg * n_unique + canon[glob]
    first = torch.full((int(key.max().item()) + 1,), total, dtype=torch.long, device=dev)
    first.scatter_reduce_(0, key, pos + off[seg], reduce="amin")
    keep = first[key] == pos + off[seg]
    new_cnt = torch.zeros(S, dtype=torch.long, device=dev).index_add_(0, seg, keep.long())
    new_base = torch.zeros(S, dtype=torch.long, device=dev)
    new_base[1:] = torch.cumsum(new_cnt, 0)[:-1]
    return Candidates(new_base.to(torch.int32), new_cnt.to(torch.int32), int(new_cnt.max().item()) if S else 0,
                      glob[keep].to(torch.int32).contiguous(), cand.flags, lid_in[keep].to(torch.int32).contiguous())


class AssignWorkspace:
    """Re-usable scratch for rqsid_assign (rows needing an fp64 re-score)."""

    def __init__(self, n_rows: int, device):
        self.bytes = int(lib().rqsid_assign_workspace_bytes(n_rows))
        self.buf = torch.empty(self.bytes, dtype=torch.uint8, device=device)
        self.buf[240:256].zero_()  # the sticky error word (include/rqsid.h)
        self.n_rows = n_rows

    def rescored(self) -> int:
        """Rows re-scored in fp64 by the last assign (host sync)."""
        return int(self.buf[:4].view(torch.int32).item())

    def error(self) -> int:
        """Sticky error word of every assign on this workspace (host sync; csrc/assign_common.h kErrSlot):
        bit 0 compaction past n_rows, bit 1 overflow list past n_rows, bit 2 a list entry outside work[],
        bit 3 a tile count past the tile maps / descriptors (clamped). Every such write or count is bounded by
        its slot's capacity; a non-zero word means one was dropped."""
        return int(self.error_word().item())

    def error_word(self) -> torch.Tensor:
        return self.buf[240:244].view(torch.int32)


def check_error_words(words, what: str, meaning: Optional[str] = None) -> None:
    """One host sync over device error words (AssignWorkspace / Buckets / QuantErrorWorkspace); raise if any is
    non-zero: a counter-driven write was dropped, so the IDs of that call are not trustworthy (``meaning``: what a
    set word says when it is not one of those)."""
    ws = [w for w in words if w is not None]
    if not ws:
        return
    vals = torch.cat(ws).cpu().tolist()
    if any(vals):
        raise RuntimeError(f"{what}: a device error word is set ({vals}): " + (meaning or (
            "a counter-driven list write fell outside "
            "its slot and was dropped (csrc/assign_common.h kErrSlot, rqsid_bucket)")))


@dataclass
class FusedResidual:
    """On-the-fly residual chain for rqsid_assign (res_levels 1 or 2, one dimension group).
    The subtracted centres are per SEGMENT s (the segment of a level determines its parents):

    levels=1: v = x - ca[seg_ca[s]]            (normalize: / (||v|| + 1e-8), written to den_out)
    levels=2: v = (x - ca[seg_ca[s]])[/den_in] - cb[seg_cb[s]]   (normalize: / (||v|| + 1e-8))
    seg_ca None = identity (segment s subtracts ca[s])."""
    levels: int
    normalize: bool
    ca: torch.Tensor
    seg_ca: Optional[torch.Tensor] = None
    cb: Optional[torch.Tensor] = None
    seg_cb: Optional[torch.Tensor] = None
    den_in: Optional[torch.Tensor] = None
    den_out: Optional[torch.Tensor] = None


PAIR_CAND = 128  # kPairCand: the widest segment list a pair table covers


def pair_table(pc: PreparedCenters, cand: Candidates) -> Optional[torch.Tensor]:
    """The pair table of a level's segment lists (rqsid_pair_table: fp16 upper bounds of |c_j - c_k| per list),
    for ``assign(..., pair=...)``; None where a list is wider than PAIR_CAND.  Build it once per codebook and
    candidate lists (after any dedup_candidates): 32 KiB per segment."""
    if cand.count_max > PAIR_CAND or cand.count_max <= 0:
        return None
    _require_device(pc.centers, cand.base, cand.count, cand.idx)
    n_seg = cand.base.numel()
    t = torch.empty(int(lib().rqsid_pair_table_bytes(n_seg)) // 2, dtype=torch.int16, device=pc.centers.device)
    _lib.check(lib().rqsid_pair_table(_ptr(pc.centers), pc.centers.shape[1], _ptr(pc.meta), pc.k, n_seg, _ptr(cand.base),
                                      _ptr(cand.count), cand.count_max, _ptr(cand.idx), _ptr(t), _stream()),
               "rqsid_pair_table")
    return t


def assign_plan_pair(x: torch.Tensor, buckets: Buckets, cand: Candidates, fused: Optional[FusedResidual] = None,
                     screen_terms: int = 0, pair: Optional[torch.Tensor] = None) -> bool:
    """True if ``assign`` with these arguments runs the 2-term pairwise screen (host-only query of the plan)."""
    f = fused
    return bool(lib().rqsid_assign_plan_pair(
        ROW_FORMATS[x.dtype], x.shape[0], x.shape[1], buckets.n_segments, cand.count_max,
        0 if f is None else f.levels, 0 if f is None else int(f.normalize), int(screen_terms),
        int(cand.lid is not None), int(f is not None and f.den_out is not None), int(pair is not None)))


def assign(x: torch.Tensor, pc: PreparedCenters, buckets: Buckets, cand: Candidates,
           out_local: Optional[torch.Tensor] = None, out_global: Optional[torch.Tensor] = None,
           workspace: Optional[AssignWorkspace] = None, fused: Optional[FusedResidual] = None,
           screen_terms: int = 0, pair: Optional[torch.Tensor] = None):
    """Exact segmented argmin. Returns (local i32[N], global i32[N]).  ``screen_terms`` (0 auto, 1, 2, 3)
    only changes how much work the exact answer takes.  ``x``: float32, or float16 / bfloat16 rows, which
    the kernels read as they are (rqsid_assign_x: no fp32 copy; IDs bit-identical to ``x.float()``).
    ``pair``: ``pair_table(pc, cand)`` of the same centres and lists; with it the 3-term levels of fp32 rows run
    the 2-term pairwise screen (rqsid_assign_pair), and ``screen_terms=2`` asks for that form."""
    _require_device(x, pc.centers, cand.base, cand.count, cand.idx, cand.flags)
    x_format = ROW_FORMATS.get(x.dtype)
    if x_format is None:
        raise ValueError(f"rqsid_assign reads float32, float16 or bfloat16 rows, not {x.dtype}")
    n, d = x.shape
    if d != pc.centers.shape[1]:
        raise ValueError(f"dimension mismatch: x has {d}, centres {pc.centers.shape[1]}")
    dev = x.device
    if out_local is None:
        out_local = torch.empty(n, dtype=torch.int32, device=dev)
    if out_global is None:
        out_global = torch.empty(n, dtype=torch.int32, device=dev)
    if workspace is None or workspace.n_rows < n:
        workspace = AssignWorkspace(n, dev)
    f = fused
    if f is not None:
        _require_device(f.ca, f.seg_ca, f.cb, f.seg_cb, f.den_in, f.den_out)
    tail = ()
    if pair is not None:
        _require_device(pair)
        if pair.numel() * pair.element_size() < int(lib().rqsid_pair_table_bytes(buckets.n_segments)):
            raise ValueError("pair table smaller than rqsid_pair_table_bytes(n_segments)")
        fn, head, tail, what = lib().rqsid_assign_pair, (x_format,), (_ptr(pair),), "rqsid_assign_pair"
    elif x_format == 0:
        fn, head, what = lib().rqsid_assign, (), "rqsid_assign"
    else:
        fn, head, what = lib().rqsid_assign_x, (x_format,), "rqsid_assign_x"
    _lib.check(fn(
        _ptr(x), *head, n, d, _ptr(buckets.row_index), buckets.n_segments, _ptr(buckets.seg_row_off),
        _ptr(buckets.seg_tile_off), buckets.max_tiles,
        _ptr(pc.centers), _ptr(pc.c16), _ptr(pc.c16h), _ptr(pc.meta), pc.k,
        _ptr(cand.base), _ptr(cand.count), cand.count_max, _ptr(cand.idx), _ptr(cand.lid), _ptr(cand.flags),
        0 if f is None else f.levels, 0 if f is None else int(f.normalize),
        None if f is None else _ptr(f.ca), None if f is None else _ptr(f.seg_ca),
        None if f is None else _ptr(f.cb), None if f is None else _ptr(f.seg_cb),
        None if f is None else _ptr(f.den_in), None if f is None else _ptr(f.den_out),
        _ptr(out_local), _ptr(out_global), int(screen_terms), _ptr(workspace.buf), workspace.bytes, _stream(), *tail),
        what)
    return out_local, out_global


def nearest(x: torch.Tensor, pc: PreparedCenters, workspace: Optional[AssignWorkspace] = None,
            screen_terms: int = 0) -> torch.Tensor:
    """Unconstrained nearest centre (KMeans.predict / pairwise_distance_full + argmin)."""
    n = x.shape[0]
    b = single_segment(n, x.device)
    if pc.nearest_cand is None:
        cand = Candidates(torch.zeros(1, dtype=torch.int32, device=x.device),
                          torch.full((1,), pc.k, dtype=torch.int32, device=x.device), pc.k)
        # bitwise-duplicate centres (e.g. several K-Means centres initialised from equal rows): only the
        # first copy can be the argmin, and with the copies in the list every row nearest to them is an
        # exact > 8-way tie that no screen can split, i.e. an all-candidate fp64 re-score
        pc.nearest_cand = dedup_candidates(cand, pc.centers) if pc.k > kMaxList else cand
    return assign(x, pc, b, pc.nearest_cand, workspace=workspace, screen_terms=screen_terms)[1]

TOPK_MAX = 8  # RQSID_TOPK_MAX (include/rqsid.h)
TOPK_WORD = ("1: the device tile count exceeded max_tiles (tiles beyond were not ranked), 2: a row position or "
             "row_index entry outside the rows (skipped), 4: a candidate's centre row outside the table "
             "(include/rqsid.h rqsid_assign_topk)")


class TopKWorkspace:
    """Header of rqsid_assign_topk: bytes [0, 4) the sticky error word (zeroed here once, never by a call), bytes
    [4, 16) the three per-call counters."""

    def __init__(self, n_rows: int, k: int, device):
        self.bytes = int(lib().rqsid_assign_topk_workspace_bytes(n_rows, k))
        self.buf = torch.empty(self.bytes, dtype=torch.uint8, device=device)
        self.buf[:16].zero_()
        self.n_rows, self.k = n_rows, k

    def error_word(self) -> torch.Tensor:
        return self.buf[:4].view(torch.int32)

    def counters(self) -> dict:
        """The last call's counters (host sync): rows ranked from their list, rows that took the all-candidate
        pass, non-finite rows."""
        a, b, c = self.buf[4:16].view(torch.int32).tolist()
        return {"listed_rows": a, "all_candidate_rows": b, "nonfinite_rows": c}


def assign_topk(x: torch.Tensor, pc: PreparedCenters, buckets: Buckets, cand: Candidates, k: int,
                fused: Optional[FusedResidual] = None, workspace: Optional[TopKWorkspace] = None,
                check: Optional[bool] = None, out=None):
    """The k nearest allowed centres of every row (include/rqsid.h rqsid_assign_topk): ``(local, global, dist)``,
    i32 / i32 / f32 [N, k], slot t = the t-th smallest (fp64 squared distance, list position).  ``cand`` is ranked as
    given: pass the list before any removal of duplicate centres.  ``x``, ``buckets``, ``cand`` and ``fused`` as in
    ``assign``.  ``check`` (default: on unless the stream is being captured): read the workspace's error word after
    the call (one host sync) and raise RuntimeError if it is set.  ``out``: three [N, k] tensors to write into."""
    if check is None:
        check = not torch.cuda.is_current_stream_capturing()
    _require_device(x, pc.centers, cand.base, cand.count, cand.idx, cand.flags, cand.lid)
    x_format = ROW_FORMATS.get(x.dtype)
    if x_format is None:
        raise ValueError(f"rqsid_assign reads float32, float16 or bfloat16 rows, not {x.dtype}")
    n, d = x.shape
    if d != pc.centers.shape[1]:
        raise ValueError(f"dimension mismatch: x has {d}, centres {pc.centers.shape[1]}")
    k = int(k)
    if not 1 <= k <= TOPK_MAX:
        raise ValueError(f"rqsid_assign_topk: k = {k} (1..{TOPK_MAX})")
    dev = x.device
    if out is None:
        out = (torch.empty((n, k), dtype=torch.int32, device=dev), torch.empty((n, k), dtype=torch.int32, device=dev),
               torch.empty((n, k), dtype=torch.float32, device=dev))
    loc, glob, dist = out
    _require_device(loc, glob, dist)
    if workspace is None:
        workspace = TopKWorkspace(n, k, dev)
    f = fused
    if f is not None:
        _require_device(f.ca, f.seg_ca, f.cb, f.seg_cb, f.den_in, f.den_out)
    _lib.check(lib().rqsid_assign_topk(
        _ptr(x), x_format, n, d, _ptr(buckets.row_index), buckets.n_segments, _ptr(buckets.seg_row_off),
        _ptr(buckets.seg_tile_off), buckets.max_tiles, _ptr(pc.centers), _ptr(pc.meta), pc.k,
        _ptr(cand.base), _ptr(cand.count), cand.count_max, _ptr(cand.idx), _ptr(cand.lid), _ptr(cand.flags),
        0 if f is None else f.levels, 0 if f is None else int(f.normalize),
        None if f is None else _ptr(f.ca), None if f is None else _ptr(f.seg_ca),
        None if f is None else _ptr(f.cb), None if f is None else _ptr(f.seg_cb),
        None if f is None else _ptr(f.den_in), None if f is None else _ptr(f.den_out),
        k, _ptr(loc), _ptr(glob), _ptr(dist), _ptr(workspace.buf), workspace.bytes, _stream()), "rqsid_assign_topk")
    if check:
        check_error_words([workspace.error_word()], "rqsid_assign_topk", TOPK_WORD)
    return loc, glob, dist


def nearest_topk(x: torch.Tensor, pc: PreparedCenters, k: int, workspace: Optional[TopKWorkspace] = None,
                 check: Optional[bool] = None):
    """The k nearest of ALL centres of ``pc`` per row, one segment: ``(local, global, dist)`` [N, k] (local ==
    global).  The raw table is
    ranked (not ``pc.nearest_cand``, whose duplicate centres are removed: a duplicate is a valid second place)."""
    n = x.shape[0]
    cand = Candidates(torch.zeros(1, dtype=torch.int32, device=x.device),
                      torch.full((1,), pc.k, dtype=torch.int32, device=x.device), pc.k)
    return assign_topk(x, pc, single_segment(n, x.device), cand, k, workspace=workspace, check=check)


class BeamWorkspace:
    """Header of rqsid_beam_expand, laid out as rqsid_assign_topk's: bytes [0, 4) the sticky error word (zeroed here
    once, never by a call), bytes [4, 16) the three per-call counters (they count items)."""

    def __init__(self, n_items: int, k: int, device):
        self.bytes = int(lib().rqsid_beam_expand_workspace_bytes(n_items, k))
        self.buf = torch.empty(self.bytes, dtype=torch.uint8, device=device)
        self.buf[:16].zero_()
        self.n_items, self.k = n_items, k

    def error_word(self) -> torch.Tensor:
        return self.buf[:4].view(torch.int32)

    def counters(self) -> dict:
        """The last call's counters (host sync): items ranked from their list, items that took the all-candidate
        pass, non-finite items."""
        a, b, c = self.buf[4:16].view(torch.int32).tolist()
        return {"listed_rows": a, "all_candidate_rows": b, "nonfinite_rows": c}


def beam_expand(x: torch.Tensor, beam: int, pc: PreparedCenters, buckets: Buckets, cand: Candidates, k: int,
                fused: Optional[FusedResidual] = None, workspace: Optional[BeamWorkspace] = None,
                check: Optional[bool] = None, out=None):
    """``assign_topk`` over ``N * beam`` items, item ``i`` (hypothesis ``i % beam`` of row ``i // beam``) reading row
    ``i // beam`` of ``x`` [N, D] (include/rqsid.h rqsid_beam_expand): ``(local, global, dist)`` [N * beam, k].
    ``buckets`` group the ITEMS by their hypothesis's segment (dead items in one extra segment whose ``cand.count`` is
    0); ``fused.den_in`` / ``fused.den_out`` are per item, and ``den_out`` is written at levels 1 and 2.  ``check``,
    ``out`` as in ``assign_topk``."""
    if check is None:
        check = not torch.cuda.is_current_stream_capturing()
    _require_device(x, pc.centers, cand.base, cand.count, cand.idx, cand.flags, cand.lid)
    x_format = ROW_FORMATS.get(x.dtype)
    if x_format is None:
        raise ValueError(f"rqsid_beam_expand reads float32, float16 or bfloat16 rows, not {x.dtype}")
    n, d = x.shape
    if d != pc.centers.shape[1]:
        raise ValueError(f"dimension mismatch: x has {d}, centres {pc.centers.shape[1]}")
    k, beam = int(k), int(beam)
    if not 1 <= k <= TOPK_MAX or not 1 <= beam <= TOPK_MAX:
        raise ValueError(f"rqsid_beam_expand: k = {k}, beam = {beam} (1..{TOPK_MAX})")
    items = n * beam
    dev = x.device
    if out is None:
        out = (torch.empty((items, k), dtype=torch.int32, device=dev),
               torch.empty((items, k), dtype=torch.int32, device=dev),
               torch.empty((items, k), dtype=torch.float32, device=dev))
    loc, glob, dist = out
    _require_device(loc, glob, dist)
    if min(loc.numel(), glob.numel(), dist.numel()) < items * k:
        raise ValueError("rqsid_beam_expand: an output holds fewer than N * beam * k values")
    if workspace is None:
        workspace = BeamWorkspace(items, k, dev)
    f = fused
    if f is not None:
        _require_device(f.ca, f.seg_ca, f.cb, f.seg_cb, f.den_in, f.den_out)
        for t in (f.den_in, f.den_out):
            if t is not None and t.numel() < items:
                raise ValueError("rqsid_beam_expand: den_in / den_out are per item (N * beam values)")
    _lib.check(lib().rqsid_beam_expand(
        _ptr(x), x_format, items, beam, d, _ptr(buckets.row_index), buckets.n_segments, _ptr(buckets.seg_row_off),
        _ptr(buckets.seg_tile_off), buckets.max_tiles, _ptr(pc.centers), _ptr(pc.meta), pc.k,
        _ptr(cand.base), _ptr(cand.count), cand.count_max, _ptr(cand.idx), _ptr(cand.lid), _ptr(cand.flags),
        0 if f is None else f.levels, 0 if f is None else int(f.normalize),
        None if f is None else _ptr(f.ca), None if f is None else _ptr(f.seg_ca),
        None if f is None else _ptr(f.cb), None if f is None else _ptr(f.seg_cb),
        None if f is None else _ptr(f.den_in), None if f is None else _ptr(f.den_out),
        k, _ptr(loc), _ptr(glob), _ptr(dist), _ptr(workspace.buf), workspace.bytes, _stream()), "rqsid_beam_expand")
    if check:
        check_error_words([workspace.error_word()], "rqsid_beam_expand", TOPK_WORD)
    return loc, glob, dist


@dataclass
class BeamStep:
    """What ``beam_merge`` writes, per output item ``row * beam_out + t`` (include/rqsid.h rqsid_beam_merge)."""
    path: torch.Tensor      # i32 [N * beam_out, level + 1]; -1 in a dead slot
    scale: torch.Tensor     # f32: S_l of the slot's parent
    den_next: torch.Tensor  # f32: the parent's divisor (the next level's den_in)
    rec: torch.Tensor       # f32: fl32(S_l d), +inf in a dead slot, NaN in a non-finite row
    key: torch.Tensor       # i32: the next level's segment key (dead_key in a dead slot)
    src: torch.Tensor       # i32: parent * k + place, -1 in a dead slot


def beam_merge(n_rows: int, beam_in: int, k: int, beam_out: int, level: int, exp_local: torch.Tensor,
               exp_global: torch.Tensor, exp_dist: torch.Tensor, scale_in: Optional[torch.Tensor] = None,
               den: Optional[torch.Tensor] = None, path_in: Optional[torch.Tensor] = None, use_global: bool = False,
               key_mult: int = 0, dead_key: int = 0, out: Optional[BeamStep] = None) -> BeamStep:
    """Per row, the next beam out of the ``beam_in * k`` expansions (include/rqsid.h rqsid_beam_merge): slot 0 the
    greedy continuation, the others by ascending (rec, parent, place).  A pure function of its inputs (no workspace,
    no error word).  ``out``: a ``BeamStep`` of buffers to write into."""
    _require_device(exp_local, exp_global, exp_dist, scale_in, den, path_in)
    n_rows, beam_in, k, beam_out, level = int(n_rows), int(beam_in), int(k), int(beam_out), int(level)
    n_in = n_rows * beam_in
    for t, dt in ((exp_local, torch.int32), (exp_global, torch.int32), (exp_dist, torch.float32)):
        if t.dtype != dt or t.numel() < n_in * k:
            raise ValueError("rqsid_beam_merge: the expansions are int32 / int32 / float32 [N * beam_in, k]")
    for t in (scale_in, den):
        if t is not None and (t.dtype != torch.float32 or t.numel() < n_in):
            raise ValueError("rqsid_beam_merge: scale_in / den are float32 [N * beam_in]")
    if level >= 1 and (path_in is None or path_in.dtype != torch.int32 or path_in.numel() < n_in * level):
        raise ValueError("rqsid_beam_merge: path_in is int32 [N * beam_in, level]")
    dev = exp_dist.device
    n_out = n_rows * max(beam_out, 0)
    if out is None:
        out = BeamStep(torch.empty((n_out, level + 1), dtype=torch.int32, device=dev),
                       torch.empty(n_out, dtype=torch.float32, device=dev),
                       torch.empty(n_out, dtype=torch.float32, device=dev),
                       torch.empty(n_out, dtype=torch.float32, device=dev),
                       torch.empty(n_out, dtype=torch.int32, device=dev),
                       torch.empty(n_out, dtype=torch.int32, device=dev))
    _require_device(out.path, out.scale, out.den_next, out.rec, out.key, out.src)
    _lib.check(lib().rqsid_beam_merge(
        n_rows, beam_in, k, beam_out, level, _ptr(exp_local), _ptr(exp_global), _ptr(exp_dist), _ptr(scale_in),
        _ptr(den), _ptr(path_in), int(bool(use_global)), int(key_mult), int(dead_key), _ptr(out.path),
        _ptr(out.scale), _ptr(out.den_next), _ptr(out.rec), _ptr(out.key), _ptr(out.src), _stream()),
        "rqsid_beam_merge")
    return out


def with_dead_segment(cand: Candidates) -> Candidates:
    """``cand`` plus one last segment without candidates and without the penalty flag: where ``beam_expand`` keeps
    the dead items (every slot -1 / -1 / +inf)."""
    dev = cand.base.device
    z = torch.zeros(1, dtype=torch.int32, device=dev)
    flags = None if cand.flags is None else torch.cat([cand.flags, torch.zeros(1, dtype=torch.uint8, device=dev)])
    return Candidates(torch.cat([cand.base, z]), torch.cat([cand.count, z]), cand.count_max, cand.idx, flags, cand.lid)


MAX_GROUPS = 16  # kMaxGroups (csrc/rqsid.hip)


def _groups_tensor(group_dims: Sequence[int], device, dim: Optional[int] = None, who: str = "") -> torch.Tensor:
    """The dimension groups as a device tensor.  With ``dim``: the widths must be positive, at most MAX_GROUPS and
    sum to dim (the kernels give whatever lies past the listed widths to the last group)."""
    gd = [int(g) for g in group_dims]
    if dim is not None:
        if not 1 <= len(gd) <= MAX_GROUPS:
            raise ValueError("%s: %d dimension groups (1 .. %d are supported)" % (who, len(gd), MAX_GROUPS))
        if min(gd) <= 0 or sum(gd) != dim:
            raise ValueError("%s: group_dims %s do not split the %d dimensions" % (who, gd, dim))
    return torch.tensor(gd, dtype=torch.int32, device=device)


def residual(x: torch.Tensor, centers: torch.Tensor, ids: torch.Tensor, group_dims: Sequence[int] = (),
             normalize: bool = True, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    _require_f32("residual", x, out)
    ids = ids.to(torch.int32).contiguous()
    centers = centers.float().contiguous()
    _require_device(x, centers, ids, out)
    n, d = x.shape
    if out is None:
        out = torch.empty_like(x)
    gd = list(group_dims) or [d]
    g = _groups_tensor(gd, x.device, d if normalize else None, "residual")
    _lib.check(lib().rqsid_residual(_ptr(x), n, d, _ptr(centers), centers.shape[0], _ptr(ids), _ptr(g), len(gd), int(normalize),
                                    _ptr(out), _stream()), "rqsid_residual")
    return out


QUANT_ERROR_WORD = ("1: an id lies outside its codebook (that row's err is NaN from that level on and it is left out "
                    "of the sums), 2: a row_order entry lies outside the rows (include/rqsid.h rqsid_quant_error)")


class QuantErrorWorkspace:
    """Scratch of rqsid_quant_error: per-block fp64 partial sums and, in bytes [0, 4), the sticky error word
    (1: an id outside its codebook, 2: a row_order entry outside the rows), zeroed here once."""

    def __init__(self, n_rows: int, device):
        self.bytes = int(lib().rqsid_quant_error_workspace_bytes(n_rows))
        self.buf = torch.empty(self.bytes, dtype=torch.uint8, device=device)
        self.buf[:256].zero_()
        self.n_rows = n_rows

    def error_word(self) -> torch.Tensor:
        return self.buf[:4].view(torch.int32)


def quant_error(x: torch.Tensor, centers: Sequence[torch.Tensor], ids: Sequence[torch.Tensor],
                normalize: bool = True, row_order: Optional[torch.Tensor] = None, want_x_norm: bool = True,
                want_sums: bool = True, workspace: Optional[QuantErrorWorkspace] = None,
                check: Optional[bool] = None):
    """Quantisation error of an encoding in one pass over the rows (include/rqsid.h rqsid_quant_error).

    ``x``: float32 / float16 / bfloat16 [N, D]; ``centers[l]``: f32 [K_l, D]; ``ids[l]``: i32 [N], the GLOBAL row of
    ``centers[l]`` each row was given; ``row_order``: i32 [N] permutation that only sets the processing order.
    Returns ``(err, x_norm, sums)``: err f32 [N, L] (a transposed view of the level-major buffer), x_norm f32 [N]
    or None, sums f64 [L + 1] or None.  ``check`` (default: on unless the stream is being captured): read the
    workspace's error word after the call (one host sync) and raise RuntimeError if an id was out of range."""
    if check is None:
        check = not torch.cuda.is_current_stream_capturing()
    L = len(centers)
    if L != len(ids) or not 1 <= L <= 3:
        raise ValueError(f"rqsid_quant_error takes 1..3 levels with one id vector each, not {L} / {len(ids)}")
    x_format = ROW_FORMATS.get(x.dtype)
    if x_format is None:
        raise ValueError(f"rqsid_quant_error reads float32, float16 or bfloat16 rows, not {x.dtype}")
    _require_device(x, row_order, *centers, *ids)
    n, d = x.shape
    for c, i in zip(centers, ids):
        if c.dtype != torch.float32 or c.dim() != 2 or c.shape[1] != d:
            raise ValueError("rqsid_quant_error: centres must be float32 [K, D] with the rows' D")
        if i.dtype != torch.int32 or i.numel() != n:
            raise ValueError("rqsid_quant_error: ids must be int32 [N]")
    if row_order is not None and (row_order.dtype != torch.int32 or row_order.numel() != n):
        raise ValueError("rqsid_quant_error: row_order must be int32 [N]")
    dev = x.device
    err = torch.empty((L, n), dtype=torch.float32, device=dev)
    x_norm = torch.empty(n, dtype=torch.float32, device=dev) if want_x_norm else None
    sums = torch.empty(L + 1, dtype=torch.float64, device=dev) if want_sums else None
    if workspace is None:
        workspace = QuantErrorWorkspace(n, dev)
    lv = []
    for l in range(3):
        lv += [_ptr(centers[l]), centers[l].shape[0], _ptr(ids[l])] if l < L else [None, 0, None]
    _lib.check(lib().rqsid_quant_error(_ptr(x), x_format, n, d, _ptr(row_order), L, int(normalize), *lv,
                                       _ptr(err), _ptr(x_norm), _ptr(sums), _ptr(workspace.buf), workspace.bytes,
                                       _stream()), "rqsid_quant_error")
    if check:
        check_error_words([workspace.error_word()], "rqsid_quant_error", QUANT_ERROR_WORD)
    return err.t(), x_norm, sums


class _RowPairWorkspace:
    """What the workspaces of rqsid_silhouette and rqsid_row_knn share: ``bytes`` from the entry's size query,
    ``buf``, and its 256-byte header, zeroed here once, whose bytes [0, 4) are the sticky error word (1: a row_index /
    query_self entry outside the rows, 2: a query_seg entry outside [-1, n_segments), 4: a seg_row_off entry outside
    [0, n_rows] or decreasing)."""

    def __init__(self, what: str, size: int, device):
        self.bytes = int(size)
        if self.bytes < 0:
            _lib.check(self.bytes, what)
        self.buf = torch.empty(max(self.bytes, 256), dtype=torch.uint8, device=device)
        self.buf[:256].zero_()

    def error_word(self) -> torch.Tensor:
        return self.buf[:4].view(torch.int32)


class SilhouetteWorkspace(_RowPairWorkspace):
    """Scratch of rqsid_silhouette: squared norms of rows and queries and one record per query and chunk."""

    def __init__(self, n_rows: int, n_queries: int, device, chunk_rows: int = 0):
        super().__init__("rqsid_silhouette_workspace_bytes",
                         lib().rqsid_silhouette_workspace_bytes(n_rows, n_queries, chunk_rows), device)
        self.n_rows, self.n_queries, self.chunk_rows = n_rows, n_queries, chunk_rows


SILHOUETTE_WORD = ("bit 1: a row_index or query_self entry outside [0, n_rows) was skipped; bit 2: a query_seg entry "
                   "outside [-1, n_segments) was taken as -1; bit 4: a seg_row_off entry outside [0, n_rows] or "
                   "decreasing was clamped (include/rqsid.h rqsid_silhouette)")


def _row_pair_args(who: str, x, q, order, seg_row_off, query_self, query_seg, seg_optional: bool):
    """The tensors rqsid_silhouette and rqsid_row_knn share, validated: ``(x_format, N, D, M)``.  ``seg_optional``:
    ``seg_row_off`` may be None (and ``query_seg`` then has to be)."""
    x_format = ROW_FORMATS.get(x.dtype)
    if x_format is None:
        raise ValueError(f"{who} reads float32, float16 or bfloat16 rows, not {x.dtype}")
    if x.dim() != 2 or q.dim() != 2 or q.shape[1] != x.shape[1] or q.dtype != x.dtype:
        raise ValueError(f"{who}: x [N, D] and q [M, D] must share dtype and D")
    _require_device(x, q, order, seg_row_off, query_self, query_seg)
    n, d = x.shape
    m = q.shape[0]
    if order is not None and (order.dtype != torch.int32 or order.numel() != n):
        raise ValueError(f"{who}: order must be int32 [N]")
    if not (seg_optional and seg_row_off is None) and (
            seg_row_off.dtype != torch.int32 or seg_row_off.dim() != 1 or seg_row_off.numel() < 2):
        raise ValueError(f"{who}: seg_row_off must be int32 [S + 1]")
    if query_seg is not None and seg_row_off is None:
        raise ValueError(f"{who}: query_seg needs seg_row_off")
    for name, t in (("query_self", query_self), ("query_seg", query_seg)):
        if t is not None and (t.dtype != torch.int32 or t.numel() != m):
            raise ValueError(f"{who}: {name} must be int32 [M]")
    return x_format, n, d, m


def silhouette_tile_rows() -> int:
    return int(lib().rqsid_silhouette_tile_rows())


def silhouette(x: torch.Tensor, order: Optional[torch.Tensor], seg_row_off: torch.Tensor, q: torch.Tensor,
               query_self: Optional[torch.Tensor], query_seg: Optional[torch.Tensor], chunk_rows: int = 0,
               workspace: Optional[SilhouetteWorkspace] = None, check: Optional[bool] = None):
    """Exact silhouette sums of the rows ``q`` against the clusters of ``x`` (include/rqsid.h rqsid_silhouette).

    ``x``: float32 / float16 / bfloat16 [N, D]; ``order``: i32 [N], the rows grouped by cluster (``Buckets.row_index``;
    None = identity); ``seg_row_off``: i32 [S + 1]; ``q``: [M, D] of x's dtype; ``query_self``: i32 [M], the row of x
    that is the query, or -1 (None = all -1); ``query_seg``: i32 [M], the query's own cluster, or -1 (None = all -1).
    Returns ``(a, b, b_seg, s)``: f32 [M], f32 [M], i32 [M], f32 [M].  ``check`` (default: on unless the stream is being
    captured): read the workspace's error word after the call (one host sync) and raise if a table entry was clamped."""
    if check is None:
        check = not torch.cuda.is_current_stream_capturing()
    x_format, n, d, m = _row_pair_args("rqsid_silhouette", x, q, order, seg_row_off, query_self, query_seg, False)
    dev = x.device
    a = torch.empty(m, dtype=torch.float32, device=dev)
    b = torch.empty(m, dtype=torch.float32, device=dev)
    b_seg = torch.empty(m, dtype=torch.int32, device=dev)
    s = torch.empty(m, dtype=torch.float32, device=dev)
    if workspace is None or workspace.bytes < int(lib().rqsid_silhouette_workspace_bytes(n, m, chunk_rows)):
        workspace = SilhouetteWorkspace(n, m, dev, chunk_rows)
    _lib.check(lib().rqsid_silhouette(_ptr(x), x_format, n, d, _ptr(order), seg_row_off.numel() - 1, _ptr(seg_row_off),
                                      _ptr(q), m, _ptr(query_self), _ptr(query_seg), chunk_rows, _ptr(a), _ptr(b),
                                      _ptr(b_seg), _ptr(s), _ptr(workspace.buf), workspace.bytes, _stream()),
               "rqsid_silhouette")
    if check:
        check_error_words([workspace.error_word()], "rqsid_silhouette", SILHOUETTE_WORD)
    return a, b, b_seg, s


KNN_MAX = 16
KNN_METRICS = {"l2": 0, "cosine": 1}


class RowKnnWorkspace(_RowPairWorkspace):
    """Scratch of rqsid_row_knn: the norm terms of rows and queries, one list of k + 8 (value, row) pairs and one
    record per query and chunk; bytes [4, 16) of the header are the call's three counters."""

    def __init__(self, n_rows: int, n_queries: int, k: int, device, chunk_rows: int = 0):
        super().__init__("rqsid_row_knn_workspace_bytes",
                         lib().rqsid_row_knn_workspace_bytes(n_rows, n_queries, k, chunk_rows), device)
        self.n_rows, self.n_queries, self.k, self.chunk_rows = n_rows, n_queries, k, chunk_rows

    def counters(self) -> dict:
        """Of the last call (one host sync): queries ranked from their lists alone, (query, chunk) pairs that took
        the all-rows pass, queries without an answer."""
        c = self.buf[4:16].view(torch.int32).tolist()
        return {"from_lists": c[0], "all_rows_pairs": c[1], "non_finite_queries": c[2]}


def row_knn_tile_rows() -> int:
    return int(lib().rqsid_row_knn_tile_rows())


def row_knn(x: torch.Tensor, q: torch.Tensor, k: int, metric: str = "l2", order: Optional[torch.Tensor] = None,
            seg_row_off: Optional[torch.Tensor] = None, query_self: Optional[torch.Tensor] = None,
            query_seg: Optional[torch.Tensor] = None, chunk_rows: int = 0,
            workspace: Optional[RowKnnWorkspace] = None, check: Optional[bool] = None):
    """The exact k nearest rows of ``x`` for every row of ``q`` (include/rqsid.h rqsid_row_knn).

    ``x``: float32 / float16 / bfloat16 [N, D]; ``q``: [M, D] of x's dtype; ``metric``: "l2" or "cosine"; ``order``:
    i32 [N], the rows grouped by segment (``Buckets.row_index``; None = identity); ``seg_row_off``: i32 [S + 1] or
    None (no segments: every query searches every row); ``query_self``: i32 [M], the row of x that is the query, or
    -1 (None = all -1); ``query_seg``: i32 [M], the segment the query searches, or -1 for every row (None = all -1).
    Returns ``(rows, val)``: i32 [M, k], f32 [M, k] (distance or cosine similarity; -1 / +inf past the eligible
    rows).  ``check`` (default: on unless the stream is being captured): read the workspace's error word after the
    call (one host sync) and raise if a table entry was clamped."""
    if check is None:
        check = not torch.cuda.is_current_stream_capturing()
    if metric not in KNN_METRICS:
        raise ValueError(f"rqsid_row_knn: metric must be 'l2' or 'cosine', not {metric!r}")
    if not 1 <= int(k) <= KNN_MAX:
        raise ValueError(f"rqsid_row_knn: k must lie in 1..{KNN_MAX}, not {k}")
    x_format, n, d, m = _row_pair_args("rqsid_row_knn", x, q, order, seg_row_off, query_self, query_seg, True)
    dev = x.device
    rows = torch.empty((m, k), dtype=torch.int32, device=dev)
    val = torch.empty((m, k), dtype=torch.float32, device=dev)
    need = int(lib().rqsid_row_knn_workspace_bytes(n, m, k, chunk_rows))
    if need < 0:
        _lib.check(need, "rqsid_row_knn_workspace_bytes")
    if workspace is None or workspace.bytes < need:
        workspace = RowKnnWorkspace(n, m, k, dev, chunk_rows)
    n_seg = 0 if seg_row_off is None else seg_row_off.numel() - 1
    _lib.check(lib().rqsid_row_knn(_ptr(x), x_format, n, d, _ptr(order), n_seg, _ptr(seg_row_off), _ptr(q), m,
                                   _ptr(query_self), _ptr(query_seg), KNN_METRICS[metric], int(k), chunk_rows,
                                   _ptr(rows), _ptr(val), _ptr(workspace.buf), workspace.bytes, _stream()),
               "rqsid_row_knn")
    if check:
        check_error_words([workspace.error_word()], "rqsid_row_knn", SILHOUETTE_WORD)
    return rows, val


PROBE_MAX = 32  # RQSID_PROBE_MAX
PROBE_KNN_WORD = ("bit 1: a row_index or query_self entry outside [0, n_rows) was skipped; bit 4: a probe range end "
                  "outside [0, n_rows] or lo > hi was clamped (lo > hi: empty); bit 8: two ranges of one query "
                  "overlapped and the one with the higher probe index was dropped for that query "
                  "(include/rqsid.h rqsid_probe_knn)")


class ProbeKnnWorkspace(_RowPairWorkspace):
    """Scratch of rqsid_probe_knn: the norm terms of rows and queries, the cleaned ranges, the items' order and one
    list of k + 8 (value, row) pairs and one record per (query, probe) item; bytes [4, 20) of the header are the
    call's four counters."""

    def __init__(self, n_rows: int, n_queries: int, n_probes: int, k: int, device):
        super().__init__("rqsid_probe_knn_workspace_bytes",
                         lib().rqsid_probe_knn_workspace_bytes(n_rows, n_queries, n_probes, k), device)
        self.n_rows, self.n_queries, self.n_probes, self.k = n_rows, n_queries, n_probes, k

    def counters(self) -> dict:
        """Of the last call (one host sync): queries ranked from their lists alone, (query, probe) items that took
        the all-rows pass, queries without an answer, tile visits of the screen."""
        c = self.buf[4:20].view(torch.int32).tolist()
        return {"from_lists": c[0], "all_rows_items": c[1], "non_finite_queries": c[2], "tile_visits": c[3]}


def probe_knn(x: torch.Tensor, q: torch.Tensor, k: int, probe_lo: torch.Tensor, probe_hi: torch.Tensor,
              metric: str = "l2", order: Optional[torch.Tensor] = None, query_self: Optional[torch.Tensor] = None,
              workspace: Optional[ProbeKnnWorkspace] = None, check: Optional[bool] = None):
    """The exact k nearest rows of ``x`` for every row of ``q`` among the rows at a few position ranges of ``order``
    (include/rqsid.h rqsid_probe_knn): the search through an ID index.

    ``x``, ``q``, ``k``, ``metric``, ``order`` (i32 [N], position -> row; None = identity) and ``query_self`` as for
    ``row_knn``; ``probe_lo`` / ``probe_hi``: i32 [M, P], half-open position ranges (``IdCells.prefix_ranges``, or
    ``Buckets.seg_row_off`` entries).  Query i searches the union of its ranges.  Returns ``(rows, val, scanned)``:
    i32 [M, k], f32 [M, k], i32 [M] (the positions in the query's cleaned ranges).  ``check`` (default: on unless the
    stream is being captured): read the workspace's error word after the call (one host sync) and raise if a table
    entry was clamped or a range dropped."""
    if check is None:
        check = not torch.cuda.is_current_stream_capturing()
    if metric not in KNN_METRICS:
        raise ValueError(f"rqsid_probe_knn: metric must be 'l2' or 'cosine', not {metric!r}")
    if not 1 <= int(k) <= KNN_MAX:
        raise ValueError(f"rqsid_probe_knn: k must lie in 1..{KNN_MAX}, not {k}")
    x_format, n, d, m = _row_pair_args("rqsid_probe_knn", x, q, order, None, query_self, None, True)
    _require_device(probe_lo, probe_hi)
    if probe_lo.dim() != 2 or probe_lo.shape != probe_hi.shape or probe_lo.shape[0] != m or \
            probe_lo.dtype != torch.int32 or probe_hi.dtype != torch.int32:
        raise ValueError("rqsid_probe_knn: probe_lo and probe_hi must be int32 [M, P]")
    n_probes = probe_lo.shape[1]
    if not 1 <= n_probes <= PROBE_MAX:
        raise ValueError(f"rqsid_probe_knn: 1..{PROBE_MAX} probes per query, not {n_probes}")
    probe_lo, probe_hi = probe_lo.contiguous(), probe_hi.contiguous()
    dev = x.device
    rows = torch.empty((m, k), dtype=torch.int32, device=dev)
    val = torch.empty((m, k), dtype=torch.float32, device=dev)
    scanned = torch.zeros(m, dtype=torch.int32, device=dev)
    need = int(lib().rqsid_probe_knn_workspace_bytes(n, m, n_probes, k))
    if need < 0:
        _lib.check(need, "rqsid_probe_knn_workspace_bytes")
    if workspace is None or workspace.bytes < need:
        workspace = ProbeKnnWorkspace(n, m, n_probes, k, dev)
    _lib.check(lib().rqsid_probe_knn(_ptr(x), x_format, n, d, _ptr(order), _ptr(q), m, _ptr(query_self), n_probes,
                                     _ptr(probe_lo), _ptr(probe_hi), KNN_METRICS[metric], int(k), _ptr(rows),
                                     _ptr(val), _ptr(scanned), _ptr(workspace.buf), workspace.bytes, _stream()),
               "rqsid_probe_knn")
    if check:
        check_error_words([workspace.error_word()], "rqsid_probe_knn", PROBE_KNN_WORD)
    return rows, val, scanned


CELLS_FINE_MAX = 8192        # RQSID_CELLS_FINE_MAX
CELLS_GROUPS_MAX = 1 << 24   # the wrapper's limit on the product of every level's size but the last
CELLS_COUNTERS = 37
ID_CELLS_WORD = ("bit 1: a row_index entry outside the rows was skipped; bit 2: a seg_row_off entry was clamped; "
                 "bit 4: a last-level ID at or above its level's size (that row has rank / size / cell -1) "
                 "(include/rqsid.h rqsid_id_cells)")


def id_cells_lds_rows() -> int:
    return int(lib().rqsid_id_cells_lds_rows())


class IdCellsWorkspace:
    """Scratch of rqsid_id_cells: per-group cell counts and bases, the sorted runs of cells beyond the LDS buffer, and
    a 256-byte header zeroed here once: bytes [0, 4) the sticky error word, bytes [4, 152) the call's counters."""

    def __init__(self, n_rows: int, n_groups: int, n_fine: int, device):
        self.bytes = int(lib().rqsid_id_cells_workspace_bytes(n_rows, n_groups, n_fine))
        if self.bytes < 0:
            _lib.check(self.bytes, "rqsid_id_cells_workspace_bytes")
        self.buf = torch.empty(max(self.bytes, 256), dtype=torch.uint8, device=device)
        self.buf[:256].zero_()

    def error_word(self) -> torch.Tensor:
        return self.buf[:4].view(torch.int32)

    def counters(self) -> torch.Tensor:
        return self.buf[4:4 + 4 * CELLS_COUNTERS].view(torch.int32)


def _prod(values) -> int:
    out = 1
    for v in values:
        out *= int(v)
    return out


@dataclass
class IdCells:
    """What ``id_cells`` returns (device tensors; include/rqsid.h rqsid_id_cells).  By row: ``rank``, ``size``,
    ``cell`` (-1 for a row whose ID names no cell); by position: ``order``; by cell: ``cell_off`` [capacity + 1],
    ``cell_group``, ``cell_fine`` (the first ``n_cells`` entries are written); ``counters``: i32 [37] (n_cells, cells
    of size >= 2, rows in them, cells of size 1, the largest cell, 32 bins of cells with size in [2^b, 2^(b+1)))."""
    order: torch.Tensor
    rank: torch.Tensor
    size: torch.Tensor
    cell: torch.Tensor
    cell_off: torch.Tensor
    cell_group: torch.Tensor
    cell_fine: torch.Tensor
    counters: torch.Tensor
    sizes: tuple            # the levels' sizes the IDs were read with
    invalid: torch.Tensor   # i64 scalar on the device: rows parked in the skipped group
    _n_cells: Optional[int] = None
    _keys: Optional[torch.Tensor] = None

    @property
    def n_cells(self) -> int:
        """Number of non-empty cells (one host read, then cached)."""
        if self._n_cells is None:
            self._n_cells = int(self.counters[0].item())
        return self._n_cells

    @property
    def n_invalid(self) -> int:
        return int(self.invalid.item())

    @property
    def n_fine(self) -> int:
        return self.sizes[-1] if len(self.sizes) > 1 else 1

    def keys(self) -> torch.Tensor:
        """The cells' IDs as mixed-radix numbers, i64 [n_cells], ascending."""
        if self._keys is None:
            n = self.n_cells
            self._keys = self.cell_group[:n].long() * self.n_fine + self.cell_fine[:n].long()
        return self._keys

    def prefix_range(self, prefix):
        """``(first cell, last cell, first position, last position)`` of the IDs that start with ``prefix`` (1 .. L
        values): half-open ranges of cells and of ``order``; an absent prefix gives an empty range."""
        prefix = [int(v) for v in prefix]
        L = len(self.sizes)
        if not 1 <= len(prefix) <= L:
            raise ValueError(f"a prefix holds 1 .. {L} values, not {len(prefix)}")
        if any(not 0 <= v < s for v, s in zip(prefix, self.sizes)):
            return 0, 0, 0, 0
        lo = 0
        for v, s in zip(prefix, self.sizes):
            lo = lo * s + v
        below = _prod(self.sizes[len(prefix):])
        keys = self.keys()
        bounds = torch.tensor([lo * below, (lo + 1) * below], dtype=torch.int64, device=keys.device)
        first, last = torch.searchsorted(keys, bounds).tolist()
        p0, p1 = self.cell_off[torch.tensor([first, last], device=keys.device)].tolist()
        return first, last, (p0 if last > first else p1), p1

    def prefix_ranges(self, prefixes: torch.Tensor):
        """``prefix_range``'s positions for a batch: ``prefixes`` int [..., p] with 1 <= p <= L gives ``(lo, hi)``,
        int32 tensors of shape [...] on the index's device, without a host read (beyond ``n_cells``, read once and
        cached).  A prefix with a negative or out-of-range value gives (0, 0), an absent one lo == hi."""
        dev = self.cell_off.device
        prefixes = torch.as_tensor(prefixes, device=dev)
        L = len(self.sizes)
        if prefixes.dim() < 1 or not 1 <= prefixes.shape[-1] <= L or prefixes.dtype.is_floating_point:
            raise ValueError(f"prefixes must be an int tensor [..., p] with 1 <= p <= {L}")
        p = prefixes.shape[-1]
        v = prefixes.long()
        sizes = torch.tensor(self.sizes[:p], dtype=torch.int64, device=dev)
        bad = ((v < 0) | (v >= sizes)).any(-1)
        num = torch.zeros(v.shape[:-1], dtype=torch.int64, device=dev)
        for j in range(p):
            num = num * self.sizes[j] + v[..., j].clamp(0, self.sizes[j] - 1)
        below = _prod(self.sizes[p:])
        keys = self.keys()
        first = torch.searchsorted(keys, (num * below).reshape(-1)).reshape(num.shape)
        last = torch.searchsorted(keys, ((num + 1) * below).reshape(-1)).reshape(num.shape)
        off = self.cell_off.long()
        p0, p1 = off[first], off[last]
        lo = torch.where(last > first, p0, p1)
        zero = torch.zeros_like(lo)
        return torch.where(bad, zero, lo).to(torch.int32), torch.where(bad, zero, p1).to(torch.int32)

    def ids_of(self, cells) -> torch.Tensor:
        """The ID tuples of cell numbers ``cells``: i32 [M, L]."""
        cells = torch.as_tensor(cells, dtype=torch.int64, device=self.cell_group.device).reshape(-1)
        g = self.cell_group[cells].long()
        cols = [self.cell_fine[cells].long()] if len(self.sizes) > 1 else []
        for s in reversed(self.sizes[:-1] if len(self.sizes) > 1 else self.sizes):
            cols.append(g % s)
            g = g // s
        return torch.stack(cols[::-1], 1).to(torch.int32)


def id_cells(ids: torch.Tensor, sizes: Optional[Sequence[int]] = None, rank_key: Optional[torch.Tensor] = None,
             workspace: Optional[IdCellsWorkspace] = None, check: bool = True) -> IdCells:
    """The cell index of semantic IDs (include/rqsid.h rqsid_id_cells): which rows share an ID, each row's place among
    them by ``rank_key`` (f32 [N]; None: by row number), and the collision counters.

    ``ids``: i32 [N, L]; ``sizes``: the levels' sizes (default: the per-level ``max + 1``, one host read).  The last
    level is the fine ID (size <= CELLS_FINE_MAX), the mixed-radix number of the others the group key (product <=
    2^24); with L = 1 level 0 is the group.  A row with a negative ID at any level, or with an ID at or above its
    level's size in a group level, names no cell: it is parked in one extra skipped group (rank / size / cell -1,
    after every cell in ``order``) and counted in ``n_invalid``.  A last-level ID at or above its size sets bit 4 of the
    error word.  ``check``: read the error words after the call (one host sync) and raise RuntimeError if one is set."""
    if ids.dim() != 2 or ids.shape[1] < 1 or ids.dtype != torch.int32:
        raise ValueError("rqsid_id_cells: ids must be int32 [N, L]")
    if ids.device.type != "cuda":
        raise RuntimeError("rqsid kernels run on the GPU only: got a %s tensor" % ids.device.type)
    _require_device(rank_key)
    n, L = ids.shape
    if rank_key is not None and (rank_key.dtype != torch.float32 or rank_key.numel() != n):
        raise ValueError("rqsid_id_cells: rank_key must be float32 [N]")
    if sizes is None:
        sizes = [int(v) + 1 for v in ids.max(0).values.clamp_min(0).tolist()] if n else [1] * L
    sizes = tuple(int(s) for s in sizes)
    if len(sizes) != L or any(s < 1 for s in sizes):
        raise ValueError(f"rqsid_id_cells: sizes must hold {L} positive values, got {sizes}")
    group_sizes = sizes[:-1] if L > 1 else sizes
    n_fine = sizes[-1] if L > 1 else 1
    G = _prod(group_sizes)
    if n_fine > CELLS_FINE_MAX:
        raise ValueError(f"rqsid_id_cells: the last level's size {n_fine} exceeds {CELLS_FINE_MAX}")
    if G > CELLS_GROUPS_MAX:
        raise ValueError(f"rqsid_id_cells: the group levels' sizes multiply to {G} > 2^24")
    dev = ids.device
    cap = min(n, (G + 1) * n_fine)

    def i32(m):
        return torch.empty(m, dtype=torch.int32, device=dev)

    if workspace is None or workspace.bytes < int(lib().rqsid_id_cells_workspace_bytes(n, G + 1, n_fine)):
        workspace = IdCellsWorkspace(n, G + 1, n_fine, dev)
    if n == 0:
        return IdCells(i32(0), i32(0), i32(0), i32(0), torch.zeros(1, dtype=torch.int32, device=dev), i32(0), i32(0),
                       torch.zeros(CELLS_COUNTERS, dtype=torch.int32, device=dev), sizes,
                       torch.zeros((), dtype=torch.int64, device=dev), 0)
    key = torch.zeros(n, dtype=torch.int64, device=dev)
    bad = torch.zeros(n, dtype=torch.bool, device=dev)
    for l, s in enumerate(group_sizes):
        col = ids[:, l].long()
        key = key * s + col
        bad |= (col < 0) | (col >= s)
    fine = None
    if L > 1:
        fine = ids[:, L - 1].contiguous()
        bad |= fine < 0
    key = torch.where(bad, G, key).to(torch.int32)
    buckets = bucket(key, G + 1)
    flags = torch.zeros(G + 1, dtype=torch.uint8, device=dev)
    flags[G] = 1
    out = IdCells(i32(n), i32(n), i32(n), i32(n), i32(cap + 1), i32(cap), i32(cap), workspace.counters(), sizes,
                  bad.sum())
    _lib.check(lib().rqsid_id_cells(n, _ptr(buckets.row_index), G + 1, _ptr(buckets.seg_row_off), _ptr(flags),
                                    _ptr(fine), n_fine, _ptr(rank_key), _ptr(out.order), _ptr(out.rank),
                                    _ptr(out.size), _ptr(out.cell), _ptr(out.cell_off), _ptr(out.cell_group),
                                    _ptr(out.cell_fine), _ptr(workspace.buf), workspace.bytes, _stream()),
               "rqsid_id_cells")
    out.counters = workspace.counters().clone()  # the workspace may serve another call
    if check:
        check_error_words([buckets.error_word(), workspace.error_word()], "rqsid_id_cells", ID_CELLS_WORD)
    return out


TRIE_LEVELS_MAX = 8       # RQSID_TRIE_LEVELS_MAX
TRIE_VOCAB_MAX = 1 << 20  # RQSID_TRIE_VOCAB_MAX
TRIE_BEAM_MAX = 64        # RQSID_TRIE_BEAM_MAX
IDS_FORMATS = {torch.int32: 0, torch.int64: 1}  # RQSID_IDS_*
ID_TRIE_WORD = "bit 1: a cell outside sizes, or not above the cell before it, was dropped"
TRIE_MASK_WORD = ("bit 1: a child range outside the counts was clamped; bit 2: a level_tok entry outside [-1, vocab) "
                  "was skipped")
TRIE_KIND_WALK, TRIE_KIND_COMPLETE, TRIE_KIND_DEAD = 0, 1, 2


def _sizes_array(sizes):
    return (ctypes.c_int32 * len(sizes))(*sizes)


@dataclass
class IdTrie:
    """The trie tables of ``id_trie`` (device tensors; include/rqsid.h rqsid_id_trie): ``count`` i32 [L + 1],
    ``value`` i32 [L, capacity], ``child_off`` i32 [L, capacity + 1], ``leaf_cell`` i32 [capacity]; entries past the
    counts are not written.  ``sizes``: the levels' sizes."""
    count: torch.Tensor
    value: torch.Tensor
    child_off: torch.Tensor
    leaf_cell: torch.Tensor
    sizes: tuple
    _counts: Optional[tuple] = None
    error: Optional[torch.Tensor] = None  # i32 [1]: the build's error word (a copy)

    @property
    def levels(self) -> int:
        return len(self.sizes)

    @property
    def capacity(self) -> int:
        return int(self.leaf_cell.numel())

    def counts(self) -> tuple:
        """Nodes per depth 0 .. L (one host read, then cached)."""
        if self._counts is None:
            self._counts = tuple(int(v) for v in self.count.tolist())
        return self._counts

    def _table_args(self):
        return (self.capacity, self.levels, _sizes_array(self.sizes), _ptr(self.count), _ptr(self.value),
                _ptr(self.child_off))

    def to_arrays(self) -> dict:
        """The written part of the tables as numpy arrays (for ``numpy.savez``)."""
        import numpy as np
        cnt = self.counts()
        out = {"sizes": np.asarray(self.sizes, dtype=np.int32), "count": np.asarray(cnt, dtype=np.int32),
               "leaf_cell": self.leaf_cell[:cnt[-1]].cpu().numpy()}
        for d in range(self.levels):
            out[f"value{d}"] = self.value[d, :cnt[d + 1]].cpu().numpy()
            out[f"child_off{d}"] = self.child_off[d, :cnt[d] + 1].cpu().numpy()
        return out

    @classmethod
    def from_arrays(cls, arrays, device) -> "IdTrie":
        sizes = tuple(int(s) for s in arrays["sizes"])
        cnt = [int(c) for c in arrays["count"]]
        L, cap = len(sizes), cnt[-1]
        value = torch.zeros(L, cap, dtype=torch.int32, device=device)
        child_off = torch.zeros(L, cap + 1, dtype=torch.int32, device=device)
        for d in range(L):
            value[d, :cnt[d + 1]] = torch.as_tensor(arrays[f"value{d}"], dtype=torch.int32).to(device)
            child_off[d, :cnt[d] + 1] = torch.as_tensor(arrays[f"child_off{d}"], dtype=torch.int32).to(device)
        return cls(torch.tensor(cnt, dtype=torch.int32, device=device), value, child_off,
                   torch.as_tensor(arrays["leaf_cell"], dtype=torch.int32).to(device).contiguous(), sizes, tuple(cnt))


def id_trie_tables(cell_group: torch.Tensor, cell_fine: torch.Tensor, sizes: Sequence[int],
                   keep: Optional[torch.Tensor] = None, check: bool = True) -> IdTrie:
    """rqsid_id_trie on bare cell arrays (i32 [n_cells] each, as rqsid_id_cells writes them)."""
    _require_device(cell_group, cell_fine, keep)
    sizes = tuple(int(s) for s in sizes)
    n = int(cell_group.numel())
    if cell_group.dtype != torch.int32 or cell_fine.dtype != torch.int32 or cell_fine.numel() != n:
        raise ValueError("rqsid_id_trie: cell_group and cell_fine must be int32 [n_cells]")
    if keep is not None:
        if keep.numel() != n or keep.dtype not in (torch.uint8, torch.bool):
            raise ValueError("rqsid_id_trie: keep must be uint8 or bool [n_cells]")
        keep = keep.to(torch.uint8)
    dev = cell_group.device
    L = len(sizes)
    nbytes = int(lib().rqsid_id_trie_workspace_bytes(n, L))
    if nbytes < 0:
        _lib.check(nbytes, "rqsid_id_trie_workspace_bytes")
    ws = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=dev)
    ws[:256].zero_()
    rows = max(L, 0)
    trie = IdTrie(torch.zeros(rows + 1, dtype=torch.int32, device=dev),
                  torch.empty(rows, n, dtype=torch.int32, device=dev),
                  (torch.empty if n else torch.zeros)(rows, n + 1, dtype=torch.int32, device=dev),
                  torch.empty(n, dtype=torch.int32, device=dev), sizes)
    if n == 0:
        trie.count[0] = 1  # (the entry touches nothing without cells: count = {1, 0, ...}, child_off = 0)
    _lib.check(lib().rqsid_id_trie(n, _ptr(cell_group), _ptr(cell_fine), L, _sizes_array(sizes), _ptr(keep),
                                   _ptr(trie.count), _ptr(trie.value), _ptr(trie.child_off), _ptr(trie.leaf_cell),
                                   _ptr(ws), nbytes, _stream()), "rqsid_id_trie")
    trie.error = ws[:4].view(torch.int32).clone()
    if check:
        check_error_words([ws[:4].view(torch.int32)], "rqsid_id_trie", ID_TRIE_WORD)
    return trie


def id_trie(index: IdCells, keep: Optional[torch.Tensor] = None, check: bool = True) -> IdTrie:
    """The trie of a cell index (include/rqsid.h rqsid_id_trie).  ``keep``: uint8 / bool [n_cells] (None: every cell); a
    cell with ``keep == 0`` is left out, as the reference leaves out a sequence with an unknown token
    (``TokenMap.keep_cells``).  ``leaf_cell`` numbers the index's cells, so ``index.cell_off[trie.leaf_cell[j]]`` is where
    leaf j's rows start in ``index.order``.  ``check``: read the error word (one host sync) and raise if it is set."""
    n = index.n_cells
    return id_trie_tables(index.cell_group[:n].contiguous(), index.cell_fine[:n].contiguous(), index.sizes, keep, check)


class TokenMap:
    """The tokenizer as two tables of token numbers, on the device: ``tok_code`` i32 [vocab_size] (-1 for a token that
    is no ID token, else ``level << 24 | value``) and ``level_tok`` i32 [sum(sizes)] (the levels one after another: the
    token number of (level, value), or -1).  ``level_tokens``: per level, the token number of each value (-1: none).
    Raises ValueError if two (level, value) pairs share a token number or a token number is outside the vocabulary."""

    def __init__(self, vocab_size: int, level_tokens, eos_token_id: int, device=None):
        import numpy as np
        self.vocab_size = int(vocab_size)
        self.eos_token_id = int(eos_token_id)
        levels = [np.asarray(t, dtype=np.int64).reshape(-1) for t in level_tokens]
        self.sizes = tuple(len(t) for t in levels)
        if not 1 <= len(levels) <= TRIE_LEVELS_MAX or any(s < 1 for s in self.sizes):
            raise ValueError(f"TokenMap: 1 .. {TRIE_LEVELS_MAX} non-empty levels are needed, got sizes {self.sizes}")
        if not 1 <= self.vocab_size <= TRIE_VOCAB_MAX:
            raise ValueError(f"TokenMap: vocab_size = {self.vocab_size} outside [1, {TRIE_VOCAB_MAX}]")
        if not 0 <= self.eos_token_id < self.vocab_size:
            raise ValueError(f"TokenMap: eos_token_id = {self.eos_token_id} outside the vocabulary")
        if any(s > 1 << 24 for s in self.sizes):
            raise ValueError("TokenMap: a level holds more than 2^24 values")
        code = np.full(self.vocab_size, -1, dtype=np.int32)
        for l, toks in enumerate(levels):
            if ((toks < -1) | (toks >= self.vocab_size)).any():
                bad = int(toks[(toks < -1) | (toks >= self.vocab_size)][0])
                raise ValueError(f"TokenMap: token number {bad} of level {l} is outside the vocabulary "
                                 f"[0, {self.vocab_size})")
            have = np.nonzero(toks >= 0)[0]
            t = toks[have]
            if len(np.unique(t)) != len(t) or (code[t] != -1).any():
                raise ValueError(f"TokenMap: a token number of level {l} names more than one (level, value) pair")
            code[t] = (l << 24) | have.astype(np.int32)
        self.level_tok_host = np.concatenate(levels).astype(np.int32)
        self.tok_code_host = code
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else device
        self.tok_code = torch.from_numpy(code).to(dev)
        self.level_tok = torch.from_numpy(self.level_tok_host).to(dev)
        self.level_off = tuple(int(v) for v in np.concatenate([[0], np.cumsum(self.sizes)]))

    @classmethod
    def identity(cls, sizes, device=None) -> "TokenMap":
        """token = the level's offset + value, eos = sum(sizes), vocab_size = sum(sizes) + 1."""
        sizes = [int(s) for s in sizes]
        offs = [sum(sizes[:l]) for l in range(len(sizes))]
        return cls(sum(sizes) + 1, [range(o, o + s) for o, s in zip(offs, sizes)], sum(sizes), device)

    @classmethod
    def from_tokenizer(cls, tokenizer, eos_token_id: int, levels: int = 3, device=None) -> "TokenMap":
        """From an object shaped like the reference's tokenizer: ``tokenizer.base_tokenizer.convert_tokens_to_ids`` and
        ``.unk_token_id``, ``tokenizer.layer_vocab_sizes['l1' ...]``, tokens named ``<id_l{n}_{v}>``.  An unknown token
        at level >= 1 becomes -1 (the cells that use it are dropped through ``keep_cells``, as the reference drops
        them).  An unknown level-0 token raises ValueError: the reference would then take the unknown-token number
        itself for a level-1 token and start a prefix at every unknown token of the input; that is refused here."""
        base = tokenizer.base_tokenizer
        unk = base.unk_token_id
        tables = []
        for l in range(levels):
            n = int(tokenizer.layer_vocab_sizes[f"l{l + 1}"])
            toks = [base.convert_tokens_to_ids(f"<id_l{l + 1}_{v}>") for v in range(n)]
            if l == 0 and any(t == unk or t is None for t in toks):
                v = [t == unk or t is None for t in toks].index(True)
                raise ValueError(f"TokenMap.from_tokenizer: <id_l1_{v}> is unknown to the tokenizer; the reference "
                                 "would treat the unknown-token number as a level-1 token, which is refused here")
            tables.append([-1 if (t == unk or t is None) else int(t) for t in toks])
        vocab = getattr(tokenizer, "vocab_size", None)
        if vocab is None:
            vocab = len(base)
        return cls(int(vocab), tables, eos_token_id, device)

    def with_eos(self, eos_token_id: int) -> "TokenMap":
        """The same tables (shared, not copied) with another eos."""
        if not 0 <= int(eos_token_id) < self.vocab_size:
            raise ValueError(f"TokenMap: eos_token_id = {eos_token_id} outside the vocabulary")
        other = copy.copy(self)
        other.eos_token_id = int(eos_token_id)
        return other

    def with_vocab(self, vocab_size: int) -> "TokenMap":
        """The same (level, value) -> token table for scores of another width (a model's logits may be padded beyond
        the tokenizer's vocabulary); raises ValueError if a token number or eos does not fit."""
        offs = self.level_off
        return TokenMap(vocab_size, [self.level_tok_host[offs[l]:offs[l + 1]] for l in range(len(self.sizes))],
                        self.eos_token_id, self.level_tok.device)

    def keep_cells(self, index: IdCells) -> torch.Tensor:
        """uint8 [n_cells]: 1 for a cell whose every level value has a token."""
        n = index.n_cells
        ids = index.ids_of(torch.arange(n, device=self.level_tok.device)).long()
        keep = torch.ones(n, dtype=torch.bool, device=self.level_tok.device)
        for l in range(len(self.sizes)):
            keep &= self.level_tok[self.level_off[l] + ids[:, l]] >= 0
        return keep.to(torch.uint8)


class TrieMaskWorkspace:
    """Scratch of rqsid_trie_mask: 16 bytes per row behind a 256-byte header zeroed here once: bytes [0, 4) the sticky
    error word, bytes [4, 16) the call's counters (rows of kind 0 / 1 / 2)."""

    def __init__(self, n_rows: int, device):
        self.bytes = int(lib().rqsid_trie_mask_workspace_bytes(n_rows))
        if self.bytes < 0:
            _lib.check(self.bytes, "rqsid_trie_mask_workspace_bytes")
        self.buf = torch.empty(self.bytes, dtype=torch.uint8, device=device)
        self.buf[:256].zero_()

    def error_word(self) -> torch.Tensor:
        return self.buf[:4].view(torch.int32)

    def counters(self) -> torch.Tensor:
        return self.buf[4:16].view(torch.int32)


@dataclass
class TrieMaskRows:
    """Per row of ``trie_mask``: ``kind`` (0 walked, 1 complete, 2 dead), ``node`` (the node reached, -1 unless kind 0),
    ``count`` (allowed tokens); ``kinds``: i32 [3], the rows of each kind."""
    kind: torch.Tensor
    node: torch.Tensor
    count: torch.Tensor
    kinds: torch.Tensor


def _check_tokens(who: str, trie: IdTrie, tokens: TokenMap) -> None:
    if tuple(tokens.sizes) != tuple(trie.sizes):
        raise ValueError(f"{who}: the token map's sizes {tokens.sizes} are not the trie's {trie.sizes}")


def trie_mask(trie: IdTrie, tokens: TokenMap, input_ids: torch.Tensor, scores: torch.Tensor,
              workspace: Optional[TrieMaskWorkspace] = None, check: bool = True) -> TrieMaskRows:
    """Constrained-decoding mask in place (include/rqsid.h rqsid_trie_mask): ``scores`` [B, V] (f32 / f16 / bf16, unit
    stride inside a row, any row stride >= V) keeps the entries of the tokens the trie allows after each row of
    ``input_ids`` [B, T] (int32 / int64) and gets -inf everywhere else.  One launch sequence, no host read (``check``:
    read the error word afterwards, one host sync, and raise if it is set)."""
    who = "rqsid_trie_mask"
    _check_tokens(who, trie, tokens)
    for t in (input_ids, scores):
        if t.device.type != "cuda":
            raise RuntimeError("rqsid kernels run on the GPU only: got a %s tensor" % t.device.type)
    if scores.dim() != 2 or scores.dtype not in ROW_FORMATS:
        raise ValueError(f"{who}: scores must be float32 / float16 / bfloat16 [B, V]")
    B, V = scores.shape
    if input_ids.dim() != 2 or input_ids.shape[0] != B or input_ids.dtype not in IDS_FORMATS:
        raise ValueError(f"{who}: input_ids must be int32 / int64 [B, T] with the scores' B")
    if V != tokens.vocab_size:
        raise ValueError(f"{who}: scores hold {V} tokens a row, the token map {tokens.vocab_size}")
    T = input_ids.shape[1]
    if T and B and input_ids.stride(1) != 1:
        input_ids = input_ids.contiguous()
    if B and V and (scores.stride(1) != 1 or (B > 1 and scores.stride(0) < V)):
        raise ValueError(f"{who}: scores need unit stride inside a row and a row stride >= V")
    dev = scores.device
    if workspace is None or workspace.bytes < 256 + 16 * B:
        workspace = TrieMaskWorkspace(B, dev)
    out = TrieMaskRows(*(torch.empty(B, dtype=torch.int32, device=dev) for _ in range(3)), workspace.counters())
    ld = scores.stride(0) if B > 1 else max(V, 1)
    ids_ld = input_ids.stride(0) if (B > 1 and T) else max(T, 1)
    _lib.check(lib().rqsid_trie_mask(*trie._table_args(), _ptr(input_ids) if T and B else None,
                                     IDS_FORMATS[input_ids.dtype], B, T, ids_ld, _ptr(scores),
                                     ROW_FORMATS[scores.dtype], V, ld, _ptr(tokens.tok_code), _ptr(tokens.level_tok),
                                     tokens.eos_token_id, _ptr(out.kind), _ptr(out.node), _ptr(out.count),
                                     _ptr(workspace.buf), workspace.bytes, _stream()), who)
    out.kinds = workspace.counters().clone() if B and V else torch.zeros(3, dtype=torch.int32, device=dev)
    if check:
        check_error_words([workspace.error_word()], who, TRIE_MASK_WORD)
    return out


@dataclass
class TrieBeamStep:
    """``trie_beam_step``'s slots, [B, beam_out] each: ``node`` (depth d + 1), ``score`` f32, ``parent`` (the hypothesis
    it extends), ``value`` (its level-d ID value), ``token``; an unfilled slot holds -1 / -inf / -1 / -1 / -1."""
    node: torch.Tensor
    score: torch.Tensor
    parent: torch.Tensor
    value: torch.Tensor
    token: torch.Tensor


def trie_beam_step(trie: IdTrie, tokens: TokenMap, depth: int, node_in: torch.Tensor,
                   score_in: Optional[torch.Tensor], logp: torch.Tensor, beam_out: int) -> TrieBeamStep:
    """One constrained beam step over trie nodes (include/rqsid.h rqsid_trie_beam_step): ``node_in`` i32 [B, beam_in]
    depth-``depth`` nodes, ``score_in`` f32 [B, beam_in] or None, ``logp`` [B * beam_in, V] (f32 / f16 / bf16, unit
    stride inside a row); the best ``beam_out`` children by (score descending, hypothesis, value)."""
    who = "rqsid_trie_beam_step"
    _check_tokens(who, trie, tokens)
    _require_device(node_in, score_in)
    if logp.device.type != "cuda":
        raise RuntimeError("rqsid kernels run on the GPU only: got a %s tensor" % logp.device.type)
    if node_in.dim() != 2 or node_in.dtype != torch.int32:
        raise ValueError(f"{who}: node_in must be int32 [B, beam_in]")
    B, beam_in = node_in.shape
    if score_in is not None and (score_in.dtype != torch.float32 or tuple(score_in.shape) != (B, beam_in)):
        raise ValueError(f"{who}: score_in must be float32 [B, beam_in]")
    if logp.dim() != 2 or logp.dtype not in ROW_FORMATS or logp.shape[0] != B * beam_in:
        raise ValueError(f"{who}: logp must be float32 / float16 / bfloat16 [B * beam_in, V]")
    V = logp.shape[1]
    if V != tokens.vocab_size:
        raise ValueError(f"{who}: logp holds {V} tokens a row, the token map {tokens.vocab_size}")
    if logp.shape[0] and (logp.stride(1) != 1 or (logp.shape[0] > 1 and logp.stride(0) < V)):
        raise ValueError(f"{who}: logp needs unit stride inside a row and a row stride >= V")
    ld = logp.stride(0) if logp.shape[0] > 1 else V
    dev = node_in.device
    n_out = max(int(beam_out), 0)
    out = TrieBeamStep(torch.empty(B, n_out, dtype=torch.int32, device=dev),
                       torch.empty(B, n_out, dtype=torch.float32, device=dev),
                       *(torch.empty(B, n_out, dtype=torch.int32, device=dev) for _ in range(3)))
    _lib.check(lib().rqsid_trie_beam_step(*trie._table_args(), int(depth), B, beam_in, int(beam_out), _ptr(node_in),
                                          _ptr(score_in), _ptr(logp), ROW_FORMATS[logp.dtype], V, ld,
                                          _ptr(tokens.level_tok), _ptr(out.node), _ptr(out.score), _ptr(out.parent),
                                          _ptr(out.value), _ptr(out.token), _stream()), who)
    return out


def scale_groups(x: torch.Tensor, group_dims: Sequence[int], weights: Sequence[float]) -> torch.Tensor:
    _require_f32("scale_groups", x)
    _require_device(x)
    n, d = x.shape
    g = _groups_tensor(group_dims, x.device, d, "scale_groups")
    if len(weights) != len(group_dims):
        raise ValueError("scale_groups: %d weights for %d dimension groups" % (len(weights), len(group_dims)))
    out = torch.empty_like(x)
    w = torch.tensor(list(weights), dtype=torch.float32, device=x.device)
    _lib.check(lib().rqsid_scale_groups(_ptr(x), n, d, _ptr(g), len(group_dims), _ptr(w), _ptr(out), _stream()),
               "rqsid_scale_groups")
    return out


def centroid_update(x: torch.Tensor, assignment: torch.Tensor, k: int, centers: torch.Tensor):
    """New centres = per-cluster means of x (fp64 sums) written into ``centers`` where the
    cluster is non-empty.  Rows whose assignment lies outside [0, k) belong to no cluster: they enter no sum and
    no count.  Returns (centers, counts i32[k])."""
    _require_f32("centroid_update", x, centers)
    _require_device(x, centers)
    n, d = x.shape
    b = bucket(assignment, k, rows_per_tile=centroid_tile_rows())
    sums = torch.zeros((k, d), dtype=torch.float64, device=x.device)
    _lib.check(lib().rqsid_centroid_accumulate(_ptr(x), d, _ptr(b.row_index), k, _ptr(b.seg_row_off),
                                               _ptr(b.seg_tile_off), b.max_tiles, _ptr(sums), _stream()),
               "rqsid_centroid_accumulate")
    _lib.check(lib().rqsid_centroid_finalize(_ptr(sums), _ptr(b.seg_row_off), k, d, _ptr(centers), _stream()),
               "rqsid_centroid_finalize")
    counts = b.seg_row_off[1:] - b.seg_row_off[:-1]
    return centers, counts


def pairwise_distance(x: torch.Tensor, c: torch.Tensor) -> torch.Tensor:
    _require_f32("pairwise_distance", x)
    c = c.float().contiguous()
    _require_device(x, c)
    n, d = x.shape
    out = torch.empty((n, c.shape[0]), dtype=torch.float32, device=x.device)
    _lib.check(lib().rqsid_pairwise_distance(_ptr(x), n, d, _ptr(c), c.shape[0], _ptr(out), _stream()),
               "rqsid_pairwise_distance")
    return out


def pairwise_cosine(x: torch.Tensor, c: torch.Tensor, scores: bool = False) -> torch.Tensor:
    """Cosine distances 1 - x.c / (|x||c|): fp32 [N, K], or with ``scores`` the auction's worker-major fp16
    [K][N] = -distance (include/rqsid.h rqsid_pairwise_cosine)."""
    _require_f32("pairwise_cosine", x)
    c = c.float().contiguous()
    _require_device(x, c)
    n, d = x.shape
    if scores:
        out = torch.empty((c.shape[0], n), dtype=torch.float16, device=x.device)
        _lib.check(lib().rqsid_pairwise_cosine(_ptr(x), n, d, _ptr(c), c.shape[0], None, _ptr(out), _stream()),
                   "rqsid_pairwise_cosine")
        return out
    out = torch.empty((n, c.shape[0]), dtype=torch.float32, device=x.device)
    _lib.check(lib().rqsid_pairwise_cosine(_ptr(x), n, d, _ptr(c), c.shape[0], _ptr(out), None, _stream()),
               "rqsid_pairwise_cosine")
    return out


def auction_scores(x: torch.Tensor, c: torch.Tensor, half: bool = False) -> torch.Tensor:
    """Worker-major fp16 scores W[k][n] = -distance (the auction's input), see include/rqsid.h."""
    _require_f32("auction_scores", x)
    c = c.float().contiguous()
    _require_device(x, c)
    n, d = x.shape
    out = torch.empty((c.shape[0], n), dtype=torch.float16, device=x.device)
    _lib.check(lib().rqsid_auction_scores(_ptr(x), n, d, _ptr(c), c.shape[0], int(half), _ptr(out), _stream()),
               "rqsid_auction_scores")
    return out


def auction(scores_wj: torch.Tensor, max_rounds: int = 0):
    """Balanced assignment on worker-major fp16 scores [K][N]. Returns (assignment i32[N], rounds)."""
    scores_wj = scores_wj.to(torch.float16).contiguous()
    _require_device(scores_wj)
    k, n = scores_wj.shape
    out = torch.empty(n, dtype=torch.int32, device=scores_wj.device)
    wsb = int(lib().rqsid_auction_workspace_bytes(n, k))
    ws = torch.empty(max(wsb, 1), dtype=torch.uint8, device=scores_wj.device)
    rounds = ctypes.c_int32(0)
    _lib.check(lib().rqsid_auction_lap_half(_ptr(scores_wj), k, n, int(max_rounds), _ptr(out), ctypes.addressof(rounds),
                                            _ptr(ws), wsb, _stream()), "rqsid_auction_lap_half")
    return out, int(rounds.value)


def auction_full(scores_wj: torch.Tensor, max_rounds: int = 0):
    """fp32 balanced assignment on worker-major scores [K][N] (include/rqsid.h rqsid_auction_lap_full).
    Returns (assignment i32[N], rounds)."""
    scores_wj = scores_wj.to(torch.float32).contiguous()
    _require_device(scores_wj)
    k, n = scores_wj.shape
    out = torch.empty(n, dtype=torch.int32, device=scores_wj.device)
    if n == 0:
        return out, 0
    wsb = int(lib().rqsid_auction_full_workspace_bytes(n, k))
    ws = torch.empty(max(wsb, 1), dtype=torch.uint8, device=scores_wj.device)
    rounds = ctypes.c_int32(0)
    _lib.check(lib().rqsid_auction_lap_full(_ptr(scores_wj), k, n, int(max_rounds), _ptr(out), ctypes.addressof(rounds),
                                            _ptr(ws), wsb, _stream()), "rqsid_auction_lap_full")
    return out, int(rounds.value)


def greedy_match(dist: torch.Tensor, sub_off: torch.Tensor, max_take: int):
    """Greedy unique-nearest columns per group (see include/rqsid.h rqsid_greedy_match).
    dist: f32 [total_sub, C]; sub_off: i32 [G+1].  Returns (match u8 [G, C], n_selected i32 [G])."""
    dist = dist.float().contiguous()
    sub_off = sub_off.to(torch.int32).contiguous()
    _require_device(dist, sub_off)
    g = sub_off.numel() - 1
    c = dist.shape[1]
    match = torch.empty((g, c), dtype=torch.uint8, device=dist.device)
    nsel = torch.empty(max(g, 1), dtype=torch.int32, device=dist.device)
    _lib.check(lib().rqsid_greedy_match(_ptr(dist), _ptr(sub_off), g, c, int(max_take), _ptr(match), _ptr(nsel),
                                        _stream()), "rqsid_greedy_match")
    return match, nsel[:g]


def centroid_sums(x: torch.Tensor, assignment: torch.Tensor, k: int):
    """Per-cluster fp64 sums and counts of the rows of x (the first half of the Lloyd update; the
    multi-GPU fit all-reduces these).  Rows whose assignment lies outside [0, k) enter no sum and no count.
    Returns (sums f64 [k, D], counts i32 [k])."""
    _require_f32("centroid_sums", x)
    _require_device(x)
    n, d = x.shape
    b = bucket(assignment, k, rows_per_tile=centroid_tile_rows())
    sums = torch.zeros((k, d), dtype=torch.float64, device=x.device)
    _lib.check(lib().rqsid_centroid_accumulate(_ptr(x), d, _ptr(b.row_index), k, _ptr(b.seg_row_off),
                                               _ptr(b.seg_tile_off), b.max_tiles, _ptr(sums), _stream()),
               "rqsid_centroid_accumulate")
    return sums, b.seg_row_off[1:] - b.seg_row_off[:-1]


class SegmentLayout:
    """Rows grouped by segment (segment s = rows off[s] .. off[s+1] of a segment-ordered matrix), with the
    tile and chunk tables of the segmented auction kernels (include/rqsid.h rqsid_seg_auction_*)."""

    def __init__(self, sizes, device):
        import numpy as np
        sizes = np.asarray(sizes, dtype=np.int64)
        if sizes.ndim != 1 or len(sizes) == 0 or (sizes < 0).any():
            raise ValueError("segment sizes must be a non-empty 1-D array of counts")
        self.sizes = sizes
        self.n_seg = len(sizes)
        off = np.zeros(self.n_seg + 1, dtype=np.int64)
        off[1:] = np.cumsum(sizes)
        if off[-1] > 2**31 - 1:
            raise ValueError("segmented auction: more than 2^31 - 1 rows")
        self.off = off
        self.n = int(off[-1])
        tiles = (sizes + 63) // 64
        ch = int(lib().rqsid_seg_auction_chunk_jobs())
        chunks = (sizes + ch - 1) // ch
        toff = np.concatenate([[0], np.cumsum(tiles)])
        coff = np.concatenate([[0], np.cumsum(chunks)])
        self.n_tiles = int(toff[-1])
        self.total_chunks = int(coff[-1])
        self.n_multi = int((chunks > 1).sum())
        self.seg_off = torch.as_tensor(off, dtype=torch.int32).to(device)
        self.tile_off = torch.as_tensor(toff, dtype=torch.int32).to(device)
        self.chunk_off = torch.as_tensor(coff, dtype=torch.int32).to(device)
        self.seg_of_row = torch.repeat_interleave(torch.arange(self.n_seg, device=device),
                                                  torch.as_tensor(sizes).to(device))


def seg_auction_scores(x: torch.Tensor, centers: torch.Tensor, k: int, layout: SegmentLayout,
                       half: bool = False) -> torch.Tensor:
    """Per-segment worker-major fp16 scores -distance (segment s: rows of layout, centres s*k..s*k+k-1),
    concatenated: a flat fp16 tensor of k * N values."""
    _require_f32("seg_auction_scores", x)
    centers = centers.float().contiguous()
    _require_device(x, centers)
    n, d = x.shape
    if n != layout.n or centers.shape[0] != layout.n_seg * k or centers.shape[1] != d:
        raise ValueError("seg_auction_scores: rows / centres do not match the segment layout")
    out = torch.empty(max(k * n, 1), dtype=torch.float16, device=x.device)
    _lib.check(lib().rqsid_seg_auction_scores(_ptr(x), n, d, _ptr(centers), k, layout.n_seg, _ptr(layout.seg_off),
                                              _ptr(layout.tile_off), layout.n_tiles, int(half), _ptr(out), _stream()),
               "rqsid_seg_auction_scores")
    return out


def seg_auction(scores: torch.Tensor, k: int, layout: SegmentLayout, active: Optional[torch.Tensor] = None,
                max_rounds: int = 0, out: Optional[torch.Tensor] = None):
    """One balanced auction per segment, all advanced in lockstep.  Returns (assignment i32 [N] local to
    each segment, rounds i32 [S] on the device).  Segments with active[s] == 0 keep ``out``'s entries."""
    scores = scores.to(torch.float16).contiguous()
    _require_device(scores, active)
    n = layout.n
    if out is None:
        out = torch.full((max(n, 1),), -1, dtype=torch.int32, device=scores.device)
    rounds = torch.zeros(layout.n_seg, dtype=torch.int32, device=scores.device)
    wsb = int(lib().rqsid_seg_auction_workspace_bytes(n, k, layout.n_seg, layout.total_chunks, layout.n_multi))
    ws = torch.empty(max(wsb, 1), dtype=torch.uint8, device=scores.device)
    act = None if active is None else active.to(torch.uint8).contiguous()
    _lib.check(lib().rqsid_seg_auction_lap_half(_ptr(scores), k, layout.n_seg, _ptr(layout.seg_off),
                                                _ptr(layout.chunk_off), layout.total_chunks, layout.n_multi, n,
                                                _ptr(act), int(max_rounds), _ptr(out), _ptr(rounds), _ptr(ws), wsb,
                                                _stream()), "rqsid_seg_auction_lap_half")
    return out[:n], rounds
