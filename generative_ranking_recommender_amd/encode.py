"""Multi-level residual-quantisation encoder on the HIP kernels (the bench hot path).

One ``RQEncoder`` holds the trained codebooks of every level, already prepared
for ``rqsid_assign`` (fp16 copy, norms, candidate lists), and turns an fp32
(or fp16 / bf16) [N, D] device matrix into int32 [N, L] semantic IDs with no
host round trip.

Level semantics:

* level 0: nearest of ``need[0]`` centres (``_predict_layer_0``,
  hierarchical_rq_kmeans.py:1146-1173; simplified :202).
* middle level l: segment = the previous level's ID p; allowed centres are the
  block ``[p*need[l], (p+1)*need[l])``; the ID is the local index in the block
  (``_predict_middle_layer`` :1175-1233 / ``_reassign_clusters_middle_layer_with_
  residuals`` :839-904 / simplified :145-172).
* last level: group = ``ids[l-2]*mult + ids[l-1]`` (mult = ``need[l-2]`` in the
  hierarchical path :824,1256, ``need[-2]`` in the simplified path :311); allowed
  centres = the group's match-matrix row.  ID = rank of the chosen column among
  the allowed ones (``_merge_match_matrix_cluster_ids`` :1055-1086) or the raw
  column (simplified :305-331).

Switches reproduce the reference's predict-time quirks (Appendix A item 2):
``match_lookup`` False = the `match_matrices[layer-1]` miss at :1248 (the last
level is then an unconstrained argmin over every candidate, raw IDs);
``residual_global_id`` False = predict's residual indexing ``centers[id % need]``
(:577,1143) instead of the raw block index the trainer uses (:901).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional, Sequence

import torch

from . import ops


@dataclass
class LevelSemantics:
    normalize_residual: bool = True      # hierarchical: r/(||r||+1e-8) per group; simplified: plain
    match_lookup: bool = True            # False: reference predict bug (:1248)
    residual_global_id: bool = True      # False: reference predict bug (:1143 with modded ids)
    remap_last: bool = True              # hierarchical rank remap; simplified keeps raw column
    last_group_mult: str = "need_l_minus_2"  # or "need_minus_2" (simplified)
    residual_from_weighted: bool = False  # train-time residuals use weighted data (:442 vs :577)


HIERARCHICAL_PREDICT_REFERENCE = LevelSemantics(match_lookup=False, residual_global_id=False)
HIERARCHICAL_TRAIN = LevelSemantics(residual_from_weighted=True)
SIMPLIFIED = LevelSemantics(normalize_residual=False, remap_last=False, last_group_mult="need_minus_2")


@dataclass
class QuantError:
    """What ``RQEncoder.quant_error`` returns (device tensors)."""
    ids: torch.Tensor        # i32 [N, L] semantic IDs the errors belong to
    err: torch.Tensor        # f32 [N, L]: distance from level l's input vector to its assigned centre
    x_norm: torch.Tensor     # f32 [N]: ||x||
    recon_err: torch.Tensor  # f32 [N]: ||x - decode(ids, err)||, from the chain's own norms
    sums: torch.Tensor       # f64 [L + 1]: per level sum of err^2 over the rows, then sum of ||x||^2
    recon_levels: Optional[torch.Tensor] = None  # f32 [N, L]: recon_err had the chain stopped at level l


@dataclass
class TopK:
    """What ``RQEncoder.encode_topk`` returns (device tensors; the [N, L, k] ones are permuted views of the
    level-major buffers the kernel writes).  Level l ranks the allowed centres of the segment the greedy path
    reached (``ids[:, :l]``) for the level's own input vector, by (fp64 squared distance, list position)."""
    ids: torch.Tensor    # i32 [N, L], equal to encode(x)
    local: torch.Tensor  # i32 [N, L, k]: the id each place would have given (local[:, :, 0] == ids); -1: no such place
    glob: torch.Tensor   # i32 [N, L, k]: its codebook row
    dist: torch.Tensor   # f32 [N, L, k]: its distance (dist[:, l, 0] is the level's quantisation distance)


@dataclass
class Beam:
    """What ``RQEncoder.encode_beam`` returns (device tensors)."""
    ids: torch.Tensor        # i32 [N, L]: the best path
    recon_err: torch.Tensor  # f32 [N]: its original-space reconstruction error ||x - x_hat||
    paths: torch.Tensor      # i32 [N, B, L]: every slot's path (slot 0 is greedy; -1 in a dead slot)
    path_err: torch.Tensor   # f32 [N, B]: every slot's error (+inf in a dead slot, NaN in a non-finite row)
    slot: torch.Tensor       # i32 [N]: the slot ``ids`` came from


@dataclass
class IndexSearch:
    """What ``RQEncoder.search`` returns (device tensors)."""
    rows: torch.Tensor      # i32 [M, k]: the nearest rows among those under the probed prefixes, -1 past their end
    val: torch.Tensor       # f32 [M, k]: distance or cosine similarity
    scanned: torch.Tensor   # i32 [M]: catalogue positions read
    prefixes: torch.Tensor  # i32 [M, probes, depth]: the probed ID prefixes (-1: a dead slot)


class _TopKLevels:
    """Collects rqsid_assign_topk's outputs level by level while an encode runs (RQEncoder.encode_topk)."""

    def __init__(self, enc, n, k, device):
        self.enc, self.k = enc, k
        self.local = torch.empty((enc.L, n, k), dtype=torch.int32, device=device)
        self.glob = torch.empty((enc.L, n, k), dtype=torch.int32, device=device)
        self.dist = torch.empty((enc.L, n, k), dtype=torch.float32, device=device)

    def level(self, l, x, buckets, fused=None):
        enc = self.enc
        if fused is not None and fused.den_out is not None:  # the assign of this level has written it
            fused = ops.FusedResidual(fused.levels, fused.normalize, fused.ca, fused.seg_ca, fused.cb, fused.seg_cb,
                                      fused.den_in, None)
        ops.assign_topk(x, enc.pcs[l], buckets, enc.raw_cands[l], self.k, fused=fused, workspace=enc._tws,
                        check=False, out=(self.local[l], self.glob[l], self.dist[l]))
        last_raw_column = l == enc.L - 1 and l > 0 and not (enc.sem.match_lookup and enc.sem.remap_last)
        if l == 0 or last_raw_column:  # these levels' ids are codebook rows
            self.local[l].copy_(self.glob[l])


class RQEncoder:
    def __init__(self, centers: Sequence[torch.Tensor], need_clusters: Sequence[int],
                 match: Optional[torch.Tensor] = None, group_dims: Sequence[int] = (),
                 weights: Optional[Sequence[Sequence[float]]] = None,
                 semantics: LevelSemantics = LevelSemantics(), device=None):
        device = device or torch.device("cuda", torch.cuda.current_device())
        self.device = device
        self.L = len(centers)
        self.need = list(need_clusters)
        self.sem = semantics
        self.dim = centers[0].shape[1]
        self.group_dims = list(group_dims) or [self.dim]
        self.weights = None
        if weights is not None and any(any(w != 1.0 for w in ws) for ws in weights):
            self.weights = [list(ws) for ws in weights]
        self.pcs = [ops.prepare_centers(c.to(device)) for c in centers]
        self.cands: List[Optional[ops.Candidates]] = []
        self.has_penalty = False
        self.n_groups = 1
        self._last_raw: Optional[ops.Candidates] = None  # the last level's lists before deduplication
        self._qws = None  # rqsid_quant_error workspace (sticky error word)
        self._tws = None  # rqsid_assign_topk workspace (sticky error word)
        self._xws = None  # rqsid_beam_expand workspace (sticky error word)
        # every level's list as built, before the duplicates leave it: what encode_topk ranks
        self.raw_cands: List[ops.Candidates] = []
        for l in range(self.L):
            if l == 0:
                c = ops.Candidates(torch.zeros(1, dtype=torch.int32, device=device),
                                   torch.full((1,), self.pcs[0].k, dtype=torch.int32, device=device), self.pcs[0].k)
            elif l < self.L - 1:
                c = ops.contiguous_candidates(self.need[l - 1], self.need[l], device)
            else:
                if match is not None and semantics.match_lookup:
                    m = match.to(device)
                    c = ops.match_to_candidates(m)
                    self._last_raw = c  # position = rank among the allowed columns (quant_error / decode)
                    self.has_penalty = bool((c.count == 0).any().item())
                    self.n_groups = m.shape[0]
                else:
                    k = self.pcs[l].k
                    c = ops.Candidates(torch.zeros(1, dtype=torch.int32, device=device),
                                       torch.full((1,), k, dtype=torch.int32, device=device), k)
            self.raw_cands.append(c)
            # bitwise-duplicate centres can never be the first minimum: drop them from the lists
            self.cands.append(ops.dedup_candidates(c, self.pcs[l].centers))
        # middle levels: the pair table of the deduplicated lists (the 2-term pairwise screen; None where a list
        # is wider than it covers), built once: codebook and lists are fixed for the encoder's life
        self.pairs: List[Optional[torch.Tensor]] = [
            ops.pair_table(self.pcs[l], self.cands[l]) if 0 < l < self.L - 1 else None for l in range(self.L)]
        self._ws = None
        self._bws = {}  # n_segments -> reusable rqsid_bucket workspace (sticky error word)
        self.last_rescored = []
        self.last_row_format = "f32"
        self.force_materialized = False

    def _workspace(self, n):
        if self._ws is None or self._ws.n_rows < n:
            if self._ws is not None:  # a bigger workspace replaces it: keep what its word recorded
                ops.check_error_words([self._ws.error_word()], "RQEncoder")
            self._ws = ops.AssignWorkspace(n, self.device)
        return self._ws

    def _bucket(self, keys, n_segments):
        ws = self._bws.get(n_segments)
        if ws is None:
            ws = self._bws[n_segments] = ops.bucket_workspace(n_segments, self.device)
        return ops.bucket(keys, n_segments, workspace=ws)

    def error_words(self):
        """Device views of the sticky error words this encoder's calls write (assign and bucketing)."""
        return ([self._ws.error_word()] if self._ws is not None else []) + \
            [ops.bucket_error_word(w, s) for s, w in self._bws.items()] + \
            ([self._qws.error_word()] if self._qws is not None else []) + \
            ([self._tws.error_word()] if self._tws is not None else []) + \
            ([self._xws.error_word()] if self._xws is not None else [])

    def check_errors(self) -> None:
        """Raise RuntimeError if any counter-driven write of this encoder's calls was dropped (one host sync)."""
        ops.check_error_words(self.error_words(), "RQEncoder.encode")

    def _weighted(self, x, l):
        if self.weights is None:
            return x
        return ops.scale_groups(x, self.group_dims, self.weights[l])

    def _last_mult(self) -> int:
        return self.need[self.L - 3] if self.sem.last_group_mult == "need_l_minus_2" else self.need[-2]

    @property
    def fused(self) -> bool:
        """Residuals computed inside the assignment kernels (no residual matrices in HBM).

        The kernels subtract per-SEGMENT residual centres, so the last level fuses only when its
        group id ``l1*mult + l2`` determines (l1, l2), i.e. mult >= need[1] (true for every shipped
        preset; the reference itself only makes sense there, Appendix A item 8), and only when the
        match lookup is on (the reference-bug predict mode is one unconstrained segment)."""
        if self.L > 3 or len(self.group_dims) != 1 or self.weights is not None or self.force_materialized:
            return False
        if self.L == 3 and not (self.sem.match_lookup and self._last_mult() >= self.need[1]):
            return False
        return True

    def encode(self, x: torch.Tensor, count_rescored: bool = False, check: Optional[bool] = None) -> torch.Tensor:
        """x: f32 (or, read natively on the fused path, f16 / bf16) [N, D] on the device -> int32 [N, L]
        semantic IDs (a transposed view of the level-major [L, N] buffer the kernels write; no copy).
        ``last_row_format`` ("f32", "f16", "bf16") records the row format the kernels read.  ``check`` (default: on unless the stream is
        being captured into a graph): read the device error words after the call (one host sync) and raise
        if a counter-driven list write was dropped; a captured step checks with ``check_errors()``."""
        if check is None:
            check = not torch.cuda.is_current_stream_capturing()
        if x.dim() != 2 or x.shape[1] != self.dim:
            raise ValueError(f"Input dimension {x.shape[-1]} does not match config embedding_dim {self.dim}")
        # 16-bit rows stay as they are on the fused path (every level reads x itself, rqsid_assign_x); the
        # materialised path writes fp32 residual matrices anyway and upcasts once, like any other dtype
        if not (self.fused and x.dtype in (torch.float16, torch.bfloat16)):
            x = x.float()
        x = x.contiguous()
        self.last_row_format = ops.ROW_FORMAT_NAMES[x.dtype]
        if self.L == 2:
            raise IndexError("list index out of range")  # reference: all_cluster_ids[-2] with one level
        n = x.shape[0]
        out = torch.empty((self.L, n), dtype=torch.int32, device=x.device)
        if n == 0:
            self.last_rescored = []
            return out.t()
        ws = self._workspace(n)
        self.last_rescored = []
        if self.fused:
            self._encode_fused(x, out, ws, count_rescored)
        else:
            self._encode_materialized(x, out, ws, count_rescored)
        if check:
            self.check_errors()
        return out.t()

    def encode_topk(self, x: torch.Tensor, k: int, check: Optional[bool] = None) -> TopK:
        """``encode(x)`` and, per level, the k nearest allowed centres of the segment the greedy path reached, for
        the level's own input vector (rqsid_assign_topk on the lists BEFORE deduplication, so duplicate centres
        take their places; on the last level with ``remap_last`` the local id is the rank among the allowed
        columns, as in ``encode``).  Fused encoders pass the fused residual chain (16-bit rows stay 16-bit);
        everything else ranks the matrices ``_encode_materialized`` builds.  1 <= k <= ops.TOPK_MAX.  ``check`` as
        in ``encode``."""
        if check is None:
            check = not torch.cuda.is_current_stream_capturing()
        k = int(k)
        if not 1 <= k <= ops.TOPK_MAX:
            raise ValueError(f"encode_topk: k = {k} (1..{ops.TOPK_MAX})")
        if x.dim() != 2 or x.shape[1] != self.dim:
            raise ValueError(f"Input dimension {x.shape[-1]} does not match config embedding_dim {self.dim}")
        if not (self.fused and x.dtype in (torch.float16, torch.bfloat16)):
            x = x.float()
        x = x.contiguous()
        self.last_row_format = ops.ROW_FORMAT_NAMES[x.dtype]
        if self.L == 2:
            raise IndexError("list index out of range")  # as encode: the reference has no two-level form
        n = x.shape[0]
        out = torch.empty((self.L, n), dtype=torch.int32, device=x.device)
        tk = _TopKLevels(self, n, k, x.device)
        self.last_rescored = []
        if n:
            ws = self._workspace(n)
            if self._tws is None:
                self._tws = ops.TopKWorkspace(n, k, self.device)
            if self.fused:
                self._encode_fused(x, out, ws, False, tk)
            else:
                self._encode_materialized(x, out, ws, False, tk)
            if check:
                self.check_errors()
        return TopK(out.t(), tk.local.permute(1, 0, 2), tk.glob.permute(1, 0, 2), tk.dist.permute(1, 0, 2))

    # ------------------------------------------------------------------ beam search
    def _beam_tables(self, dev):
        """Per level the candidate lists before deduplication plus the dead items' segment, and the last level's
        per-group residual centre rows with that segment's entry (row 0) appended; built once."""
        key = str(dev)
        if getattr(self, "_beam_tables_key", None) != key:
            cands = [ops.with_dead_segment(c) for c in self.raw_cands]
            zero = torch.zeros(1, dtype=torch.int32, device=dev)
            seg1 = torch.cat([torch.arange(self.need[0], dtype=torch.int32, device=dev), zero])
            seg2 = None
            if self.L == 3:
                seg2 = tuple(torch.cat([t, zero]) for t in self._last_segment_rows(dev))
            self._beam_tab, self._beam_tables_key = (cands, seg1, seg2), key
        return self._beam_tab

    def _beam_input(self, x, beam):
        """encode_beam's domain and refusals; the rows as the kernels read them and the beam as an int."""
        beam = int(beam)
        if not 1 <= beam <= ops.TOPK_MAX:
            raise ValueError(f"encode_beam: beam = {beam} (1..{ops.TOPK_MAX})")
        if x.dim() != 2 or x.shape[1] != self.dim:
            raise ValueError(f"Input dimension {x.shape[-1]} does not match config embedding_dim {self.dim}")
        if not self.sem.residual_global_id:
            raise ValueError("encode_beam: with residual_global_id=False the residual subtracts a centre other than "
                             "the one assigned (the reference's predict quirk): a path has no reconstruction error")
        if self.L == 2:
            raise IndexError("list index out of range")  # as encode: the reference has no two-level form
        if not self.fused or (self.L == 3 and self._last_raw is None):
            raise ValueError("encode_beam: fused encoders only (one dimension group, no weights, one or three levels "
                             "with the match lookup)")
        if x.dtype not in (torch.float16, torch.bfloat16):
            x = x.float()
        x = x.contiguous()
        self.last_row_format = ops.ROW_FORMAT_NAMES[x.dtype]
        return x, beam

    def encode_beam(self, x: torch.Tensor, beam: int, chunk_rows: Optional[int] = None,
                    check: Optional[bool] = None) -> Beam:
        """Beam-search encode: ``beam`` partial paths per row, each scored by its original-space
        reconstruction error, slot 0 always the greedy path (``paths[:, 0] == encode(x)``), the answer the slot with
        the smallest finite error (lowest slot on ties), so never worse than greedy.  1 <= beam <= ops.TOPK_MAX.
        Domain: the fused encoders (``self.fused``: one dimension group, no weights, L in {1, 3}) with
        ``residual_global_id=True``; anything else raises ValueError.  f16 / bf16 rows stay 16-bit.  A row with a
        non-finite value gets ids -1 and NaN errors; a row without a live path (penalty groups only) raises the
        KeyError ``encode`` raises.  Rows are processed in chunks of ``chunk_rows`` (default ``2**21 // beam``, so a
        chunk holds at most 2^21 items and its temporaries, about ``items * (12 * beam + 48)`` bytes, stay under
        300 MB at beam 8).  ``check`` as in ``encode``."""
        if check is None:
            check = not torch.cuda.is_current_stream_capturing()
        x, beam = self._beam_input(x, beam)
        n, dev, B, L = x.shape[0], x.device, beam, self.L
        chunk = int(chunk_rows) if chunk_rows else max(1, (1 << 21) // B)
        chunk = max(1, min(chunk, (2 ** 31 - 1) // B))
        paths = torch.empty((n, B, L), dtype=torch.int32, device=dev)
        perr = torch.empty((n, B), dtype=torch.float32, device=dev)
        if n:
            if self._tws is None:
                self._tws = ops.TopKWorkspace(min(n, chunk), B, self.device)
            if self._xws is None:
                self._xws = ops.BeamWorkspace(min(n, chunk) * B, B, self.device)
        for r0 in range(0, n, chunk):
            self._beam_chunk(x[r0:r0 + chunk], B, paths[r0:r0 + chunk], perr[r0:r0 + chunk])
        fin = torch.where(torch.isfinite(perr), perr, torch.full_like(perr, float("inf")))
        best = fin.min(1, keepdim=True).values
        slots = torch.arange(B, dtype=torch.int32, device=dev).expand(n, B)
        slot = torch.where(fin == best, slots, torch.full_like(slots, B)).min(1).values  # the lowest slot wins ties
        pick = slot.long()
        ids = paths.gather(1, pick.view(n, 1, 1).expand(n, 1, L)).reshape(n, L)
        rec = perr.gather(1, pick.view(n, 1)).reshape(n)
        if self.has_penalty and n:
            bad = torch.nonzero(torch.isinf(rec))
            if bad.numel():  # no live path: the row's groups allow no centre (encode: _finish_last)
                raise KeyError(int(bad[0, 0].item()))
        if check:
            self.check_errors()
        return Beam(ids, rec, paths, perr, slot)

    def _beam_chunk(self, x, B, paths, perr, depth=None):
        """One chunk of encode_beam: level 0 is rqsid_assign_topk with k = B and a merge with beam_in = 1; the
        later levels expand the B items of every row under their own parents and merge B * B expansions.
        ``depth``: stop after level depth - 1 (probe_prefixes); ``paths`` is then [n, B, depth]."""
        depth = self.L if depth is None else depth
        n, dev = x.shape[0], x.device
        norm = self.sem.normalize_residual
        cands, seg1, seg2 = self._beam_tables(dev)
        c0 = self.pcs[0].centers
        loc, glob, dist = ops.assign_topk(x, self.pcs[0], ops.single_segment(n, dev), self.raw_cands[0], B,
                                          workspace=self._tws, check=False)
        st = ops.beam_merge(n, 1, B, B, 0, loc, glob, dist, use_global=True, dead_key=self.need[0])
        if self.L == 3 and depth >= 2:
            items = n * B
            mult, n_groups = self._last_mult(), self.n_groups
            den1 = torch.empty(items, dtype=torch.float32, device=dev) if norm else None
            b = self._bucket(st.key, self.need[0] + 1)
            fr = ops.FusedResidual(1, norm, c0, seg1, den_out=den1)
            exp = ops.beam_expand(x, B, self.pcs[1], b, cands[1], B, fused=fr, workspace=self._xws, check=False)
            st = ops.beam_merge(n, B, B, B, 1, *exp, scale_in=st.scale, den=den1, path_in=st.path, use_global=False,
                                key_mult=mult, dead_key=n_groups)
            if depth == 2:
                paths.copy_(st.path.view(n, B, 2))
                perr.copy_(st.rec.view(n, B))
                return
            if (self.need[0] - 1) * mult + self.need[1] - 1 >= n_groups:  # as _last_level_buckets (one host sync)
                gmax = int(st.key.max().item())
                if gmax > n_groups:
                    raise IndexError(f"index {gmax} is out of bounds for axis 0 with size {n_groups}")
            den2 = torch.empty(items, dtype=torch.float32, device=dev) if norm else None
            b = self._bucket(st.key, n_groups + 1)
            fr = ops.FusedResidual(2, norm, c0, seg2[0], self.pcs[1].centers, seg2[1], den_in=st.den_next,
                                   den_out=den2)
            exp = ops.beam_expand(x, B, self.pcs[2], b, cands[2], B, fused=fr, workspace=self._xws, check=False)
            st = ops.beam_merge(n, B, B, B, 2, *exp, scale_in=st.scale, den=den2, path_in=st.path,
                                use_global=not self.sem.remap_last)
        paths.copy_(st.path.view(n, B, depth))
        perr.copy_(st.rec.view(n, B))

    def probe_prefixes(self, q: torch.Tensor, depth: int, probes: int, chunk_rows: Optional[int] = None,
                       check: Optional[bool] = None) -> torch.Tensor:
        """The ``probes`` ID prefixes of length ``depth`` nearest to every row of ``q``: i32 [M, probes, depth], the
        beam of ``encode_beam`` stopped after level ``depth - 1``.  Slot 0 is
        ``encode(q)[:, :depth]``; the live slots hold pairwise distinct prefixes in ascending (error, parent, place)
        order after slot 0; a dead slot is -1.  ``probe_prefixes(q, L, B)`` equals ``encode_beam(q, B).paths``.
        Domain and refusals are ``encode_beam``'s."""
        if check is None:
            check = not torch.cuda.is_current_stream_capturing()
        depth = int(depth)
        if not 1 <= depth <= self.L:
            raise ValueError(f"probe_prefixes: depth = {depth} (1..{self.L})")
        q, B = self._beam_input(q, probes)
        n, dev = q.shape[0], q.device
        chunk = int(chunk_rows) if chunk_rows else max(1, (1 << 21) // B)
        chunk = max(1, min(chunk, (2 ** 31 - 1) // B))
        paths = torch.empty((n, B, depth), dtype=torch.int32, device=dev)
        perr = torch.empty((n, B), dtype=torch.float32, device=dev)
        if n:
            if self._tws is None:
                self._tws = ops.TopKWorkspace(min(n, chunk), B, self.device)
            if self._xws is None:
                self._xws = ops.BeamWorkspace(min(n, chunk) * B, B, self.device)
        for r0 in range(0, n, chunk):
            self._beam_chunk(q[r0:r0 + chunk], B, paths[r0:r0 + chunk], perr[r0:r0 + chunk], depth)
        if check:
            self.check_errors()
        return paths

    def search(self, x: torch.Tensor, index: "ops.IdCells", q: torch.Tensor, k: int = 10, probes: int = 4,
               depth: Optional[int] = None, metric: str = "cosine",
               query_self: Optional[torch.Tensor] = None,
               workspace: Optional["ops.ProbeKnnWorkspace"] = None) -> "IndexSearch":
        """The k nearest rows of the catalogue ``x`` for every row of ``q``, looked up through the IDs alone
        (DESIGN.md §3.3f): ``probe_prefixes(q, depth, probes)``, their position ranges in ``index`` (the ``IdCells``
        of the catalogue's IDs) and one ``ops.probe_knn`` over ``index.order``.  ``depth`` defaults to
        max(1, L - 1).  ``scanned`` counts the catalogue positions each query read.  ``workspace``: a reusable
        ``ops.ProbeKnnWorkspace`` (its ``counters()`` then describe this search)."""
        depth = max(1, self.L - 1) if depth is None else int(depth)
        prefixes = self.probe_prefixes(q, depth, probes)
        lo, hi = index.prefix_ranges(prefixes)
        if q.dtype != x.dtype:
            q = q.to(x.dtype)
        rows, val, scanned = ops.probe_knn(x, q.contiguous(), k, lo, hi, metric=metric, order=index.order,
                                           query_self=query_self, workspace=workspace)
        return IndexSearch(rows, val, scanned, prefixes)

    def _last_level_buckets(self, out, l, n, device):
        if self.sem.match_lookup:
            mult = self.need[l - 2] if self.sem.last_group_mult == "need_l_minus_2" else self.need[-2]
            grp = out[l - 2] * mult + out[l - 1]
            # the reference indexes match_matrix_np[before] (hierarchical_rq_kmeans.py:1279-1281) and raises
            # IndexError past the last group; bucketing would silently drop such rows.  Check on the device
            # values only when the largest possible id can reach it (never for the shipped presets:
            # need[l-2] == need[l-1]), so the common encode has no host sync here.
            if (self.need[l - 2] - 1) * mult + self.need[l - 1] - 1 >= self.n_groups:
                gmax = int(grp.max().item())
                if gmax >= self.n_groups:
                    raise IndexError(f"index {gmax} is out of bounds for axis 0 with size {self.n_groups}")
            return self._bucket(grp, self.n_groups)
        return ops.single_segment(n, device)

    def _finish_last(self, out, l, glob):
        if not (self.sem.match_lookup and self.sem.remap_last):
            out[l].copy_(glob)
        elif self.has_penalty:
            bad = torch.nonzero(out[l] < 0)
            if bad.numel():
                # reference: mapping_result[prev_id][cur_id] KeyError (:1084)
                raise KeyError(int(glob[bad[0, 0]].item()))

    def _encode_fused(self, x, out, ws, count_rescored, tk=None):
        n = x.shape[0]
        dev = x.device
        norm = self.sem.normalize_residual
        # level 0 is one segment over every centre: the local id IS the global id
        b = ops.single_segment(n, dev)
        ops.assign(x, self.pcs[0], b, self.cands[0], out_local=out[0], out_global=out[0], workspace=ws)
        if tk is not None:
            tk.level(0, x, b)
        if count_rescored:
            self.last_rescored.append(ws.rescored())
        if self.L == 1:
            return
        n1 = torch.empty(n, dtype=torch.float32, device=dev) if norm else None
        glob1 = torch.empty(n, dtype=torch.int32, device=dev)
        b = self._bucket(out[0], self.need[0]) if self.L == 3 else self._last_level_buckets(out, 1, n, dev)
        fr1 = ops.FusedResidual(1, norm, self.pcs[0].centers, None, den_out=n1)
        ops.assign(x, self.pcs[1], b, self.cands[1], out_local=out[1], out_global=glob1, workspace=ws, fused=fr1,
                   pair=self.pairs[1])
        if tk is not None:
            tk.level(1, x, b, fr1)
        if count_rescored:
            self.last_rescored.append(ws.rescored())
        glob2 = torch.empty(n, dtype=torch.int32, device=dev)
        b = self._last_level_buckets(out, 2, n, dev)
        seg_ca, seg_cb = self._last_segment_rows(dev)
        fr2 = ops.FusedResidual(2, norm, self.pcs[0].centers, seg_ca, self.pcs[1].centers, seg_cb, den_in=n1)
        ops.assign(x, self.pcs[2], b, self.cands[2], out_local=out[2], out_global=glob2, workspace=ws, fused=fr2)
        if tk is not None:
            tk.level(2, x, b, fr2)
        if count_rescored:
            self.last_rescored.append(ws.rescored())
        self._finish_last(out, 2, glob2)

    def _last_segment_rows(self, dev):
        """Per-group residual centre rows of the last level: group g = l1*mult + l2 subtracts
        c0[l1] and c1[l1*need1 + l2] (training / raw id, :901) or c1[l2] (predict's modded id, :1143)."""
        key = (str(dev), self.sem.residual_global_id)
        if getattr(self, "_seg_rows_key", None) != key:
            mult, n1 = self._last_mult(), self.need[1]
            g = torch.arange(self.n_groups, dtype=torch.int64, device=dev)
            l1, l2 = g // mult, (g % mult).clamp(max=n1 - 1)
            seg_ca = l1.clamp(max=self.pcs[0].k - 1).to(torch.int32)
            cb = l1 * n1 + l2 if self.sem.residual_global_id else l2
            seg_cb = cb.clamp(max=self.pcs[1].k - 1).to(torch.int32)
            self._seg_rows, self._seg_rows_key = (seg_ca, seg_cb), key
        return self._seg_rows

    def _encode_materialized(self, x, out, ws, count_rescored, tk=None):
        n = x.shape[0]
        cur = x
        glob = torch.empty(n, dtype=torch.int32, device=x.device)
        for l in range(self.L):
            w = self._weighted(cur, l)
            if l == 0:
                b = ops.single_segment(n, x.device)
                ops.assign(w, self.pcs[0], b, self.cands[0], out_local=out[0], out_global=glob, workspace=ws)
                out[0].copy_(glob)
            elif l < self.L - 1:
                b = self._bucket(out[l - 1], self.need[l - 1])
                ops.assign(w, self.pcs[l], b, self.cands[l], out_local=out[l], out_global=glob, workspace=ws,
                           pair=self.pairs[l])
            else:
                b = self._last_level_buckets(out, l, n, x.device)
                ops.assign(w, self.pcs[l], b, self.cands[l], out_local=out[l], out_global=glob, workspace=ws)
                self._finish_last(out, l, glob)
            if tk is not None:
                tk.level(l, w, b)
            if count_rescored:
                self.last_rescored.append(ws.rescored())
            if l < self.L - 1:
                src = w if self.sem.residual_from_weighted else cur
                cid = glob if self.sem.residual_global_id else out[l]
                cur = ops.residual(src, self.pcs[l].centers, cid, self.group_dims, self.sem.normalize_residual)

    # ------------------------------------------------------------------ quantisation error / decode
    def global_rows(self, ids: torch.Tensor) -> List[torch.Tensor]:
        """Per level the GLOBAL codebook row behind semantic IDs ``ids`` [N, L] (i32 [N] each; -1 where an id
        does not name a centre): level 0 the id, a middle level ``parent * need[l] + id``, the last level the
        ``id``-th allowed column of the group's match row (rank remap) or the raw column."""
        if ids.dim() != 2 or ids.shape[1] != self.L:
            raise ValueError(f"ids must be [N, {self.L}], got {tuple(ids.shape)}")
        col = [ids[:, l].to(torch.int64) for l in range(self.L)]
        out = []
        for l in range(self.L):
            if l == 0:
                g = col[0]
            elif l < self.L - 1:
                ok = (col[l] >= 0) & (col[l] < self.need[l]) & (col[l - 1] >= 0)
                g = torch.where(ok, col[l - 1] * self.need[l] + col[l], -1)
            elif self._last_raw is not None and self.sem.remap_last:
                c = self._last_raw
                grp = col[l - 2] * self._last_mult() + col[l - 1]
                gc = grp.clamp(0, self.n_groups - 1)
                ok = (grp == gc) & (col[l] >= 0) & (col[l] < c.count.long()[gc])
                pos = (c.base.long()[gc] + col[l]).clamp(0, c.idx.numel() - 1)
                g = torch.where(ok, c.idx.long()[pos], -1)
            else:
                g = col[l]
            out.append(g.to(torch.int32).contiguous())
        return out

    @property
    def quant_error_fused(self) -> bool:
        """rqsid_quant_error's domain: one dimension group, no weights, at most three levels."""
        return self.L <= 3 and len(self.group_dims) == 1 and self.weights is None and not self.force_materialized

    def quant_error(self, x: torch.Tensor, ids: Optional[torch.Tensor] = None,
                    check: Optional[bool] = None) -> QuantError:
        """Quantisation error of ``ids`` (default: ``encode(x)``) for the rows ``x``: per level the distance from the
        level's input vector to the centre it was given, the row norms, the reconstruction error in the original
        space and fp64 totals.  One streaming HIP pass (rqsid_quant_error) for one dimension group without weights
        and L <= 3; otherwise the same quantities from ops.residual / ops.scale_groups and fp64 torch norms.
        ``check`` as in ``encode``: an id that names no centre raises RuntimeError (its rows hold NaN)."""
        if not self.sem.residual_global_id:
            raise ValueError("quant_error: with residual_global_id=False the residual subtracts a centre other than "
                             "the one assigned (the reference's predict quirk): the error of the encoding is undefined")
        if check is None:
            check = not torch.cuda.is_current_stream_capturing()
        if x.dim() != 2 or x.shape[1] != self.dim:
            raise ValueError(f"Input dimension {x.shape[-1]} does not match config embedding_dim {self.dim}")
        if not (self.quant_error_fused and x.dtype in (torch.float16, torch.bfloat16)):
            x = x.float()
        x = x.contiguous()
        if ids is None:
            ids = self.encode(x, check=check)
        else:
            ids = ids.to(device=x.device, dtype=torch.int32)
            if self.L == 2:
                raise IndexError("list index out of range")  # as encode: the reference has no two-level form
        if ids.shape[0] != x.shape[0]:
            raise ValueError(f"ids has {ids.shape[0]} rows, x {x.shape[0]}")
        glob = self.global_rows(ids)
        n = x.shape[0]
        if not self.quant_error_fused:
            return self._quant_error_materialized(x, ids, glob, check)
        order = None
        if self.L == 3 and self._last_raw is not None and n > 0:
            # process in the order of the last level's groups: c0 / c1 rows change once per group
            grp = (ids[:, 0] * self._last_mult() + ids[:, 1]).clamp(0, self.n_groups - 1)
            order = self._bucket(grp, self.n_groups).row_index
        if self._qws is None:
            self._qws = ops.QuantErrorWorkspace(n, self.device)
        err, x_norm, sums = ops.quant_error(x, [pc.centers for pc in self.pcs], glob, self.sem.normalize_residual,
                                            row_order=order, workspace=self._qws, check=False)
        if check:
            try:
                ops.check_error_words([self._qws.error_word()], "RQEncoder.quant_error", ops.QUANT_ERROR_WORD)
            except RuntimeError:
                self._qws = None  # the word is sticky: the next call starts from a clean workspace
                raise
        rec = err.clone()
        if self.sem.normalize_residual:
            for l in range(1, self.L):
                rec[:, l:] *= (err[:, l - 1] + 1e-8).unsqueeze(1)
        return QuantError(ids, err, x_norm, rec[:, self.L - 1], sums, rec)

    def _quant_error_materialized(self, x, ids, glob, check) -> QuantError:
        """quant_error outside the kernel's domain (several groups, weights, L > 3): the chain of
        _encode_materialized with every norm taken in fp64.  Original-space error: group g of level l's raw residual
        stands for ``prod_{j<l} den_jg / prod_{j<=l} w_jg`` times as much of x (weights enter only when the
        residuals are taken from the weighted data)."""
        n, G = x.shape[0], len(self.group_dims)
        dev = x.device
        cur = x
        err = torch.empty((n, self.L), dtype=torch.float32, device=dev)
        rec = torch.empty((n, self.L), dtype=torch.float32, device=dev)
        scale = torch.ones((n, G), dtype=torch.float64, device=dev)
        bad = torch.zeros(n, dtype=torch.bool, device=dev)
        for l in range(self.L):
            w = self._weighted(cur, l)
            src = w if self.sem.residual_from_weighted else cur
            if self.sem.residual_from_weighted and self.weights is not None:
                scale = scale / torch.tensor(self.weights[l], dtype=torch.float64, device=dev)
            c = self.pcs[l].centers
            bad |= (glob[l] < 0) | (glob[l] >= c.shape[0])
            d = ops.residual(src, c, glob[l], self.group_dims, normalize=False)
            gs = torch.stack([blk.double().pow(2).sum(1) for blk in d.split(self.group_dims, dim=1)], 1)
            err[:, l] = gs.sum(1).sqrt().float()
            rec[:, l] = (gs * scale * scale).sum(1).sqrt().float()
            err[bad, l] = float("nan")
            rec[bad, l] = float("nan")
            if l < self.L - 1:
                if self.sem.normalize_residual:
                    scale = scale * (gs.sqrt().float() + 1e-8).double()
                cur = ops.residual(src, c, glob[l], self.group_dims, self.sem.normalize_residual)
        x_norm = x.double().pow(2).sum(1).sqrt().float()
        good = ~bad
        sums = torch.cat([err[good].double().pow(2).sum(0), x_norm[good].double().pow(2).sum().reshape(1)])
        if check and bool(bad.any().item()):
            raise RuntimeError("RQEncoder.quant_error: an id names no centre")
        return QuantError(ids, err, x_norm, rec[:, self.L - 1], sums, rec)

    def cluster_report(self, x: torch.Tensor, ids: Optional[torch.Tensor] = None, **kw):
        """The reference's quality check of these IDs (silhouette, Calinski-Harabasz, Davies-Bouldin per prefix depth,
        in the original space): ``cluster_report.cluster_report(self, x, ids, **kw)``."""
        from .cluster_report import cluster_report
        return cluster_report(self, x, ids, **kw)

    # ------------------------------------------------------------------ ID cells: collisions, unique IDs
    def id_sizes(self) -> List[int]:
        """Per level the exclusive upper bound of the IDs ``encode`` returns (the radices of the cell index)."""
        sizes = [self.pcs[0].k] + [self.need[l] for l in range(1, self.L - 1)]
        if self.L > 1:
            remap = self._last_raw is not None and self.sem.remap_last
            sizes.append(max(self._last_raw.count_max, 1) if remap else self.pcs[-1].k)
        return sizes

    def id_index(self, ids: torch.Tensor, rank_key: Optional[torch.Tensor] = None) -> "ops.IdCells":
        """The cell index of ``ids`` [N, L] (``ops.id_cells`` with this encoder's level sizes): which rows share an
        ID, each row's rank in its cell by ``rank_key`` (None: by row number), prefix ranges and counters."""
        ids = ids.to(device=self.device, dtype=torch.int32).contiguous()
        if ids.dim() != 2 or ids.shape[1] != self.L:
            raise ValueError(f"ids must be [N, {self.L}], got {tuple(ids.shape)}")
        return ops.id_cells(ids, self.id_sizes(), rank_key)

    def id_trie(self, ids: torch.Tensor, tokens: Optional["ops.TokenMap"] = None, comm=None):
        """The ``SemanticIDTrie`` of ``ids`` [N, L] (semantic_id_trie.py): the trie a constrained decoder walks, over
        this encoder's level sizes; ``tokens`` None: the identity token map.  Single process only."""
        if comm is not None:
            raise NotImplementedError("id_trie: the multi-GPU form is not built (single process only)")
        from .semantic_id_trie import SemanticIDTrie
        return SemanticIDTrie.from_index(self.id_index(ids), tokens)

    def unique_ids(self, x: torch.Tensor, ids: Optional[torch.Tensor] = None) -> torch.Tensor:
        """int32 [N, L + 1]: the semantic IDs of ``x`` (default ``encode(x)``) with one more token that makes every row
        distinct: the row's rank among the rows that share its ID, by original-space reconstruction error
        (``quant_error(x, ids).recon_err``; ties and NaN fall to row order), so token 0 is the row the ID describes
        best.  Raises ValueError with ``residual_global_id=False``, as ``quant_error`` does."""
        qe = self.quant_error(x, ids)
        index = self.id_index(qe.ids, qe.recon_err.contiguous())
        return torch.cat([qe.ids, index.rank.unsqueeze(1)], 1).contiguous()

    def collision_report(self, x: torch.Tensor, ids: Optional[torch.Tensor] = None, **kw):
        """Which IDs are shared and by how many rows: ``collision_report.collision_report(self, x, ids, **kw)``."""
        from .collision_report import collision_report
        return collision_report(self, x, ids, **kw)

    def decode(self, ids: torch.Tensor, err: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Reconstruction f32 [N, D] of semantic IDs (plain torch gathers).  Plain residuals: the sum of the levels'
        centres.  Normalised residuals: ``c0 + d0 (c1 + d1 c2)`` with ``d_l = err[:, l] + 1e-8`` from ``quant_error``
        (the divisors are not recoverable from the IDs, so ``err`` is required)."""
        if not self.sem.residual_global_id:
            raise ValueError("decode: undefined with residual_global_id=False (see quant_error)")
        if self.weights is not None or (self.sem.normalize_residual and len(self.group_dims) != 1):
            raise ValueError("decode: one dimension group without weights only")
        if self.sem.normalize_residual and self.L > 1 and err is None:
            raise ValueError("decode: normalised residuals need err (quant_error's per-level norms)")
        ids = ids.to(device=self.device, dtype=torch.int32)
        glob = self.global_rows(ids)
        for l, g in enumerate(glob):
            if g.numel() and (int(g.min().item()) < 0 or int(g.max().item()) >= self.pcs[l].k):
                raise IndexError(f"decode: a level-{l} id names no centre")
        rows = [self.pcs[l].centers[glob[l].long()] for l in range(self.L)]
        out = rows[self.L - 1]
        for l in range(self.L - 2, -1, -1):
            if self.sem.normalize_residual:
                out = out * (err[:, l].to(self.device).float() + 1e-8).unsqueeze(1)
            out = rows[l] + out
        return out
