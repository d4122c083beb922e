"""The reference's src/generator/semantic_id_trie.py on the device: the same class names and
signatures over the trie tables of ``ops.id_trie``.

* ``SemanticIDTrie`` holds the tables (``ops.IdTrie``), the token tables (``ops.TokenMap``) and, when it was built from
  IDs, their cell index (``ops.IdCells``), so a decoded leaf leads to its rows.
* ``ConstrainedLogitsProcessor.__call__`` is one ``ops.trie_mask`` call for the whole batch, where the reference loops
  over the rows in Python (``tolist``, a backwards scan, a dict walk, one assignment per allowed token, ``masked_fill``).
* ``constrained_beam_search`` is the retrieval-style decode the reference does not have: ``L`` calls of
  ``ops.trie_beam_step`` over node numbers, ending in cells and, through the index, in positions of ``order``.

Nothing here imports ``transformers``: a tokenizer enters as a table of token numbers (``ops.TokenMap``).  There is no
CPU path for the mask or the beam step; the small host-side queries (``get_valid_next_tokens`` and friends) read a host
copy of the tables, fetched once.
"""
from __future__ import annotations

from collections import Counter
from dataclasses import dataclass
from typing import Callable, Dict, List, Optional, Sequence, Set

import numpy as np
import torch

from . import io as rq_io
from . import ops


class SemanticIDTrie:
    """``SemanticIDTrie(tokenizer, semantic_ids_file)`` as in the reference: reads the jsonl, skips entries whose
    ``semantic_ids`` do not hold 3 values, never inserts an ID with a token the tokenizer does not know."""

    def __init__(self, tokenizer, semantic_ids_file: str, device=None):
        tokens = ops.TokenMap.from_tokenizer(tokenizer, getattr(tokenizer, "eos_token_id", None) or 0, levels=3,
                                             device=device)
        _, ids = rq_io.read_semantic_ids(semantic_ids_file, levels=3)
        self.tokenizer = tokenizer
        self._init(self._index_of(ids, tokens.sizes, tokens), tokens)

    @staticmethod
    def _index_of(ids, sizes, tokens: ops.TokenMap) -> ops.IdCells:
        ids = np.asarray(ids).reshape(-1, len(sizes)).astype(np.int64)
        # an ID outside its level's size has no token name the tokenizer could know: dropped, as the reference does
        ok = ((ids >= 0) & (ids < np.asarray(sizes, dtype=np.int64))).all(1)
        dev = tokens.level_tok.device
        return ops.id_cells(torch.from_numpy(ids[ok].astype(np.int32)).to(dev).contiguous(), tuple(sizes))

    def _init(self, index: Optional[ops.IdCells], tokens: ops.TokenMap, trie: Optional[ops.IdTrie] = None):
        self.tokens = tokens
        self.index = index
        self.trie = trie if trie is not None else ops.id_trie(index, tokens.keep_cells(index))
        self._host = None
        self._leaf_ids = None
        self._valid = None

    @classmethod
    def from_ids(cls, ids, sizes: Sequence[int], tokens: Optional[ops.TokenMap] = None) -> "SemanticIDTrie":
        """From ID tuples (int [N, L], numpy or tensor) with the levels' ``sizes``; ``tokens`` None: the identity map."""
        if isinstance(ids, torch.Tensor):
            ids = ids.cpu().numpy()
        tokens = tokens if tokens is not None else ops.TokenMap.identity(sizes)
        if tuple(tokens.sizes) != tuple(int(s) for s in sizes):
            raise ValueError(f"SemanticIDTrie: the token map's sizes {tokens.sizes} are not {tuple(sizes)}")
        self = cls.__new__(cls)
        self.tokenizer = None
        self._init(cls._index_of(ids, tokens.sizes, tokens), tokens)
        return self

    @classmethod
    def from_index(cls, index: ops.IdCells, tokens: Optional[ops.TokenMap] = None) -> "SemanticIDTrie":
        """From a cell index (``ops.id_cells``, ``RQEncoder.id_index``); ``tokens`` None: the identity map."""
        tokens = tokens if tokens is not None else ops.TokenMap.identity(index.sizes)
        if tuple(tokens.sizes) != tuple(index.sizes):
            raise ValueError(f"SemanticIDTrie: the token map's sizes {tokens.sizes} are not the index's {index.sizes}")
        self = cls.__new__(cls)
        self.tokenizer = None
        self._init(index, tokens)
        return self

    # ------------------------------------------------------------------ host-side queries (the reference's methods)
    @property
    def levels(self) -> int:
        return len(self.tokens.sizes)

    def host_tables(self) -> dict:
        """The written part of the tables as numpy arrays (``ops.IdTrie.to_arrays``), fetched once."""
        if self._host is None:
            self._host = self.trie.to_arrays()
        return self._host

    def _walk(self, prefix_tokens):
        """(depth, node) reached by the token sequence, or None."""
        h = self.host_tables()
        node = 0
        if len(prefix_tokens) > self.levels:
            return None
        for d, tok in enumerate(prefix_tokens):
            tok = int(tok)
            code = int(self.tokens.tok_code_host[tok]) if 0 <= tok < self.tokens.vocab_size else -1
            if code < 0 or code >> 24 != d:
                return None
            off, vals = h[f"child_off{d}"], h[f"value{d}"]
            lo, hi = int(off[node]), int(off[node + 1])
            at = lo + int(np.searchsorted(vals[lo:hi], code & 0xFFFFFF))
            if at >= hi or int(vals[at]) != code & 0xFFFFFF:
                return None
            node = at
        return len(prefix_tokens), node

    def get_valid_next_tokens(self, prefix_tokens: List[int]) -> Set[int]:
        """The token numbers that may follow ``prefix_tokens`` (empty for a prefix the trie does not hold)."""
        at = self._walk(list(prefix_tokens))
        if at is None or at[0] >= self.levels:
            return set()
        d, node = at
        h = self.host_tables()
        lo, hi = int(h[f"child_off{d}"][node]), int(h[f"child_off{d}"][node + 1])
        toks = self.tokens.level_tok_host[self.tokens.level_off[d] + h[f"value{d}"][lo:hi]]
        return {int(t) for t in toks if t >= 0}

    def is_valid_sequence(self, token_sequence: List[int]) -> bool:
        return len(token_sequence) == self.levels and self._walk(list(token_sequence)) is not None

    def leaf_ids(self) -> np.ndarray:
        """int32 [leaves, L]: the IDs in the trie, in lexicographic order (from the tables alone)."""
        if self._leaf_ids is None:
            h = self.host_tables()
            ids = np.zeros((1, 0), dtype=np.int32)
            for d in range(self.levels):
                parent = np.repeat(np.arange(len(ids)), np.diff(h[f"child_off{d}"]))
                ids = np.concatenate([ids[parent], h[f"value{d}"][:, None]], 1)
            self._leaf_ids = ids.astype(np.int32)
        return self._leaf_ids

    def get_all_valid_sequences(self) -> List[List[int]]:
        """Every valid token sequence, in lexicographic order of the IDs.  (The reference returns them in the order
        its dicts were filled, the file's order; the set is the same.)"""
        ids = self.leaf_ids()
        toks = np.stack([self.tokens.level_tok_host[self.tokens.level_off[l] + ids[:, l]] for l in range(self.levels)], 1)
        return [[int(t) for t in row] for row in toks]

    @property
    def valid_semantic_ids(self) -> Set[tuple]:
        """The IDs in the trie as a set of tuples (built on first use)."""
        if self._valid is None:
            self._valid = {tuple(int(v) for v in row) for row in self.leaf_ids()}
        return self._valid

    def get_statistics(self) -> Dict:
        """The reference's four keys for three levels (``total_valid_sequences``, ``unique_l1_tokens``,
        ``l2_distribution``, ``l3_distribution``: how many nodes have how many children); with L levels,
        ``l{d + 1}_distribution`` for every depth d in 1 .. L - 1."""
        h = self.host_tables()
        cnt = [int(c) for c in h["count"]]
        stats = {"total_valid_sequences": cnt[-1], "unique_l1_tokens": cnt[1]}
        for d in range(1, self.levels):
            fan = Counter(int(v) for v in np.diff(h[f"child_off{d}"]))
            stats[f"l{d + 1}_distribution"] = dict(fan)
        return stats

    def report(self) -> Dict:
        """``trie_report.json``: ``get_statistics`` with string keys, the nodes per depth, and the mean and the largest
        number of children of a node per depth."""
        h = self.host_tables()
        stats = {k: ({str(n): c for n, c in sorted(v.items())} if isinstance(v, dict) else v)
                 for k, v in self.get_statistics().items()}
        fan = []
        for d in range(self.levels):
            n = np.diff(h[f"child_off{d}"])
            fan.append({"depth": d, "nodes": int(len(n)), "mean_children": float(n.mean()) if len(n) else None,
                        "max_children": int(n.max()) if len(n) else 0})
        return {"statistics": stats, "nodes_per_depth": [int(c) for c in h["count"]], "children_per_depth": fan}


class ConstrainedLogitsProcessor:
    """``ConstrainedLogitsProcessor(trie, tokenizer, eos_token_id)``: ``__call__(input_ids, scores)`` masks ``scores``
    in place with one ``ops.trie_mask`` call and returns it.  No host read per step; ``last`` holds the per-row kind /
    node / count of the latest call and ``error_word()`` the sticky device error word."""

    def __init__(self, trie: SemanticIDTrie, tokenizer, eos_token_id: int):
        self.trie = trie
        self.tokenizer = tokenizer
        self.eos_token_id = int(eos_token_id)
        self.tokens = trie.tokens.with_eos(self.eos_token_id)
        self.workspace = None
        self.last = None

    def __call__(self, input_ids: torch.Tensor, scores: torch.Tensor) -> torch.Tensor:
        if scores.shape[1] != self.tokens.vocab_size:  # logits padded beyond the tokenizer's vocabulary (built once)
            self.tokens = self.tokens.with_vocab(scores.shape[1])
        if self.workspace is None or self.workspace.bytes < 256 + 16 * scores.shape[0]:
            self.workspace = ops.TrieMaskWorkspace(scores.shape[0], scores.device)
        self.last = ops.trie_mask(self.trie.trie, self.tokens, input_ids, scores, self.workspace, check=False)
        return scores

    def error_word(self) -> Optional[torch.Tensor]:
        return None if self.workspace is None else self.workspace.error_word()


def create_constrained_logits_processor(trie: SemanticIDTrie, tokenizer) -> ConstrainedLogitsProcessor:
    return ConstrainedLogitsProcessor(trie, tokenizer, tokenizer.eos_token_id)


@dataclass
class BeamSearchResult:
    """``constrained_beam_search``'s answer, [B, beam] each (an unfilled slot: -1 / -inf / -1s / 0 / 0): ``cells`` (cell
    numbers of the index), ``scores`` f32, ``ids`` i32 [B, beam, L], and the half-open ranges ``lo`` / ``hi`` of the
    found IDs' rows in ``index.order`` (None without an index)."""
    cells: torch.Tensor
    scores: torch.Tensor
    ids: torch.Tensor
    lo: Optional[torch.Tensor]
    hi: Optional[torch.Tensor]


def constrained_beam_search(trie: SemanticIDTrie, step_fn: Callable, batch: int, beam: int) -> BeamSearchResult:
    """Decode ``batch`` IDs along the trie with ``beam`` hypotheses each: ``L`` calls of ``ops.trie_beam_step``.
    ``step_fn(depth, values_so_far)`` gets the hypotheses' ID values so far (i32 [B, beam_in, depth]; beam_in is 1 at
    depth 0; -1 in a dead hypothesis) and returns log-probabilities [B * beam_in, V] (f32 / f16 / bf16)."""
    t, tok = trie.trie, trie.tokens
    dev = tok.level_tok.device
    node = torch.zeros(batch, 1, dtype=torch.int32, device=dev)
    score = None
    values = torch.zeros(batch, 1, 0, dtype=torch.int32, device=dev)
    for d in range(trie.levels):
        step = ops.trie_beam_step(t, tok, d, node, score, step_fn(d, values), beam)
        parent = step.parent.clamp_min(0).long().unsqueeze(-1).expand(-1, -1, d)
        values = torch.cat([torch.gather(values, 1, parent), step.value.unsqueeze(-1)], 2)
        values = torch.where((step.node < 0).unsqueeze(-1), torch.full_like(values, -1), values)
        node, score = step.node, step.score
    found = node >= 0
    cells = torch.where(found, t.leaf_cell[node.clamp_min(0).long()] if t.capacity else node, torch.full_like(node, -1))
    lo = hi = None
    if trie.index is not None:
        off = trie.index.cell_off
        at = cells.clamp_min(0).long()
        zero = torch.zeros_like(cells)
        lo, hi = torch.where(found, off[at], zero), torch.where(found, off[at + 1], zero)
    return BeamSearchResult(cells, score, values, lo, hi)
