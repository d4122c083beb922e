"""Plain numpy / dict model of the ID trie, of rqsid_trie_mask's rules 1 - 5 and of rqsid_trie_beam_step's order
(include/rqsid.h), written from those rules: the yardstick of the trie tests, checked itself against the reference's
recorded outputs (tests/golden/trie.npz, trie_long.npz) in test_trie_model.py."""
import numpy as np

KIND_WALK, KIND_COMPLETE, KIND_DEAD = 0, 1, 2


def tables(cells, levels, keep=None):
    """The trie tables of ``cells`` (int [n, L], distinct, lexicographically ascending) by numpy.unique over prefixes:
    ``count`` [L + 1], ``value`` (list of L arrays), ``child_off`` (list of L arrays, count[d] + 1 entries each),
    ``leaf_cell``."""
    cells = np.asarray(cells, dtype=np.int64).reshape(-1, levels)
    idx = np.arange(len(cells))
    if keep is not None:
        idx = idx[np.asarray(keep).astype(bool)]
    kept = cells[idx]
    count, value, child_off = [1], [], []
    prev = np.zeros((1, 0), dtype=np.int64)  # the root
    for d in range(1, levels + 1):
        uniq = np.unique(kept[:, :d], axis=0) if len(kept) else np.zeros((0, d), dtype=np.int64)
        count.append(len(uniq))
        value.append(uniq[:, d - 1].astype(np.int32))
        # numpy.unique sorts the rows, so a node's children are a run; its parent is the number of runs before it
        new_parent = np.ones(len(uniq), dtype=bool)
        if len(uniq) > 1:
            new_parent[1:] = (uniq[1:, :d - 1] != uniq[:-1, :d - 1]).any(1)
        parent = np.cumsum(new_parent) - 1
        assert len(uniq) == 0 or parent[-1] == len(prev) - 1
        child_off.append(np.searchsorted(parent, np.arange(len(prev) + 1)).astype(np.int32))
        prev = uniq
    return dict(count=np.asarray(count, dtype=np.int32), value=value, child_off=child_off,
                leaf_cell=idx.astype(np.int32))


def tables_sorted(cells, levels, keep=None):
    """``tables`` for millions of cells, from the order alone: a kept cell starts a depth-d node where its d-prefix
    differs from the kept cell before it (an OR along the levels of the element-wise comparison), a node's number is
    the count of such heads before it (``cumsum``), and a node's first child is where its number first appears among
    the parents of the depth below (``searchsorted``).  Checked against ``tables`` in test_trie_model.py."""
    cells = np.asarray(cells, dtype=np.int64).reshape(-1, levels)
    idx = np.arange(len(cells))
    if keep is not None:
        idx = idx[np.asarray(keep).astype(bool)]
    kept = cells[idx]
    head = np.ones((len(kept), levels), dtype=bool)
    if len(kept) > 1:
        head[1:] = np.logical_or.accumulate(kept[1:] != kept[:-1], axis=1)
    count, value, child_off = [1], [], []
    above = np.zeros(len(kept), dtype=np.int64)  # each kept cell's node number at the depth above
    for d in range(1, levels + 1):
        h = head[:, d - 1]
        child_off.append(np.searchsorted(above[h], np.arange(count[-1] + 1)).astype(np.int32))
        value.append(kept[h, d - 1].astype(np.int32))
        count.append(int(h.sum()))
        above = np.cumsum(h) - 1
    return dict(count=np.asarray(count, dtype=np.int32), value=value, child_off=child_off,
                leaf_cell=idx[head[:, levels - 1]].astype(np.int32))


class TrieModel:
    """``ids``: the kept ID tuples; ``level_tok``: per level, the token number of each value (-1: none);
    ``tok_code`` is derived from it."""

    def __init__(self, ids, sizes, level_tok, eos, vocab):
        self.sizes = tuple(int(s) for s in sizes)
        self.L = len(self.sizes)
        self.level_tok = [np.asarray(t, dtype=np.int64) for t in level_tok]
        self.eos, self.V = int(eos), int(vocab)
        self.code = {}
        for l, toks in enumerate(self.level_tok):
            for v, t in enumerate(toks):
                if 0 <= t < self.V:
                    self.code[int(t)] = (l, v)
        self.children = {}  # value prefix -> set of child values
        self.nodes = [set() for _ in range(self.L + 1)]
        for t in ids:
            t = tuple(int(v) for v in t)
            for d in range(self.L):
                self.children.setdefault(t[:d], set()).add(t[d])
            for d in range(self.L + 1):
                self.nodes[d].add(t[:d])
        self.nodes[0].add(())
        self.node_no = [{p: j for j, p in enumerate(sorted(s))} for s in self.nodes]

    def _token(self, level, value):
        t = int(self.level_tok[level][value])
        return t if 0 <= t < self.V else -1

    def row(self, seq):
        """(kind, allowed set, node number or -1) after the token sequence ``seq``."""
        seq = [int(t) for t in seq]
        start = -1
        for i in range(len(seq) - 1, -1, -1):  # rule 1
            if self.code.get(seq[i], (-1, 0))[0] == 0 and 0 <= seq[i] < self.V:
                start = i
                break
        prefix = [] if start < 0 else seq[start:start + self.L]
        if len(prefix) == self.L:  # rule 2
            allowed = {self._token(0, v) for v in range(self.sizes[0])} - {-1}
            return KIND_COMPLETE, allowed | {self.eos}, -1
        values = ()
        for t, tok in enumerate(prefix):  # rule 3
            level, v = self.code.get(tok, (-1, 0))
            if level != t or v not in self.children.get(values, ()):
                return KIND_DEAD, {self.eos}, -1
            values += (v,)
        allowed = {self._token(len(values), v) for v in self.children.get(values, ())} - {-1}
        if not allowed:  # rule 4
            return KIND_DEAD, {self.eos}, -1
        return KIND_WALK, allowed, self.node_no[len(values)][values]

    def rows(self, input_ids):
        """(kind [B], node [B], count [B], allowed bool [B, V]) of a batch."""
        B = len(input_ids)
        kind, node, count = (np.zeros(B, dtype=np.int32) for _ in range(3))
        allowed = np.zeros((B, self.V), dtype=bool)
        for b, seq in enumerate(input_ids):
            kind[b], toks, node[b] = self.row(seq)
            count[b] = len(toks)
            allowed[b, sorted(toks)] = True
        return kind, node, count, allowed

    def beam_step(self, depth, node_in, score_in, logp, beam_out):
        """One batch row: ``node_in`` [beam_in] node numbers, ``score_in`` f32 [beam_in], ``logp`` [beam_in, V] already
        widened to f32.  Returns the slots (node, score, parent, value, token) in order."""
        prefixes = sorted(self.nodes[depth])
        cands = []
        for h, n in enumerate(node_in):
            s_in = np.float32(score_in[h])
            if not 0 <= n < len(prefixes) or np.isnan(s_in):
                continue
            for v in sorted(self.children.get(prefixes[n], ())):
                tok = self._token(depth, v)
                if tok < 0:
                    continue
                with np.errstate(invalid="ignore"):
                    s = np.float32(s_in + np.float32(logp[h, tok]))
                if np.isnan(s) or s == -np.inf:
                    continue
                cands.append((-float(s), h, v, s, tok))
        cands.sort(key=lambda c: c[:3])  # s descending, h ascending, value ascending (-0.0 == 0.0)
        out = []
        for _, h, v, s, tok in cands[:beam_out]:
            out.append((self.node_no[depth + 1][prefixes[node_in[h]] + (v,)], s, h, v, tok))
        while len(out) < beam_out:
            out.append((-1, np.float32(-np.inf), -1, -1, -1))
        return out


    def candidates(self, depth, node_in, score_in, logp):
        """Every live candidate of one batch row as arrays (s f32, h, value, token, score_in[h], logp[h, token]), one
        numpy expression per hypothesis: the same rule as ``beam_step``, for nodes of thousands of children."""
        prefixes = sorted(self.nodes[depth])
        cols = [[] for _ in range(6)]
        for h, n in enumerate(node_in):
            s_in = np.float32(score_in[h])
            if not 0 <= n < len(prefixes) or np.isnan(s_in):
                continue
            vals = np.asarray(sorted(self.children.get(prefixes[n], ())), dtype=np.int64)
            toks = self.level_tok[depth][vals]
            vals = vals[(toks >= 0) & (toks < self.V)]
            toks = self.level_tok[depth][vals]
            lp = np.asarray(logp[h], dtype=np.float32)[toks]
            with np.errstate(invalid="ignore"):
                s = (s_in + lp).astype(np.float32)
            live = ~np.isnan(s) & (s != -np.inf)
            for c, a in zip(cols, (s, np.full(len(s), h), vals, toks, np.full(len(s), s_in, np.float32), lp)):
                c.append(a[live])
        kinds = (np.float32, np.int64, np.int64, np.int64, np.float32, np.float32)
        return tuple(np.concatenate(c).astype(k) if c else np.zeros(0, k) for c, k in zip(cols, kinds))

    def beam_step_wide(self, depth, node_in, score_in, logp, beam_out):
        """``beam_step`` by one ``lexsort`` of ``candidates`` (checked against ``beam_step`` in test_trie_model.py)."""
        s, h, v, tok, _, _ = self.candidates(depth, node_in, score_in, logp)
        order = np.lexsort((v, h, -s))[:beam_out]  # -0.0 == 0.0 for lexsort as well
        prefixes = sorted(self.nodes[depth])
        out = [(self.node_no[depth + 1][prefixes[node_in[h[i]]] + (int(v[i]),)], s[i], int(h[i]), int(v[i]),
                int(tok[i])) for i in order]
        while len(out) < beam_out:
            out.append((-1, np.float32(-np.inf), -1, -1, -1))
        return out


class FakeTokenizer:
    """An object of the shape the reference's classes read (``base_tokenizer.convert_tokens_to_ids`` /
    ``.unk_token_id``, ``layer_vocab_sizes``, ``eos_token_id``), from per-level token tables (-1: unknown)."""

    class _Base:
        def __init__(self, table, unk):
            self.table, self.unk_token_id = table, unk

        def convert_tokens_to_ids(self, token):
            return self.table.get(token, self.unk_token_id)

    def __init__(self, level_tok, vocab, eos, unk):
        table = {f"<id_l{l + 1}_{v}>": int(t) for l, toks in enumerate(level_tok) for v, t in enumerate(toks) if t >= 0}
        self.base_tokenizer = self._Base(table, int(unk))
        self.layer_vocab_sizes = {f"l{l + 1}": len(toks) for l, toks in enumerate(level_tok)}
        self.eos_token_id = int(eos)
        self.vocab_size = int(vocab)


def golden_parts(g):
    """(sizes, per-level token tables, kept IDs) of tests/golden/trie.npz."""
    sizes = tuple(int(s) for s in g["sizes"])
    offs = np.concatenate([[0], np.cumsum(sizes)])
    level_tok = [g["level_tok"][offs[l]:offs[l + 1]].astype(np.int64) for l in range(len(sizes))]
    entries = [tuple(int(v) for v in row[:n]) for row, n in zip(g["entry_ids"], g["entry_len"])]
    kept = sorted({e for e in entries if len(e) == len(sizes) and all(level_tok[l][v] >= 0 for l, v in enumerate(e))})
    return sizes, level_tok, kept
