"""Inputs of the trie tests that are made and judged without a GPU: the named trie setups, long token rows with a
deciding level-0 token at a chosen place, sampled cells for the large builds, and beam scores over both signs, the
infinities and the subnormal range.  test_trie_model.py asserts what the rows and scores are meant to hold;
test_gpu_trie_edges.py runs them through the kernels."""
import functools

import numpy as np

from tests import _trie_model as M


def scattered(sizes, vocab, seed, first=2):
    """Per level, token numbers drawn from [first, vocab) in no monotone order."""
    numbers = np.random.default_rng(seed).permutation(np.arange(first, vocab))[:sum(sizes)].astype(np.int64)
    offs = np.concatenate([[0], np.cumsum(sizes)])
    return [numbers[offs[l]:offs[l + 1]].copy() for l in range(len(sizes))]


class Case:
    """A set of random (or given) IDs with a token table of one's choosing, as the model."""

    def __init__(self, sizes, level_tok, vocab, eos, rows, seed, ids=None):
        rng = np.random.default_rng(seed)
        if ids is None:
            ids = np.stack([rng.integers(0, s, rows) for s in sizes], 1)
        self.ids = np.asarray(ids).astype(np.int32)
        self.sizes, self.V, self.eos = tuple(sizes), vocab, eos
        self.level_tok = [np.asarray(t, dtype=np.int64) for t in level_tok]
        kept = sorted({tuple(int(v) for v in r) for r in self.ids
                       if all(self.level_tok[l][v] >= 0 for l, v in enumerate(r))})
        self.kept = kept
        self.model = M.TrieModel(kept, sizes, self.level_tok, eos, vocab)

    def tok(self, level, value):
        return int(self.level_tok[level][value])

    def rows_of_every_kind(self, T, seed, n_random=0):
        """Token rows [B, T] (T >= 3): no ID token, each prefix length, complete, dead ones, out-of-range entries."""
        rng = np.random.default_rng(seed)
        L = len(self.sizes)
        fill = [t for t in range(self.V) if t not in self.model.code and t != self.eos][:1] or [self.eos]
        rows = []

        def row(*tail):
            rows.append(([fill[0]] * T + list(tail))[-T:])
        row()
        for n in range(min(len(self.kept), 6)):
            a = self.kept[(n * 7) % len(self.kept)]
            toks = [self.tok(l, v) for l, v in enumerate(a)]
            for d in range(1, L + 1):
                row(*toks[:d])
            row(*toks, *toks[:1])                 # a second ID under way
            row(toks[0], -100)                    # then an entry that is no token at all
            row(toks[0], self.V + 5)
            row(*toks[:L - 1], toks[0])
            row(toks[0], toks[-1])                # a last-level token at place 1: dead
        absent = []
        if L > 1:  # (with one level there are no pairs)
            absent = [(a, b) for a in range(self.sizes[0]) for b in range(self.sizes[1])
                      if (a, b) not in self.model.nodes[2] and self.tok(1, b) >= 0]
        for a, b in absent[:3]:
            row(self.tok(0, a), self.tok(1, b))
        for _ in range(n_random):
            rows.append(rng.integers(-3, self.V + 3, T).tolist())
        return np.asarray(rows, dtype=np.int64)


# ------------------------------------------------------------------------------------------------ the named setups
def _edge():
    V = 1003  # the `edge` fixture of test_gpu_trie_mask.py
    return dict(sizes=(5, 4, 7), level_tok=[[0, V - 1, 3, 4, 500], [7, 8, -1, 16], [15, 31, 32, 33, -1, V - 2, 1]],
                vocab=V, eos=2, rows=45, seed=11)


def _levels(sizes, vocab, hole, rows, seed):
    level_tok = scattered(sizes, vocab, seed)
    if hole is not None:
        level_tok[hole[0]][hole[1]] = -1  # a value without a token at a level >= 1
    return dict(sizes=sizes, level_tok=level_tok, vocab=vocab, eos=1, rows=rows, seed=seed + 1)


def _eos_inside(level):
    sizes, V, seed = (5, 4, 7), 37, 70 + level
    level_tok = scattered(sizes, V, seed)
    ids = np.stack([np.random.default_rng(seed + 1).integers(0, s, 40) for s in sizes], 1)
    # level 0: eos is a level-0 token; level 1: eos is the token of a child of a node that rows walk to
    eos = int(level_tok[0][2]) if level == 0 else int(level_tok[1][min(tuple(r) for r in ids.tolist())[1]])
    return dict(sizes=sizes, level_tok=level_tok, vocab=V, eos=eos, rows=40, seed=seed + 1, ids=ids)


def _vocab(V):
    if V == 1:  # only eos: no value has a token, no ID is kept
        return dict(sizes=(1, 1), level_tok=[[-1], [-1]], vocab=1, eos=0, rows=1, seed=1)
    if V == 2:
        return dict(sizes=(1,), level_tok=[[0]], vocab=2, eos=1, rows=1, seed=1)
    if V == 7:
        return dict(sizes=(2, 2), level_tok=[[0, 6], [3, 5]], vocab=7, eos=2, rows=6, seed=1)
    # allowed tokens at 0, at a slice's last element, at the next slice's first and at V - 1, where they exist
    l0 = [t for t in (8191, 8192, V - 1, 0) if t < V]
    l0 = list(dict.fromkeys(l0))
    l1 = list(dict.fromkeys(t for t in (8190, 8193, V - 2, 1) if t < V and t not in l0))
    return dict(sizes=(len(l0), len(l1)), level_tok=[l0, l1], vocab=V, eos=2, rows=12, seed=V)


def _fan8192():
    sizes, V = (3, 8192), 9000  # every ID present: three nodes of 8192 children, tokens on both sides of 8192
    ids = np.stack(np.unravel_index(np.arange(3 * 8192), sizes), 1)
    return dict(sizes=sizes, level_tok=scattered(sizes, V, 81), vocab=V, eos=1, rows=0, seed=82, ids=ids)


SPECS = {
    "edge": _edge,
    "levels1": lambda: _levels((9,), 23, None, 6, 101),
    "levels4": lambda: _levels((3, 4, 2, 6), 41, (2, 1), 60, 104),
    "levels8": lambda: _levels((2, 2, 2, 2, 2, 2, 2, 3), 31, (7, 2), 50, 108),
    "eos_level0": lambda: _eos_inside(0),
    "eos_level1": lambda: _eos_inside(1),
    "fan8192": _fan8192,
    **{f"v{V}": functools.partial(_vocab, V) for V in (1, 2, 7, 8192, 8193, 16384, 1 << 20)},
    # cells are dropped (a value without a token), so the tables' capacity exceeds every count
    "poison": lambda: _levels((5, 4, 7), 37, (1, 2), 60, 120),
}


def spec(name):
    return SPECS[name]()


# ------------------------------------------------------------------------------------------------------- long rows
LONG_T = (63, 64, 65, 127, 128, 129, 300)


def long_rows(level_tok, vocab, kept, T, seed, fill):
    """Token rows [B, T] whose last level-0 token sits at a chosen place p, and ``where`` [B] (p, or -1 for a row
    without one).  From p on: each prefix length 1 .. L, a complete ID followed by the next one's first token (that
    token at p), and a dead continuation; cut at the row's end.  Before p: a level-0 token at p - 1, one in every
    earlier chunk of 64 places counted from the row's end, deeper-level tokens and entries outside the vocabulary.
    Behind p + L: entries outside the vocabulary.  Everything else is ``fill`` (tokens that are no ID token)."""
    rng = np.random.default_rng(seed)
    L = len(level_tok)
    level0 = [int(t) for t in level_tok[0] if t >= 0]
    deeper = [int(t) for l in range(1, L) for t in level_tok[l] if t >= 0]
    outside = [-100, vocab + 5, -3, vocab]
    places = sorted({p for p in (T - 1, T - L, T - L - 1, T - 63, T - 64, T - 65, T - 66, 64, 63, 1, 0,
                                 *range(T - L + 1, T)) if 0 <= p < T})
    rows, where, n = [], [], 0
    for p in places:
        for shape in range(L + 2):
            a, b = kept[(n * 7) % len(kept)], kept[(n * 7 + 3) % len(kept)]
            n += 1
            toks = [int(level_tok[l][v]) for l, v in enumerate(a)]
            lead = []
            if shape < L:
                tail = toks[:shape + 1]
            elif shape == L:
                lead, tail = toks[max(0, L - p):], [int(level_tok[0][b[0]])]
            else:
                tail = [toks[0], toks[-1] if L > 2 else -100]
            row = rng.choice(fill, T).astype(np.int64)
            start = p - len(lead)
            if start >= 1:
                at = rng.choice(start, min(start, 6), replace=False)
                row[at] = [(deeper + outside)[(n + i) % len(deeper + outside)] for i in range(len(at))]
                for base in range(T - 1, -1, -64):
                    if base < start:
                        row[rng.integers(max(base - 63, 0), base + 1)] = level0[rng.integers(len(level0))]
                row[start - 1] = next(t for t in level0 if t != tail[0])
            row[start:p] = lead
            row[p:p + len(tail)] = tail[:T - p]
            if p + L < T:
                at = p + L + rng.choice(T - p - L, min(T - p - L, 3), replace=False)
                row[at] = outside[:len(at)]
            rows.append(row)
            where.append(p)
    for shape in range(2):  # no ID token at all; deeper-level tokens and outside entries, but no level-0 token
        row = rng.choice(fill, T).astype(np.int64)
        if shape:
            at = rng.choice(T, min(T, 40), replace=False)
            row[at] = [(deeper + outside)[i % len(deeper + outside)] for i in range(len(at))]
        rows.append(row)
        where.append(-1)
    return np.stack(rows), np.asarray(where)


def long_fill(case):
    return [t for t in range(case.V) if t not in case.model.code and t != case.eos][:5]


def check_long_rows(model, rows, where, T):
    """What the long rows are meant to hold; returns the rows' kinds."""
    found = [max([i for i, t in enumerate(r) if model.code.get(int(t), (-1, 0))[0] == 0], default=-1) for r in rows]
    assert found == where.tolist()
    kind = model.rows(rows)[0]
    assert set(kind.tolist()) == {0, 1, 2}
    for p in (T - 64, T - 65):  # the first place of the second chunk of 64, and the last of the first
        assert p < 0 or p in where, (T, p)
    assert -1 in where
    return kind


# ---------------------------------------------------------------------------------------------- cells for the build
BUILD_SIZES = (13, 11, 31, 600)
BUILD_N = (2048, 2049, 4096, 2048 * 1024, 2048 * 1024 + 1, 2048 * 1027 + 5)
BUILD_KEEPS = ("all", "fraction", "tile0", "subtree", "multiple")


@functools.lru_cache(maxsize=1)
def sampled_cells(n):
    """``n`` distinct IDs over BUILD_SIZES in ascending order: a sample without replacement of the ID space, less one
    whole level-0 value and two (level 0, level 1) pairs, so that nodes are absent at depth 1 and 2."""
    rng = np.random.default_rng(n)
    codes = rng.permutation(int(np.prod(BUILD_SIZES)))
    l0, l1 = codes // (11 * 31 * 600), codes // (31 * 600) % 11
    ok = (l0 != 5) & ~((l0 == 2) & (l1 == 3)) & ~((l0 == 12) & (l1 == 10))
    codes = np.sort(codes[ok][:n])
    assert len(codes) == n
    return np.stack(np.unravel_index(codes, BUILD_SIZES), 1).astype(np.int64)


def build_keep(cells, which):
    n = len(cells)
    rng = np.random.default_rng(n + 1)
    if which == "all":
        return None
    if which == "fraction":
        return rng.random(n) < 0.6
    keep = np.ones(n, dtype=bool)
    if which == "tile0":
        keep[:2048] = False  # the first tile of the scans keeps nothing
    elif which == "subtree":
        keep = cells[:, 0] != cells[n // 2, 0]  # every cell under one level-0 value
    else:  # the number of kept cells is a multiple of the tile: the last tile of the second scan is full
        drop = n % 2048 if n % 2048 else 2048
        keep[rng.choice(n, drop, replace=False)] = False
        assert keep.sum() % 2048 == 0
    return keep


def check_build_cells(cells, want):
    s = BUILD_SIZES
    assert want["count"][1] < s[0] and want["count"][2] < s[0] * s[1] and want["count"][-1] == len(cells)


# ------------------------------------------------------------------------------------------------------ beam scores
FORMATS = ("f32", "f16", "bf16")
SUBNORMAL = {"f32": 2.0 ** -149, "f16": 2.0 ** -24, "bf16": 2.0 ** -133}  # the smallest of each format
DENORMALS = [-1e-40, -2e-40, 3e-41, 1e-40, -3e-41, 7e-42, -7e-42, 5e-43, -5e-43, 1.4e-45, -1.4e-45, 9e-41, -9e-41,
             6e-41, -6e-41, 2e-41, -2.5e-41]  # of fp32, pairwise distinct


def edge_scores(B, beam_in, vocab, fmt, seed, live=1.0):
    """(score_in f32 [B, beam_in], logp f32 [B * beam_in, vocab], every value exact in ``fmt``).  Hypotheses take
    turns in four classes, built so that two candidates of a row have the same fp32 sum only where their inputs are
    the same (check_ties_are_planned), and only in IEEE arithmetic with subnormals:

    0  score_in (j - 32) / 64 with distinct j, logp whole numbers in [-24, 24]: both signs, order by logp first;
    1  score_in j * U with distinct small j, logp = k * the format's smallest subnormal, (j, k) -> sum one-to-one
       (f16: U = 2^-13, |k| < 2^10; bf16 and f32: U an fp32 denormal, the sums fp32 denormals or just above them);
    2  score_in one of DENORMALS, logp +0 or -0: the sum is the denormal itself;
    3  score_in +inf (row 0), -inf, NaN, +0, -0 with whole-number logp.

    A share ``live`` of every logp row stays, the rest is -inf; of what stays 3 % is NaN and, outside row 1, 1 % +inf.
    In row 1 the whole-number logp are negative, so the candidates around zero are the best."""
    assert beam_in <= 64
    rng = np.random.default_rng(seed)
    sub = np.float32(SUBNORMAL[fmt])
    score = np.zeros((B, beam_in), dtype=np.float32)
    logp = np.zeros((B * beam_in, vocab), dtype=np.float32)
    for b in range(B):
        frac, small, den = rng.permutation(64), rng.permutation(17) - 8, rng.permutation(len(DENORMALS))
        special = [np.inf if b == 0 else 0.0, -np.inf, np.nan, -0.0]
        for h in range(beam_in):
            r, cls, turn = b * beam_in + h, (h + b) % 4, h // 4
            if cls == 0:
                score[b, h] = (frac[h] - 32) / 64
                logp[r] = rng.integers(-24, 0 if b == 1 else 25, vocab)
            elif cls == 1:
                j = int(small[turn])
                if fmt == "f16":
                    score[b, h], k = j * 2.0 ** -13, rng.integers(1, 1024, vocab)
                elif fmt == "bf16":
                    score[b, h], k = np.float32(j * 3001 * 2.0 ** -149), rng.integers(1, 128, vocab)
                else:
                    score[b, h], k = np.float32(j * 2.0 ** -129), rng.integers(1 << 18, 1 << 19, vocab)
                if j == 0 and b % 2:
                    score[b, h] = -0.0
                logp[r] = (k * rng.choice([-1, 1], vocab)).astype(np.float32) * sub
                logp[r, rng.random(vocab) < 0.1] = 0.0
            elif cls == 2:
                score[b, h] = np.float32(DENORMALS[den[turn]])
                logp[r] = np.where(rng.random(vocab) < 0.5, np.float32(0.0), np.float32(-0.0))
            else:
                score[b, h] = special[turn % 4]
                logp[r] = rng.integers(-24, 0 if b == 1 else 25, vocab)
            # a hypothesis with score +inf keeps about a dozen entries, so that it does not fill every slot alone
            share = min(1.0, 12 / vocab) if score[b, h] == np.inf else live
            u = rng.random(vocab)
            logp[r, u < 0.03] = np.nan
            if b != 1:
                logp[r, (u >= 0.03) & (u < 0.04)] = np.inf
            logp[r, rng.random(vocab) >= share] = -np.inf
    return score, logp


def check_ties_are_planned(model, depth, node_in, score_in, logp):
    """No two candidates of one batch row have the same finite fp32 sum unless their inputs are equal as numbers
    (+0 and -0 are).  Returns the number of candidates and of distinct finite sums."""
    s, _, _, _, a, l = model.candidates(depth, node_in, score_in, logp)
    fin = np.isfinite(s)
    s, a, l = s[fin], a[fin], l[fin]
    order = np.lexsort((l, a, s))
    s, a, l = s[order], a[order], l[order]
    same = s[1:] == s[:-1]
    assert ((a[1:] == a[:-1]) & (l[1:] == l[:-1]))[same].all()
    return len(s), len(np.unique(s))


def dead_hypotheses(node_in, score_in, n_nodes):
    """Hypotheses that yield nothing, in every row: node -1, the node count, 2^31 - 1, and a NaN score."""
    beam_in = node_in.shape[1]
    for b in range(len(node_in)):
        at = [(5 * b + 7 * i) % beam_in for i in range(4)]
        if beam_in >= 8:
            node_in[b, at[0]], node_in[b, at[1]], node_in[b, at[2]] = -1, n_nodes, 2 ** 31 - 1
            score_in[b, at[3]] = np.nan
