"""Record tests/golden/trie.npz and tests/golden/trie_long.npz by running the REFERENCE's
src/generator/semantic_id_trie.py on the CPU::

    python tests/golden/make_trie_golden.py <path of the reference checkout> trie|long

``trie`` rewrites trie.npz, ``long`` trie_long.npz; each recording leaves the other file alone (an .npz holds the time
it was written, so a rewrite is never byte-identical).

The module is loaded by path (it imports json / logging / typing / collections, and torch inside __call__) with a
fake tokenizer object of the shape it reads.  The fixture holds data only: the inputs (the jsonl's entries, the token
table, token sequences, scores) and the reference's own outputs (masked scores in fp32 / fp16 / bf16,
get_valid_next_tokens of every prefix of length 0 .. 2, is_valid_sequence samples, get_statistics).  trie_long.npz
holds rows of 130 tokens over the same IDs and token table (tests/_trie_cases.long_rows: the last level-0 token at
chosen places up to the row's start, decoys before it), a seed of its own, and per row what the reference's processor
derived (the length of its prefix, the tokens it allowed) beside the masked scores.  Nothing in the package or the
tests imports this file.
"""
import importlib.util
import itertools
import json
import sys
import tempfile
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
SIZES = (5, 4, 7)
VOCAB = 37
EOS, UNK = 1, 2
UNKNOWN_L3 = 5  # <id_l3_5> is not in the tokenizer


class _Base:
    unk_token_id = UNK

    def __init__(self, table):
        self.table = table

    def convert_tokens_to_ids(self, token):
        return self.table.get(token, UNK)


class _Tokenizer:
    eos_token_id = EOS

    def __init__(self, table):
        self.base_tokenizer = _Base(table)
        self.layer_vocab_sizes = {f"l{l + 1}": s for l, s in enumerate(SIZES)}


def setup(reference: Path):
    """The reference's trie and processor over the fixture's IDs and token table (the same for both recordings)."""
    spec = importlib.util.spec_from_file_location("ref_semantic_id_trie",
                                                  reference / "src" / "generator" / "semantic_id_trie.py")
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    rng = np.random.default_rng(20261021)
    # the ID tokens take scattered numbers among ordinary ones, in no monotone order
    numbers = rng.permutation(np.arange(8, VOCAB))[:sum(SIZES)]
    level_tok, table, at = [], {}, 0
    for l, s in enumerate(SIZES):
        toks = numbers[at:at + s].astype(np.int64)
        at += s
        if l == 2:
            toks[UNKNOWN_L3] = -1
        for v, t in enumerate(toks):
            if t >= 0:
                table[f"<id_l{l + 1}_{v}>"] = int(t)
        level_tok.append(toks)
    tokenizer = _Tokenizer(table)
    # 40 random IDs (with repeats among songs), some using the unknown level-3 token, and one entry of length 2
    ids = np.stack([rng.integers(0, s, 40) for s in SIZES], 1)
    ids[3, 2] = ids[17, 2] = UNKNOWN_L3
    entries = [[int(v) for v in row] for row in ids]
    entries.insert(9, [2, 1])
    with tempfile.TemporaryDirectory() as d:
        path = Path(d) / "song_semantic_ids.jsonl"
        with open(path, "w") as f:
            for n, e in enumerate(entries):
                f.write(json.dumps({"song_id": f"s{n}", "semantic_ids": e}) + "\n")
        trie = ref.SemanticIDTrie(tokenizer, str(path))
    proc = ref.ConstrainedLogitsProcessor(trie, tokenizer, EOS)
    return rng, level_tok, ids, entries, trie, proc


def masked(proc, input_ids, scores):
    out = {}
    for name, dt in (("f32", torch.float32), ("f16", torch.float16), ("bf16", torch.bfloat16)):
        got = proc(input_ids, scores.to(dt).clone())
        out[f"masked_{name}"] = got.view(torch.int32 if dt == torch.float32 else torch.int16).numpy()
    return out


def record_long(reference: Path):
    sys.path.insert(0, str(HERE.parent.parent))
    from tests import _trie_cases as C
    _, level_tok, _, _, trie, proc = setup(reference)
    T, seed = 130, 20261022
    kept = sorted(trie.valid_semantic_ids)
    rows, where = C.long_rows(level_tok, VOCAB, kept, T, seed, fill=[0, 3, 4, 5, 6, 7])
    # what the reference's processor derives for each row, by its own methods
    prefix_len, kind, allowed = [], [], np.zeros((len(rows), VOCAB), dtype=np.uint8)
    for b, row in enumerate(rows.tolist()):
        prefix = proc._extract_current_prefix(row)
        valid = trie.get_valid_next_tokens(prefix)
        if len(prefix) == 3:
            valid, k = set(proc.l1_token_ids) | {EOS}, 1
        elif valid:
            k = 0
        else:
            valid, k = {EOS}, 2
        prefix_len.append(len(prefix))
        kind.append(k)
        allowed[b, sorted(valid)] = 1
    rng = np.random.default_rng(seed + 1)
    scores = torch.from_numpy(rng.standard_normal((len(rows), VOCAB)).astype(np.float32) * 3)
    scores[:, ::7] = float("nan")
    scores[5, 9] = float("inf")
    input_ids = torch.from_numpy(rows)
    out = masked(proc, input_ids, scores)
    keep = torch.from_numpy(allowed.astype(bool))
    assert torch.equal(out["masked_f32"] == torch.tensor(float("-inf")).view(torch.int32), ~keep | (scores == -np.inf))
    np.savez_compressed(
        HERE / "trie_long.npz", input_ids=rows.astype(np.int16), where=where.astype(np.int32),
        prefix_len=np.asarray(prefix_len, dtype=np.int32), kind=np.asarray(kind, dtype=np.int32), allowed=allowed,
        scores=scores.numpy().view(np.int32), **out)
    print("wrote", HERE / "trie_long.npz", (HERE / "trie_long.npz").stat().st_size, "bytes;", len(rows), "rows of", T,
          "tokens; kinds", np.bincount(kind).tolist())


def record_trie(reference: Path):
    rng, level_tok, ids, entries, trie, proc = setup(reference)

    def tok(l, v):
        return int(level_tok[l][v])

    # get_valid_next_tokens of every prefix of length 0 .. 2 (absent ones included)
    prefixes = [()] + [(a,) for a in range(SIZES[0])] + list(itertools.product(range(SIZES[0]), range(SIZES[1])))
    pre_len, pre_val, nxt_off, nxt_tok = [], [], [0], []
    for p in prefixes:
        got = sorted(trie.get_valid_next_tokens([tok(l, v) for l, v in enumerate(p)]))
        pre_len.append(len(p))
        pre_val.append(list(p) + [-1] * (2 - len(p)))
        nxt_tok += got
        nxt_off.append(len(nxt_tok))
    # is_valid_sequence samples: present, absent, the unknown token, wrong lengths, wrong order
    seqs = [[tok(0, a), tok(1, b), tok(2, c) if c != UNKNOWN_L3 else UNK] for a, b, c in ids[:12]]
    seqs += [[tok(0, a), tok(1, b), tok(2, c)] for a, b, c in itertools.product((0, 4), (0, 3), (0, 6))]
    seqs += [[tok(0, 1), tok(1, 1)], [tok(1, 1), tok(0, 1), tok(2, 1)], [tok(0, 1), tok(1, 1), tok(2, 1), EOS]]
    valid = [bool(trie.is_valid_sequence(s)) for s in seqs]
    seq_arr = np.full((len(seqs), 4), -7, dtype=np.int64)
    for n, s in enumerate(seqs):
        seq_arr[n, :len(s)] = s
    # token rows of every kind: 6 columns, filled from the left with ordinary tokens
    a0, b0, c0 = (int(v) for v in ids[0])
    a1, b1, c1 = (int(v) for v in ids[1])
    pairs = {(int(x), int(y)) for x, y, _ in ids}
    absent_a, absent_b = next((a, b) for a, b in itertools.product(sorted({a for a, _ in pairs}), range(SIZES[1]))
                              if (a, b) not in pairs)
    rows = [
        [0, 3, 4, 5, 6, 7],                                        # no ID token: the level-1 tokens
        [0, 3, 4, 5, 6, tok(0, a0)],                               # one level: its level-2 children
        [0, 3, 4, 5, tok(0, a0), tok(1, b0)],                      # two levels: level-3 children
        [0, 3, 4, tok(0, a0), tok(1, b0), tok(2, c0)],             # complete
        [tok(0, a0), tok(1, b0), tok(2, c0), tok(0, a1), tok(1, b1), tok(2, c1)],  # a second ID, complete
        [0, tok(0, a0), tok(1, b0), tok(2, c0), tok(0, a1), tok(1, b1)],           # a second ID under way
        [0, 3, 4, 5, tok(0, a0), 6],                               # the last level-1 token, then a non-ID token
        [0, 3, 4, tok(0, a0), tok(1, b0), 7],                      # three tokens from the level-1 token: complete
        [0, 3, 4, 5, tok(0, absent_a), tok(1, absent_b)],             # an absent pair: dead
        [0, 3, 4, 5, tok(0, a0), tok(2, c0)],                      # a level-3 token at place 1: dead
        [0, 3, tok(0, a0), tok(1, b0), tok(2, c0), EOS],           # complete, then eos: still the last ID's prefix
        [0, 3, 4, 5, tok(1, b0), tok(2, c0)],                      # ID tokens without a level-1 token: empty prefix
        [0, 3, 4, 5, tok(0, int(ids[3, 0])), tok(1, int(ids[3, 1]))],  # may hold the dropped ID
    ]
    input_ids = torch.tensor(rows, dtype=torch.int64)
    scores = torch.from_numpy(rng.standard_normal((len(rows), VOCAB)).astype(np.float32) * 3)
    scores[:, ::5] = float("nan")
    scores[2, :] = float("nan")
    scores[4, 7] = float("inf")
    out = masked(proc, input_ids, scores)
    stats = trie.get_statistics()

    def dist(d):
        return np.asarray(sorted((int(k), int(v)) for k, v in d.items()), dtype=np.int64).reshape(-1, 2)

    np.savez_compressed(
        HERE / "trie.npz", sizes=np.asarray(SIZES, dtype=np.int32), vocab=np.int32(VOCAB), eos=np.int32(EOS),
        unk=np.int32(UNK), level_tok=np.concatenate(level_tok).astype(np.int32),
        entry_ids=np.asarray([e + [-1] * (3 - len(e)) for e in entries], dtype=np.int32),
        entry_len=np.asarray([len(e) for e in entries], dtype=np.int32),
        valid_ids=np.asarray(sorted(trie.valid_semantic_ids), dtype=np.int32),
        prefix_len=np.asarray(pre_len, dtype=np.int32), prefix_val=np.asarray(pre_val, dtype=np.int32),
        next_off=np.asarray(nxt_off, dtype=np.int32), next_tok=np.asarray(nxt_tok, dtype=np.int32),
        seqs=seq_arr, seqs_valid=np.asarray(valid), input_ids=input_ids.numpy(), scores=scores.numpy().view(np.int32),
        all_sequences=np.asarray(sorted(trie.get_all_valid_sequences()), dtype=np.int32),
        stat_total=np.int64(stats["total_valid_sequences"]), stat_l1=np.int64(stats["unique_l1_tokens"]),
        stat_l2=dist(stats["l2_distribution"]), stat_l3=dist(stats["l3_distribution"]), **out)
    print("wrote", HERE / "trie.npz", (HERE / "trie.npz").stat().st_size, "bytes;", len(trie.valid_semantic_ids),
          "valid IDs")


if __name__ == "__main__":
    if len(sys.argv) != 3 or sys.argv[2] not in ("trie", "long"):
        sys.exit(__doc__)
    (record_trie if sys.argv[2] == "trie" else record_long)(Path(sys.argv[1]))
