"""The trie model (tests/_trie_model.py) against the reference's recorded outputs (tests/golden/trie.npz), and the
host-only pieces of the trie layer: TokenMap's tables and refusals, io.read_semantic_ids."""
import json

import numpy as np
import pytest
import torch

from generative_ranking_recommender_amd import io as rq_io
from generative_ranking_recommender_amd import ops
from tests import _trie_model as M


@pytest.fixture(scope="module")
def g(golden):
    return golden("trie")


@pytest.fixture(scope="module")
def model(g):
    sizes, level_tok, kept = M.golden_parts(g)
    return M.TrieModel(kept, sizes, level_tok, int(g["eos"]), int(g["vocab"]))


def test_kept_ids_are_the_references_valid_ids(g):
    _, _, kept = M.golden_parts(g)
    assert kept == [tuple(int(v) for v in row) for row in g["valid_ids"]]
    assert (g["entry_len"] == 2).sum() == 1  # the entry of length 2 is in the file


def test_valid_next_tokens_of_every_prefix(g, model):
    for n, (plen, vals) in enumerate(zip(g["prefix_len"], g["prefix_val"])):
        want = set(int(t) for t in g["next_tok"][g["next_off"][n]:g["next_off"][n + 1]])
        prefix = tuple(int(v) for v in vals[:plen])
        got = {model._token(plen, v) for v in model.children.get(prefix, ())} - {-1}
        assert got == want, prefix
    assert any(g["next_off"][n] == g["next_off"][n + 1] for n in range(len(g["prefix_len"])))  # an absent prefix


def test_tables_agree_with_the_statistics(g):
    sizes, _, kept = M.golden_parts(g)
    t = M.tables(kept, len(sizes))
    assert t["count"].tolist() == [1, int(g["stat_l1"]), t["count"][2], int(g["stat_total"])]
    for d, key in ((1, "stat_l2"), (2, "stat_l3")):
        fan = np.diff(t["child_off"][d])
        got = sorted((int(k), int((fan == k).sum())) for k in np.unique(fan))
        assert got == [tuple(int(v) for v in row) for row in g[key]]
    for d in range(len(sizes)):  # nested, ascending inside a node
        off = t["child_off"][d]
        assert off[0] == 0 and off[-1] == t["count"][d + 1] and (np.diff(off) > 0).all()
        for j in range(t["count"][d]):
            assert (np.diff(t["value"][d][off[j]:off[j + 1]]) > 0).all()


@pytest.mark.parametrize("name, dtype", [("f32", torch.float32), ("f16", torch.float16), ("bf16", torch.bfloat16)])
def test_masked_scores_equal_the_references_bytes(g, model, name, dtype):
    kind, _, count, allowed = model.rows(g["input_ids"])
    assert set(kind.tolist()) == {0, 1, 2}
    assert (count == allowed.sum(1)).all()
    scores = torch.from_numpy(g["scores"].view(np.float32)).to(dtype)
    got = torch.where(torch.from_numpy(allowed), scores, torch.full_like(scores, float("-inf")))
    bits = torch.int32 if dtype == torch.float32 else torch.int16
    assert torch.equal(got.view(bits), torch.from_numpy(g[f"masked_{name}"]))


def test_is_valid_sequence_samples(g, model):
    assert g["seqs_valid"].any() and not g["seqs_valid"].all()
    for seq, want in zip(g["seqs"], g["seqs_valid"]):
        seq = [int(t) for t in seq if t != -7]
        values, ok = (), len(seq) == 3
        for d, tok in enumerate(seq if ok else ()):
            level, v = model.code.get(tok, (-1, 0))
            ok = ok and level == d and v in model.children.get(values, ())
            values += (v,)
        assert ok == bool(want), seq


def test_beam_order_of_the_model():
    m = M.TrieModel([(0, 0), (0, 1), (1, 0)], (2, 2), [[0, 1], [2, 3]], 4, 5)
    logp = np.zeros((2, 5), dtype=np.float32)
    logp[1, 2] = -0.0
    out = m.beam_step(1, [0, 1], np.zeros(2, np.float32), logp, 4)
    assert [(o[2], o[3]) for o in out] == [(0, 0), (0, 1), (1, 0), (-1, -1)]  # equal scores: by (h, value)
    logp[0, 2], logp[0, 3] = -np.inf, np.nan
    out = m.beam_step(1, [0, 1], np.zeros(2, np.float32), logp, 2)
    assert [(o[0], o[2], o[3]) for o in out] == [(2, 1, 0), (-1, -1, -1)]


# ------------------------------------------------------------------------------------------------- TokenMap, io
def test_token_map_tables(g):
    sizes, level_tok, _ = M.golden_parts(g)
    tm = ops.TokenMap(int(g["vocab"]), level_tok, int(g["eos"]), device="cpu")
    assert tm.sizes == sizes and tm.level_tok.tolist() == g["level_tok"].tolist()
    code = tm.tok_code.numpy()
    for l, toks in enumerate(level_tok):
        for v, t in enumerate(toks):
            if t >= 0:
                assert code[t] == (l << 24) | v
    assert (code >= 0).sum() == sum(int((t >= 0).sum()) for t in level_tok)
    fake = M.FakeTokenizer(level_tok, int(g["vocab"]), int(g["eos"]), int(g["unk"]))
    tm2 = ops.TokenMap.from_tokenizer(fake, fake.eos_token_id, levels=3, device="cpu")
    assert torch.equal(tm2.tok_code, tm.tok_code) and torch.equal(tm2.level_tok, tm.level_tok)
    ident = ops.TokenMap.identity((3, 2), device="cpu")
    assert ident.level_tok.tolist() == [0, 1, 2, 3, 4] and ident.eos_token_id == 5 and ident.vocab_size == 6
    assert ident.with_eos(0).eos_token_id == 0 and ident.eos_token_id == 5
    wide = ident.with_vocab(9)
    assert wide.tok_code.tolist() == ident.tok_code.tolist() + [-1] * 3 and wide.eos_token_id == 5
    with pytest.raises(ValueError):
        ident.with_vocab(4)


def test_token_map_refusals(g):
    sizes, level_tok, _ = M.golden_parts(g)
    V, eos = int(g["vocab"]), int(g["eos"])
    with pytest.raises(ValueError, match="more than one"):
        ops.TokenMap(V, [[10, 11], [11, 12]], eos, device="cpu")       # two levels share a token number
    with pytest.raises(ValueError, match="more than one"):
        ops.TokenMap(V, [[10, 10], [11, 12]], eos, device="cpu")       # two values of a level share one
    with pytest.raises(ValueError, match="outside the vocabulary"):
        ops.TokenMap(V, [[10, V], [11, 12]], eos, device="cpu")
    with pytest.raises(ValueError, match="outside the vocabulary"):
        ops.TokenMap(V, [[10, -2], [11, 12]], eos, device="cpu")
    with pytest.raises(ValueError, match="eos_token_id"):
        ops.TokenMap(V, [[10, 11]], V, device="cpu")
    with pytest.raises(ValueError):
        ops.TokenMap(V, [], eos, device="cpu")
    with pytest.raises(ValueError):
        ops.TokenMap(ops.TRIE_VOCAB_MAX + 1, [[1]], 0, device="cpu")
    unknown_l1 = [t.copy() for t in level_tok]
    unknown_l1[0][2] = -1
    fake = M.FakeTokenizer(unknown_l1, V, eos, int(g["unk"]))
    with pytest.raises(ValueError, match="id_l1_2"):
        ops.TokenMap.from_tokenizer(fake, eos, levels=3, device="cpu")


def test_read_semantic_ids(tmp_path):
    path = tmp_path / "ids.jsonl"
    rows = [("a", [1, 2, 3]), ("b", [4, 5]), ("c", [0, 0, 6]), ("d", [1, 2, 3, 4])]
    path.write_text("".join(json.dumps({"song_id": s, "semantic_ids": i}) + "\n" for s, i in rows) + "\n")
    song_ids, ids = rq_io.read_semantic_ids(str(path))
    assert song_ids == ["a", "c"] and ids.dtype == np.int32 and ids.tolist() == [[1, 2, 3], [0, 0, 6]]
    song_ids, ids = rq_io.read_semantic_ids(str(path), levels=2)
    assert song_ids == ["b"] and ids.tolist() == [[4, 5]]
    song_ids, ids = rq_io.read_semantic_ids(str(path), levels=5)
    assert song_ids == [] and ids.shape == (0, 5)
