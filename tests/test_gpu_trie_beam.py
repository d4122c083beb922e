"""rqsid_trie_beam_step on the GPU against the model of its order (tests/_trie_model.py), every output for equality;
then constrained_beam_search, exhaustive on a small trie, against the brute-force ranking of all cells."""
import numpy as np
import pytest
import torch

from generative_ranking_recommender_amd import ops
from generative_ranking_recommender_amd.semantic_id_trie import SemanticIDTrie, constrained_beam_search
from tests import _trie_model as M

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
SIZES = (4, 3, 5)
V = 29


@pytest.fixture(scope="module")
def setup():
    rng = np.random.default_rng(31)
    numbers = rng.permutation(np.arange(2, V))[:sum(SIZES)]
    level_tok = [numbers[:4].copy(), numbers[4:7].copy(), numbers[7:12].copy()]
    ids = np.stack([rng.integers(0, s, 40) for s in SIZES], 1).astype(np.int32)
    trie = SemanticIDTrie.from_ids(ids, SIZES, ops.TokenMap(V, level_tok, 1, device=DEV))
    kept = sorted({tuple(int(v) for v in r) for r in ids})
    # the step's token table names no token for two level-1 values: their children exist in the trie but are no
    # candidates (the tables were built with every token known)
    holes = [t.copy() for t in level_tok]
    holes[1][1] = -1
    holes[2][3] = -1
    step_tokens = ops.TokenMap(V, holes, 1, device=DEV)
    return trie, step_tokens, M.TrieModel(kept, SIZES, holes, 1, V)


def make_logp(B, beam_in, dtype, seed):
    gen = torch.Generator().manual_seed(seed)
    # multiples of 1/2 in a narrow range: many equal scores, exact in every format
    logp = (torch.randint(-6, 1, (B * beam_in, V + 3), generator=gen).float() / 2)
    logp[torch.rand(B * beam_in, V + 3, generator=gen) < 0.08] = float("-inf")
    logp[torch.rand(B * beam_in, V + 3, generator=gen) < 0.05] = float("nan")
    logp[0, :] = -0.0  # a row of equal scores: the order falls to (h, value)
    return logp.to(dtype)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16])
@pytest.mark.parametrize("depth, beam_in", [(0, 1), (1, 4), (2, 4)])
@pytest.mark.parametrize("beam_out", [1, 5, 64])
def test_step_equals_the_model(setup, dtype, depth, beam_in, beam_out):
    trie, tokens, model = setup
    B = 3
    rng = np.random.default_rng(depth * 100 + beam_in * 10 + beam_out)
    n_nodes = len(model.nodes[depth])
    node_in = rng.integers(0, n_nodes, (B, beam_in)).astype(np.int32)
    score_in = (rng.integers(-8, 1, (B, beam_in)) / 4).astype(np.float32)
    if beam_in > 1:
        node_in[0, 1], node_in[1, 0], node_in[2, 3] = -1, n_nodes, 2**31 - 1   # dead hypotheses
        node_in[1, 2] = node_in[1, 1]                                          # the same node twice
        score_in[2, 0], score_in[0, 2] = np.nan, -np.inf
    logp = make_logp(B, beam_in, dtype, seed=beam_out)
    logp_dev = logp.to(DEV)[:, :V]  # a strided view: ld = V + 3
    got = ops.trie_beam_step(trie.trie, tokens, depth, torch.from_numpy(node_in).to(DEV),
                             torch.from_numpy(score_in).to(DEV), logp_dev, beam_out)
    wide = logp.float().numpy()
    filled = 0
    for b in range(B):
        want = model.beam_step(depth, node_in[b].tolist(), score_in[b], wide[b * beam_in:(b + 1) * beam_in], beam_out)
        assert got.node[b].tolist() == [w[0] for w in want]
        assert got.score[b].cpu().numpy().view(np.int32).tolist() == [
            int(np.float32(w[1]).view(np.int32)) for w in want]
        assert got.parent[b].tolist() == [w[2] for w in want]
        assert got.value[b].tolist() == [w[3] for w in want]
        assert got.token[b].tolist() == [w[4] for w in want]
        filled += sum(w[0] >= 0 for w in want)
    assert filled > 0
    again = ops.trie_beam_step(trie.trie, tokens, depth, torch.from_numpy(node_in).to(DEV),
                               torch.from_numpy(score_in).to(DEV), logp_dev, beam_out)
    assert torch.equal(again.node, got.node) and torch.equal(again.score.view(torch.int32), got.score.view(torch.int32))
    if depth == 0:  # score_in None is a score of 0
        score0 = ops.trie_beam_step(trie.trie, tokens, 0, torch.zeros(B, 1, dtype=torch.int32, device=DEV), None,
                                    logp_dev, beam_out)
        for b in range(B):
            want = model.beam_step(0, [0], np.zeros(1, np.float32), wide[b:b + 1], beam_out)
            assert score0.node[b].tolist() == [w[0] for w in want]


def test_beam_search_is_the_brute_force_ranking():
    sizes, beam, B = (3, 3, 4), 64, 2
    rng = np.random.default_rng(41)
    ids = np.stack([rng.integers(0, s, 60) for s in sizes], 1).astype(np.int32)
    trie = SemanticIDTrie.from_ids(ids, sizes)  # the identity token map: V = 11, eos = 10
    vocab = trie.tokens.vocab_size
    table = torch.from_numpy(-rng.random((B, 3, vocab)).astype(np.float32) * 5)
    table_dev = table.to(DEV)

    def step_fn(depth, values):
        assert values.shape[0] == B and values.shape[2] == depth
        return table_dev[:, depth, :].repeat_interleave(values.shape[1], 0).contiguous()

    out = constrained_beam_search(trie, step_fn, B, beam)
    cells = np.unique(ids, axis=0)
    offs = trie.tokens.level_off
    for b in range(B):
        t = table[b].numpy()
        score = np.zeros(len(cells), dtype=np.float32)
        for l in range(3):
            score = (score + t[l, offs[l] + cells[:, l]]).astype(np.float32)
        order = np.argsort(-score, kind="stable")
        assert len(np.unique(score)) == len(score)  # no ties: the ranking is the scores' alone
        n = len(cells)
        assert out.cells[b, :n].tolist() == order.tolist() and (out.cells[b, n:] == -1).all()
        assert out.scores[b, :n].cpu().numpy().view(np.int32).tolist() == score[order].view(np.int32).tolist()
        assert np.array_equal(out.ids[b, :n].cpu().numpy(), cells[order])
        assert (out.scores[b, n:] == float("-inf")).all() and (out.ids[b, n:] == -1).all()
    lo, hi = trie.index.prefix_ranges(out.ids.clamp_min(0))
    found = out.cells >= 0
    assert torch.equal(out.lo[found], lo[found]) and torch.equal(out.hi[found], hi[found])
    assert (out.hi[found] > out.lo[found]).all() and int(out.lo[~found].abs().sum() + out.hi[~found].abs().sum()) == 0


@pytest.mark.parametrize("beam_out", [8, 64])
def test_step_with_more_candidates_than_threads(beam_out):
    """Wide nodes: a thread owns several candidates, so the thread whose candidate is taken has to find its next."""
    sizes, B, beam_in = (3, 700), 2, 3
    rng = np.random.default_rng(51)
    ids = np.stack([rng.integers(0, s, 1500) for s in sizes], 1).astype(np.int32)
    trie = SemanticIDTrie.from_ids(ids, sizes)
    vocab = trie.tokens.vocab_size
    model = M.TrieModel(sorted({tuple(int(v) for v in r) for r in ids}), sizes,
                        [np.arange(3), 3 + np.arange(700)], vocab - 1, vocab)
    gen = torch.Generator().manual_seed(beam_out)
    logp = torch.randint(-3, 1, (B * beam_in, vocab), generator=gen).float()  # four values: ties everywhere
    node_in = np.asarray([[0, 1, 2], [2, 2, 0]], dtype=np.int32)
    score_in = np.asarray([[0, -1, 0], [-2, -2, -1]], dtype=np.float32)
    got = ops.trie_beam_step(trie.trie, trie.tokens, 1, torch.from_numpy(node_in).to(DEV),
                             torch.from_numpy(score_in).to(DEV), logp.to(DEV), beam_out)
    for b in range(B):
        want = model.beam_step(1, node_in[b].tolist(), score_in[b], logp[b * beam_in:(b + 1) * beam_in].numpy(),
                               beam_out)
        assert got.node[b].tolist() == [w[0] for w in want]
        assert got.score[b].tolist() == [float(w[1]) for w in want]
        assert got.parent[b].tolist() == [w[2] for w in want]
        assert got.value[b].tolist() == [w[3] for w in want]
        assert got.token[b].tolist() == [w[4] for w in want]
