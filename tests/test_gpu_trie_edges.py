"""The trie kernels where the first tests did not reach: token rows longer than a wave, 1 / 4 / 8
levels in the mask and the beam step, builds of more than 1024 scan tiles, the caps (64 hypotheses, 8192 children,
2^20 tokens, slices of exactly one and one-plus-one elements), scores of both signs down to the subnormals, eos among
the ID tokens, and what the consumers may not read: entries past the counts, corrupted child offsets (error bit 1) and
level_tok entries (bit 2).  Every comparison is for equality, against tests/_trie_model.py; the inputs come from
tests/_trie_cases.py, where test_trie_model.py checks what they hold."""
import copy
import functools
import re

import numpy as np
import pytest
import torch

from generative_ranking_recommender_amd import ops
from generative_ranking_recommender_amd.semantic_id_trie import constrained_beam_search
from tests import _trie_cases as C
from tests import _trie_model as M
from tests.test_gpu_id_trie import build
from tests.test_gpu_trie_mask import DEV, DTYPES, Setup, run_and_check

pytestmark = pytest.mark.gpu
FORMAT = {torch.float32: "f32", torch.float16: "f16", torch.bfloat16: "bf16"}


@functools.lru_cache(maxsize=None)
def setup_of(name):
    return Setup(**C.spec(name))


def wider(dtype):
    return 1 if dtype == torch.float32 else 3


# ------------------------------------------------------------------------------------------------------- long rows
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("T", C.LONG_T)
def test_mask_rows_longer_than_a_wave(T, dtype):
    s = setup_of("edge")
    rows, where = C.long_rows(s.level_tok, s.V, s.kept, T, seed=T, fill=C.long_fill(s))
    C.check_long_rows(s.model, rows, where, T)
    for n, (ids_dtype, wide_ids) in enumerate([(torch.int64, False), (torch.int32, True), (torch.int32, False),
                                               (torch.int64, True)]):
        run_and_check(s, rows, dtype, s.V + (n % 2) * wider(dtype), ids_dtype=ids_dtype, seed=n, wide_ids=wide_ids)
    run_and_check(s, rows[5:6], dtype, s.V, wide_ids=True)  # B = 1: the row base alone is off the buffer's start


# ---------------------------------------------------------------------------------------------- levels 1, 4 and 8
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["levels1", "levels4", "levels8"])
def test_mask_with_other_numbers_of_levels(name, dtype):
    s = setup_of(name)
    L = len(s.sizes)
    rows = s.rows_of_every_kind(T=max(L + 2, 5), seed=3, n_random=6)
    kind = run_and_check(s, rows, dtype, s.V + wider(dtype))
    assert set(kind.tolist()) == ({0, 1} if L == 1 else {0, 1, 2})
    run_and_check(s, rows, dtype, s.V, ids_dtype=torch.int32, seed=2)


def step_and_check(trie, tokens, model, depth, node_in, score_in, logp, dtype, beam_out, wide=False):
    """One beam step against the model, every output for equality (scores by their bits), twice; returns the model's
    slots per batch row.  ``logp``: f32 numpy [B * beam_in, V] of values exact in ``dtype``."""
    B, beam_in = node_in.shape
    t = torch.from_numpy(logp).to(dtype)
    padded = torch.full((len(t), t.shape[1] + 3), float("nan"), dtype=dtype)
    padded[:, :t.shape[1]] = t
    logp_dev = padded.to(DEV)[:, :t.shape[1]]  # a strided view: ld = V + 3
    args = (trie, tokens, depth, torch.from_numpy(node_in).to(DEV), torch.from_numpy(score_in).to(DEV), logp_dev,
            beam_out)
    got = ops.trie_beam_step(*args)
    seen = t.float().numpy()
    wants = []
    for b in range(B):
        step = model.beam_step_wide if wide else model.beam_step
        want = step(depth, node_in[b].tolist(), score_in[b], seen[b * beam_in:(b + 1) * beam_in], beam_out)
        assert got.node[b].tolist() == [w[0] for w in want]
        assert got.score[b].cpu().numpy().view(np.int32).tolist() == [
            int(np.float32(w[1]).view(np.int32)) for w in want]
        assert got.parent[b].tolist() == [w[2] for w in want]
        assert got.value[b].tolist() == [w[3] for w in want]
        assert got.token[b].tolist() == [w[4] for w in want]
        wants.append(want)
    again = ops.trie_beam_step(*args)
    for a, g in zip((again.node, again.score.view(torch.int32), again.parent, again.value, again.token),
                    (got.node, got.score.view(torch.int32), got.parent, got.value, got.token)):
        assert torch.equal(a, g)
    return wants, got


def step_inputs(model, depth, beam_in, B, V, dtype, seed, live=1.0):
    n_nodes = len(model.nodes[depth])
    node_in = np.random.default_rng(seed).integers(0, n_nodes, (B, beam_in)).astype(np.int32)
    score_in, logp = C.edge_scores(B, beam_in, V, FORMAT[dtype], seed=seed + 10, live=live)
    C.dead_hypotheses(node_in, score_in, n_nodes)
    for b in range(B):
        C.check_ties_are_planned(model, depth, node_in[b].tolist(), score_in[b], logp[b * beam_in:(b + 1) * beam_in])
    return node_in, score_in, logp


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["levels1", "levels4", "levels8"])
def test_step_at_every_depth_of_other_numbers_of_levels(name, dtype):
    s = setup_of(name)
    filled = 0
    for depth in range(len(s.sizes)):
        beam_in = 1 if depth == 0 else 8
        node_in, score_in, logp = step_inputs(s.model, depth, beam_in, 4, s.V, dtype, seed=depth)
        wants, _ = step_and_check(s.trie.trie, s.tokens, s.model, depth, node_in, score_in, logp, dtype, 6)
        filled += sum(w[0] >= 0 for want in wants for w in want)
    assert filled > 0


def brute_force_search(s, beam, B, seed, trie=None):
    """constrained_beam_search with beam >= the number of IDs kept, against the ranking of all kept cells."""
    L = len(s.sizes)
    rng = np.random.default_rng(seed)
    table = torch.from_numpy(-rng.random((B, L, s.V)).astype(np.float32) * 5)
    table_dev = table.to(DEV)

    def step_fn(depth, values):
        assert values.shape[0] == B and values.shape[2] == depth
        return table_dev[:, depth, :].repeat_interleave(values.shape[1], 0).contiguous()

    out = constrained_beam_search(s.trie if trie is None else trie, step_fn, B, beam)
    cells = np.unique(s.ids, axis=0)  # the index's cells, in its order
    kept = np.asarray([i for i, c in enumerate(cells) if tuple(int(v) for v in c) in set(s.kept)])
    assert 0 < len(kept) <= beam and len(kept) < len(cells)
    for b in range(B):
        t = table[b].numpy()
        score = np.zeros(len(kept), dtype=np.float32)
        for l in range(L):
            score = (score + t[l, s.level_tok[l][cells[kept, l]]]).astype(np.float32)
        order = np.argsort(-score, kind="stable")
        assert len(np.unique(score)) == len(score)  # no ties: the ranking is the scores' alone
        n = len(kept)
        assert out.cells[b, :n].tolist() == kept[order].tolist() and (out.cells[b, n:] == -1).all()
        assert out.scores[b, :n].cpu().numpy().view(np.int32).tolist() == score[order].view(np.int32).tolist()
        assert np.array_equal(out.ids[b, :n].cpu().numpy(), cells[kept][order])
        assert (out.scores[b, n:] == float("-inf")).all() and (out.ids[b, n:] == -1).all()
    return out


def test_beam_search_over_eight_levels_is_the_brute_force_ranking():
    brute_force_search(setup_of("levels8"), beam=64, B=2, seed=43)


# ------------------------------------------------------------------------------ builds beyond one run of scan tiles
@pytest.mark.parametrize("n, which", [(n, w) for n in C.BUILD_N for w in C.BUILD_KEEPS if (n, w) != (2048, "multiple")])
def test_tables_of_sampled_cells_equal_the_sorted_model(n, which):
    """2048 cells a tile and 1024 threads over the tile sums: from 2048 * 1024 + 1 cells on a thread scans a run of
    two tiles, the last run is partly filled and the last threads have none."""
    cells = C.sampled_cells(n)
    keep = C.build_keep(cells, which)
    want = M.tables_sorted(cells, 4, keep)
    if which == "all":
        C.check_build_cells(cells, want)
    trie = build(cells, C.BUILD_SIZES, keep, check=False)
    assert int(trie.error.item()) == 0
    got = trie.to_arrays()
    assert got["count"].tolist() == want["count"].tolist()
    for d in range(4):
        assert np.array_equal(got[f"value{d}"], want["value"][d]), d
        assert np.array_equal(got[f"child_off{d}"], want["child_off"][d]), d
    assert np.array_equal(got["leaf_cell"], want["leaf_cell"])
    if which in ("all", "fraction"):
        again = build(cells, C.BUILD_SIZES, keep).to_arrays()
        assert all(got[k].tobytes() == again[k].tobytes() for k in got)  # two calls give identical bytes


# ---------------------------------------------------------------------------------------------- caps, slice edges
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("V", [1, 2, 7, 8192, 8193, 16384])
def test_mask_vocabulary_of_one_slice_and_around(V, dtype):
    s = setup_of(f"v{V}")
    rows = s.rows_of_every_kind(T=4, seed=V, n_random=8)
    assert len(rows) >= 9
    for ld in (V, V + wider(dtype)):
        run_and_check(s, rows, dtype, ld, seed=ld)
    if dtype != torch.float32 and V in (1, 8193):
        # the last slice is one element: with ld = V row b's last slice starts at element 1 + b * V + (V - 1) of the
        # buffer, on the 16-byte grid for some rows (the element is the tail) and off it for others (the head)
        on_grid = {(1 + b * V + V - 1) % 8 == 0 for b in range(len(rows))}
        assert on_grid == {True, False}


@pytest.mark.parametrize("dtype", DTYPES)
def test_mask_largest_vocabulary(dtype):
    V = ops.TRIE_VOCAB_MAX
    s = setup_of(f"v{V}")
    a = s.kept[0]
    rows = np.asarray([[5, 6, s.tok(0, a[0]), s.tok(1, a[1])], [5, 6, 7, 9]])  # complete; the root's children
    kind = run_and_check(s, rows, dtype, V + wider(dtype))
    assert kind.tolist() == [1, 0]
    allowed = s.model.rows(rows)[3]
    assert allowed[:, [0, 8191, 8192, V - 1]].all() and allowed.sum(1).tolist() == [5, 4]


@pytest.mark.parametrize("dtype", DTYPES)
def test_mask_node_of_8192_children(dtype):
    s = setup_of("fan8192")
    rows = s.rows_of_every_kind(T=5, seed=6, n_random=4)
    kind, _, count, allowed = s.model.rows(rows)
    wide = (kind == 0) & (count == 8192)
    assert wide.any() and allowed[wide][:, :8192].any() and allowed[wide][:, 8192:].any()  # over two slices
    run_and_check(s, rows, dtype, s.V + wider(dtype))


@pytest.mark.parametrize("dtype", DTYPES)
def test_step_of_64_hypotheses_over_nodes_of_8192_children(dtype):
    s = setup_of("fan8192")
    node_in, score_in, logp = step_inputs(s.model, 1, 64, 3, s.V, dtype, seed=1, live=0.002)
    assert all(len(set(row.tolist())) < 64 for row in node_in)  # equal nodes among the hypotheses
    wants, _ = step_and_check(s.trie.trie, s.tokens, s.model, 1, node_in, score_in, logp, dtype, 64, wide=True)
    parents = {w[2] for want in wants for w in want}
    assert max(parents) >= 32 and len(parents) > 8 and all(w[0] >= 0 for want in wants for w in want)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("depth", [0, 1, 2])
def test_step_of_64_hypotheses_on_a_small_trie(depth, dtype):
    s = setup_of("poison")
    node_in, score_in, logp = step_inputs(s.model, depth, 64, 3, s.V, dtype, seed=depth)
    for beam_out in (5, 64):
        wants, _ = step_and_check(s.trie.trie, s.tokens, s.model, depth, node_in, score_in, logp, dtype, beam_out)
    parents = {w[2] for want in wants for w in want}
    scores = np.asarray([w[1] for want in wants for w in want if w[0] >= 0], dtype=np.float32)
    assert max(parents) >= 32 and (scores > 0).any() and (depth == 0 or (scores < 0).any())
    tiny = scores[(scores != 0) & (np.abs(scores) < 2.0 ** -126)] if dtype != torch.float16 else \
        scores[(scores != 0) & (np.abs(scores) < 2.0 ** -13)]
    assert len(np.unique(tiny)) > 1  # distinct sums in the subnormal range among the winners


# ------------------------------------------------------------------------------------------ eos among the ID tokens
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["eos_level0", "eos_level1"])
def test_mask_with_eos_among_the_id_tokens(name, dtype):
    s = setup_of(name)
    rows = s.rows_of_every_kind(T=5, seed=3, n_random=6)
    kind = run_and_check(s, rows, dtype, s.V + wider(dtype))
    assert set(kind.tolist()) == {0, 1, 2}
    with_eos = np.concatenate([rows, np.full((len(rows), 1), s.eos)], 1)  # eos as the last token of every row
    run_and_check(s, with_eos, dtype, s.V, ids_dtype=torch.int32)


# ------------------------------------------------------------------- what the consumers may not read, the error word
def clone_tables(t):
    return ops.IdTrie(t.count.clone(), t.value.clone(), t.child_off.clone(), t.leaf_cell.clone(), t.sizes, t.counts())


def consumers(s, trie, dtype, tokens=None, model=None, word=0):
    """Mask, beam step at every depth and (with the setup's own tokens) the exhaustive search over ``trie``, each
    against the model; returns the outputs for a comparison between tries."""
    tokens = s.tokens if tokens is None else tokens
    model = s.model if model is None else model
    rows = s.rows_of_every_kind(T=5, seed=3, n_random=6)
    ws = ops.TrieMaskWorkspace(len(rows), DEV)
    run_and_check(s, rows, dtype, s.V + 3, trie=trie, tokens=tokens, model=model, workspace=ws, check=False)
    assert int(ws.error_word().item()) == word
    outs = []
    for depth in range(len(s.sizes)):
        beam_in = 1 if depth == 0 else 8
        node_in, score_in, logp = step_inputs(model, depth, beam_in, 3, s.V, dtype, seed=depth)
        _, got = step_and_check(trie, tokens, model, depth, node_in, score_in, logp, dtype, 7)
        outs += [got.node, got.score.view(torch.int32), got.parent, got.value, got.token]
    return outs


def test_entries_past_the_counts_are_not_read_and_capacity_does_not_matter():
    s = setup_of("poison")
    t, L = s.trie.trie, len(s.sizes)
    cnt = t.counts()
    assert t.capacity > max(cnt[1:])  # cells were dropped: there are entries past every count
    plain = consumers(s, t, torch.float32)
    found = brute_force_search(s, beam=64, B=2, seed=47)
    tries = [ops.IdTrie.from_arrays(t.to_arrays(), DEV)]  # capacity = the number of leaves
    assert tries[0].capacity == cnt[L] < t.capacity
    for poison in (0x7fffffff, -1):
        p = clone_tables(t)
        for d in range(L):
            p.value[d, cnt[d + 1]:] = poison
            p.child_off[d, cnt[d] + 1:] = poison
        p.leaf_cell[cnt[L]:] = poison
        tries.append(p)
    for other in tries:
        for dtype in DTYPES:
            outs = consumers(s, other, dtype)
            if dtype == torch.float32:
                assert all(torch.equal(a, b) for a, b in zip(outs, plain))
        whole = copy.copy(s.trie)
        whole.trie = other
        again = brute_force_search(s, beam=64, B=2, seed=47, trie=whole)
        assert torch.equal(again.cells, found.cells) and torch.equal(again.ids, found.ids)
        assert torch.equal(again.scores.view(torch.int32), found.scores.view(torch.int32))


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_child_range_outside_the_counts_is_clamped_and_reported(dtype):
    """Error bit 1.  Both corruptions are the clamped value's neighbours, so the answers stay those of the intact trie;
    even an unchecked use would stay inside the tables (cells were dropped: capacity > count)."""
    s = setup_of("poison")
    t = s.trie.trie
    cnt = t.counts()
    assert t.capacity > cnt[2] + 1
    fill = C.long_fill(s)[0]
    first, last = s.kept[0], s.kept[-1]
    assert first[0] != last[0]

    def rows_through(a):  # rows that ask for the children of the depth-1 node of level-0 value a[0]
        return np.asarray([[fill, fill, s.tok(0, a[0])], [fill, s.tok(0, a[0]), s.tok(1, a[1])]])
    apart = np.asarray([[fill, fill, fill], [s.tok(l, v) for l, v in enumerate(first)]])  # the root; complete
    high = clone_tables(t)
    high.child_off[1, cnt[1]] = cnt[2] + 1  # the last depth-1 node's range ends one past the count,
    spare = next(v for v in range(s.sizes[1]) if s.tok(1, v) >= 0 and last[:1] + (v,) not in s.model.nodes[2])
    high.value[1, cnt[2]] = spare           # where a value with a token waits: a reader past the count allows it
    low = clone_tables(t)
    low.child_off[1, 0] = -1                # the first one's starts below zero
    root = clone_tables(t)
    root.child_off[0, 1] = cnt[1] + 1       # the root's: every walk passes it, a complete row does not
    for bad, touched, untouched in ((high, rows_through(last), (rows_through(first), apart)),
                                    (low, rows_through(first), (rows_through(last), apart)),
                                    (root, rows_through(first), (apart[1:],))):
        ws = ops.TrieMaskWorkspace(2, DEV)
        run_and_check(s, touched, dtype, s.V + 3, trie=bad, workspace=ws, check=False)
        assert int(ws.error_word().item()) == 1
        run_and_check(s, touched, dtype, s.V + 3, trie=t, workspace=ws, check=False)
        assert int(ws.error_word().item()) == 1  # sticky: the intact trie does not clear it
        with pytest.raises(RuntimeError, match=re.escape(ops.TRIE_MASK_WORD)):
            run_and_check(s, touched, dtype, s.V, trie=bad, workspace=ops.TrieMaskWorkspace(2, DEV), check=True)
        for rows in untouched:
            ws = ops.TrieMaskWorkspace(2, DEV)
            run_and_check(s, rows, dtype, s.V + 3, trie=bad, workspace=ws, check=False)
            assert int(ws.error_word().item()) == 0


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_level_tok_entry_outside_the_vocabulary_is_skipped_and_reported(dtype):
    """Error bit 2.  The constructor refuses such a table, so the device tensor is patched; tok_code still knows the
    tokens, and the model takes a number outside [0, V) for "no token" as the kernel must.  ld = V + 3, so a store at
    V + 1 would land in the padding that run_and_check compares."""
    s = setup_of("poison")
    seconds = sorted({k[1] for k in s.kept})
    v1, v2, v0 = s.kept[0][1], next(v for v in seconds if v != s.kept[0][1]), s.kept[3][0]
    for level, patches in ((1, ((v1, s.V + 1), (v2, -5))), (0, ((v0, s.V + 1),))):
        tokens = copy.copy(s.tokens)
        tokens.level_tok = s.tokens.level_tok.clone()
        model = copy.deepcopy(s.model)
        for v, number in patches:
            tokens.level_tok[tokens.level_off[level] + v] = number
            model.level_tok[level][v] = number
        assert model.code == s.model.code
        kind, _, count, _ = model.rows(s.rows_of_every_kind(T=5, seed=3, n_random=6))
        plain = s.model.rows(s.rows_of_every_kind(T=5, seed=3, n_random=6))[2]
        changed = count != plain
        assert changed[kind == (1 if level == 0 else 0)].any()  # the patched entry is among some row's children
        consumers(s, s.trie.trie, dtype, tokens=tokens, model=model, word=2)
        with pytest.raises(RuntimeError, match=re.escape(ops.TRIE_MASK_WORD)):
            rows = torch.from_numpy(s.rows_of_every_kind(T=5, seed=3)).to(DEV)
            ops.trie_mask(s.trie.trie, tokens, rows, torch.zeros(len(rows), s.V, dtype=dtype, device=DEV))
