"""rqsid_assign_topk / RQEncoder.encode_topk / margin_report on the GPU.

The oracle is numpy: per row the fp64 ``((v - c)^2).sum()`` of every allowed centre, stable-sorted (ties keep list
order).  Random cases first assert that the oracle's adjacent gaps among the first k + 1 places exceed 1e-12
relative (the expected order is then no accident of fp64 summation order); constructed exact ties are exempt.  The
expected distance is fl32(sqrt(d2)), accepted within 1 fp32 ulp (fp64 summation order moves d2 by ~ dim 2^-53,
which can flip at most one rounding).
"""
import functools
import json
import os
import socket
import types

import numpy as np
import pytest
import torch

from generative_ranking_recommender_amd import io as rq_io
from generative_ranking_recommender_amd import ops, synth
from generative_ranking_recommender_amd.encode import HIERARCHICAL_TRAIN, SIMPLIFIED, RQEncoder
from generative_ranking_recommender_amd.hierarchical_rq_kmeans import HierarchicalRQKMeans, HierarchicalRQKMeansConfig
from generative_ranking_recommender_amd.margin_report import margin_report

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
F32 = np.float32
INF = float("inf")


def gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(t):
    return t.contiguous().view(torch.int32)


def oracle(v, c, lists, seg, k, tie_ok=False):
    """v [n, d] f32, c [K, d] f32, lists[s] = allowed centre rows of segment s in list order, seg [n].
    Returns (pos, glob, d) [n, k]: position in the list, centre row, fp64 distance; -1 / -1 / inf past the list."""
    n = len(v)
    pos = np.full((n, k), -1, dtype=np.int64)
    glob = np.full((n, k), -1, dtype=np.int64)
    dist = np.full((n, k), INF)
    c64 = c.astype(np.float64)
    for s in np.unique(seg):
        rows = np.nonzero(seg == s)[0]
        idx = np.asarray(lists[s], dtype=np.int64)
        if len(idx) == 0:
            continue
        d2 = np.empty((len(rows), len(idx)))
        for j0 in range(0, len(idx), 256):
            diff = v[rows].astype(np.float64)[:, None, :] - c64[idx[j0:j0 + 256]][None]
            d2[:, j0:j0 + 256] = (diff ** 2).sum(-1)
        order = np.argsort(d2, axis=1, kind="stable")
        top = order[:, :k + 1]
        srt = np.take_along_axis(d2, top, 1)
        if not tie_ok and srt.shape[1] > 1:
            gap = np.diff(srt, axis=1)
            assert (gap > 1e-12 * srt[:, 1:]).all(), "oracle places closer than 1e-12 relative"
        m = min(k, len(idx))
        pos[rows, :m] = order[:, :m]
        glob[rows, :m] = idx[order[:, :m]]
        dist[rows, :m] = np.sqrt(np.take_along_axis(d2, order[:, :m], 1))
    return pos, glob, dist


def assert_dist(got, want64):
    """got f32 against fl32(sqrt(d2)) within one fp32 ulp; inf where the oracle has no place."""
    got = np.asarray(got)
    want = want64.astype(F32)
    fin = np.isfinite(want64)
    assert (np.isinf(got[~fin]) & (got[~fin] > 0)).all()
    ulp = np.spacing(np.abs(want[fin]))
    assert (np.abs(got[fin].astype(np.float64) - want[fin].astype(np.float64)) <= ulp).all(), \
        float(np.abs(got[fin].astype(np.float64) - want[fin]).max())


def run_topk(x, c, buckets, cand, k, **kw):
    pc = c if isinstance(c, ops.PreparedCenters) else ops.prepare_centers(gpu(c))
    ws = kw.pop("workspace", None) or ops.TopKWorkspace(len(x), k, DEV)
    xd = x if isinstance(x, torch.Tensor) else gpu(x)
    loc, glob, dist = ops.assign_topk(xd, pc, buckets, cand, k, workspace=ws, **kw)
    assert int(ws.error_word().item()) == 0
    return loc.cpu().numpy(), glob.cpu().numpy(), dist.cpu().numpy(), ws.counters()


def all_cand(K):
    return ops.Candidates(torch.zeros(1, dtype=torch.int32, device=DEV),
                          torch.full((1,), K, dtype=torch.int32, device=DEV), K)


# ------------------------------------------------------------------------------ 1. one segment, unconstrained
@functools.lru_cache(maxsize=None)
def _dense(n, d, K, scale, seed=11):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((n, d)) * scale).astype(F32)
    c = (rng.standard_normal((K, d)) * scale).astype(F32)
    return x, c


@pytest.mark.parametrize("scale", [1e-3, 1.0, 1e3])
@pytest.mark.parametrize("k", [1, 3, 8])
def test_one_segment(k, scale):
    n, d, K = 300, 64, 40
    x, c = _dense(n, d, K, scale)
    pos, glob, dist = oracle(x, c, [np.arange(K)], np.zeros(n, dtype=np.int64), k)
    pc = ops.prepare_centers(gpu(c))
    loc, g, dd, cnt = run_topk(x, pc, ops.single_segment(n, DEV), all_cand(K), k)
    assert (loc == pos).all() and (g == glob).all()
    assert_dist(dd, dist)
    assert (g[:, 0] == ops.nearest(gpu(x), pc).cpu().numpy()).all()
    assert cnt["listed_rows"] + cnt["all_candidate_rows"] == n and cnt["nonfinite_rows"] == 0
    l3, g3, d3 = (t.cpu().numpy() for t in ops.nearest_topk(gpu(x), pc, k))
    assert (g3 == g).all() and (l3 == loc).all() and (d3.view(np.int32) == dd.view(np.int32)).all()


@pytest.mark.parametrize("d", [32, 1024])
def test_narrowest_and_widest_rows(d):
    n, K, k = 300, 40, 2
    x, c = _dense(n, d, K, 1.0, seed=12)
    pos, glob, dist = oracle(x, c, [np.arange(K)], np.zeros(n, dtype=np.int64), k)
    loc, g, dd, _ = run_topk(x, c, ops.single_segment(n, DEV), all_cand(K), k)
    assert (loc == pos).all() and (g == glob).all()
    assert_dist(dd, dist)


# ------------------------------------------------------------------------------------------- 2. short lists
def test_short_lists_empty_and_penalty_segments():
    rng = np.random.default_rng(21)
    d, K, k = 64, 16, 8
    match = np.zeros((5, K), dtype=np.uint8)
    match[0, [3]] = 1
    match[1, [2, 9]] = 1
    match[2, [0, 4, 5, 11, 15]] = 1
    match[3, [1, 6, 7]] = 1   # a segment without rows
    # row 4 stays empty: a penalty segment, with rows
    seg = np.repeat([0, 1, 2, 4], [150, 7, 130, 40])
    rng.shuffle(seg)
    n = len(seg)
    x = rng.standard_normal((n, d)).astype(F32)
    c = rng.standard_normal((K, d)).astype(F32)
    cand = ops.match_to_candidates(gpu(match))
    assert cand.flags.cpu().tolist() == [0, 0, 0, 0, 1]
    b = ops.bucket(gpu(seg.astype(np.int32)), 5)
    lists = [np.nonzero(r)[0] for r in match]
    pos, glob, dist = oracle(x, c, lists, seg, k)
    loc, g, dd, cnt = run_topk(x, c, b, cand, k)
    assert (loc == pos).all() and (g == glob).all()
    assert_dist(dd, dist)
    for s, m in ((0, 1), (1, 2), (2, 5), (4, 0)):
        r = seg == s
        assert (loc[r][:, m:] == -1).all() and (g[r][:, m:] == -1).all() and np.isposinf(dd[r][:, m:]).all()
        assert (loc[r][:, :m] >= 0).all()
    assert cnt["nonfinite_rows"] == 0


# -------------------------------------------------------------------------------------------- 3. wide lists
def test_wide_segment():
    n, d, K, k = 130, 32, 2560, 8
    x, c = _dense(n, d, K, 1.0, seed=31)
    pos, glob, dist = oracle(x, c, [np.arange(K)], np.zeros(n, dtype=np.int64), k)
    loc, g, dd, cnt = run_topk(x, c, ops.single_segment(n, DEV), all_cand(K), k)
    assert (loc == pos).all() and (g == glob).all()
    assert_dist(dd, dist)
    assert cnt["all_candidate_rows"] == 0, cnt  # twenty screen groups, and no list overflowed


def test_list_driven_ragged_counts():
    rng = np.random.default_rng(32)
    n, d, K, k, S = 700, 64, 300, 4, 6
    match = (rng.random((S, K)) < np.array([0.01, 0.05, 0.2, 0.5, 0.9, 1.0])[:, None]).astype(np.uint8)
    match[0, :] = 0
    match[0, [7, 200]] = 1
    seg = rng.integers(0, S, n)
    x = rng.standard_normal((n, d)).astype(F32)
    c = rng.standard_normal((K, d)).astype(F32)
    cand = ops.match_to_candidates(gpu(match))
    b = ops.bucket(gpu(seg.astype(np.int32)), S)
    pos, glob, dist = oracle(x, c, [np.nonzero(r)[0] for r in match], seg, k)
    loc, g, dd, _ = run_topk(x, c, b, cand, k)
    assert (loc == pos).all() and (g == glob).all()
    assert_dist(dd, dist)
    pc = ops.prepare_centers(gpu(c))
    a_loc, a_glob = ops.assign(gpu(x), pc, b, cand)
    assert (a_loc.cpu().numpy() == loc[:, 0]).all() and (a_glob.cpu().numpy() == g[:, 0]).all()


# --------------------------------------------------------------------------------------------------- 4. ties
def test_duplicate_centres_and_equidistant_rows_rank_by_list_position():
    rng = np.random.default_rng(41)
    n, d, K, k = 200, 64, 12, 5
    c = rng.standard_normal((K, d)).astype(F32)
    c[7] = c[3]
    c[9] = c[3]
    # centres 0 and 1 mirror each other in coordinate 0; rows with x_0 = 0 are exactly equidistant from them
    c[1] = c[0]
    c[0, 0], c[1, 0] = 1.5, -1.5
    x = rng.standard_normal((n, d)).astype(F32)
    x[:60, 0] = 0.0
    x[:60] += 0.7 * c[0]
    x[:60, 0] = 0.0
    x[60:120] = c[3] + 0.3 * x[60:120]  # rows whose first places are the three copies
    pos, glob, dist = oracle(x, c, [np.arange(K)], np.zeros(n, dtype=np.int64), k, tie_ok=True)
    assert (pos[:60, :2] == [0, 1]).all() and (dist[:60, 0] == dist[:60, 1]).all()
    assert (pos[60:120, :3] == [3, 7, 9]).all()
    loc, g, dd, _ = run_topk(x, c, ops.single_segment(n, DEV), all_cand(K), k)
    assert (loc == pos).all() and (g == glob).all()
    assert_dist(dd, dist)
    assert (dd[60:120, 0].view(np.int32) == dd[60:120, 2].view(np.int32)).all()


def test_forty_identical_centres():
    rng = np.random.default_rng(42)
    n, d, K, k = 150, 64, 40, 8
    c = np.repeat(rng.standard_normal((1, d)).astype(F32), K, 0)
    x = rng.standard_normal((n, d)).astype(F32)
    loc, g, dd, cnt = run_topk(x, c, ops.single_segment(n, DEV), all_cand(K), k)
    assert (loc == np.arange(k)).all() and (g == np.arange(k)).all()
    _, _, dist = oracle(x, c, [np.arange(K)], np.zeros(n, dtype=np.int64), k, tie_ok=True)
    assert_dist(dd, dist)
    assert cnt["all_candidate_rows"] > 0, cnt  # forty equal keys fit no list


def test_centres_one_ulp_apart():
    rng = np.random.default_rng(43)
    n, d, K, k = 200, 64, 16, 4
    base = rng.standard_normal((4, d)).astype(F32)
    c = np.repeat(base, 4, 0)
    for j in range(K):  # copy j % 4 of a base centre is moved j % 4 ulps in one coordinate
        col = 5 + j // 4
        for _ in range(j % 4):
            c[j, col] = np.nextafter(c[j, col], F32(np.inf))
    x = base[rng.integers(0, 4, n)] + 0.5 * rng.standard_normal((n, d))
    x[:, 5:9] += 3.0  # well off the centres in the moved coordinates: one ulp there moves d2 by far more than 1e-12
    x = x.astype(F32)
    pos, glob, dist = oracle(x, c, [np.arange(K)], np.zeros(n, dtype=np.int64), k)
    loc, g, dd, _ = run_topk(x, c, ops.single_segment(n, DEV), all_cand(K), k)
    assert (loc == pos).all() and (g == glob).all()
    assert_dist(dd, dist)


# ------------------------------------------------------------------------------------ 5. encoder, three levels
NEED = [4, 4, 8]
ENC_D, ENC_ROWS, ENC_CAND = 64, 2000, 40
SEM = {"hier": HIERARCHICAL_TRAIN, "simplified": SIMPLIFIED}


@functools.lru_cache(maxsize=None)
def _enc_data(dup=False):
    rng = np.random.default_rng(51)
    x = synth.small_mixture(ENC_ROWS, d=ENC_D, m=16, seed=52)
    # (near four rows, not on them: a row that IS its centre has a zero residual, equidistant from unit centres)
    c0 = (x[rng.choice(ENC_ROWS, NEED[0], replace=False)] + 0.05 * rng.standard_normal((NEED[0], ENC_D))).astype(F32)

    def unit(m):
        v = rng.standard_normal((m, ENC_D)).astype(F32)
        return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F32)
    c1, c2 = unit(NEED[0] * NEED[1]), unit(ENC_CAND)
    match = np.zeros((NEED[0] * NEED[1], ENC_CAND), dtype=np.uint8)
    for gi in range(len(match)):
        match[gi, rng.choice(ENC_CAND, NEED[2], replace=False)] = 1
    if dup:  # bitwise copies inside every list of every level
        c0[2] = c0[1]
        c1[2::4] = c1[0::4]
        c2[5] = c2[2]
        c2[30] = c2[2]
        match[:] = 1
    return x, c0, c1, c2, match


def _make_encoder(sem_name, materialized, dup=False):
    _, c0, c1, c2, match = _enc_data(dup)
    enc = RQEncoder([torch.from_numpy(c) for c in (c0, c1, c2)], NEED, match=torch.from_numpy(match),
                    semantics=SEM[sem_name], device=DEV)
    enc.force_materialized = materialized
    assert enc.fused == (not materialized)
    return enc


def _check_levels(enc, sem_name, tk, k, dup=False):
    """Level by level against the oracle on the residual rows ops.residual produces."""
    x, c0, c1, c2, match = _enc_data(dup)
    ids = tk.ids.cpu().numpy().astype(np.int64)
    loc, glob, dist = (t.cpu().numpy() for t in (tk.local, tk.glob, tk.dist))
    norm = SEM[sem_name].normalize_residual
    n = len(x)
    cols = [np.nonzero(r)[0] for r in match]
    g1 = ids[:, 0] * NEED[1] + ids[:, 1]
    v0 = gpu(x)
    v1 = ops.residual(v0, gpu(c0), gpu(ids[:, 0].astype(np.int32)), normalize=norm)
    v2 = ops.residual(v1, gpu(c1), gpu(g1.astype(np.int32)), normalize=norm)
    grp = ids[:, 0] * NEED[0] + ids[:, 1]  # both semantics: mult = 4 here
    cases = [
        (v0, c0, [np.arange(NEED[0])], np.zeros(n, dtype=np.int64), "glob"),
        (v1, c1, [np.arange(p * NEED[1], (p + 1) * NEED[1]) for p in range(NEED[0])], ids[:, 0], "pos"),
        (v2, c2, cols, grp, "pos" if sem_name == "hier" else "glob"),
    ]
    for l, (v, c, lists, seg, kind) in enumerate(cases):
        pos, gl, dd = oracle(v.cpu().numpy(), c, lists, seg, k, tie_ok=dup)
        assert (glob[:, l] == gl).all(), l
        assert (loc[:, l] == (pos if kind == "pos" else gl)).all(), l
        assert_dist(dist[:, l], dd)


@pytest.mark.parametrize("sem_name", ["hier", "simplified"])
def test_encoder_three_levels(sem_name):
    x = _enc_data()[0]
    k = 3
    out = {}
    for mat in (False, True):
        enc = _make_encoder(sem_name, mat)
        tk = enc.encode_topk(gpu(x), k)
        assert tk.local.shape == tk.glob.shape == tk.dist.shape == (len(x), 3, k)
        assert torch.equal(tk.ids, enc.encode(gpu(x)))
        assert torch.equal(tk.local[:, :, 0], tk.ids)
        _check_levels(enc, sem_name, tk, k)
        assert all(int(w.item()) == 0 for w in enc.error_words())
        out[mat] = tk
    f, m = out[False], out[True]
    assert torch.equal(f.ids, m.ids) and torch.equal(f.local, m.local) and torch.equal(f.glob, m.glob)
    fd, md = f.dist.cpu().numpy(), m.dist.cpu().numpy()
    assert (np.abs(fd.astype(np.float64) - md) <= np.spacing(np.abs(md))).all()
    # the level's first distance is its quantisation distance
    qe = _make_encoder(sem_name, False).quant_error(gpu(x))
    qd = qe.err.cpu().numpy()
    assert (np.abs(fd[:, :, 0].astype(np.float64) - qd) <= np.spacing(np.abs(qd))).all()


@pytest.mark.parametrize("sem_name", ["hier", "simplified"])
def test_encoder_with_duplicate_centres_ranks_the_duplicates(sem_name):
    x = _enc_data(True)[0]
    k = 3
    for mat in (False, True):
        enc = _make_encoder(sem_name, mat, dup=True)
        assert enc.cands[2].count_max < enc.raw_cands[2].count_max  # encode's own lists lost the copies
        tk = enc.encode_topk(gpu(x), k)
        assert torch.equal(tk.ids, enc.encode(gpu(x)))
        assert torch.equal(tk.local[:, :, 0], tk.ids)
        _check_levels(enc, sem_name, tk, k, dup=True)
        glob = tk.glob.cpu().numpy()
        first = glob[:, 2, 0] == 2  # rows nearest to the tripled last-level centre: its copies follow it
        assert first.any() and (glob[first, 2, 1] == 5).all() and (glob[first, 2, 2] == 30).all()
        assert (glob[:, 0] == 2).any() and (glob[:, 1] % 4 == 2).any()


def test_encoder_single_level_and_two_levels():
    x, c0 = _enc_data()[0], _enc_data()[1]
    enc = RQEncoder([torch.from_numpy(c0)], [4], device=DEV)
    tk = enc.encode_topk(gpu(x), 2)
    pos, gl, dd = oracle(x, c0, [np.arange(4)], np.zeros(len(x), dtype=np.int64), 2)
    assert (tk.glob.cpu().numpy()[:, 0] == gl).all() and torch.equal(tk.local, tk.glob)
    assert_dist(tk.dist.cpu().numpy()[:, 0], dd)
    two = RQEncoder([torch.from_numpy(c0), torch.from_numpy(_enc_data()[2])], [4, 4], device=DEV)
    with pytest.raises(IndexError):
        two.encode_topk(gpu(x), 2)
    with pytest.raises(ValueError):
        enc.encode_topk(gpu(x), 9)


# ---------------------------------------------------------------------------------------------- 6. 16-bit rows
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_16bit_rows_equal_their_fp32_widening(dtype):
    rng = np.random.default_rng(61)
    n, d, K, k = 300, 64, 40, 3
    c = rng.standard_normal((K, d)).astype(F32)
    x16 = gpu(rng.standard_normal((n, d)).astype(F32)).to(dtype)
    pc = ops.prepare_centers(gpu(c))
    b, cand = ops.single_segment(n, DEV), all_cand(K)
    a = ops.assign_topk(x16, pc, b, cand, k)
    w = ops.assign_topk(x16.float(), pc, b, cand, k)
    for ta, tw in zip(a, w):
        assert torch.equal(bits(ta), bits(tw))
    for sem_name in ("hier", "simplified"):
        enc = _make_encoder(sem_name, False)
        e16 = gpu(_enc_data()[0]).to(dtype)
        ta = enc.encode_topk(e16, k)
        assert enc.last_row_format == ("f16" if dtype == torch.float16 else "bf16")
        ta = [t.clone() for t in (ta.ids, ta.local, ta.glob, ta.dist)]
        tw = enc.encode_topk(e16.float(), k)
        for p, q in zip(ta, (tw.ids, tw.local, tw.glob, tw.dist)):
            assert torch.equal(bits(p), bits(q))


# ---------------------------------------------------------------------------------------------- 7. non-finite
def test_non_finite_rows():
    n, d, K, k = 300, 64, 40, 3
    x, c = _dense(n, d, K, 1.0, seed=71)
    x = x.copy()
    clean = run_topk(x, c, ops.single_segment(n, DEV), all_cand(K), k)
    bad = np.array([0, 5, 127, 128, 299])
    x[0, 3] = np.nan
    x[5, 63] = np.inf
    x[127, 0] = -np.inf
    x[128, :] = np.nan
    x[299, 17] = np.inf
    loc, g, dd, cnt = run_topk(x, c, ops.single_segment(n, DEV), all_cand(K), k)
    assert (loc[bad] == -1).all() and (g[bad] == -1).all() and np.isnan(dd[bad]).all()
    assert cnt["nonfinite_rows"] == len(bad)
    good = np.setdiff1d(np.arange(n), bad)
    assert (loc[good] == clean[0][good]).all() and (g[good] == clean[1][good]).all()
    assert (dd[good].view(np.int32) == clean[2][good].view(np.int32)).all()


# ------------------------------------------------------------------------------ 8. offsets past 2^31 elements
def test_row_offsets_past_2_31_elements():
    n, d, K, k = 4_194_560, 512, 32, 2
    gen = torch.Generator(device=DEV).manual_seed(8)
    x = torch.empty((n, d), dtype=torch.float32, device=DEV)
    step = 1 << 19
    for i in range(0, n, step):
        torch.randn((min(step, n - i), d), generator=gen, device=DEV, dtype=torch.float32, out=x[i:i + step])
    c = torch.randn((K, d), generator=gen, device=DEV, dtype=torch.float32)
    ws = ops.TopKWorkspace(n, k, DEV)
    loc, glob, dist = ops.assign_topk(x, ops.prepare_centers(c), ops.single_segment(n, DEV), all_cand(K), k, workspace=ws)
    rng = np.random.default_rng(9)
    pick = np.concatenate([rng.choice(1000, 512, replace=False), n - 1000 + rng.choice(1000, 512, replace=False)])
    pd = torch.from_numpy(pick).to(DEV)
    pos, gl, dd = oracle(x[pd].cpu().numpy(), c.cpu().numpy(), [np.arange(K)], np.zeros(len(pick), dtype=np.int64), k)
    assert (glob[pd].cpu().numpy() == gl).all() and (loc[pd].cpu().numpy() == pos).all()
    assert_dist(dist[pd].cpu().numpy(), dd)
    cnt = ws.counters()
    assert cnt["listed_rows"] + cnt["all_candidate_rows"] == n and cnt["nonfinite_rows"] == 0


# ------------------------------------------------------------------------------------ 9. graph, 10. determinism
def test_graph_replays_equal_eager():
    x = gpu(_enc_data()[0])
    enc = _make_encoder("hier", False)
    eager = enc.encode_topk(x, 2)
    eager = [t.clone() for t in (eager.ids, eager.local, eager.glob, eager.dist)]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            enc.encode_topk(x, 2, check=False)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = enc.encode_topk(x, 2)
    for _ in range(2):
        for t in (out.ids, out.local, out.glob, out.dist):
            t.zero_()
        g.replay()
        torch.cuda.synchronize()
        for got, want in zip((out.ids, out.local, out.glob, out.dist), eager):
            assert torch.equal(bits(got), bits(want))
    enc.check_errors()
    assert all(int(w.item()) == 0 for w in enc.error_words())
    del g


def test_two_calls_give_identical_bytes():
    rng = np.random.default_rng(101)
    n, d, K, k, S = 700, 64, 300, 8, 4
    match = (rng.random((S, K)) < 0.5).astype(np.uint8)
    seg = rng.integers(0, S, n)
    x, c = gpu(rng.standard_normal((n, d)).astype(F32)), ops.prepare_centers(gpu(rng.standard_normal((K, d)).astype(F32)))
    cand = ops.match_to_candidates(gpu(match))
    b = ops.bucket(gpu(seg.astype(np.int32)), S)
    a = [t.clone() for t in ops.assign_topk(x, c, b, cand, k)]
    w = ops.assign_topk(x, c, b, cand, k)
    for p, q in zip(a, w):
        assert torch.equal(bits(p), bits(q))


# ------------------------------------------------------------------------------------------ 11. margin report
def _small_model(group=None):
    _, c0, c1, c2, match = _enc_data()
    cfg = HierarchicalRQKMeansConfig(layer_clusters=[4, 16, ENC_CAND], need_clusters=NEED, embedding_dim=ENC_D)
    m = HierarchicalRQKMeans(cfg, device=DEV, group=group)
    m.cluster_centers_list = [torch.from_numpy(c) for c in (c0, c1, c2)]
    m.match_matrices = [match]
    m.is_trained = True
    return m


LEVEL_KEYS = {"level", "rows_ranked", "mean_margin", "mean_silhouette", "min_margin", "share_below"}


def _same_margins(rep, ref, rows):
    """Counts and minima equal; the means come from fp64 totals another sharding adds in another order."""
    assert set(rep) == set(ref) == {"rows", "thresholds", "levels"}
    assert rep["rows"] == ref["rows"] == rows and rep["thresholds"] == ref["thresholds"]
    for lv, lr in zip(rep["levels"], ref["levels"]):
        assert set(lv) == set(lr) == LEVEL_KEYS
        for key in ("level", "rows_ranked", "min_margin", "share_below"):
            assert lv[key] == lr[key], key
        for key in ("mean_margin", "mean_silhouette"):
            np.testing.assert_allclose(lv[key], lr[key], rtol=rows * 2.0 ** -52)


def test_margin_report_against_numpy():
    x = _enc_data()[0]
    enc = _make_encoder("hier", False)
    th = (1e-3, 1e-2, 1e-1, 0.5)
    rep = margin_report(enc, gpu(x), thresholds=th)
    d = enc.encode_topk(gpu(x), 2).dist.cpu().numpy().astype(np.float64)
    assert rep["rows"] == len(x) and rep["thresholds"] == list(th) and len(rep["levels"]) == 3
    for l, lv in enumerate(rep["levels"]):
        assert set(lv) == LEVEL_KEYS and lv["level"] == l + 1
        d1, d2 = d[:, l, 0], d[:, l, 1]
        ok = np.isfinite(d1) & np.isfinite(d2)
        assert lv["rows_ranked"] == int(ok.sum()) == len(x)
        sil = np.where(d2[ok] > 0, (d2[ok] - d1[ok]) / np.where(d2[ok] > 0, d2[ok], 1.0), 0.0)
        np.testing.assert_allclose(lv["mean_margin"], (d2[ok] - d1[ok]).mean(), rtol=len(x) * 2.0 ** -52)
        np.testing.assert_allclose(lv["mean_silhouette"], sil.mean(), rtol=len(x) * 2.0 ** -52)
        assert lv["min_margin"] == float((d2[ok] - d1[ok]).min())
        assert lv["share_below"] == {f"{t:g}": float((sil < t).sum()) / ok.sum() for t in th}
        assert 0 < lv["mean_silhouette"] < 1 and lv["min_margin"] >= 0
    m = _small_model()
    _same_margins(m.assignment_margins(x), margin_report(enc, gpu(x)), len(x))
    ids, alt, dist = m.predict_topk(x, 3)
    assert ids.dtype == np.int64 and alt.dtype == np.int64 and dist.dtype == F32
    assert alt.shape == dist.shape == (len(x), 3, 3)
    assert (ids == m.predict(x, reference_quirks=False)).all() and (alt[:, :, 0] == ids).all()


def test_margin_report_with_unranked_rows():
    """A one-candidate group has no runner-up: its rows leave rows_ranked, and the means are over the rest."""
    x, c0, c1, c2, match = _enc_data()
    match = match.copy()
    match[0] = 0
    match[0, 3] = 1
    enc = RQEncoder([torch.from_numpy(c) for c in (c0, c1, c2)], NEED, match=torch.from_numpy(match),
                    semantics=HIERARCHICAL_TRAIN, device=DEV)
    tk = enc.encode_topk(gpu(x), 2)
    ids = tk.ids.cpu().numpy()
    lone = (ids[:, 0] == 0) & (ids[:, 1] == 0)
    assert lone.any()
    d = tk.dist.cpu().numpy()
    assert np.isposinf(d[lone, 2, 1]).all() and (tk.local.cpu().numpy()[lone, 2, 1] == -1).all()
    rep = margin_report(enc, gpu(x))
    assert rep["levels"][2]["rows_ranked"] == int((~lone).sum())
    assert rep["levels"][0]["rows_ranked"] == len(x)


def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _margin_worker(rank, world, port, out):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        m = _small_model(group=dist.group.WORLD)
        x = _enc_data()[0]
        out.put((rank, m.assignment_margins(x), m.predict_topk(x, 2), None))
    except Exception:  # report instead of leaving the parent waiting
        import traceback
        out.put((rank, None, None, traceback.format_exc()))
    dist.destroy_process_group()


def test_two_ranks_return_the_single_process_margins():
    import torch.multiprocessing as mp
    x = _enc_data()[0]
    m = _small_model()
    ref, ref_topk = m.assignment_margins(x), m.predict_topk(x, 2)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _port()
    procs = [ctx.Process(target=_margin_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=240) for _ in range(2)], key=lambda r: r[0])
    for p in procs:
        p.join(60)
    for rank, rep, topk, tb in res:
        assert rep is not None, tb
        _same_margins(rep, ref, len(x))
        for got, want in zip(topk, ref_topk):  # per-row results do not depend on the sharding
            assert got.dtype == want.dtype and got.shape == want.shape
            assert (got.view(np.int32 if got.dtype == F32 else np.int64) ==
                    want.view(np.int32 if want.dtype == F32 else np.int64)).all()


# --------------------------------------------------------------------------------------------------- 12. trainer
TRAIN_CFG = dict(layer_clusters=[4, 8, 8], need_clusters=[4, 4, 4], embedding_dim=64, iter_limit=3)


def _trainer_cfg(root, csv_path):
    return types.SimpleNamespace(
        output_dir=os.path.join(root, "outputs"), model_dir=os.path.join(root, "models"),
        h_rqkmeans_test=HierarchicalRQKMeansConfig(**TRAIN_CFG), h_rqkmeans=None,
        data=types.SimpleNamespace(song_vectors_file=csv_path,
                                   semantic_ids_file=os.path.join(root, "outputs", "semantic_id",
                                                                  "song_semantic_ids.jsonl")))


def test_trainer_writes_the_margins_only_when_asked(tmp_path):
    from generative_ranking_recommender_amd.train_semantic_ids import SemanticIDTrainer
    x = synth.small_mixture(600, d=64, m=16, seed=5)
    csv_path = str(tmp_path / "vec.csv")
    rq_io.write_song_vectors(csv_path, [f"song{i}" for i in range(len(x))], x)
    out = {}
    for name, kw in (("plain", {}), ("margins", {"report_margins": True})):
        np.random.seed(7)
        torch.manual_seed(7)
        root = str(tmp_path / name)
        out[name] = (root, SemanticIDTrainer(_trainer_cfg(root, csv_path), use_test_config=True, device=DEV,
                                             **kw).train(resume=False))
    files = {n: sorted(os.listdir(os.path.join(r, "outputs", "semantic_id"))) for n, (r, _) in out.items()}
    assert files["plain"] == sorted(["checkpoints", "song_semantic_ids.jsonl", "training_config.json",
                                     "training_statistics.json"])
    assert files["margins"] == sorted(files["plain"] + ["assignment_margin_report.json"])
    assert "assignment_margin_report" not in out["plain"][1]
    for rel in ("training_statistics.json", "training_config.json", "song_semantic_ids.jsonl"):
        a, b = (open(os.path.join(r, "outputs", "semantic_id", rel), "rb").read() for r, _ in out.values())
        assert a == b, rel
    with open(os.path.join(out["margins"][0], "outputs", "semantic_id", "assignment_margin_report.json")) as f:
        written = json.load(f)
    assert written == out["margins"][1]["assignment_margin_report"]
    assert written["rows"] == len(x) and len(written["levels"]) == 3
    again = out["margins"][1]["model"].assignment_margins(rq_io.load_song_vectors(csv_path, 64)[1])
    _same_margins(again, written, len(x))
