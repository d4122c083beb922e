"""rqsid_beam_expand / rqsid_beam_merge / RQEncoder.encode_beam / predict_beam on the GPU.

Oracles are numpy.  The expand is checked like rqsid_assign_topk: per item the fp64 ``((v - c)^2).sum()`` of every
allowed centre on the item's residual row (built with ops.residual), stable-sorted, adjacent gaps above 1e-12
relative, distances within 1 fp32 ulp.  The merge is checked bit for bit against a float32 restatement.  The
end-to-end score of a path is the fp32 chain of the kernels restated in numpy float32 (elementwise IEEE operations
are the same in both; only the fp64 summation order of a distance or a divisor differs, ~ dim 2^-53 relative, which
can flip at most one fp32 rounding).
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
from generative_ranking_recommender_amd.encode import (HIERARCHICAL_PREDICT_REFERENCE, HIERARCHICAL_TRAIN, SIMPLIFIED,
                                                       LevelSemantics, RQEncoder)
from generative_ranking_recommender_amd.hierarchical_rq_kmeans import HierarchicalRQKMeans, HierarchicalRQKMeansConfig

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
F32 = np.float32
INF = float("inf")
SEM = {"hier": HIERARCHICAL_TRAIN, "simplified": SIMPLIFIED}


def gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bytes(a, b):
    return torch.equal(bits(a), bits(b))


# ------------------------------------------------------------------------------------------------ data
NEED = [4, 4, 8]
ENC_D, ENC_ROWS, ENC_CAND = 64, 600, 40


@functools.lru_cache(maxsize=None)
def enc_data(need=tuple(NEED), rows=ENC_ROWS, seed=51):
    """test_gpu_topk's encoder data: mixture rows, c0 near four of them, unit-norm c1 / c2, need[2] allowed columns
    per group."""
    rng = np.random.default_rng(seed)
    x = synth.small_mixture(rows, d=ENC_D, m=16, seed=seed + 1)
    c0 = (x[rng.choice(rows, need[0], replace=False)] + 0.05 * rng.standard_normal((need[0], ENC_D))).astype(F32)

    def unit(m):
        v = rng.standard_normal((m, ENC_D)).astype(F32)
        return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F32)
    c1, c2 = unit(need[0] * need[1]), unit(ENC_CAND)
    # group = id0 * mult + id1 with mult = need[0] (hierarchical) or need[1] (simplified): rows for either
    match = np.zeros((need[0] * max(need[0], need[1]), ENC_CAND), dtype=np.uint8)
    for gi in range(len(match)):
        match[gi, rng.choice(ENC_CAND, need[2], replace=False)] = 1
    return x, c0, c1, c2, match


def make_encoder(sem_name, need=tuple(NEED), match=None, **kw):
    _, c0, c1, c2, m = enc_data(need, **kw)
    enc = RQEncoder([torch.from_numpy(c) for c in (c0, c1, c2)], list(need),
                    match=torch.from_numpy(m if match is None else match), semantics=SEM[sem_name], device=DEV)
    assert enc.fused
    return enc


# ------------------------------------------------------------------------------- numpy: the chain and the scores
def np_den(u):
    """fl32(sqrt(fp64 sum u_i^2)) + 1e-8f"""
    return (np.sqrt((u.astype(np.float64) ** 2).sum(-1)).astype(F32) + F32(1e-8)).astype(F32)


def np_dist(v, c):
    return np.sqrt(((v.astype(np.float64) - c.astype(np.float64)) ** 2).sum(-1))


def path_scores(x, c0, c1, c2, match, need, mult, norm):
    """Every allowed path of every row with its score of §3.1h: a list over rows of (paths int [P, 3] holding
    (id0, id1, column), rec float32 [P]) -- the brute force."""
    cols = [np.nonzero(r)[0] for r in match]
    out = []
    one = np.ones(len(x), dtype=F32)
    per_path = {}
    for g0 in range(need[0]):
        u = (x - c0[g0]).astype(F32)
        den1 = np_den(u) if norm else one
        v1 = (u / den1[:, None]).astype(F32) if norm else u
        s1 = (one * den1).astype(F32)
        for j1 in range(need[1]):
            w = (v1 - c1[g0 * need[1] + j1]).astype(F32)
            den2 = np_den(w) if norm else one
            v2 = (w / den2[:, None]).astype(F32) if norm else w
            s2 = (s1 * den2).astype(F32)
            for col in cols[g0 * mult + j1]:
                d = np_dist(v2, c2[col]).astype(F32)
                per_path[(g0, j1, int(col))] = (s2 * d).astype(F32)
    keys = sorted(per_path)
    rec = np.stack([per_path[k] for k in keys], 1)
    return np.array(keys, dtype=np.int64), rec


def last_id(match, mult, g0, j1, col, remap):
    """The last level's id of a column: its rank among the group's allowed columns, or the column itself."""
    return int(np.nonzero(np.nonzero(match[g0 * mult + j1])[0] == col)[0][0]) if remap else int(col)


# ------------------------------------------------------------------------------------ numpy: the expand's oracle
def oracle(v, c, lists, seg, k):
    """test_gpu_topk's oracle: (pos, glob, d) [n, k]; -1 / -1 / inf past the list.  Asserts the adjacent gaps."""
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
        diff = v[rows].astype(np.float64)[:, None, :] - c64[idx][None]
        d2 = (diff ** 2).sum(-1)
        order = np.argsort(d2, axis=1, kind="stable")
        srt = np.take_along_axis(d2, order[:, :k + 1], 1)
        if srt.shape[1] > 1:
            assert (np.diff(srt, axis=1) > 1e-12 * srt[:, 1:]).all(), "oracle places closer than 1e-12 relative"
        m = min(k, len(idx))
        pos[rows, :m] = order[:, :m]
        glob[rows, :m] = idx[order[:, :m]]
        dist[rows, :m] = np.sqrt(np.take_along_axis(d2, order[:, :m], 1))
    return pos, glob, dist


def assert_dist(got, want64):
    got = np.asarray(got)
    want = want64.astype(F32)
    fin = np.isfinite(want64)
    assert (np.isinf(got[~fin]) & (got[~fin] > 0)).all()
    ulp = np.spacing(np.abs(want[fin]))
    assert (np.abs(got[fin].astype(np.float64) - want[fin].astype(np.float64)) <= ulp).all()


# ------------------------------------------------------------------------------------------ 1. expand, beam = 1
@pytest.mark.parametrize("sem_name", ["hier", "simplified"])
def test_expand_with_beam_1_is_assign_topk(sem_name):
    x = gpu(enc_data()[0])
    n = len(x)
    enc = make_encoder(sem_name)
    norm = enc.sem.normalize_residual
    ids = enc.encode(x).t().contiguous()
    k = 3
    seg_ca, seg_cb = enc._last_segment_rows(DEV)
    den1 = torch.empty(n, dtype=torch.float32, device=DEV) if norm else None
    levels = [
        (ops.single_segment(n, DEV), None),
        (ops.bucket(ids[0], NEED[0]), ops.FusedResidual(1, norm, enc.pcs[0].centers, None, den_out=den1)),
        (ops.bucket(ids[0] * NEED[0] + ids[1], enc.n_groups),
         ops.FusedResidual(2, norm, enc.pcs[0].centers, seg_ca, enc.pcs[1].centers, seg_cb, den_in=den1)),
    ]
    tws, xws = ops.TopKWorkspace(n, k, DEV), ops.BeamWorkspace(n, k, DEV)
    for l, (b, fr) in enumerate(levels):
        want = ops.assign_topk(x, enc.pcs[l], b, enc.raw_cands[l], k, fused=fr, workspace=tws)
        want_den = None if fr is None or fr.den_out is None else fr.den_out.clone()
        if want_den is not None:
            fr.den_out.fill_(-1.0)
        got = ops.beam_expand(x, 1, enc.pcs[l], b, enc.raw_cands[l], k, fused=fr, workspace=xws)
        for g, w in zip(got, want):
            assert same_bytes(g, w), l
        if want_den is not None:
            assert same_bytes(fr.den_out, want_den)
        assert xws.counters() == tws.counters()
    assert int(xws.error_word().item()) == 0


# -------------------------------------------------------------------------------- 2. expand against the oracle
B3 = 3


@functools.lru_cache(maxsize=None)
def hypotheses():
    """Hand-made beams of three for every row: (p0, p1) [n, 3], -1 = dead.  Hypotheses 0 and 1 share their level-0
    parent on half the rows (and the whole path on some), hypothesis 2 is dead on a third of the rows."""
    rng = np.random.default_rng(77)
    n = ENC_ROWS
    p0 = rng.integers(0, NEED[0], (n, B3))
    p1 = rng.integers(0, NEED[1], (n, B3))
    same = rng.random(n) < 0.5
    p0[same, 1] = p0[same, 0]
    twin = rng.random(n) < 0.1
    p0[twin, 1], p1[twin, 1] = p0[twin, 0], p1[twin, 0]
    dead = rng.random((n, B3)) < np.array([0.02, 0.05, 0.33])
    p0[dead], p1[dead] = -1, -1
    return p0.reshape(-1), p1.reshape(-1)


@functools.lru_cache(maxsize=None)
def expand_case(sem_name):
    """Both residual levels of the hand-made beams: the item residual rows (ops.residual on replicated rows), the
    level-1 divisors (ops.assign's fused den_out) and what rqsid_beam_expand returned."""
    x, c0, c1, c2, match = enc_data()
    match = match.copy()
    match[5] = 0  # a penalty group, with hypotheses in it
    enc = make_encoder(sem_name, match=match)
    assert enc.has_penalty
    norm = enc.sem.normalize_residual
    p0, p1 = hypotheses()
    live = p0 >= 0
    xd = gpu(x)
    xrep = xd.repeat_interleave(B3, 0).contiguous()
    q0 = gpu(np.where(live, p0, 0).astype(np.int32))  # the dead items' segment subtracts row 0
    items = len(p0)
    cands = [ops.with_dead_segment(c) for c in enc.raw_cands]
    zero = torch.zeros(1, dtype=torch.int32, device=DEV)
    xws = ops.BeamWorkspace(items, B3, DEV)
    # level 1
    key1 = gpu(np.where(live, p0, NEED[0]).astype(np.int32))
    den1 = torch.full((items,), -1.0, dtype=torch.float32, device=DEV) if norm else None
    seg1 = torch.cat([torch.arange(NEED[0], dtype=torch.int32, device=DEV), zero])
    got1 = ops.beam_expand(xd, B3, enc.pcs[1], ops.bucket(key1, NEED[0] + 1), cands[1], B3,
                           fused=ops.FusedResidual(1, norm, enc.pcs[0].centers, seg1, den_out=den1), workspace=xws)
    got1 = [t.cpu().numpy() for t in got1]
    cnt1 = xws.counters()
    ref_den1 = torch.empty(items, dtype=torch.float32, device=DEV) if norm else None
    ops.assign(xrep, enc.pcs[1], ops.bucket(q0, NEED[0]), enc.cands[1],
               fused=ops.FusedResidual(1, norm, enc.pcs[0].centers, None, den_out=ref_den1))
    v1 = ops.residual(xrep, gpu(c0), q0, normalize=norm)
    # level 2
    g1 = gpu(np.where(live, p0 * NEED[1] + p1, 0).astype(np.int32))
    key2 = gpu(np.where(live, p0 * NEED[0] + p1, enc.n_groups).astype(np.int32))
    seg_ca, seg_cb = (torch.cat([t, zero]) for t in enc._last_segment_rows(DEV))
    den2 = torch.full((items,), -1.0, dtype=torch.float32, device=DEV) if norm else None
    got2 = ops.beam_expand(xd, B3, enc.pcs[2], ops.bucket(key2, enc.n_groups + 1), cands[2], B3,
                           fused=ops.FusedResidual(2, norm, enc.pcs[0].centers, seg_ca, enc.pcs[1].centers, seg_cb,
                                                   den_in=ref_den1, den_out=den2), workspace=xws)
    got2 = [t.cpu().numpy() for t in got2]
    cnt2 = xws.counters()
    v2 = ops.residual(v1, gpu(c1), g1, normalize=norm)
    w2 = ops.residual(v1, gpu(c1), g1, normalize=False)
    assert int(xws.error_word().item()) == 0
    return dict(match=match, live=live, p0=p0, p1=p1, got1=got1, got2=got2, cnt1=cnt1, cnt2=cnt2,
                den1=None if den1 is None else den1.cpu().numpy(),
                ref_den1=None if ref_den1 is None else ref_den1.cpu().numpy(),
                den2=None if den2 is None else den2.cpu().numpy(),
                v1=v1.cpu().numpy(), v2=v2.cpu().numpy(), w2=w2.cpu().numpy())


@pytest.mark.parametrize("sem_name", ["hier", "simplified"])
def test_expand_level_1_against_the_oracle(sem_name):
    _, c0, c1, c2, _ = enc_data()
    e = expand_case(sem_name)
    live, p0 = e["live"], e["p0"]
    per_parent = np.bincount(p0[live], minlength=NEED[0])
    assert (per_parent > 256).all() and (per_parent % 128 != 0).all()  # several tiles and a ragged tail each
    lists = [np.arange(p * NEED[1], (p + 1) * NEED[1]) for p in range(NEED[0])] + [[]]
    pos, glob, dist = oracle(e["v1"], c1, lists, np.where(live, p0, NEED[0]), B3)
    loc, g, dd = e["got1"]
    assert (loc == pos).all() and (g == glob).all()
    assert_dist(dd, dist)
    assert (loc[~live] == -1).all() and np.isposinf(dd[~live]).all() and (~live).sum() > 100
    assert e["cnt1"]["nonfinite_rows"] == 0
    if e["den1"] is not None:
        assert (e["den1"].view(np.int32) == e["ref_den1"].view(np.int32)).all()


@pytest.mark.parametrize("sem_name", ["hier", "simplified"])
def test_expand_level_2_against_the_oracle(sem_name):
    _, c0, c1, c2, _ = enc_data()
    e = expand_case(sem_name)
    live, p0, p1, match = e["live"], e["p0"], e["p1"], e["match"]
    n_groups = len(match)
    grp = np.where(live, p0 * NEED[0] + p1, n_groups)
    lists = [np.nonzero(r)[0] for r in match] + [[]]
    pos, glob, dist = oracle(e["v2"], c2, lists, grp, B3)
    loc, g, dd = e["got2"]
    assert (loc == pos).all() and (g == glob).all()
    assert_dist(dd, dist)
    pen = grp == 5
    assert pen.sum() > 20 and (loc[pen] == -1).all() and (g[pen] == -1).all() and np.isposinf(dd[pen]).all()
    # two hypotheses of one row under the same parent give the same expansions
    same = np.nonzero((p0.reshape(-1, B3)[:, 0] == p0.reshape(-1, B3)[:, 1]) &
                      (p1.reshape(-1, B3)[:, 0] == p1.reshape(-1, B3)[:, 1]) & live.reshape(-1, B3)[:, 0])[0]
    assert len(same) > 10
    assert (g[same * B3] == g[same * B3 + 1]).all()
    assert (dd[same * B3].view(np.int32) == dd[same * B3 + 1].view(np.int32)).all()
    if e["den2"] is not None:  # (the items of a penalty segment get no divisor)
        ok = live & ~pen
        assert (e["den2"][ok].view(np.int32) == np_den(e["w2"])[ok].view(np.int32)).all()
        assert (e["den2"][pen] == -1.0).all()


# ------------------------------------------------------------------------------- 3. merge against numpy, bit for bit
def np_merge(n, bi, k, bo, level, el, eg, ed, scale, den, pin, use_global, key_mult, dead_key):
    """§3.1h restated in numpy float32."""
    pl = level + 1
    path = np.full((n * bo, pl), -1, dtype=np.int32)
    so = np.ones(n * bo, dtype=F32)
    dn = np.ones(n * bo, dtype=F32)
    rec_o = np.full(n * bo, INF, dtype=F32)
    key = np.full(n * bo, dead_key, dtype=np.int32)
    src = np.full(n * bo, -1, dtype=np.int32)
    el, eg, ed = el.reshape(n, bi, k), eg.reshape(n, bi, k), ed.reshape(n, bi, k)
    sc = np.ones((n, bi), dtype=F32) if scale is None else scale.reshape(n, bi)
    dd = np.ones((n, bi), dtype=F32) if den is None else den.reshape(n, bi)
    with np.errstate(all="ignore"):
        S = (sc * dd).astype(F32)
        ids = eg if use_global else el
        rec = np.where((eg >= 0) & (ids >= 0), (S[:, :, None] * ed).astype(F32), F32(INF)).astype(F32)
    for r in range(n):
        if np.isnan(ed[r]).any() or np.isnan(sc[r]).any():
            rec_o[r * bo:(r + 1) * bo] = np.nan
            so[r * bo:(r + 1) * bo] = np.nan
            continue
        hh, pp = np.meshgrid(np.arange(bi), np.arange(k), indexing="ij")
        flat_rec, hh, pp = rec[r].reshape(-1), hh.reshape(-1), pp.reshape(-1)
        others = np.nonzero(np.isfinite(flat_rec) & (np.arange(bi * k) != 0))[0]
        order = others[np.lexsort((pp[others], hh[others], flat_rec[others]))]
        chosen = {0: 0} if np.isfinite(flat_rec[0]) else {}
        for t, e in enumerate(order[:bo - 1]):
            chosen[t + 1] = e
        for t, e in chosen.items():
            o, h = r * bo + t, hh[e]
            item = r * bi + h
            if level:
                path[o, :level] = pin[item]
            path[o, level] = ids[r, h, pp[e]]
            so[o], dn[o], rec_o[o] = S[r, h], dd[r, h], flat_rec[e]
            key[o] = (pin[item, level - 1] * key_mult if level else 0) + ids[r, h, pp[e]]
            src[o] = e
    return path, so, dn, rec_o, key, src


@pytest.mark.parametrize("bi, k, bo, level, use_global, with_scale", [
    (1, 8, 8, 0, True, False),
    (1, 3, 2, 0, True, True),
    (3, 3, 3, 1, False, True),
    (8, 8, 8, 2, False, True),
    (2, 4, 5, 1, True, True),
    (4, 4, 4, 2, False, False),
])
def test_merge_equals_numpy_bit_for_bit(bi, k, bo, level, use_global, with_scale):
    rng = np.random.default_rng(300 + 10 * bi + k)
    n = 301  # no multiple of the rows per block
    items = n * bi
    ed = rng.choice(np.linspace(0.25, 4.0, 16).astype(F32), (items, k))  # few values: exact rec ties
    ed = np.where(rng.random((items, k)) < 0.5, rng.random((items, k)).astype(F32) + F32(0.1), ed).astype(F32)
    eg = rng.integers(0, 50, (items, k)).astype(np.int32)
    el = rng.integers(0, 8, (items, k)).astype(np.int32)
    short = rng.random((items, k)) < 0.2   # places past the list
    eg[short], el[short], ed[short] = -1, -1, INF
    el[rng.random((items, k)) < 0.03] = -1  # a place without a local id (ranked out unless the id is the global)
    dead_items = rng.random(items) < 0.1
    eg[dead_items], el[dead_items], ed[dead_items] = -1, -1, INF
    ed.reshape(n, bi, k)[5, 0, 0] = INF   # slot 0 dead, others live
    eg.reshape(n, bi, k)[5, 0, 0] = -1
    ed.reshape(n, bi, k)[7] = INF         # a row without a live expansion
    eg.reshape(n, bi, k)[7] = -1
    nan_rows = [11, 12, 300]
    ed.reshape(n, bi, k)[11, bi - 1, k - 1] = np.nan
    ed.reshape(n, bi, k)[12] = np.nan
    ed.reshape(n, bi, k)[300, 0, 0] = np.nan
    scale = den = None
    if with_scale:
        scale = (rng.random(items).astype(F32) + F32(0.5)).astype(F32)
        den = (rng.random(items).astype(F32) * F32(3) + F32(1e-3)).astype(F32)
        scale[rng.random(items) < 0.3] = 1.0
        den[rng.random(items) < 0.3] = 2.0
        scale.reshape(n, bi)[20, 0] = np.nan  # a non-finite row passed on by the level before
        nan_rows.append(20)
    pin = rng.integers(0, 4, (items, max(level, 1))).astype(np.int32)
    want = np_merge(n, bi, k, bo, level, el, eg, ed, scale, den, pin, use_global, 4, 99)
    out = ops.beam_merge(n, bi, k, bo, level, gpu(el), gpu(eg), gpu(ed), None if scale is None else gpu(scale),
                         None if den is None else gpu(den), gpu(pin) if level else None, use_global=use_global,
                         key_mult=4, dead_key=99)
    got = [t.cpu().numpy() for t in (out.path, out.scale, out.den_next, out.rec, out.key, out.src)]
    for name, g, w in zip(("path", "scale", "den_next", "rec", "key", "src"), got, want):
        if g.dtype == F32:  # NaN payloads aside, the same bits
            assert (np.isnan(g) == np.isnan(w)).all(), name
            assert (np.where(np.isnan(g), 0, g).view(np.int32) == np.where(np.isnan(w), 0, w).view(np.int32)).all(), name
        else:
            assert (g == w).all(), name
    path, rec, src = got[0].reshape(n, bo, level + 1), got[3].reshape(n, bo), got[5].reshape(n, bo)
    assert np.isnan(rec[nan_rows]).all() and (path[nan_rows] == -1).all()
    assert np.isposinf(rec[7]).all() and (src[7] == -1).all()
    assert np.isposinf(rec[5, 0]) and (bo == 1 or np.isfinite(rec[5, 1]))
    live0 = np.isfinite(rec[:, 0])
    assert (src[live0, 0] == 0).all()  # slot 0 is the greedy continuation
    tail = np.where(np.isfinite(rec[:, 1:]), rec[:, 1:], np.inf)
    assert (tail[:, 1:] >= tail[:, :-1]).all()  # ascending, dead slots last
    again = ops.beam_merge(n, bi, k, bo, level, gpu(el), gpu(eg), gpu(ed), None if scale is None else gpu(scale),
                           None if den is None else gpu(den), gpu(pin) if level else None, use_global=use_global,
                           key_mult=4, dead_key=99)
    for a, b in zip((out.path, out.scale, out.den_next, out.rec, out.key, out.src),
                    (again.path, again.scale, again.den_next, again.rec, again.key, again.src)):
        assert same_bytes(a, b)


# ------------------------------------------------------------------------------------- 4. end-to-end optimality
# need[0] * need[1] <= 8 and <= 8 allowed columns per group: with B = 8 no path is ever pruned.  The hierarchical
# semantics fuse only when need[0] >= need[1] (the group id need[0] * id0 + id1 must determine (id0, id1)), so they
# take [4, 2, 8] where the simplified ones take [2, 4, 8].
OPT_NEED = {"hier": (4, 2, 8), "simplified": (2, 4, 8)}


def brute_force(sem_name):
    need = OPT_NEED[sem_name]
    x, c0, c1, c2, match = enc_data(need, seed=61)
    mult = need[0] if sem_name == "hier" else need[1]
    keys, rec = path_scores(x, c0, c1, c2, match, need, mult, SEM[sem_name].normalize_residual)
    order = np.argsort(rec, axis=1, kind="stable")
    best, second = (np.take_along_axis(rec, order[:, i:i + 1], 1)[:, 0] for i in (0, 1))
    clear = (second.astype(np.float64) - best) > 4 * np.spacing(best)
    ids = keys[order[:, 0]].copy()
    remap = SEM[sem_name].remap_last
    ids[:, 2] = [last_id(match, mult, g0, j1, col, remap) for g0, j1, col in ids]
    return ids, best, clear


@pytest.mark.parametrize("sem_name", ["hier", "simplified"])
def test_wide_beam_finds_the_best_path(sem_name):
    need = OPT_NEED[sem_name]
    ids, best, clear = brute_force(sem_name)
    assert (~clear).mean() <= 0.01  # rows whose two best paths are within 4 fp32 ulps are left out
    enc = make_encoder(sem_name, need, seed=61)
    bm = enc.encode_beam(gpu(enc_data(need, seed=61)[0]), 8)
    got = bm.ids.cpu().numpy()
    assert (got[clear] == ids[clear]).all()
    rec = bm.recon_err.cpu().numpy()
    assert (np.abs(rec[clear].astype(np.float64) - best[clear]) <= 4 * np.spacing(best[clear])).all()
    assert all(int(w.item()) == 0 for w in enc.error_words())


# ---------------------------------------------------------------------------------------------- 5. invariants
@functools.lru_cache(maxsize=None)
def beams(sem_name, B):
    enc = make_encoder(sem_name)
    bm = enc.encode_beam(gpu(enc_data()[0]), B)
    assert all(int(w.item()) == 0 for w in enc.error_words())
    return bm


@functools.lru_cache(maxsize=None)
def greedy(sem_name):
    return make_encoder(sem_name).encode(gpu(enc_data()[0])).contiguous()


@pytest.mark.parametrize("B", [1, 2, 4])
@pytest.mark.parametrize("sem_name", ["hier", "simplified"])
def test_beam_invariants(sem_name, B):
    bm = beams(sem_name, B)
    n = ENC_ROWS
    assert bm.ids.shape == (n, 3) and bm.paths.shape == (n, B, 3) and bm.path_err.shape == (n, B)
    assert bm.ids.dtype == bm.paths.dtype == bm.slot.dtype == torch.int32
    assert bm.recon_err.dtype == bm.path_err.dtype == torch.float32
    assert torch.equal(bm.paths[:, 0], greedy(sem_name))
    if B == 1:
        assert torch.equal(bm.ids, greedy(sem_name))
    perr = bm.path_err.cpu().numpy()
    rec, slot = bm.recon_err.cpu().numpy(), bm.slot.cpu().numpy()
    assert np.isfinite(perr[:, 0]).all() and (rec <= perr[:, 0]).all()
    assert (slot == np.argmin(perr, 1)).all()  # (numpy's argmin takes the first of equal minima)
    assert (rec == perr[np.arange(n), slot]).all()
    assert torch.equal(bm.ids, bm.paths[torch.arange(n, device=DEV), bm.slot.long()])
    if B == 4:
        assert (rec < perr[:, 0]).sum() >= 1


# ----------------------------------------------------------------------------------- 6. agreement with quant_error
@pytest.mark.parametrize("sem_name", ["hier", "simplified"])
def test_recon_err_agrees_with_quant_error(sem_name):
    """1 ulp between dist and err, plus <= 0.5 ulp for each of the four fp32 products on the two sides: 4 ulps."""
    bm = beams(sem_name, 4)
    qe = make_encoder(sem_name).quant_error(gpu(enc_data()[0]), ids=bm.ids)
    assert torch.equal(qe.ids, bm.ids)
    want = qe.recon_err.cpu().numpy()
    got = bm.recon_err.cpu().numpy()
    assert (np.abs(got.astype(np.float64) - want) <= 4 * np.spacing(np.abs(want))).all()


# ------------------------------------------------------------------------------------ 7. row formats and capture
def _fields(bm):
    return (bm.ids, bm.recon_err, bm.paths, bm.path_err, bm.slot)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_16bit_rows_equal_their_fp32_widening(dtype):
    for sem_name in ("hier", "simplified"):
        enc = make_encoder(sem_name)
        x16 = gpu(enc_data()[0]).to(dtype)
        a = [t.clone() for t in _fields(enc.encode_beam(x16, 3))]
        assert enc.last_row_format == ("f16" if dtype == torch.float16 else "bf16")
        w = _fields(enc.encode_beam(x16.float(), 3))
        assert enc.last_row_format == "f32"
        for p, q in zip(a, w):
            assert same_bytes(p, q)


def test_chunks_do_not_change_the_result():
    enc = make_encoder("hier")
    x = gpu(enc_data()[0])
    whole = [t.clone() for t in _fields(enc.encode_beam(x, 4))]
    for p, q in zip(whole, _fields(enc.encode_beam(x, 4, chunk_rows=257))):
        assert same_bytes(p, q)


def test_graph_replays_equal_eager_and_two_calls_agree():
    x = gpu(enc_data()[0])
    enc = make_encoder("hier")
    eager = [t.clone() for t in _fields(enc.encode_beam(x, 4))]
    for p, q in zip(eager, _fields(enc.encode_beam(x, 4))):
        assert same_bytes(p, q)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            enc.encode_beam(x, 4, check=False)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = enc.encode_beam(x, 4, check=False)
    for _ in range(2):
        for t in _fields(out):
            t.zero_()
        g.replay()
        torch.cuda.synchronize()
        for got, want in zip(_fields(out), eager):
            assert same_bytes(got, want)
    enc.check_errors()
    assert all(int(w.item()) == 0 for w in enc.error_words())
    del g


def test_single_level_and_non_finite_rows():
    x, c0 = enc_data()[0].copy(), enc_data()[1]
    one = RQEncoder([torch.from_numpy(c0)], [4], device=DEV)
    bm = one.encode_beam(gpu(x), 3)
    assert torch.equal(bm.ids, one.encode(gpu(x))) and (bm.slot == 0).all()
    want = np.sort(np_dist(x[:, None, :], c0[None]), 1)[:, :3]
    assert_dist(bm.path_err.cpu().numpy(), want)
    bad = [0, 127, 128, 599]
    x[0, 3], x[127, 0], x[128, :], x[599, 63] = np.nan, np.inf, np.nan, -np.inf
    enc = make_encoder("hier")
    clean = beams("hier", 4)
    bm = enc.encode_beam(gpu(x), 4)
    assert (bm.ids[bad] == -1).all() and (bm.paths[bad] == -1).all()
    assert torch.isnan(bm.recon_err[bad]).all() and torch.isnan(bm.path_err[bad]).all()
    good = torch.from_numpy(np.setdiff1d(np.arange(len(x)), bad)).to(DEV)
    for p, q in zip(_fields(bm), _fields(clean)):
        assert same_bytes(p[good], q[good])
    assert all(int(w.item()) == 0 for w in enc.error_words())


# ------------------------------------------------------------------------------------------------- 8. refusals
def test_refusals():
    x, c0, c1, c2, match = enc_data()
    xd = gpu(x)
    enc = make_encoder("hier")
    for B in (0, 9):
        with pytest.raises(ValueError):
            enc.encode_beam(xd, B)
    enc.force_materialized = True
    assert not enc.fused
    with pytest.raises(ValueError, match="fused"):
        enc.encode_beam(xd, 2)
    cs = [torch.from_numpy(c) for c in (c0, c1, c2)]
    quirk = RQEncoder(cs, NEED, match=torch.from_numpy(match), semantics=LevelSemantics(residual_global_id=False),
                      device=DEV)
    with pytest.raises(ValueError, match="residual_global_id"):
        quirk.encode_beam(xd, 2)
    ref = RQEncoder(cs, NEED, match=torch.from_numpy(match), semantics=HIERARCHICAL_PREDICT_REFERENCE, device=DEV)
    with pytest.raises(ValueError):
        ref.encode_beam(xd, 2)
    two = RQEncoder(cs[:2], [4, 4], device=DEV)
    with pytest.raises(IndexError):
        two.encode_beam(xd, 2)
    with pytest.raises(IndexError):
        two.encode(xd)


def test_penalty_groups():
    x, c0, c1, c2, match = enc_data()
    xd = gpu(x)
    ids = greedy("hier").cpu().numpy()
    grp = ids[:, 0] * NEED[0] + ids[:, 1]
    g = int(np.bincount(grp).argmax())
    m1 = match.copy()
    m1[g] = 0
    enc = make_encoder("hier", match=m1)
    assert enc.has_penalty
    with pytest.raises(KeyError):
        enc.encode(xd)  # greedy cannot encode the rows of group g
    bm = enc.encode_beam(xd, 4)  # another slot is live
    hit = grp == g
    slot, perr, out = bm.slot.cpu().numpy(), bm.path_err.cpu().numpy(), bm.ids.cpu().numpy()
    assert hit.sum() > 10 and (slot[hit] > 0).all() and np.isposinf(perr[hit, 0]).all()
    assert (bm.paths[torch.from_numpy(hit).to(DEV), 0] == -1).all()
    assert (out >= 0).all() and np.isfinite(bm.recon_err.cpu().numpy()).all()
    assert ((out[hit, 0] * NEED[0] + out[hit, 1]) != g).all()
    with pytest.raises(KeyError):
        enc.encode_beam(xd, 1)  # one slot: nothing else to take
    with pytest.raises(KeyError):
        make_encoder("hier", match=np.zeros_like(match)).encode_beam(xd, 4)  # no group allows anything


# --------------------------------------------------------------------------------- 9. predict_beam and the trainer
def _small_model(group=None):
    _, c0, c1, c2, match = enc_data()
    cfg = HierarchicalRQKMeansConfig(layer_clusters=[4, 16, ENC_CAND], need_clusters=NEED, embedding_dim=ENC_D)
    m = HierarchicalRQKMeans(cfg, device=DEV, group=group)
    m.cluster_centers_list = [torch.from_numpy(c) for c in (c0, c1, c2)]
    m.match_matrices = [match]
    m.is_trained = True
    return m


def test_predict_beam():
    x = enc_data()[0]
    m = _small_model()
    ids, rec, greedy_rec = m.predict_beam(x, 4)
    assert ids.dtype == np.int64 and rec.dtype == F32 and greedy_rec.dtype == F32
    assert ids.shape == (len(x), 3) and rec.shape == greedy_rec.shape == (len(x),)
    assert (rec <= greedy_rec).all() and (rec < greedy_rec).any()
    same = rec == greedy_rec
    assert (ids[same] == m.predict(x, reference_quirks=False)[same]).all()
    bm = beams("hier", 4)
    assert (ids == bm.ids.cpu().numpy()).all() and (rec.view(np.int32) == bm.recon_err.cpu().numpy().view(np.int32)).all()
    rep = m.beam_report(x, 4)
    assert rep["rows"] == len(x) and rep["beam"] == 4
    assert rep["changed_share"] == float((bm.slot != 0).sum().item()) / len(x)
    np.testing.assert_allclose(rep["beam_mse"], (rec.astype(np.float64) ** 2).mean(), rtol=len(x) * 2.0 ** -52)


def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _beam_worker(rank, world, port, out):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        m = _small_model(group=dist.group.WORLD)
        x = enc_data()[0]
        out.put((rank, m.predict_beam(x, 4), m.beam_report(x, 4), None))
    except Exception:  # report instead of leaving the parent waiting
        import traceback
        out.put((rank, None, None, traceback.format_exc()))
    dist.destroy_process_group()


def test_two_ranks_return_the_single_process_arrays():
    import torch.multiprocessing as mp
    x = enc_data()[0]
    m = _small_model()
    ref, ref_rep = m.predict_beam(x, 4), m.beam_report(x, 4)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _port()
    procs = [ctx.Process(target=_beam_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=240) for _ in range(2)], key=lambda r: r[0])
    for p in procs:
        p.join(60)
    for rank, arrays, rep, tb in res:
        assert arrays is not None, tb
        for got, want in zip(arrays, ref):
            assert got.dtype == want.dtype and got.shape == want.shape
            assert (got.view(np.int32 if got.dtype == F32 else np.int64) ==
                    want.view(np.int32 if want.dtype == F32 else np.int64)).all()
        assert rep["rows"] == ref_rep["rows"] and rep["changed_share"] == ref_rep["changed_share"]
        for key in ("greedy_mse", "beam_mse"):
            np.testing.assert_allclose(rep[key], ref_rep[key], rtol=len(x) * 2.0 ** -52)


TRAIN_CFG = dict(layer_clusters=[4, 8, 8], need_clusters=[4, 4, 4], embedding_dim=64, iter_limit=3)


def _trainer_cfg(root, csv_path):
    return types.SimpleNamespace(
        output_dir=os.path.join(root, "outputs"), model_dir=os.path.join(root, "models"),
        h_rqkmeans_test=HierarchicalRQKMeansConfig(**TRAIN_CFG), h_rqkmeans=None,
        data=types.SimpleNamespace(song_vectors_file=csv_path,
                                   semantic_ids_file=os.path.join(root, "outputs", "semantic_id",
                                                                  "song_semantic_ids.jsonl")))


def test_trainer_writes_the_beam_report_only_when_asked(tmp_path):
    from generative_ranking_recommender_amd.train_semantic_ids import SemanticIDTrainer
    x = synth.small_mixture(600, d=64, m=16, seed=5)
    csv_path = str(tmp_path / "vec.csv")
    rq_io.write_song_vectors(csv_path, [f"song{i}" for i in range(len(x))], x)
    out = {}
    for name, kw in (("plain", {}), ("beam", {"report_beam": 4, "report_quantization": True})):
        np.random.seed(7)
        torch.manual_seed(7)
        root = str(tmp_path / name)
        out[name] = (root, SemanticIDTrainer(_trainer_cfg(root, csv_path), use_test_config=True, device=DEV,
                                             **kw).train(resume=False))
    files = {n: sorted(os.listdir(os.path.join(r, "outputs", "semantic_id"))) for n, (r, _) in out.items()}
    assert files["plain"] == sorted(["checkpoints", "song_semantic_ids.jsonl", "training_config.json",
                                     "training_statistics.json"])
    assert files["beam"] == sorted(files["plain"] + ["beam_report.json", "quantization_report.json"])
    assert "beam_report" not in out["plain"][1]
    for rel in ("training_statistics.json", "training_config.json", "song_semantic_ids.jsonl"):
        a, b = (open(os.path.join(r, "outputs", "semantic_id", rel), "rb").read() for r, _ in out.values())
        assert a == b, rel
    with open(os.path.join(out["beam"][0], "outputs", "semantic_id", "beam_report.json")) as f:
        written = json.load(f)
    assert written == out["beam"][1]["beam_report"]
    assert set(written) == {"rows", "beam", "changed_share", "greedy_mse", "beam_mse"}
    assert written["rows"] == len(x) and written["beam"] == 4 and 0 <= written["changed_share"] <= 1
    assert written["beam_mse"] <= written["greedy_mse"]
    # greedy's error is quantization_report's: fp64 sums in another order, and per row the 4 ulps of section 6
    qmse = out["beam"][1]["quantization_report"]["levels"][-1]["recon_mse"]
    assert abs(written["greedy_mse"] - qmse) <= qmse * (len(x) * 2.0 ** -52 + 2 * 4 * 2.0 ** -23)
