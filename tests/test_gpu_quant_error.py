"""rqsid_quant_error and what sits on it: RQEncoder.quant_error / decode, the models' quantization_error report and
the training driver's opt-in quantization_report.json.

Yardstick (host, from the oracle): cur_0 = x; d_l = fl32(cur_l - c_l[g_l]); e_ref_l = fl32(sqrt(sum (double)d_l^2));
cur_{l+1} = oracle.residual(cur_l, c_l, g_l, normalize).  Tolerances: a norm taken in fp64 and rounded once can
differ by one fp32 ulp between two summation orders; with normalised residuals an upstream divisor that differs by
one ulp moves each element of cur_l by at most 1.5 ulp, hence ulp32(e_ref) + 2^-22 ||cur_l|| from level 1 on.
"""
import functools
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
from oracle import rq_oracle as O

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
F32 = np.float32
NEED = {"small": [16, 16, 32], "prod": [128, 128, 256]}
ROWS = {"small": 3000, "prod": 20_000}
SEM = {"hier": HIERARCHICAL_TRAIN, "simplified": SIMPLIFIED}
LEVEL_KEYS = {"level", "mse", "rmse", "max", "recon_mse", "relative", "unique_clusters", "cluster_distribution"}


def gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def ulp32(v):
    return np.spacing(np.abs(np.asarray(v, F32))).astype(np.float64)


def norm32(a):
    return np.sqrt((a.astype(np.float64) ** 2).sum(1)).astype(F32)


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


def yardstick(x, cents, globs, normalize, group_dims=(), weights=None):
    """(e_ref [N, L] f32, ||cur_l|| [N, L] f64) of the chain above; weighted levels take their residual from the
    weighted rows (the training-consistent semantics)."""
    gd = list(group_dims) or [x.shape[1]]
    cur = x.astype(F32)
    e, cn = [], []
    for l, (c, g) in enumerate(zip(cents, globs)):
        w = cur if weights is None else O.apply_weights(cur, gd, weights[l])
        e.append(norm32((w - c.astype(F32)[g]).astype(F32)))
        cn.append(np.sqrt((w.astype(np.float64) ** 2).sum(1)))
        if l < len(cents) - 1:
            cur = O.residual(w, c, g, gd, normalize)
    return np.stack(e, 1), np.stack(cn, 1)


def assert_chain(err, e_ref, cur_norm, normalize):
    err = err.astype(np.float64)
    for l in range(e_ref.shape[1]):
        tol = ulp32(e_ref[:, l])
        if normalize and l >= 1:
            tol = tol + 2.0 ** -22 * cur_norm[:, l]
        bad = np.abs(err[:, l] - e_ref[:, l].astype(np.float64)) > tol
        assert not bad.any(), (l, int(bad.sum()), float(np.abs(err[:, l] - e_ref[:, l]).max()))


@functools.lru_cache(maxsize=None)
def _codebooks(shape):
    if shape == "small":
        return synth.encode_codebooks(seed=5, need=(16, 16, 32), n_cand=320, pool_rows=8192)
    return synth.encode_codebooks(seed=99)


@functools.lru_cache(maxsize=None)
def _encoder(shape, sem_name):
    cb = _codebooks(shape)
    return RQEncoder([torch.from_numpy(cb[k]) for k in ("c0", "c1", "c2")], NEED[shape],
                     match=torch.from_numpy(cb["match"]), semantics=SEM[sem_name], device=DEV)


@functools.lru_cache(maxsize=None)
def _rows(shape):
    return synth.mixture_rows(0, ROWS[shape])


def host_globals(ids, shape, sem_name):
    """Global codebook rows of semantic IDs, restated on the host from the level rules (encode.py's docstring)."""
    cb, need = _codebooks(shape), NEED[shape]
    g0 = ids[:, 0].astype(np.int64)
    g1 = g0 * need[1] + ids[:, 1]
    if sem_name == "simplified":
        return [g0, g1, ids[:, 2].astype(np.int64)]
    rows, cols = np.nonzero(cb["match"])  # row-major: each group's allowed columns, ascending
    start = np.concatenate([[0], np.cumsum(cb["match"].sum(1, dtype=np.int64))])
    grp = ids[:, 0].astype(np.int64) * need[0] + ids[:, 1]
    return [g0, g1, cols[start[grp] + ids[:, 2]]]


@functools.lru_cache(maxsize=None)
def _case(shape, sem_name):
    """x, the GPU encode's IDs, their global rows and the yardstick, computed once per (shape, semantics)."""
    x = _rows(shape)
    enc = _encoder(shape, sem_name)
    ids = enc.encode(gpu(x)).cpu().numpy()
    cb = _codebooks(shape)
    cents = [cb["c0"], cb["c1"], cb["c2"]]
    globs = host_globals(ids, shape, sem_name)
    e_ref, cur_norm = yardstick(x, cents, globs, SEM[sem_name].normalize_residual)
    return x, ids, globs, e_ref, cur_norm


# ------------------------------------------------------------------------------------------- 1. single level
@pytest.mark.parametrize("n,k,d", [(1, 8, 512), (129, 128, 512), (777, 300, 64)])
def test_single_level(n, k, d):
    x = synth.small_mixture(n, d=d, m=50, seed=n + k)
    c = synth.small_mixture(k, d=d, m=50, seed=n + k + 1)
    g = O.nearest(x, c, exact=True)
    err, xn, sums = ops.quant_error(gpu(x), [gpu(c)], [gpu(g.astype(np.int32))])
    assert err.shape == (n, 1) and xn.shape == (n,) and sums.shape == (2,)
    e_ref = norm32(x - c[g])
    assert (np.abs(err[:, 0].cpu().numpy().astype(np.float64) - e_ref) <= ulp32(e_ref)).all()
    xr = norm32(x)
    assert (np.abs(xn.cpu().numpy().astype(np.float64) - xr) <= ulp32(xr)).all()
    want = np.array([(err.cpu().numpy().astype(np.float64) ** 2).sum(), (xn.cpu().numpy().astype(np.float64) ** 2).sum()])
    np.testing.assert_allclose(sums.cpu().numpy(), want, rtol=max(n, 2) * 2.0 ** -52)


# ----------------------------------------------------------------------------------- 2. chain, both semantics
@pytest.mark.parametrize("sem_name", ["hier", "simplified"])
@pytest.mark.parametrize("shape", ["small", "prod"])
def test_chain_against_the_oracle(shape, sem_name):
    x, ids, globs, e_ref, cur_norm = _case(shape, sem_name)
    enc = _encoder(shape, sem_name)
    norm = SEM[sem_name].normalize_residual
    xd = gpu(x)
    qe = enc.quant_error(xd, ids=gpu(ids.astype(np.int32)))
    for g_dev, g_host in zip(enc.global_rows(qe.ids), globs):
        assert (g_dev.cpu().numpy() == g_host).all()
    assert_chain(qe.err.cpu().numpy(), e_ref, cur_norm, norm)
    xr = norm32(x)
    assert (np.abs(qe.x_norm.cpu().numpy().astype(np.float64) - xr) <= ulp32(xr)).all()
    own = enc.quant_error(xd)  # ids=None: encodes first
    assert torch.equal(own.ids, enc.encode(xd)) and (own.ids.cpu().numpy() == ids).all()
    assert same_bits(own.err, qe.err) and same_bits(own.recon_err, qe.recon_err)
    # (each call buckets the rows anew, and the order inside a bucket is not fixed: the totals may round differently)
    np.testing.assert_allclose(own.sums.cpu().numpy(), qe.sums.cpu().numpy(), rtol=len(x) * 2.0 ** -52)
    assert all(int(w.item()) == 0 for w in enc.error_words())


# ---------------------------------------------------------------------- 3. the encode's own level-1 divisor
def test_level0_error_is_the_encode_divisor():
    enc = _encoder("prod", "hier")
    x = gpu(_rows("prod"))
    n = x.shape[0]
    ids0 = ops.nearest(x, enc.pcs[0])
    den = torch.zeros(n, dtype=torch.float32, device=DEV)
    fr = ops.FusedResidual(1, True, enc.pcs[0].centers, None, den_out=den)
    ops.assign(x, enc.pcs[1], ops.bucket(ids0, NEED["prod"][0]), enc.cands[1], fused=fr)
    err, _, _ = ops.quant_error(x, [enc.pcs[0].centers], [ids0])
    mine = (err[:, 0] + torch.tensor(1e-8, dtype=torch.float32, device=DEV)).cpu().numpy()
    den = den.cpu().numpy()
    assert (np.abs(mine.astype(np.float64) - den) <= ulp32(den)).all()
    # two fp64 summation orders round to different fp32 values with probability ~1e-6 per row
    assert int((mine.view(np.int32) != den.view(np.int32)).sum()) <= n // 10_000


# ------------------------------------------------------------------------------------------- 4. 16-bit rows
@pytest.mark.parametrize("fmt", ["f16", "bf16"])
@pytest.mark.parametrize("shape,sem_name", [("small", "hier"), ("small", "simplified"), ("prod", "hier")])
def test_16bit_rows_equal_their_fp32_widening(shape, sem_name, fmt):
    x = _rows(shape).copy()
    if fmt == "f16":
        x[5] *= 1e-6     # almost every element an fp16 subnormal
    else:
        x[7] *= 1e5      # beyond the fp16 range
    t16 = torch.from_numpy(x).to({"f16": torch.float16, "bf16": torch.bfloat16}[fmt])
    x32 = t16.float()
    if fmt == "f16":
        sub = x32[5].abs()
        assert bool(((sub < 2.0 ** -14) & (sub > 0)).float().mean() > 0.5)
    else:
        assert bool((x32[7].abs() > 65504).float().mean() > 0.5)
    enc = _encoder(shape, sem_name)
    ids = enc.encode(x32.to(DEV))
    # one bucketing for both calls: the totals are bit-reproducible for a fixed processing order
    need = NEED[shape]
    order = ops.bucket(ids[:, 0] * need[0] + ids[:, 1], need[0] * need[1]).row_index
    cents, globs, norm = [pc.centers for pc in enc.pcs], enc.global_rows(ids), SEM[sem_name].normalize_residual
    for ro in (order, None):
        a = ops.quant_error(t16.to(DEV), cents, globs, norm, row_order=ro)
        b = ops.quant_error(x32.to(DEV), cents, globs, norm, row_order=ro)
        assert same_bits(a[0], b[0]) and same_bits(a[1], b[1]) and same_bits(a[2], b[2])
        assert bool(torch.isfinite(a[0]).all()) and bool((a[1] > 0).all())
    # and through the encoder, which reads the 16-bit rows as they are
    qa, qb = enc.quant_error(t16.to(DEV), ids=ids), enc.quant_error(x32.to(DEV), ids=ids)
    assert same_bits(qa.err, qb.err) and same_bits(qa.err, a[0]) and same_bits(qa.recon_err, qb.recon_err)


# ------------------------------------------------------------------------------------ 5. order, determinism
def test_row_order_changes_nothing_per_row_and_sums_are_deterministic():
    x, ids, globs, _, _ = _case("prod", "hier")
    enc = _encoder("prod", "hier")
    xd = gpu(x)
    n = len(x)
    cents = [pc.centers for pc in enc.pcs]
    gl = [gpu(g.astype(np.int32)) for g in globs]
    grp = gpu((ids[:, 0] * NEED["prod"][0] + ids[:, 1]).astype(np.int32))
    orders = [None, ops.bucket(grp, NEED["prod"][0] * NEED["prod"][1]).row_index,
              torch.arange(n - 1, -1, -1, dtype=torch.int32, device=DEV)]
    res = [ops.quant_error(xd, cents, gl, True, row_order=o) for o in orders]
    again = [ops.quant_error(xd, cents, gl, True, row_order=o) for o in orders]
    for (e, xn, s), (e2, xn2, s2) in zip(res, again):
        assert same_bits(e, res[0][0]) and same_bits(xn, res[0][1])
        assert same_bits(e2, e) and same_bits(s2, s)  # same inputs, same order: the same bits
    e64 = res[0][0].cpu().numpy().astype(np.float64)
    want = np.concatenate([(e64 ** 2).sum(0), [(res[0][1].cpu().numpy().astype(np.float64) ** 2).sum()]])
    for _, _, s in res:
        np.testing.assert_allclose(s.cpu().numpy(), want, rtol=n * 2.0 ** -52)


# ------------------------------------------------------------------------------------- 6. out-of-range ids
def test_out_of_range_ids():
    x, ids, globs, _, _ = _case("small", "hier")
    enc = _encoder("small", "hier")
    n = 500
    xd = gpu(x[:n])
    cents = [pc.centers for pc in enc.pcs]
    gl = [gpu(g[:n].astype(np.int32)) for g in globs]
    clean_e, clean_xn, clean_s = ops.quant_error(xd, cents, gl, True)
    bad = [g.clone() for g in gl]
    bad[1][17] = -1
    bad[2][301] = cents[2].shape[0]
    ws = ops.QuantErrorWorkspace(n, DEV)
    e, xn, s = ops.quant_error(xd, cents, bad, True, workspace=ws, check=False)
    assert int(ws.error_word().item()) & 1
    e, clean = e.cpu().numpy(), clean_e.cpu().numpy()
    assert np.isfinite(e[17, 0]) and np.isnan(e[17, 1:]).all()
    assert np.isfinite(e[301, :2]).all() and np.isnan(e[301, 2])
    keep = np.ones(n, bool)
    keep[[17, 301]] = False
    assert (e[keep].view(np.int32) == clean[keep].view(np.int32)).all()
    assert e[17, 0].view(np.int32) == clean[17, 0].view(np.int32)
    assert same_bits(xn, clean_xn)
    c64, xn64 = clean.astype(np.float64) ** 2, clean_xn.cpu().numpy().astype(np.float64) ** 2
    want = np.concatenate([c64[keep].sum(0), [xn64[keep].sum()]])
    np.testing.assert_allclose(s.cpu().numpy(), want, rtol=n * 2.0 ** -52)
    assert (s.cpu().numpy() < clean_s.cpu().numpy()).all()
    with pytest.raises(RuntimeError):
        ops.quant_error(xd, cents, bad, True, check=True)
    fresh = ops.QuantErrorWorkspace(n, DEV)
    ops.quant_error(xd, cents, gl, True, workspace=fresh)
    assert int(fresh.error_word().item()) == 0
    # the encoder: raises, and starts the next call from a clean workspace
    wrong = gpu(ids[:n].astype(np.int32))
    wrong[3, 2] = NEED["small"][2]
    with pytest.raises(RuntimeError):
        enc.quant_error(xd, ids=wrong)
    assert same_bits(enc.quant_error(xd, ids=gpu(ids[:n].astype(np.int32))).err, clean_e)
    enc.check_errors()


# ------------------------------------------------------------------------------ 7. offsets past 2^31 elements
def test_row_offsets_past_2_31_elements():
    n, d, k = 4_200_300, 512, 128
    gen = torch.Generator(device=DEV).manual_seed(3)
    x = torch.empty((n, d), dtype=torch.float16, device=DEV)
    step = 1 << 19
    for i in range(0, n, step):
        x[i:i + step] = torch.randn((min(step, n - i), d), generator=gen, device=DEV, dtype=torch.float32).to(torch.float16)
    c = torch.randn((k, d), generator=gen, device=DEV, dtype=torch.float32)
    ids = torch.randint(0, k, (n,), generator=gen, device=DEV, dtype=torch.int32)
    err, xn, _ = ops.quant_error(x, [c], [ids])
    rng = np.random.default_rng(9)
    pick = np.concatenate([np.arange(n - 256, n), rng.integers(4_194_304, n - 256, 256)])
    pd = torch.from_numpy(pick).to(DEV)
    xs = x[pd].float().cpu().numpy()
    e_ref = norm32(xs - c.cpu().numpy()[ids[pd].cpu().numpy()])
    got = err[pd, 0].cpu().numpy().astype(np.float64)
    assert (np.abs(got - e_ref) <= ulp32(e_ref)).all()
    xr = norm32(xs)
    assert (np.abs(xn[pd].cpu().numpy().astype(np.float64) - xr) <= ulp32(xr)).all()


# ---------------------------------------------------------------------------------------- 8. graph capture
def test_graph_replays_equal_eager():
    x, ids, _, _, _ = _case("small", "hier")
    enc = _encoder("small", "hier")
    xd, idd = gpu(x), gpu(ids.astype(np.int32))
    eager = enc.quant_error(xd, ids=idd)
    eager = (eager.err.clone(), eager.x_norm.clone(), eager.sums.clone(), eager.recon_err.clone())
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            enc.quant_error(xd, ids=idd, check=False)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = enc.quant_error(xd, ids=idd)
    for _ in range(3):
        for t in (out.err, out.x_norm, out.sums, out.recon_err):
            t.zero_()
        g.replay()
        torch.cuda.synchronize()
        for got, want in zip((out.err, out.x_norm, out.recon_err), (eager[0], eager[1], eager[3])):
            assert same_bits(got, want)
        # every replay buckets the rows anew (the order inside a bucket is not fixed): totals to rounding
        np.testing.assert_allclose(out.sums.cpu().numpy(), eager[2].cpu().numpy(), rtol=len(x) * 2.0 ** -52)
    enc.check_errors()
    assert all(int(w.item()) == 0 for w in enc.error_words())
    del g


# --------------------------------------------------------------------------------------------- 9. fallback
def test_fallback_groups_weights_four_levels():
    rng = np.random.default_rng(77)
    n, d, need = 2000, 512, [4, 4, 4, 8]
    gd, weights = [256, 256], [[1, 1], [1.5, 0.5], [1, 1], [1, 1]]
    x = synth.small_mixture(n, m=32, seed=78)

    def unit(k):
        v = rng.standard_normal((k, d)).astype(F32)
        return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F32)
    cents = [x[rng.choice(n, 4, replace=False)].copy(), unit(16), unit(16), unit(32)]
    match = np.zeros((16, 32), dtype=np.uint8)
    for gi in range(16):
        match[gi, rng.choice(32, 8, replace=False)] = 1
    enc = RQEncoder([torch.from_numpy(c) for c in cents], need, match=torch.from_numpy(match), group_dims=gd,
                    weights=weights, semantics=HIERARCHICAL_TRAIN, device=DEV)
    assert not enc.quant_error_fused
    xd = gpu(x)
    qe = enc.quant_error(xd)
    ids = qe.ids.cpu().numpy().astype(np.int64)
    assert torch.equal(qe.ids, enc.encode(xd))
    cols = np.nonzero(match)[1].reshape(16, 8)
    globs = [ids[:, 0], ids[:, 0] * 4 + ids[:, 1], ids[:, 1] * 4 + ids[:, 2], cols[ids[:, 1] * 4 + ids[:, 2], ids[:, 3]]]
    e_ref, cur_norm = yardstick(x, cents, globs, True, gd, weights)
    assert_chain(qe.err.cpu().numpy(), e_ref, cur_norm, True)
    e64 = qe.err.cpu().numpy().astype(np.float64)
    np.testing.assert_allclose(qe.sums.cpu().numpy()[:4], (e64 ** 2).sum(0), rtol=n * 2.0 ** -52)
    assert qe.recon_err.shape == (n,) and bool(torch.isfinite(qe.recon_err).all())


def test_reference_predict_quirk_has_no_error_of_the_encoding():
    cb = _codebooks("small")
    for sem in (HIERARCHICAL_PREDICT_REFERENCE, LevelSemantics(residual_global_id=False)):
        enc = RQEncoder([torch.from_numpy(cb[k]) for k in ("c0", "c1", "c2")], NEED["small"],
                        match=torch.from_numpy(cb["match"]), semantics=sem, device=DEV)
        with pytest.raises(ValueError):
            enc.quant_error(gpu(_rows("small")[:64]))
        with pytest.raises(ValueError):
            enc.decode(torch.zeros((4, 3), dtype=torch.int32, device=DEV))


# ----------------------------------------------------------------------------------------------- 10. decode
@pytest.mark.parametrize("sem_name", ["hier", "simplified"])
def test_decode_reconstruction_error(sem_name):
    x, ids, _, _, _ = _case("small", sem_name)
    enc = _encoder("small", sem_name)
    qe = enc.quant_error(gpu(x), ids=gpu(ids.astype(np.int32)))
    xh = enc.decode(qe.ids, qe.err)
    assert xh.dtype == torch.float32 and xh.shape == x.shape
    xh = xh.cpu().numpy().astype(np.float64)
    x64 = x.astype(np.float64)
    dist = np.sqrt(((x64 - xh) ** 2).sum(1))
    bound = 16 * 2.0 ** -24 * (np.sqrt((x64 ** 2).sum(1)) + np.sqrt((xh ** 2).sum(1)))
    assert (np.abs(dist - qe.recon_err.cpu().numpy().astype(np.float64)) <= bound).all()
    if sem_name == "hier":
        with pytest.raises(ValueError):
            enc.decode(qe.ids)
    else:
        assert torch.equal(enc.decode(qe.ids), enc.decode(qe.ids, qe.err))
        assert same_bits(qe.recon_err, qe.err[:, 2].contiguous())


# ------------------------------------------------------------------------------------- 11. model and driver
def _small_model(group=None):
    cb = _codebooks("small")
    cfg = HierarchicalRQKMeansConfig(layer_clusters=[16, 160, 160], need_clusters=[16, 16, 32], embedding_dim=512)
    m = HierarchicalRQKMeans(cfg, device=DEV, group=group)
    m.cluster_centers_list = [torch.from_numpy(cb[k]) for k in ("c0", "c1", "c2")]
    m.match_matrices = [cb["match"]]
    m.is_trained = True
    return m


def _check_report(rep, n_levels):
    assert set(rep) == {"rows", "levels", "unique_semantic_ids", "coverage"}
    assert len(rep["levels"]) == n_levels
    for lv in rep["levels"]:
        assert set(lv) == LEVEL_KEYS
        assert set(lv["cluster_distribution"]) == {"min", "max", "mean", "std"}


def _same_report(rep, ref, rows):
    """Two reports of the same rows: counts, maxima and IDs equal; the means come from fp64 totals that another
    processing order (a new bucketing, a sharding) adds in another order, so they agree to rows * 2^-52."""
    assert rep["rows"] == ref["rows"] == rows
    assert rep["unique_semantic_ids"] == ref["unique_semantic_ids"] and rep["coverage"] == ref["coverage"]
    assert len(rep["levels"]) == len(ref["levels"])
    for lv, lr in zip(rep["levels"], ref["levels"]):
        assert set(lv) == LEVEL_KEYS
        for k in ("level", "max", "unique_clusters", "cluster_distribution"):
            assert lv[k] == lr[k], k
        for k in ("mse", "rmse", "recon_mse", "relative"):
            np.testing.assert_allclose(lv[k], lr[k], rtol=rows * 2.0 ** -52)


def test_model_quantization_error():
    m = _small_model()
    x = _rows("small")
    rep = m.quantization_error(x, return_rows=True)
    rows = {k: rep.pop(k) for k in ("ids", "err", "recon_err")}
    _check_report(rep, 3)
    assert rep["rows"] == len(x)
    assert (rows["ids"] == m.predict(x, reference_quirks=False)).all()
    qe = m._encoder(False).quant_error(gpu(x))
    sums = qe.sums.cpu().numpy()
    for l, lv in enumerate(rep["levels"]):
        # mse is sums[l] / rows of the report's own call; this call bucketed anew, so its total may round differently
        np.testing.assert_allclose(lv["mse"], sums[l] / len(x), rtol=len(x) * 2.0 ** -52)
        np.testing.assert_allclose(lv["mse"], (rows["err"][:, l].astype(np.float64) ** 2).mean(),
                                   rtol=len(x) * 2.0 ** -52)
        assert lv["rmse"] == np.sqrt(lv["mse"])
        assert lv["max"] == float(rows["err"][:, l].max())
    # relative_l = sum ||x - x_hat_l||^2 / sum ||x||^2 with ||x - x_hat_l|| = e_l prod_{j<l} (e_j + 1e-8), restated in
    # fp64 from the returned rows (the report multiplies in fp32: a few 2^-24 relative)
    e64 = rows["err"].astype(np.float64)
    energy = (x.astype(np.float64) ** 2).sum()
    scale = np.ones(len(x))
    for l, lv in enumerate(rep["levels"]):
        np.testing.assert_allclose(lv["relative"], ((e64[:, l] * scale) ** 2).sum() / energy, rtol=1e-6)
        np.testing.assert_allclose(lv["recon_mse"], ((e64[:, l] * scale) ** 2).mean(), rtol=1e-6)
        scale = scale * (e64[:, l] + 1e-8)
    np.testing.assert_allclose(rep["levels"][2]["recon_mse"], (rows["recon_err"].astype(np.float64) ** 2).mean(),
                               rtol=1e-12)
    sid = {f"s{i}": [int(v) for v in r] for i, r in enumerate(rows["ids"])}
    stats = rq_io.semantic_id_statistics(sid, [16, 16, 32])
    assert rep["unique_semantic_ids"] == stats["unique_semantic_ids"]
    assert rep["coverage"] == stats["unique_semantic_ids"] / len(x)
    for lv, st in zip(rep["levels"], stats["layer_statistics"]):
        assert lv["unique_clusters"] == st["unique_clusters"]
        assert lv["cluster_distribution"] == st["cluster_distribution"]
    # fp16 rows stay fp16 on their way to the kernel
    m.quantization_error(x.astype(np.float16))
    assert m._encoder(False).last_row_format == "f16"


def _rows_near_the_codebooks(n=3000, seed=31):
    """Rows the small codebooks quantise well: x = c0[a0] + 4 (c1[g1] + 0.3 (c2[g2] + noise)) for random valid IDs
    (g2 among the allowed columns of its group), ||noise|| ~ 0.1.  The mixture rows of the other tests are no use
    for a statement about quality: those codebooks are not fitted to them (c0 is 16 catalogue rows of a 4096-blob
    mixture, ||x - c0|| ~ 32 against ||x|| ~ 23, and the unit-norm deeper centres lie at distance > 1 from the
    unit-norm residuals), and the report says so: relative = 1.81, 1.74, 2.62 there."""
    cb, need = _codebooks("small"), NEED["small"]
    rng = np.random.default_rng(seed)
    a0, a1, r2 = rng.integers(0, need[0], n), rng.integers(0, need[1], n), rng.integers(0, need[2], n)
    cols = np.nonzero(cb["match"])[1].reshape(need[0] * need[1], need[2])
    g2 = cols[a0 * need[0] + a1, r2]
    noise = (0.1 / np.sqrt(512)) * rng.standard_normal((n, 512))
    x = cb["c0"][a0] + 4.0 * (cb["c1"][a0 * need[1] + a1] + 0.3 * (cb["c2"][g2] + noise))
    return x.astype(F32)


def test_relative_error_is_non_increasing_over_levels():
    """On rows the codebooks serve (each level's centre explains part of what the level above left), the share of the
    rows' energy left unexplained does not grow with the levels, and every level's normalised error is below 1."""
    x = _rows_near_the_codebooks()
    rep = _small_model().quantization_error(x, return_rows=True)
    rel = [lv["relative"] for lv in rep["levels"]]
    print("relative per level:", rel)
    assert rel[0] >= rel[1] >= rel[2] > 0, rel
    assert rel[0] < 1
    assert (rep["err"][:, 1:] < 1).all()
    mse = [lv["recon_mse"] for lv in rep["levels"]]
    assert mse[0] >= mse[1] >= mse[2] > 0, mse


def test_simplified_model_quantization_error():
    from generative_ranking_recommender_amd.balancekmeans import KMeans
    from generative_ranking_recommender_amd.simplified_semantic_id_generator import SimplifiedHierarchicalRQ
    cb = _codebooks("small")
    cfg = HierarchicalRQKMeansConfig(layer_clusters=[16, 16, 160], need_clusters=[16, 16, 32], embedding_dim=512)
    m = SimplifiedHierarchicalRQ(cfg, device=DEV)
    c0 = torch.from_numpy(cb["c0"]).to(DEV)
    m.trained_kmeans_models = [KMeans(n_clusters=16, cluster_centers=c0, device=DEV), None, None]
    m.middle_layer_centers = torch.from_numpy(cb["c1"]).to(DEV)
    m.final_layer_centers = torch.from_numpy(cb["c2"]).to(DEV)
    m.dynamic_match_matrix = torch.from_numpy(cb["match"].astype(np.float32))
    x, ids, _, _, _ = _case("small", "simplified")
    rep = m.quantization_error(x, return_rows=True)
    assert (rep.pop("ids") == ids).all()
    err = rep.pop("err")
    assert (rep.pop("recon_err").view(np.int32) == err[:, 2].view(np.int32)).all()
    _check_report(rep, 3)
    for lv in rep["levels"]:  # plain residuals: every level's error is already in the original space
        np.testing.assert_allclose(lv["recon_mse"], lv["mse"], rtol=1e-12)


TRAIN_CFG = dict(layer_clusters=[4, 8, 8], need_clusters=[4, 4, 4], embedding_dim=64, iter_limit=3)


def _trainer_cfg(root, csv_path):
    return types.SimpleNamespace(
        output_dir=os.path.join(root, "outputs"), model_dir=os.path.join(root, "models"),
        h_rqkmeans_test=HierarchicalRQKMeansConfig(**TRAIN_CFG), h_rqkmeans=None,
        data=types.SimpleNamespace(song_vectors_file=csv_path,
                                   semantic_ids_file=os.path.join(root, "outputs", "semantic_id",
                                                                  "song_semantic_ids.jsonl")))


def test_trainer_writes_the_report_only_when_asked(tmp_path):
    import json

    from generative_ranking_recommender_amd.train_semantic_ids import SemanticIDTrainer
    x = synth.small_mixture(600, d=64, m=16, seed=5)
    csv_path = str(tmp_path / "vec.csv")
    rq_io.write_song_vectors(csv_path, [f"song{i}" for i in range(len(x))], x)
    out = {}
    for name, kw in (("plain", {}), ("report", {"report_quantization": True})):
        np.random.seed(7)
        torch.manual_seed(7)
        root = str(tmp_path / name)
        out[name] = (root, SemanticIDTrainer(_trainer_cfg(root, csv_path), use_test_config=True, device=DEV,
                                             **kw).train(resume=False))
    files = {n: sorted(os.listdir(os.path.join(r, "outputs", "semantic_id"))) for n, (r, _) in out.items()}
    assert "quantization_report.json" not in files["plain"]
    assert files["report"] == sorted(files["plain"] + ["quantization_report.json"])
    assert "quantization_report" not in out["plain"][1]
    for rel in ("training_statistics.json", "training_config.json", "song_semantic_ids.jsonl"):
        a, b = (open(os.path.join(r, "outputs", "semantic_id", rel), "rb").read() for r, _ in out.values())
        assert a == b, rel
    with open(os.path.join(out["report"][0], "outputs", "semantic_id", "quantization_report.json")) as f:
        written = json.load(f)
    _check_report(written, 3)
    assert written == out["report"][1]["quantization_report"]
    assert written["rows"] == len(x)
    again = out["report"][1]["model"].quantization_error(rq_io.load_song_vectors(csv_path, 64)[1])
    _same_report(again, written, len(x))


def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _report_worker(rank, world, port, out):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        rep = _small_model(group=dist.group.WORLD).quantization_error(_rows("small"), return_rows=True)
        out.put((rank, rep, None))
    except Exception:  # report instead of leaving the parent waiting
        import traceback
        out.put((rank, None, traceback.format_exc()))
    dist.destroy_process_group()


def test_two_ranks_return_the_single_process_report():
    import torch.multiprocessing as mp
    ref = _small_model().quantization_error(_rows("small"), return_rows=True)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _port()
    procs = [ctx.Process(target=_report_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=240) for _ in range(2)], key=lambda r: r[0])
    for p in procs:
        p.join(60)
    for rank, rep, tb in res:
        assert rep is not None, tb
        for k in ("ids", "err", "recon_err"):  # per-row results do not depend on the sharding
            assert rep[k].dtype == ref[k].dtype and (rep[k].view(np.int32) == ref[k].view(np.int32)).all(), k
        _same_report({k: v for k, v in rep.items() if k not in ("ids", "err", "recon_err")}, ref, ROWS["small"])
