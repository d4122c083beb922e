"""The producer/consumer screen's transposed bound epilogue (csrc/assign_pc.hip: a lane owns one candidate of
every 32-candidate tile and 16 rows) against the per-tile screen, array for array, and against the exact oracle.

One rqsid_assign call per configuration, on hand-built segments chosen for the lane mapping:
 * segment row counts 1, 31, 32, 33, 127, 128, 129, 300 (single-row and ragged last tiles, several tiles);
 * candidate counts 1, 31, 32, 33, 255, 256 (the mask of the candidates at or beyond the count);
 * a segment with bitwise-duplicate centres (deduplicated: cand_lid), a penalty segment and an empty list;
 * exact ties and near ties (one centre 2^-21 farther) between candidates k, k+32 (one lane), k, k+1
   (neighbouring lanes), 15/16 and 47/48 (the two rows of 16 lanes of a wave half), 31/32 (two tiles), each on the
   eight rows r .. r+7 of a tile (rows r and r+4 sit in the two halves of a wave), and rows with exactly 8 and
   exactly 9 equidistant nearest centres (the list / "every candidate" boundary of the work item);
 * a row holding a NaN and a row holding an Inf among ordinary rows.
RQSID_SCREEN_VARIANT=9 forces the producer/consumer screen wherever the plan allows it (tests/test_assign_plan.py
pins that these shapes qualify: 512-d residual levels, <= 256 candidates, n_segments + 1 <= n_rows), 1 the
per-tile screen; the library reads the switch per call.  Compared: out_local, out_global and the re-scored row
count, all for equality, and the final IDs with oracle/rq_oracle.py's exact (fp64) argmin of the same residual
chain.  In the tie segments under normalisation the chain's fp32 roundings turn the constructed ties into gaps
of ~1e-8 relative, below what separates the kernel's exact re-score of its own chain from the oracle's fp32
residual: there a difference must be a certified near tie (relative gap < 1e-6), everywhere else none is
allowed.  The two non-finite rows and the empty-list segment have no oracle answer and are compared between the
screens only."""
import os

import numpy as np
import pytest
import torch

from generative_ranking_recommender_amd import ops
from oracle import rq_oracle as O

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
D = 512
F32 = np.float32
RHO, SIGMA, NUDGE = 0.5, 0.125, 2.0 ** -21
# (candidates that tie) per group of eight consecutive rows of a tie segment
TIES = [(5, 37), (5, 6), (15, 16), (47, 48), (31, 32), (200, 232), tuple(range(64, 72)), (3, 40, 77, 114, 151, 188, 225, 255, 9)]


def gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _with_env(env, fn):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update({k: str(v) for k, v in env.items()})
    try:
        return fn()
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def _tie_segment(rng, n_rows, nudged):
    """256 centres b + rho_j e_j around a unit b that lives on dims 256..511, and rows b + sigma sum_{j in S} e_j:
    exactly the centres of S are nearest, at equal distance (every value is a short dyadic fraction, so the
    differences and their squares are exact); nudged: odd centres sit 2^-21 (relative) farther along their axis."""
    b = np.zeros(D, F32)
    b[256:] = 1.0 / 16.0
    c = np.tile(b, (256, 1))
    rho = np.full(256, RHO, F32)
    if nudged:
        rho[1::2] = F32(RHO * (1.0 + NUDGE))
    c[np.arange(256), np.arange(256)] += rho
    v = np.tile(b, (n_rows, 1))
    for i in range(n_rows):
        for j in TIES[(i // 8) % len(TIES)]:
            v[i, j] += F32(SIGMA)
    return c, v


def _problem(rl, norm, seed):
    rng = np.random.default_rng(seed)
    # (rows, candidates, kind)
    segs = [(1, 1, "gen"), (31, 31, "gen"), (32, 32, "gen"), (33, 33, "gen"), (127, 255, "gen"), (128, 256, "gen"),
            (129, 256, "gen"), (300, 200, "gen"), (140, 256, "dup"), (37, 0, "penalty"), (5, 0, "empty"),
            (133, 256, "tie"), (133, 256, "near"), (40, 256, "nonfinite")]
    S = len(segs)
    ca = (0.05 * rng.standard_normal((S + 1, D))).astype(F32)
    cb = (0.02 * rng.standard_normal((S + 1, D))).astype(F32)  # |cb| ~ 0.45 < 1: a unit cb + beta t exists
    ca[S] = 0
    cb[S] = 0
    seg_ca = np.arange(S, dtype=np.int32)
    seg_cb = np.arange(S, dtype=np.int32)
    centres, lists, targets = [], [], []
    k0 = 0
    for s, (nr, cnt, kind) in enumerate(segs):
        if kind in ("tie", "near"):
            seg_ca[s] = seg_cb[s] = S  # the zero rows: v is the row itself (NORM off) or its direction
            c, v = _tie_segment(rng, nr, kind == "near")
        else:
            c = (rng.standard_normal((cnt, D)) / np.sqrt(D)).astype(F32)
            if kind == "dup":  # bitwise copies of an earlier entry: same lane (+32), next lane (twice), last tile
                c[40] = c[8]
                c[9] = c[8]
                c[100] = c[99]
                c[255] = c[0]
            if cnt:
                v = c[rng.integers(0, cnt, nr)] + (0.3 / np.sqrt(D)) * rng.standard_normal((nr, D))
            else:
                v = rng.standard_normal((nr, D)) / np.sqrt(D)
            v = v.astype(F32)
        centres.append(c)
        lists.append(np.arange(k0, k0 + cnt))
        targets.append(v)
        k0 += cnt
    c_all = np.concatenate(centres).astype(F32)
    rows = []
    for s, v in enumerate(targets):  # rows whose residual chain gives v (or, normalised, its direction)
        a, b = ca[seg_ca[s]], cb[seg_cb[s]]
        if rl == 1:
            x = a + v
        elif not norm:
            x = a + b + v
        else:
            t = v.astype(np.float64) / np.linalg.norm(v.astype(np.float64), axis=1, keepdims=True)
            bt = t @ b.astype(np.float64)
            beta = -bt + np.sqrt(bt * bt - float(b.astype(np.float64) @ b.astype(np.float64)) + 1.0)
            x = a + 3.0 * (b + beta[:, None] * t)
        rows.append(x.astype(F32))
    x_seg = np.concatenate(rows)
    n = len(x_seg)
    seg_of_pos = np.repeat(np.arange(S), [nr for nr, _, _ in segs])
    off = np.concatenate([[0], np.cumsum([nr for nr, _, _ in segs])]).astype(np.int32)
    nf = np.nonzero(seg_of_pos == S - 1)[0]
    x_seg[nf[3], 17] = np.nan
    x_seg[nf[9], 400] = np.inf
    no_oracle = np.zeros(n, bool)
    no_oracle[[nf[3], nf[9]]] = True
    no_oracle[seg_of_pos == 10] = True
    tie_rows = np.isin(seg_of_pos, (11, 12))
    # RL 2: the rows lie permuted in x and the segments find them through row_index; RL 1: identity order
    perm = rng.permutation(n) if rl == 2 else np.arange(n)
    x = np.empty_like(x_seg)
    x[perm] = x_seg
    return dict(segs=segs, S=S, ca=ca, cb=cb, seg_ca=seg_ca, seg_cb=seg_cb, c=c_all, lists=lists, x=x, perm=perm, off=off,
                seg_of_pos=seg_of_pos, no_oracle=no_oracle, tie_rows=tie_rows, n=n)


def _oracle(P, rl, norm):
    """(v, exact global ids, local ids, den_in) by position in segment order."""
    xs = P["x"][P["perm"]]
    s = P["seg_of_pos"]
    den = None
    if rl == 1:
        v = O.residual(xs, P["ca"], P["seg_ca"][s], normalize=False)
    else:
        r1 = O.residual(xs, P["ca"], P["seg_ca"][s], normalize=norm)
        if norm:
            r = (xs.astype(F32) - P["ca"][P["seg_ca"][s]]).astype(F32)
            den = (np.sqrt((r.astype(np.float64) ** 2).sum(1)).astype(F32) + F32(1e-8)).astype(F32)
        v = O.residual(r1, P["cb"], P["seg_cb"][s], normalize=norm)
    ok = ~P["no_oracle"]
    glob = np.full(P["n"], -1, np.int64)
    with np.errstate(all="ignore"):
        glob[ok] = O.segmented_nearest(v[ok], P["c"], s[ok], P["lists"], penalty="10000", exact=True)
    loc = np.full(P["n"], -1, np.int64)
    for i in np.nonzero(ok)[0]:
        lst = P["lists"][s[i]]
        if len(lst):
            loc[i] = glob[i] - lst[0]
    return v, glob, loc, den


def _run(P, rl, norm, den, env):
    S, n = P["S"], P["n"]
    tr = ops.tile_rows()
    nr = np.diff(P["off"])
    toff = np.concatenate([[0], np.cumsum((nr + tr - 1) // tr)]).astype(np.int32)
    buckets = ops.Buckets(gpu(P["off"]), gpu(toff), gpu(P["perm"].astype(np.int32)) if rl == 2 else None, S, int(toff[-1]))
    cnt = np.array([len(l) for l in P["lists"]], np.int32)
    base = np.concatenate([[0], np.cumsum(cnt)[:-1]]).astype(np.int32)
    flags = np.array([1 if k == "penalty" else 0 for _, _, k in P["segs"]], np.uint8)
    pc = ops.prepare_centers(gpu(P["c"]))
    if rl == 2:  # explicit lists, bitwise duplicates dropped (cand_lid); RL 1: contiguous candidates, no list
        cand = ops.Candidates(gpu(base), gpu(cnt), int(cnt.max()), gpu(np.concatenate(P["lists"]).astype(np.int32)), gpu(flags))
        cand = ops.dedup_candidates(cand, pc.centers)
        assert cand.lid is not None, "the duplicate centres were not removed"
        den_pos = None
        if norm:
            den_x = np.empty(n, F32)
            den_x[P["perm"]] = den
            den_pos = gpu(den_x)
        fr = ops.FusedResidual(2, norm, gpu(P["ca"]), gpu(P["seg_ca"]), gpu(P["cb"]), gpu(P["seg_cb"]), den_in=den_pos)
        terms = 0  # more than 128 candidates: the 1-term screen, eight candidate tiles
    else:
        cand = ops.Candidates(gpu(base), gpu(cnt), int(cnt.max()), None, gpu(flags))
        fr = ops.FusedResidual(1, False, gpu(P["ca"]), gpu(P["seg_ca"]))
        terms = 1  # (a first-level residual takes the 3-term screen by default, which stops at 128 candidates)
    ws = ops.AssignWorkspace(n, DEV)
    x = gpu(P["x"])
    loc, glob = _with_env(env, lambda: ops.assign(x, pc, buckets, cand, workspace=ws, fused=fr, screen_terms=terms))
    torch.cuda.synchronize()
    assert ws.error() == 0
    # by position in segment order
    return loc.cpu().numpy()[P["perm"]], glob.cpu().numpy()[P["perm"]], ws.rescored()


CONFIGS = {"rl2_norm": (2, True), "rl2_raw": (2, False), "rl1_raw": (1, False)}
_cache = {}


def _case(name):
    if name not in _cache:
        rl, norm = CONFIGS[name]
        P = _problem(rl, norm, seed=11 + len(name))
        v, glob, loc, den = _oracle(P, rl, norm)
        pcs = _run(P, rl, norm, den, {"RQSID_SCREEN_VARIANT": 9})
        tile = _run(P, rl, norm, den, {"RQSID_SCREEN_VARIANT": 1})
        _cache[name] = (P, v, glob, loc, pcs, tile)
    return _cache[name]


@pytest.mark.parametrize("name", list(CONFIGS))
def test_pc_screen_equals_tile_screen_array_for_array(name):
    P, _, _, _, pcs, tile = _case(name)
    print(f"{name}: rows {P['n']}, re-scored {pcs[2]} (producer/consumer) / {tile[2]} (per-tile)")
    assert (pcs[0] == tile[0]).all(), f"out_local differs on {int((pcs[0] != tile[0]).sum())} rows"
    assert (pcs[1] == tile[1]).all(), f"out_global differs on {int((pcs[1] != tile[1]).sum())} rows"
    assert pcs[2] == tile[2], "re-scored row counts differ"
    # every constructed tie has at least two candidates inside the bound: those rows are re-scored
    assert pcs[2] >= int(P["tie_rows"].sum())


@pytest.mark.parametrize("name", list(CONFIGS))
def test_pc_screen_final_ids_equal_exact_oracle(name):
    P, v, glob, loc, pcs, _ = _case(name)
    rl, norm = CONFIGS[name]
    ok = ~P["no_oracle"]
    bad = np.nonzero(ok & (pcs[1] != glob))[0]
    print(f"{name}: {len(bad)} rows differ from the exact oracle")
    if len(bad):
        assert norm and P["tie_rows"][bad].all(), f"{len(bad)} rows differ from the exact oracle outside the ties"
        nt = O.near_tie(v[bad], P["c"], pcs[1][bad], glob[bad])
        assert nt.all(), f"{int((~nt).sum())} rows differ from the exact oracle without a near tie"
    same = ok & (pcs[1] == glob)
    has_list = np.array([len(P["lists"][s]) > 0 for s in P["seg_of_pos"]])
    assert (pcs[0][same & has_list] == loc[same & has_list]).all(), "local ids differ from the list position"
    assert (pcs[0][same & ~has_list] == -1).all(), "a penalty segment's local id is -1"
    if not norm:  # exact ties: the lowest index wins
        s11 = np.nonzero(P["seg_of_pos"] == 11)[0]
        want = np.array([min(TIES[(i // 8) % len(TIES)]) for i in range(len(s11))]) + P["lists"][11][0]
        assert (pcs[1][s11] == want).all()
