"""The 2-term pairwise screen (rqsid_assign_pair, screen_terms = 2; csrc/assign.hip "Two-term pairwise screen")
against the exact oracle, the 3-term screen and the numpy model of its bound (tests/_pair_model.py).

One problem per (dim, res_levels, normalise): dim 512 and 32 (the narrowest the screen takes), RL 1 and 2, with and
without the normalised row.  Four segments of 300 / 129 / 127 / 1 rows with lists of 128 / 100 / 33 / 128
candidates, reached through a row permutation (row_index).  Every list of the first three segments holds centre
pairs at relative distance 2^-6, 2^-12 and 2^-20 and two bitwise copies of one centre (left in the list: their
pair-table entries are 0); their rows lie near those centres, halfway between each pair (ties), on the parent
centre itself (zero first residual), and one row holds a NaN, one an Inf.

Checked on every row: the IDs equal oracle/rq_oracle.py's exact (fp64) argmin of the same residual chain (the NaN
and the Inf row: the fp64 argmin of sum (v - c)^2 itself, since the oracle's expanded form is inf - inf there) and
the IDs of screen_terms = 3; the re-scored row count is at most the model's count of rows whose bound keeps more
than one candidate plus the two non-finite rows, and at most the 1-term screen's count; rqsid_assign_plan_pair
reports the 2-term form for the call (so a fall-back to 3 terms cannot pass).  The model's count is its upper one:
the device's accumulators and the model's each lie within the accumulation allowance of the exact sums, so a
candidate whose margin is inside twice that allowance may fall either way on the device and is counted as kept
(tests/_pair_model.py keep_upper; the nominal count is printed beside it).  On well-separated unit centres the model
and the kernel both leave no row to the re-score."""
import numpy as np
import pytest
import torch

from generative_ranking_recommender_amd import ops
from oracle import rq_oracle as O
from tests import _pair_model as M

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
F32 = np.float32
SEGS = [(300, 128), (129, 100), (127, 33), (1, 128)]  # (rows, candidates)
CONFIGS = [(dim, rl, norm) for dim in (512, 32) for rl in (1, 2) for norm in (False, True)]


def gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _centres(rng, cnt, dim):
    c = (rng.standard_normal((cnt, dim)) / np.sqrt(dim)).astype(np.float64)
    for j, rel in ((0, 2.0 ** -6), (2, 2.0 ** -12), (4, 2.0 ** -20)):
        u = rng.standard_normal(dim)
        c[j + 1] = c[j] + rel * np.linalg.norm(c[j]) * u / np.linalg.norm(u)
    c = c.astype(F32)
    c[7] = c[6]
    c[cnt - 1] = c[6]
    return c


def _problem(dim, rl, norm, seed):
    rng = np.random.default_rng(seed)
    S = len(SEGS)
    ca = (0.05 * rng.standard_normal((S, dim)) * np.sqrt(512 / dim)).astype(F32)
    cb = (0.02 * rng.standard_normal((S, dim)) * np.sqrt(512 / dim)).astype(F32)  # |cb| ~ 0.45 < 1
    centres, lists, rows, zero_rows = [], [], [], []
    k0 = 0
    for s, (nr, cnt) in enumerate(SEGS):
        c = _centres(rng, cnt, dim)
        v = (c[rng.integers(0, cnt, nr)] + (0.3 / np.sqrt(dim)) * rng.standard_normal((nr, dim))).astype(F32)
        if nr >= 32:
            near = np.arange(8)
            v[:8] = c[near] + (0.05 / np.sqrt(dim)) * rng.standard_normal((8, dim))
            for i, j in enumerate((0, 2, 4, 6)):  # halfway between the two of each pair
                v[8 + i] = ((c[j].astype(np.float64) + c[j + 1]) / 2).astype(F32)
            v[12:16] = c[[1, 3, 5, 6]]
        a, b = ca[s], cb[s]
        if rl == 1:
            x = a + v
        elif not norm:
            x = a + b + v
        else:  # x - a = 3 (b + beta t) with |b + beta t| = 1: the normalised first residual minus b is beta t
            t = v.astype(np.float64) / np.linalg.norm(v.astype(np.float64), axis=1, keepdims=True)
            bt = t @ b.astype(np.float64)
            beta = -bt + np.sqrt(bt * bt - float(b.astype(np.float64) @ b.astype(np.float64)) + 1.0)
            x = a + 3.0 * (b + beta[:, None] * t)
        x = x.astype(F32)
        if nr >= 32:
            x[16] = a  # the row is its parent centre: zero first residual
            zero_rows.append(sum(n for n, _ in SEGS[:s]) + 16)
        centres.append(c)
        lists.append(np.arange(k0, k0 + cnt))
        rows.append(x)
        k0 += cnt
    x_seg = np.concatenate(rows)
    n = len(x_seg)
    x_seg[20, 5 % dim] = np.nan
    x_seg[21, 17 % dim] = np.inf
    nonfinite = np.zeros(n, bool)
    nonfinite[[20, 21]] = True
    seg_of_pos = np.repeat(np.arange(S), [nr for nr, _ in SEGS])
    off = np.concatenate([[0], np.cumsum([nr for nr, _ in SEGS])]).astype(np.int32)
    perm = rng.permutation(n)
    x = np.empty_like(x_seg)
    x[perm] = x_seg
    return dict(dim=dim, S=S, ca=ca, cb=cb, c=np.concatenate(centres), lists=lists, x=x, perm=perm, off=off,
                seg_of_pos=seg_of_pos, nonfinite=nonfinite, n=n, centres=centres)


def _chain(P, rl, norm):
    """By position in segment order: the oracle's vector v (normalised where norm), the kernel's vector before its
    own normalisation (u), den_in and the RL 2 bound's dr."""
    xs = P["x"][P["perm"]]
    s = P["seg_of_pos"]
    den = None
    with np.errstate(all="ignore"):
        if rl == 1:
            v = O.residual(xs, P["ca"], s, normalize=norm)
            u = (xs - P["ca"][s]).astype(F32)
        else:
            r1 = O.residual(xs, P["ca"], s, normalize=norm)
            r = (xs - P["ca"][s]).astype(F32)
            if norm:
                den = (np.sqrt((r.astype(np.float64) ** 2).sum(1)).astype(F32) + F32(1e-8)).astype(F32)
                r = (r * (F32(1.0) / den)[:, None]).astype(F32)  # the screen multiplies by the reciprocal
            v = O.residual(r1, P["cb"], s, normalize=norm)
            u = (r - P["cb"][s]).astype(F32)
    return v, u, den


def _model_count(P, u, rl, norm):
    """(upper, nominal) counts of the finite rows the model leaves with other than one candidate: nominal with
    chain_dot's accumulators as they are, upper also keeping every candidate whose margin is inside the distance
    by which the device's accumulators may differ from them (tests/_pair_model.py, keep_upper).  The device's
    count is checked against the upper one."""
    count, nominal = 0, 0
    for s in range(P["S"]):
        rows = np.nonzero((P["seg_of_pos"] == s) & ~P["nonfinite"])[0]
        us = u[rows]
        dr = None
        if rl == 2 and norm:
            nrm = np.sqrt((us.astype(np.float64) ** 2).sum(1))
            inv_den = 1.0 / (nrm + 1e-8)
            den_eps = (0.125 * P["dim"] + 3.0) * 5.97e-8
            dr = 4.0 * 2.39e-7 * (1.0 + nrm) * inv_den + 4.0 * 5.97e-8 + 1.01 * den_eps * nrm * inv_den
        R = M.screen(us, M.Table(P["centres"][s], scale_from=P["c"]), norm=norm, rl=rl, dr=dr)
        count += int((R["npass_upper"] != 1).sum())
        nominal += int((R["npass"] != 1).sum())
    return count, nominal


def _run(P, rl, norm, den, terms, with_pair=True):
    S, n = P["S"], P["n"]
    tr = ops.tile_rows()
    nr = np.diff(P["off"])
    toff = np.concatenate([[0], np.cumsum((nr + tr - 1) // tr)]).astype(np.int32)
    buckets = ops.Buckets(gpu(P["off"]), gpu(toff), gpu(P["perm"].astype(np.int32)), S, int(toff[-1]))
    cnt = np.array([len(l) for l in P["lists"]], np.int32)
    base = np.concatenate([[0], np.cumsum(cnt)[:-1]]).astype(np.int32)
    pc = ops.prepare_centers(gpu(P["c"]))
    if rl == 2:  # explicit lists
        cand = ops.Candidates(gpu(base), gpu(cnt), int(cnt.max()), gpu(np.concatenate(P["lists"]).astype(np.int32)))
        den_pos = None
        if norm:
            den_x = np.empty(n, F32)
            den_x[P["perm"]] = den
            den_pos = gpu(den_x)
        fr = ops.FusedResidual(2, norm, gpu(P["ca"]), None, gpu(P["cb"]), gpu(np.arange(S, dtype=np.int32)), den_in=den_pos)
    else:
        cand = ops.Candidates(gpu(base), gpu(cnt), int(cnt.max()))
        fr = ops.FusedResidual(1, norm, gpu(P["ca"]), None,
                               den_out=torch.empty(n, dtype=torch.float32, device=DEV) if norm else None)
    pair = ops.pair_table(pc, cand) if with_pair else None
    assert pair is not None or not with_pair
    ws = ops.AssignWorkspace(n, DEV)
    x = gpu(P["x"])
    planned = ops.assign_plan_pair(x, buckets, cand, fused=fr, screen_terms=terms, pair=pair)
    loc, glob = ops.assign(x, pc, buckets, cand, workspace=ws, fused=fr, screen_terms=terms, pair=pair)
    torch.cuda.synchronize()
    assert ws.error() == 0
    return loc.cpu().numpy()[P["perm"]], glob.cpu().numpy()[P["perm"]], ws.rescored(), planned


_cache = {}


def _case(cfg):
    if cfg not in _cache:
        dim, rl, norm = cfg
        P = _problem(dim, rl, norm, seed=7 + dim + 2 * rl + int(norm))
        v, u, den = _chain(P, rl, norm)
        with np.errstate(all="ignore"):
            glob = O.segmented_nearest(v, P["c"], P["seg_of_pos"], P["lists"], penalty="10000", exact=True)
            # the oracle expands |v|^2 - 2 v.c + |c|^2, which is inf - inf for a row holding an Inf; the two
            # non-finite rows take the fp64 argmin of the distance itself, sum (v - c)^2 (first index on ties)
            for i in np.nonzero(P["nonfinite"])[0]:
                lst = P["lists"][P["seg_of_pos"][i]]
                d = ((v[i].astype(np.float64)[None, :] - P["c"][lst].astype(np.float64)) ** 2).sum(1)
                glob[i] = lst[int(np.argmin(d))]
        runs = {t: _run(P, rl, norm, den, t) for t in (2, 0, 3, 1)}
        _cache[cfg] = (P, glob, _model_count(P, u, rl, norm), runs)
    return _cache[cfg]


@pytest.mark.parametrize("cfg", CONFIGS, ids=lambda c: f"d{c[0]}_rl{c[1]}_{'norm' if c[2] else 'raw'}")
def test_pair_screen_ids_counts_and_plan(cfg):
    P, glob, (model, nominal), runs = _case(cfg)
    two, auto, three, one = runs[2], runs[0], runs[3], runs[1]
    nf = int(P["nonfinite"].sum())
    print(f"{cfg}: rows {P['n']}; re-scored 2-term {two[2]}, auto {auto[2]}, 3-term {three[2]}, 1-term {one[2]}; "
          f"model {model} (nominal {nominal}) + {nf} non-finite")
    # the plan: 2 and auto take the 2-term pairwise form, 3 and 1 do not
    assert two[3] and auto[3] and not three[3] and not one[3]
    lst0 = np.array([P["lists"][s][0] for s in P["seg_of_pos"]])
    for name, r in (("2-term", two), ("auto", auto)):
        bad = np.nonzero(r[1] != glob)[0]
        assert len(bad) == 0, f"{name}: {len(bad)} rows differ from the exact oracle (first {bad[:5]})"
        assert (r[0] == r[1] - lst0).all(), f"{name}: local ids are not the list positions"
        assert (r[0] == three[0]).all() and (r[1] == three[1]).all(), f"{name}: IDs differ from screen_terms = 3"
    assert two[2] <= model + nf, f"re-scored {two[2]} rows, the model allows {model} + {nf}"
    assert two[2] <= one[2], f"re-scored {two[2]} rows, the 1-term screen {one[2]}"
    assert auto[2] == two[2]


def test_switch_and_missing_table_keep_three_terms(monkeypatch):
    P, glob, _, runs = _case(CONFIGS[0])
    dim, rl, norm = CONFIGS[0]
    _, _, den = _chain(P, rl, norm)
    monkeypatch.setenv("RQSID_NO_PAIR", "1")
    off = _run(P, rl, norm, den, 0)
    monkeypatch.delenv("RQSID_NO_PAIR")
    assert not off[3] and off[2] == runs[3][2] and (off[1] == runs[3][1]).all()
    none = _run(P, rl, norm, den, 0, with_pair=False)
    assert not none[3] and none[2] == runs[3][2] and (none[1] == glob).all()
    with pytest.raises(ValueError):
        _run(P, rl, norm, den, 2, with_pair=False)


def test_well_separated_centres_leave_nothing_to_the_rescore():
    rng = np.random.default_rng(9)
    dim, k, n = 512, 128, 384
    c = rng.standard_normal((k, dim))
    c = (c / np.linalg.norm(c, axis=1, keepdims=True)).astype(F32)
    ca = (0.05 * rng.standard_normal((1, dim))).astype(F32)
    j = rng.integers(0, k, n)
    v = (c[j] + (0.1 / np.sqrt(dim)) * rng.standard_normal((n, dim))).astype(F32)
    x = (ca[0] + v).astype(F32)
    u = (x - ca[0]).astype(F32)
    assert int((M.screen(u, M.Table(c))["npass"] != 1).sum()) == 0
    pc = ops.prepare_centers(gpu(c))
    cand = ops.contiguous_candidates(1, k, DEV)
    b = ops.single_segment(n, DEV)
    fr = ops.FusedResidual(1, False, gpu(ca))
    pair = ops.pair_table(pc, cand)
    ws = ops.AssignWorkspace(n, DEV)
    xg = gpu(x)
    assert ops.assign_plan_pair(xg, b, cand, fused=fr, screen_terms=2, pair=pair)
    loc, _ = ops.assign(xg, pc, b, cand, workspace=ws, fused=fr, screen_terms=2, pair=pair)
    torch.cuda.synchronize()
    assert ws.rescored() == 0
    assert (loc.cpu().numpy() == j).all()


def test_pair_table_matches_the_model():
    """The device table, entry for entry: the model's fp16 upper bounds in the screen's lane order."""
    rng = np.random.default_rng(4)
    dim = 64
    c = np.concatenate([_centres(rng, 33, dim), _centres(rng, 128, dim)])
    pc = ops.prepare_centers(gpu(c))
    cand = ops.Candidates(gpu(np.array([0, 33], np.int32)), gpu(np.array([33, 128], np.int32)), 128)
    t = ops.pair_table(pc, cand).cpu().numpy().view(np.float16).astype(np.float64).reshape(2, 128, 128)
    k = np.arange(128)
    pos = ((k >> 2) & 1) * 64 + (k >> 5) * 16 + (k & 3) + 4 * ((k & 31) >> 3)
    for s, (k0, cnt) in enumerate(((0, 33), (33, 128))):
        want = np.zeros((128, 128))
        want[:cnt, :cnt] = M.Table(c[k0:k0 + cnt], scale_from=c).T
        got = t[s][:, pos]
        assert (got == want).all(), f"segment {s}: {int((got != want).sum())} entries differ"
