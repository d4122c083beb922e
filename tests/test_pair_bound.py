"""The 2-term pairwise screen's bound (csrc/assign.hip, "Two-term pairwise screen") checked on the CPU against a
numpy model of the screen (tests/_pair_model.py: fp16 rounding emulated, the two accumulators summed by
tools/mfma_model.py's chain_dot).

For every row i and every ordered pair of candidates (k, b) the true float64 difference of the reference's scores,
S_k - S_b with S = |c|^2 - 2 r.c, must lie within the screen's P_k - P_b by no more than the threshold the
epilogue uses for that pair, Ax T[b][k] + A2 (|c_k| + |c_b|) + 2e-30 (the epilogue only tests b = argmin P; the
statement holds for every b).  Data: random centres and rows, plus centre pairs at relative distance 2^-6, 2^-12
and 2^-20, bitwise duplicates, rows at and between those centres, a zero row, all at the scales 1e-4, 1 and 1e4
(rows and centres alike), with and without the normalised row.  Well-separated unit centres must leave no row
ambiguous in the model."""
import numpy as np
import pytest

from tests import _pair_model as M

F32 = np.float32
D = 512


def _adversarial(seed, k, dim, scale):
    rng = np.random.default_rng(seed)
    c = (rng.standard_normal((k, dim)) / np.sqrt(dim)).astype(np.float64)
    for j, rel in ((0, 2.0 ** -6), (2, 2.0 ** -12), (4, 2.0 ** -20)):
        u = rng.standard_normal(dim)
        c[j + 1] = c[j] + rel * np.linalg.norm(c[j]) * u / np.linalg.norm(u)
    c[7] = c[6]
    c[k - 1] = c[6]
    c = (c * scale).astype(F32)
    c[7] = c[6]
    c[k - 1] = c[6]
    near = np.array([0, 1, 2, 3, 4, 5, 6, 7] * 3 + list(rng.integers(0, k, 16)))
    v = c[near].astype(np.float64) + scale * (0.3 / np.sqrt(dim)) * rng.standard_normal((len(near), dim))
    mid = np.stack([(c[j].astype(np.float64) + c[j + 1]) / 2 for j in (0, 2, 4, 6)])
    at = c[[0, 3, 5, 6]].astype(np.float64)
    v = np.concatenate([v, mid, at, np.zeros((1, dim))]).astype(F32)
    return c, v


def _check_pairs(v, tab, norm):
    R = M.screen(v, tab, norm=norm)
    S = M.true_scores(v, tab, norm)
    P, G, T, Ax = R["P"], R["G"], tab.T, R["Ax"]
    assert R["finite"].all()
    # [i, k, b]: (S_k - S_b) - (P_k - P_b) against Ax_i T[b][k] + G_ik + G_ib
    err = np.abs((S[:, :, None] - S[:, None, :]) - (P[:, :, None] - P[:, None, :]))
    bound = Ax[:, None, None] * T.T[None, :, :] + G[:, :, None] + G[:, None, :]
    worst = float((err / bound).max())
    return R, worst, int((err > bound).sum())


@pytest.mark.parametrize("norm", [False, True])
@pytest.mark.parametrize("scale", [1e-4, 1.0, 1e4])
def test_true_difference_within_bound(scale, norm):
    c, v = _adversarial(3, 40, D, scale)
    tab = M.Table(c)
    R, worst, bad = _check_pairs(v, tab, norm)
    print(f"scale {scale:g} norm {norm}: worst |true - screened| / bound = {worst:.3f}; ambiguous rows "
          f"{int((R['npass'] > 1).sum())} of {len(v)}")
    assert bad == 0, f"{bad} (row, k, b) triples outside the bound (worst ratio {worst:.3f})"
    # the argmin of the true scores (and every exact tie with it) is among the candidates each row keeps
    S = M.true_scores(v, tab, norm)
    best = S == S.min(1, keepdims=True)
    assert (R["keep"] | ~best).all()


@pytest.mark.parametrize("dim", [32, D])
def test_random_rows_within_bound(dim):
    rng = np.random.default_rng(5)
    c = (rng.standard_normal((128, dim)) / np.sqrt(dim)).astype(F32)
    v = (c[rng.integers(0, 128, 48)] + (0.3 / np.sqrt(dim)) * rng.standard_normal((48, dim))).astype(F32)
    for norm in (False, True):
        _, worst, bad = _check_pairs(v, M.Table(c), norm)
        print(f"dim {dim} norm {norm}: worst ratio {worst:.3f}")
        assert bad == 0


@pytest.mark.parametrize("norm", [False, True])
def test_well_separated_unit_centres_leave_no_row_ambiguous(norm):
    rng = np.random.default_rng(9)
    c = rng.standard_normal((128, D))
    c = (c / np.linalg.norm(c, axis=1, keepdims=True)).astype(F32)
    j = rng.integers(0, 128, 256)
    v = (c[j] + (0.1 / np.sqrt(D)) * rng.standard_normal((256, D))).astype(F32)
    R = M.screen(v, M.Table(c), norm=norm)
    assert (R["npass"] == 1).all(), f"{int((R['npass'] != 1).sum())} rows ambiguous"
    assert (R["b"] == j).all()


def test_pair_table_rounds_up_and_has_no_subnormals():
    c, _ = _adversarial(3, 40, D, 1.0)
    tab = M.Table(c)
    cd = c.astype(np.float64)
    dist = np.sqrt(((cd[:, None] - cd[None]) ** 2).sum(2))
    assert (tab.T * tab.unit >= dist).all()
    assert tab.T[6, 7] == 0 and tab.T[7, 39] == 0 and (np.diag(tab.T) == 0).all()
    assert ((tab.T == 0) | (tab.T >= 2.0 ** -14)).all()
    assert np.isfinite(tab.T).all()
    # no looser than one fp16 step (2^-10 relative) above the distance, except at the floor
    loose = tab.T * tab.unit > dist * (1 + 2.0 ** -9)
    assert (~loose | (tab.T <= 2.0 ** -14)).all()
    assert M.fp16_up(np.array([70000.0, np.nan]))[0] == np.inf


def test_chain_dot_stays_inside_the_accumulation_model():
    rng = np.random.default_rng(1)
    a = M.row_f16(rng.standard_normal((16, D)) * 2.0 ** rng.integers(-10, 3, (16, D)))
    b = M.centre_f16(rng.standard_normal((32, D)) * 2.0 ** rng.integers(-4, 13, (32, D)))
    got = M.mfma_model.chain_dot(a, b).astype(np.float64)
    err = np.abs(got - a @ b.T)
    lim = M.acc_rel(D) * np.linalg.norm(a, axis=1)[:, None] * np.linalg.norm(b, axis=1)[None, :]
    assert (err <= lim).all()
    assert err.max() > 0  # it does truncate
