"""rqsid_row_knn's exactness argument, executable without a GPU (tests/_knn_model.py restates the kernel):
the interval e holds the exact value for both metrics, and the keep / fold / certify logic returns the brute-force
neighbours whatever the slack, on a fixture made of ties."""
import numpy as np
import pytest

from tests import _knn_model as M

F32 = np.float32


def test_fmaf_rounds_once():
    """The model's fmaf against exact rational arithmetic: no fp32 neighbour of the result is nearer to a b + c."""
    from fractions import Fraction
    rng = np.random.default_rng(0)
    a = np.concatenate([[1.0 + 2.0 ** -12], rng.normal(size=200)]).astype(F32)
    b = np.concatenate([[2.0 ** -12 - 2.0 ** -36], rng.normal(size=200)]).astype(F32)
    c = np.concatenate([[1.0], rng.normal(size=200) * 2.0 ** rng.integers(-30, 30, 200)]).astype(F32)
    got = M.fmaf(a, b, c)
    for x, y, z, g in zip(a, b, c, got):
        exact = Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z))
        lo, hi = np.nextafter(g, F32(-np.inf)), np.nextafter(g, F32(np.inf))
        err = abs(exact - Fraction(float(g)))
        assert err <= abs(exact - Fraction(float(lo))) and err <= abs(exact - Fraction(float(hi)))
    # the first case: a b + c = 1 + 2^-12 + 2^-24 - 2^-36 - 2^-48, just below the midpoint of two fp32 neighbours
    assert got[0] == F32(1.0 + 2.0 ** -12)


def _cases(dim, rng):
    q = rng.normal(size=(12, dim)).astype(F32)
    x = rng.normal(size=(40, dim)).astype(F32)
    yield "random", q, x
    # cancellation: x within a few ulps of q, where |q|^2 + |x|^2 - 2 q.x loses every leading digit
    near = (q[:, None, :] * (1 + rng.integers(-2, 3, (12, 3, dim)) * 2.0 ** -23)).reshape(-1, dim).astype(F32)
    yield "near-identical", q, np.concatenate([near, q])
    # norms spanning 2^-20 .. 2^20 on both sides
    yield "norms", (q * 2.0 ** rng.integers(-20, 21, (12, 1))).astype(F32), \
        (x * 2.0 ** rng.integers(-20, 21, (40, 1))).astype(F32)
    # one-signed rows: sum |q_i x_i| = |q.x|, the accumulation bound's worst direction
    yield "one-signed", np.abs(q), np.abs(x)


@pytest.mark.parametrize("metric", ["l2", "cosine"])
@pytest.mark.parametrize("dim", [32, 512, 1024])
def test_interval_holds(metric, dim):
    rng = np.random.default_rng(dim)
    for name, q, x in _cases(dim, rng):
        s, e = M.screen(q, x, metric)
        t = M.exact_keys(q, x, metric)
        assert np.isfinite(s).all() and np.isfinite(e).all(), name
        gap = np.abs(s.astype(np.float64) - t)
        assert (gap <= e).all(), (name, float((gap / e).max()))
        # ... and it is no blanket: the interval is within a few hundred of the error met on one-signed rows
        if name == "one-signed":
            assert (gap / e).max() > 1e-3, (name, float((gap / e).max()))


def test_fixture_t_is_made_of_ties():
    x = M.fixture_t()
    keys = M.exact_keys(x[:200], x, "l2")
    keys[np.arange(200), np.arange(200)] = np.inf
    srt = np.sort(keys, axis=1)
    assert (srt[:, 9] == srt[:, 10]).sum() >= 20       # a tie straddling place 10
    assert ((keys == srt[:, 9:10]).sum(1)).max() >= 40  # the 40 copies of row 7
    s, _ = M.screen(x[:200], x, "l2")
    assert (s.astype(np.float64) == M.exact_keys(x[:200], x, "l2")).all()  # every key exact in fp32 too


@pytest.mark.parametrize("metric", ["l2", "cosine"])
@pytest.mark.parametrize("slack", [0, 2, 8])
def test_keep_fold_certify_equals_brute_force(metric, slack):
    x = M.fixture_t()
    q = x[:200]
    k = 10
    s, e = M.screen(q, x, metric)
    keys = M.exact_keys(q, x, metric)
    eligible = np.ones(keys.shape, bool)
    eligible[np.arange(200), np.arange(200)] = False
    want, _ = M.rank(keys, eligible, k)
    order = np.random.default_rng(1).permutation(len(x))
    pairs = {}
    for chunk in (128, 512, 1536):
        for o in (None, order):
            got, pairs[chunk] = M.keep_fold_certify(s, e, keys, eligible, k, slack, chunk, o)
            assert (got == want).all(), (chunk, o is not None)
    if metric == "l2":
        assert pairs[1536] > 0  # the ties cannot be certified from a list: the all-rows pass is what ranks them
