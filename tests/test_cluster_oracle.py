"""tests/_cluster_oracle.py equals the functions the reference's calculate_metrics.py calls (sklearn's
silhouette_samples, calinski_harabasz_score, davies_bouldin_score), and the host-side pieces of cluster_report
(prefix keys, sampling, the None rules) do what they say.  No GPU.

Tolerance 1e-6 absolute / 1e-9 relative: sklearn expands |x - y|^2 in fp64, which differed from the direct
differences by 2e-8 on data like this."""
import numpy as np
import pytest
import torch

from generative_ranking_recommender_amd import cluster_report as CR
from tests import _cluster_oracle as CO


@pytest.fixture(scope="module")
def blobs():
    rng = np.random.default_rng(5)
    centres = rng.standard_normal((6, 32))
    lab = rng.integers(0, 6, 600)
    x = (centres[lab] + 0.8 * rng.standard_normal((600, 32))).astype(np.float32)
    lab[599] = 6             # a singleton cluster
    x[11] = x[10]            # a bitwise duplicate pair, in one cluster
    lab[11] = lab[10]
    return x, lab


def test_oracle_equals_sklearn(blobs):
    metrics = pytest.importorskip("sklearn.metrics")
    x, lab = blobs
    order, off = CO.group(lab)
    rows = np.arange(len(x))
    ref = CO.silhouette(x, order, off, x, rows, lab)
    want = metrics.silhouette_samples(x.astype(np.float64), lab)
    np.testing.assert_allclose(ref["s"], want, rtol=1e-9, atol=1e-6)
    assert ref["s"][599] == 0 and want[599] == 0
    k, ch, db = CO.centroid_scores(x, lab)
    assert k == 7
    np.testing.assert_allclose(ch, metrics.calinski_harabasz_score(x.astype(np.float64), lab), rtol=1e-9, atol=1e-6)
    np.testing.assert_allclose(db, metrics.davies_bouldin_score(x.astype(np.float64), lab), rtol=1e-9, atol=1e-6)


def test_oracle_conventions(blobs):
    x, lab = blobs
    order, off = CO.group(lab, n_clusters=9)  # clusters 7 and 8 are empty
    q = x[:5]
    with_self = CO.silhouette(x, order, off, q, np.arange(5), lab[:5])
    without = CO.silhouette(x, order, off, q, None, lab[:5])
    n_o = with_self["n_c"][lab[:5]]
    np.testing.assert_allclose(with_self["a"] * (n_o - 1), without["a"] * n_o, rtol=1e-12)  # d(i, i) = 0 exactly here
    assert np.array_equal(with_self["b_seg"], without["b_seg"]) and (with_self["b_seg"] < 7).all()
    none = CO.silhouette(x, order, off, q, None, None)  # no own cluster: a = 0, every cluster competes
    assert (none["a"] == 0).all() and (none["b"] <= with_self["b"]).all()
    alone = CO.silhouette(x[:3], None, np.array([0, 3]), x[:2], np.arange(2), np.zeros(2, dtype=int))
    assert np.isnan(alone["s"]).all() and (alone["b_seg"] == -1).all() and np.isinf(alone["b"]).all()


def test_prefix_keys_and_sampling():
    ids = torch.tensor([[1, 2, 3], [0, 5, 1], [1, 2, 4]], dtype=torch.int32)
    assert CR.prefix_keys(ids, [4, 8, 16], 1).tolist() == [1, 0, 1]
    assert CR.prefix_keys(ids, [4, 8, 16], 2).tolist() == [10, 5, 10]
    assert CR.prefix_keys(ids, [4, 8, 16], 3).tolist() == [163, 81, 164]
    assert CR.prefix_keys(ids, [4, 8, 16], 3).dtype == torch.int64
    rows = CR.sample_rows(1000, 50, 3)
    assert np.array_equal(rows, np.sort(np.random.default_rng(3).choice(1000, 50, replace=False)))
    assert len(np.unique(rows)) == 50
    assert np.array_equal(CR.sample_rows(20, 50, 0), np.arange(20))  # a sample larger than the rows: every row


def test_none_rules_of_the_assembly():
    assert CR.centroid_scores(1, 100, 0.0, 5.0, None, 32768) == (None, None)
    assert CR.centroid_scores(100, 100, 3.0, 0.0, 0.0, 32768) == (None, 0.0)        # n <= K
    assert CR.centroid_scores(4, 100, 6.0, 12.0, 0.7, 3) == ((6.0 / 3) / (12.0 / 96), None)  # K > db_max_clusters
    assert CR.centroid_scores(4, 100, 6.0, 0.0, 0.7, 8) == (1.0, 0.7)               # sklearn: W = 0 -> 1
    assert CR.silhouette_summary(np.array([np.nan, np.nan], dtype=np.float32)) == {
        "silhouette": None, "silhouette_scored": 0, "share_negative": None}
    got = CR.silhouette_summary(np.array([0.5, -0.25, np.nan, 0.0], dtype=np.float32))
    assert got == {"silhouette": 0.25 / 3, "silhouette_scored": 3, "share_negative": 1 / 3}
