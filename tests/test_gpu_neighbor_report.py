"""neighbor_report and neighbors_in_cluster on the GPU: every field against a numpy restatement computed from the
fp64 brute-force neighbours (tests/_knn_model.py) and the IDs; the reference's Evaluator.find_neighbors arithmetic
restated for the restricted search; the trainer's side file."""
import json
import os
import types

import numpy as np
import pytest
import torch

from generative_ranking_recommender_amd import io as rq_io
from generative_ranking_recommender_amd import neighbor_report as NR
from generative_ranking_recommender_amd import synth
from generative_ranking_recommender_amd.cluster_report import sample_rows
from generative_ranking_recommender_amd.encode import HIERARCHICAL_TRAIN, RQEncoder
from generative_ranking_recommender_amd.hierarchical_rq_kmeans import HierarchicalRQKMeansConfig
from tests import _knn_model as M

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
NEED = [8, 8, 16]
SAMPLE = 300
K = 10


@pytest.fixture(scope="module")
def setup():
    cb = synth.encode_codebooks(seed=3, need=tuple(NEED), n_cand=40, d=64, pool_rows=4096)
    x = synth.small_mixture(4000, d=64, m=16, seed=9)
    enc = RQEncoder([torch.from_numpy(cb[k]) for k in ("c0", "c1", "c2")], NEED, match=torch.from_numpy(cb["match"]),
                    semantics=HIERARCHICAL_TRAIN, device=DEV)
    xd = torch.from_numpy(x).to(DEV)
    ids = enc.encode(xd)
    return enc, x, xd, ids, ids.cpu().numpy().astype(np.int64)


def _keys(ids, radices, depth):
    key = np.zeros(len(ids), dtype=np.int64)
    for l in range(depth):
        key = key * radices[l] + ids[:, l]
    return key


@pytest.mark.parametrize("metric", ["cosine", "l2"])
def test_every_field_against_the_restatement(setup, metric):
    enc, x, xd, ids, ids_np = setup
    rep = NR.neighbor_report(enc, xd, ids=ids, sample=SAMPLE, k=K, metric=metric)
    rows = sample_rows(len(x), SAMPLE, 0)
    nbr, val = M.brute_force(x[rows], x, K, metric, query_self=rows)
    assert (nbr >= 0).all()
    assert {k: rep[k] for k in ("rows", "sample", "seed", "k", "metric")} == dict(rows=4000, sample=SAMPLE, seed=0,
                                                                                 k=K, metric=metric)
    # (the values are fl32 of fp64 keys summed in another order: one fp32 ulp, as in test_gpu_knn)
    assert rep["mean_neighbor_value"] == pytest.approx(val.astype(np.float64).mean(0).tolist(), rel=2.0 ** -23)
    assert set(rep["counters"]) == {"from_lists", "all_rows_pairs", "non_finite_queries"}
    assert rep["counters"]["non_finite_queries"] == 0
    assert rep["counters"]["from_lists"] + rep["counters"]["all_rows_pairs"] >= 1
    radices = [pc.k for pc in enc.pcs]
    assert [d["depth"] for d in rep["depths"]] == [1, 2, 3]
    for d in rep["depths"]:
        key = _keys(ids_np, radices, d["depth"])
        shared = (key[nbr] == key[rows][:, None]).sum(1)
        want = {"depth": d["depth"], "clusters": len(np.unique(key)), "recall": float(shared.sum()) / (SAMPLE * K),
                "all_shared": float((shared == K).sum()) / SAMPLE, "none_shared": float((shared == 0).sum()) / SAMPLE}
        assert d == want
    recall = [d["recall"] for d in rep["depths"]]
    assert recall == sorted(recall, reverse=True) and 0 < recall[0] <= 1  # a longer prefix is shared by fewer
    only = NR.neighbor_report(enc, xd, ids=ids, sample=SAMPLE, k=K, metric=metric, depths=[2])
    assert only["depths"] == [rep["depths"][1]]


def test_refusals(setup):
    enc, x, xd, ids, ids_np = setup
    with pytest.raises(NotImplementedError):
        NR.neighbor_report(enc, xd, ids=ids, comm=object())
    with pytest.raises(ValueError):
        NR.neighbor_report(enc, xd, ids=ids, depths=[4])
    with pytest.raises(ValueError):
        NR.neighbors_in_cluster(xd, ids, [pc.k for pc in enc.pcs], [1, 2], depth=0)


def test_neighbors_in_cluster_is_find_neighbors(setup):
    """evaluate_semantic_ids.py:99-127 restated: cosine of the normalised fp32 vectors, the other rows of the level-1
    cluster, sorted descending, the first top_n."""
    enc, x, xd, ids, ids_np = setup
    rows = np.random.default_rng(4).choice(len(x), 20, replace=False)  # (not sorted: the caller's order comes back)
    got_r, got_v = NR.neighbors_in_cluster(xd, ids, [pc.k for pc in enc.pcs], rows, top_n=10, depth=1)
    got_r, got_v = got_r.cpu().numpy(), got_v.cpu().numpy()
    for i, r in enumerate(rows):
        target = x[r] / np.linalg.norm(x[r])
        sims = [(j, np.dot(target, x[j] / np.linalg.norm(x[j])))
                for j in np.flatnonzero(ids_np[:, 0] == ids_np[r, 0]) if j != r]
        sims.sort(key=lambda p: p[1], reverse=True)
        top = sims[:10]
        assert len(top) == 10
        assert got_r[i].tolist() == [j for j, _ in top]
        assert np.abs(got_v[i] - np.array([s for _, s in top], np.float64)).max() <= 1e-6
    # depth 2 stays inside the longer prefix
    r2, _ = NR.neighbors_in_cluster(xd, ids, [pc.k for pc in enc.pcs], rows, top_n=5, depth=2)
    r2 = r2.cpu().numpy()
    same = (ids_np[np.maximum(r2, 0), :2] == ids_np[rows][:, None, :2]).all(-1)
    assert (same | (r2 < 0)).all()


TRAIN_CFG = dict(layer_clusters=[4, 8, 8], need_clusters=[4, 4, 4], embedding_dim=64, iter_limit=3)


def _trainer_cfg(root, csv_path):
    return types.SimpleNamespace(
        output_dir=os.path.join(root, "outputs"), model_dir=os.path.join(root, "models"),
        h_rqkmeans_test=HierarchicalRQKMeansConfig(**TRAIN_CFG), h_rqkmeans=None,
        data=types.SimpleNamespace(song_vectors_file=csv_path,
                                   semantic_ids_file=os.path.join(root, "outputs", "semantic_id",
                                                                  "song_semantic_ids.jsonl")))


def test_trainer_writes_the_neighbor_report(tmp_path):
    from generative_ranking_recommender_amd.train_semantic_ids import SemanticIDTrainer
    x = synth.small_mixture(600, d=64, m=16, seed=5)
    csv_path = str(tmp_path / "vec.csv")
    rq_io.write_song_vectors(csv_path, [f"song{i}" for i in range(len(x))], x)
    np.random.seed(7)
    torch.manual_seed(7)
    root = str(tmp_path / "run")
    result = SemanticIDTrainer(_trainer_cfg(root, csv_path), use_test_config=True, device=DEV,
                               report_neighbors=200).train(resume=False)
    with open(os.path.join(root, "outputs", "semantic_id", "neighbor_report.json")) as f:
        written = json.load(f)
    assert written == result["neighbor_report"]
    assert written["rows"] == len(x) and written["sample"] == 200 and written["k"] == 10
    assert written["metric"] == "cosine" and [d["depth"] for d in written["depths"]] == [1, 2, 3]
    for d in written["depths"]:
        assert set(d) == {"depth", "clusters", "recall", "all_shared", "none_shared"}
        assert 0 <= d["recall"] <= 1
    # the multi-GPU form is refused in the constructor, before any training (the group is never touched)
    with pytest.raises(NotImplementedError):
        SemanticIDTrainer(_trainer_cfg(str(tmp_path / "g"), csv_path), use_test_config=True, device=DEV,
                          group=object(), report_neighbors=200)
