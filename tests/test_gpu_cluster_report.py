"""cluster_report on the GPU against the fp64 oracle (tests/_cluster_oracle.py, itself pinned to sklearn): the exact
silhouette within the mean of the per-row derived bounds, Calinski-Harabasz and Davies-Bouldin within 1e-5 relative
(about 100 x the first-order fp32 roundings they inherit: the fp32 centroids and the fl32 per-row distances, 6e-8
each), the None rules, and the trainer's opt-in side file."""
import json
import os
import types

import numpy as np
import pytest
import torch

from generative_ranking_recommender_amd import cluster_report as CR
from generative_ranking_recommender_amd import io as rq_io
from generative_ranking_recommender_amd import synth
from generative_ranking_recommender_amd.encode import HIERARCHICAL_TRAIN, RQEncoder
from generative_ranking_recommender_amd.hierarchical_rq_kmeans import HierarchicalRQKMeansConfig
from tests import _cluster_oracle as CO

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
U = 2.0 ** -24
NEED = [4, 4, 8]
SAMPLE = 300


@pytest.fixture(scope="module")
def setup():
    cb = synth.encode_codebooks(seed=3, need=tuple(NEED), n_cand=40, d=64, pool_rows=4096)
    x = synth.small_mixture(4000, d=64, m=16, seed=9)
    enc = RQEncoder([torch.from_numpy(cb[k]) for k in ("c0", "c1", "c2")], NEED, match=torch.from_numpy(cb["match"]),
                    semantics=HIERARCHICAL_TRAIN, device=DEV)
    xd = torch.from_numpy(x).to(DEV)
    ids = enc.encode(xd)
    return enc, x, xd, ids, ids.cpu().numpy().astype(np.int64)


def _oracle(x, ids, radices, depth, rows, against):
    key = np.zeros(len(x), dtype=np.int64)
    for l in range(depth):
        key = key * radices[l] + ids[:, l]
    if against == "sample":
        x, key = x[rows], key[rows]
        rows = np.arange(len(rows))
    _, inv = np.unique(key, return_inverse=True)
    order, off = CO.group(inv)
    ref = CO.silhouette(x, order, off, x[rows], rows, inv[rows], dim_bound=x.shape[1])
    n_c, idx = ref["n_c"], np.arange(len(rows))
    da = ref["S_bound"][idx, inv[rows]] / np.maximum(n_c[inv[rows]] - 1, 1)
    db = ref["b_err"]
    big = np.maximum(da, db)
    ds = (da + db + big) / (np.maximum(ref["a"], ref["b"]) - big) + 2 * U  # the per-row bound of test_gpu_silhouette
    fin = np.isfinite(ref["s"])
    return dict(s=float(ref["s"][fin].mean()), s_bound=float(ds[fin].mean()), scored=int(fin.sum()),
                neg=float((ref["s"][fin] < 0).mean()), cs=CO.centroid_scores(x, inv))


@pytest.mark.parametrize("against", ["all", "sample"])
def test_report_matches_the_oracle_at_every_depth(setup, against):
    enc, x, xd, ids, ids_np = setup
    rep = CR.cluster_report(enc, xd, sample=SAMPLE, against=against)
    assert {k: rep[k] for k in ("rows", "sample", "seed", "against")} == dict(rows=4000, sample=SAMPLE, seed=0,
                                                                               against=against)
    rows = CR.sample_rows(len(x), SAMPLE, 0)
    radices = [pc.k for pc in enc.pcs]
    assert [d["depth"] for d in rep["depths"]] == [1, 2, 3]
    for d in rep["depths"]:
        ref = _oracle(x, ids_np, radices, d["depth"], rows, against)
        k, ch, db = ref["cs"]
        print(against, d, "oracle", ref)
        assert d["clusters"] == k and d["silhouette_scored"] == ref["scored"]
        assert abs(d["silhouette"] - ref["s"]) <= ref["s_bound"]
        assert abs(d["share_negative"] - ref["neg"]) <= 2.0 / SAMPLE  # a row within its bound of 0 may change side
        assert d["calinski_harabasz"] == pytest.approx(ch, rel=1e-5)
        assert d["davies_bouldin"] == pytest.approx(db, rel=1e-5)


def test_16bit_rows_score_their_widened_values(setup):
    enc, x, xd, ids, ids_np = setup
    x16 = xd.half()
    rep = CR.cluster_report(enc, x16, ids=ids, sample=SAMPLE, depths=[2])
    rows = CR.sample_rows(len(x), SAMPLE, 0)
    ref = _oracle(x16.float().cpu().numpy(), ids_np, [pc.k for pc in enc.pcs], 2, rows, "all")
    d = rep["depths"][0]
    assert abs(d["silhouette"] - ref["s"]) <= ref["s_bound"]
    assert d["calinski_harabasz"] == pytest.approx(ref["cs"][1], rel=1e-5)
    assert d["davies_bouldin"] == pytest.approx(ref["cs"][2], rel=1e-5)


def test_none_rules(setup):
    enc, x, xd, ids, ids_np = setup
    sub = xd[:SAMPLE].contiguous()
    q = torch.arange(SAMPLE, dtype=torch.int64, device=DEV)
    one = CR._depth_report(sub, torch.zeros(SAMPLE, dtype=torch.int64, device=DEV), q, 32768)
    assert one["clusters"] == 1 and one["silhouette"] is None and one["silhouette_scored"] == 0
    assert one["share_negative"] is None and one["calinski_harabasz"] is None and one["davies_bouldin"] is None
    own = CR._depth_report(sub, q.clone(), q, 32768)  # every row its own cluster: n <= K, every s = 0
    assert own["clusters"] == SAMPLE and own["silhouette"] == 0.0 and own["calinski_harabasz"] is None
    assert own["davies_bouldin"] == 0.0  # sklearn's rule when every intra-cluster distance is 0
    capped = CR.cluster_report(enc, xd, ids=ids, sample=SAMPLE, depths=[2], db_max_clusters=2)["depths"][0]
    assert capped["clusters"] > 2 and capped["davies_bouldin"] is None and capped["calinski_harabasz"] is not None
    with pytest.raises(NotImplementedError):
        CR.cluster_report(enc, xd, ids=ids, comm=object())
    with pytest.raises(ValueError):
        CR.cluster_report(enc, xd, ids=ids, against="everything")


TRAIN_CFG = dict(layer_clusters=[4, 8, 8], need_clusters=[4, 4, 4], embedding_dim=64, iter_limit=3)


def _trainer_cfg(root, csv_path):
    return types.SimpleNamespace(
        output_dir=os.path.join(root, "outputs"), model_dir=os.path.join(root, "models"),
        h_rqkmeans_test=HierarchicalRQKMeansConfig(**TRAIN_CFG), h_rqkmeans=None,
        data=types.SimpleNamespace(song_vectors_file=csv_path,
                                   semantic_ids_file=os.path.join(root, "outputs", "semantic_id",
                                                                  "song_semantic_ids.jsonl")))


def test_trainer_writes_the_cluster_report_only_when_asked(tmp_path):
    from generative_ranking_recommender_amd.train_semantic_ids import SemanticIDTrainer
    x = synth.small_mixture(600, d=64, m=16, seed=5)
    csv_path = str(tmp_path / "vec.csv")
    rq_io.write_song_vectors(csv_path, [f"song{i}" for i in range(len(x))], x)
    out = {}
    for name, kw in (("plain", {}), ("clusters", {"report_clusters": SAMPLE})):
        np.random.seed(7)
        torch.manual_seed(7)
        root = str(tmp_path / name)
        out[name] = (root, SemanticIDTrainer(_trainer_cfg(root, csv_path), use_test_config=True, device=DEV,
                                             **kw).train(resume=False))
    files = {n: sorted(os.listdir(os.path.join(r, "outputs", "semantic_id"))) for n, (r, _) in out.items()}
    assert files["clusters"] == sorted(files["plain"] + ["cluster_quality_report.json"])
    assert "cluster_quality_report" not in out["plain"][1]
    for rel in ("training_statistics.json", "training_config.json", "song_semantic_ids.jsonl"):
        a, b = (open(os.path.join(r, "outputs", "semantic_id", rel), "rb").read() for r, _ in out.values())
        assert a == b, rel
    with open(os.path.join(out["clusters"][0], "outputs", "semantic_id", "cluster_quality_report.json")) as f:
        written = json.load(f)
    assert written == out["clusters"][1]["cluster_quality_report"]
    assert written["rows"] == len(x) and written["sample"] == SAMPLE and written["against"] == "all"
    assert [d["depth"] for d in written["depths"]] == [1, 2, 3]
    for d in written["depths"]:
        assert set(d) == {"depth", "clusters", "silhouette", "silhouette_scored", "share_negative",
                          "calinski_harabasz", "davies_bouldin"}
        assert -1 <= d["silhouette"] <= 1
    # the multi-GPU form is refused in the constructor, before any training (the group is never touched)
    with pytest.raises(NotImplementedError):
        SemanticIDTrainer(_trainer_cfg(str(tmp_path / "g"), csv_path), use_test_config=True, device=DEV,
                          group=object(), report_clusters=SAMPLE)
