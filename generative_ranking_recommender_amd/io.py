"""Input/output formats around the semantic-ID path.

* ``load_song_vectors`` — the Word2Vec CSV ``song_id,v1..vD`` without header written by
  src/common/train_word2vec.py:69-73, read with the rules of simplified_semantic_id_generator.py:38-76
  and train_semantic_ids.py:72-131 (rows with < 2 fields skipped, non-numeric rows skipped, rows of
  another dimension skipped, ValueError when nothing is left, values rounded to fp16 when any
  ``layer_clusters`` entry exceeds 512).  Native multi-threaded reader (``csrc/csv_loader.cpp``,
  include/rqsid_io.h); the Python-csv restatement it is checked against is ``oracle/csv_oracle.py``.
* ``write_semantic_ids`` — one ``json.dumps({"song_id": ..., "semantic_ids": [...]})`` line per song
  (simplified :368-385, train_semantic_ids.py:239-264), byte-identical to the reference.
* ``semantic_id_statistics`` / ``training_config`` (+ ``json_bytes``) — the side files
  training_statistics.json and training_config.json of train_semantic_ids.py:266-365, byte-identical
  (``generative_ranking_recommender_amd.train_semantic_ids.SemanticIDTrainer`` writes them).
"""
from __future__ import annotations

import csv
import ctypes
import json
import logging
import os
from typing import Dict, List, Sequence, Tuple

import numpy as np

from . import _lib

logger = logging.getLogger(__name__)


def load_song_vectors(path: str, embedding_dim: int, layer_clusters: Sequence[int] = (),
                      limit: int | None = None, n_threads: int = 0) -> Tuple[List[str], np.ndarray]:
    """Returns (song_ids, vectors): float16 when any layer_clusters > 512 (the reference's
    ``.half()``), float32 otherwise.  Parsed by the native multi-threaded reader
    (``librqsid_io.so``, include/rqsid_io.h); raises if the library is missing."""
    lib = _lib.load_io()
    h = ctypes.c_void_p()
    rc = lib.rqsid_csv_open(os.fsencode(path), int(embedding_dim), int(limit or 0), int(n_threads),
                            ctypes.byref(h))
    msg = lib.rqsid_io_last_error().decode(errors="replace")
    if rc == 1:
        raise FileNotFoundError(msg)
    if rc == -1:
        raise ValueError(msg)
    if rc not in (0, 2):
        raise RuntimeError(f"rqsid_csv_open failed ({rc}): {msg}")
    try:
        bad = lib.rqsid_csv_nonnumeric(h)
        if bad:
            logger.warning("Skipped %d rows due to non-numeric vector data.", bad)
        if rc == 2:
            raise ValueError(msg)
        n, nbytes = lib.rqsid_csv_rows(h), lib.rqsid_csv_id_bytes(h)
        half = any(k > 512 for k in layer_clusters)
        x = np.empty((n, embedding_dim), dtype=np.float16 if half else np.float32)
        ids = np.empty(max(nbytes, 1), dtype=np.uint8)
        off = np.empty(n + 1, dtype=np.int64)
        vp = ctypes.c_void_p
        _check_io(lib, lib.rqsid_csv_copy(h, None if half else vp(x.ctypes.data), vp(ids.ctypes.data),
                                          vp(off.ctypes.data)))
        if half:
            _check_io(lib, lib.rqsid_csv_copy_f16(h, vp(x.ctypes.data)))
    finally:
        lib.rqsid_csv_close(h)
    blob = ids.tobytes()
    song_ids = [blob[off[i]:off[i + 1]].decode("utf-8") for i in range(n)]
    return song_ids, x


def _check_io(lib, rc: int) -> None:
    if rc != 0:
        raise RuntimeError(f"librqsid_io failed ({rc}): {lib.rqsid_io_last_error().decode(errors='replace')}")


def write_song_vectors(path: str, song_ids: Sequence[str], vectors: np.ndarray) -> None:
    """The producer's format (train_word2vec.py:69-73): ``song_id,v1,...,vD`` with repr floats."""
    with open(path, "w", encoding="utf-8", newline="") as f:
        w = csv.writer(f)
        for sid, v in zip(song_ids, vectors):
            w.writerow([sid] + [repr(float(t)) for t in v])


def semantic_id_lines(song_ids: Sequence[str], ids: np.ndarray) -> bytes:
    return "".join(json.dumps({"song_id": s, "semantic_ids": [int(v) for v in row]}) + "\n"
                   for s, row in zip(song_ids, ids)).encode("utf-8")


def write_semantic_ids(path: str, semantic_ids: Dict[str, List[int]]) -> int:
    """Write the jsonl; returns the number of unique semantic IDs (the reference logs it)."""
    d = os.path.dirname(path)
    if d:
        os.makedirs(d, exist_ok=True)
    unique = set()
    with open(path, "w", encoding="utf-8") as f:
        for song_id, sid in semantic_ids.items():
            f.write(json.dumps({"song_id": song_id, "semantic_ids": sid}) + "\n")
            unique.add(tuple(sid))
    return len(unique)


def read_semantic_ids(path: str, levels: int = 3):
    """``(song_ids, int32 [N, levels])`` of a ``song_semantic_ids.jsonl``; an entry whose ``semantic_ids`` does not
    hold ``levels`` values is skipped, as the reference's SemanticIDTrie skips it (semantic_id_trie.py:61-63)."""
    song_ids, rows = [], []
    with open(path, "r", encoding="utf-8") as f:
        for line in f:
            if not line.strip():
                continue
            item = json.loads(line)
            ids = item["semantic_ids"]
            if len(ids) != levels:
                continue
            song_ids.append(item.get("song_id"))
            rows.append([int(v) for v in ids])
    return song_ids, np.asarray(rows, dtype=np.int32).reshape(-1, levels)


def semantic_id_statistics(semantic_ids: Dict[str, List[int]], need_clusters: Sequence[int]) -> Dict:
    """train_semantic_ids.py:266-310 _generate_statistics."""
    stats = {"total_songs": len(semantic_ids),
             "unique_semantic_ids": len(set(tuple(s) for s in semantic_ids.values())),
             "layer_statistics": []}
    for layer in range(len(need_clusters)):
        layer_ids = [s[layer] for s in semantic_ids.values()]
        counts = np.bincount(layer_ids)
        stats["layer_statistics"].append({
            "layer": layer + 1,
            "unique_clusters": len(set(layer_ids)),
            "expected_clusters": need_clusters[layer],
            "min_cluster_id": min(layer_ids),
            "max_cluster_id": max(layer_ids),
            "cluster_distribution": {"min": int(counts.min()), "max": int(counts.max()),
                                     "mean": float(counts.mean()), "std": float(counts.std())},
        })
    return stats


def training_config(config, use_test_config: bool) -> Dict:
    """train_semantic_ids.py:266-288 _save_config: the side file training_config.json (same keys, same
    order)."""
    return {
        "layer_clusters": config.layer_clusters,
        "need_clusters": config.need_clusters,
        "embedding_dim": config.embedding_dim,
        "group_dims": config.group_dims,
        "hierarchical_weights": config.hierarchical_weights,
        "iter_limit": config.iter_limit,
        "use_test_config": use_test_config,
    }


def json_bytes(obj) -> bytes:
    """The reference's side-file encoding: json.dump(obj, f, indent=2, ensure_ascii=False) in UTF-8."""
    return json.dumps(obj, indent=2, ensure_ascii=False).encode("utf-8")


def write_json(path: str, obj) -> None:
    with open(path, "wb") as f:
        f.write(json_bytes(obj))
