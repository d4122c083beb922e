"""The reference's training driver, src/semantic_id_generator/train_semantic_ids.py:35-365
(``SemanticIDTrainer``), on the MI355X path: CSV -> HierarchicalRQKMeans.train -> save_model ->
training_config.json -> song_semantic_ids.jsonl -> training_statistics.json, with the same file names,
directory layout, contents and byte encoding.

``config`` is any object with the attributes the reference's ``Config`` exposes to this class:
``output_dir``, ``model_dir``, ``data.song_vectors_file``, ``data.semantic_ids_file``, ``h_rqkmeans`` and
``h_rqkmeans_test`` (config.py:42-58, 106-115).  The argparse CLI (:368-434) is not mirrored.

Multi-GPU (``group`` set, one process per GPU): every rank reads the CSV, trains on its contiguous row
block (``HierarchicalRQKMeans(group=...)``), and the semantic IDs are gathered to rank 0,
which alone writes the model, the jsonl and the side files.
"""
from __future__ import annotations

import logging
import os
from pathlib import Path
from typing import Dict, List, Tuple

import numpy as np
import torch

from . import io as rq_io
from .hierarchical_rq_kmeans import HierarchicalRQKMeans

logger = logging.getLogger(__name__)


class SemanticIDTrainer:
    """train_semantic_ids.py:35-365."""

    def __init__(self, config, use_test_config: bool = False, device=None, group=None,
                 report_quantization: bool = False, report_margins: bool = False, report_beam: int = 0,
                 report_clusters: int = 0, report_neighbors: int = 0, report_collisions: bool = False,
                 dedup_token: bool = False, report_index: int = 0, report_trie: bool = False):
        self.config = config
        # opt-in: also write trie_report.json (SemanticIDTrie.report of the training rows' IDs: the reference's
        # get_statistics, the nodes per depth and the fan-out per depth).  Single process only: refused here
        self.report_trie = bool(report_trie)
        if group is not None and self.report_trie:
            raise NotImplementedError("SemanticIDTrainer: report_trie is single-process only (the multi-GPU cell "
                                      "index is not built)")
        # opt-in: also write collision_report.json (HierarchicalRQKMeans.collision_report of the training rows: the
        # figures of the reference's debug_collisions.py and analyze_semantic_ids.py); dedup_token also writes
        # song_semantic_ids_unique.jsonl, the training-consistent IDs with one more token (the row's rank among the
        # rows that share its ID) so that every song's tuple is distinct.  Single process only: refused here,
        # before any training.  song_semantic_ids.jsonl is written as ever
        self.report_collisions = bool(report_collisions)
        self.dedup_token = bool(dedup_token)
        if group is not None and (self.report_collisions or self.dedup_token):
            raise NotImplementedError("SemanticIDTrainer: report_collisions and dedup_token are single-process only "
                                      "(the multi-GPU cell index is not built)")
        # opt-in (a sample size): also write neighbor_report.json (HierarchicalRQKMeans.neighbor_quality of the
        # training rows: how many of a row's exact nearest rows share its ID prefix, per depth).  Single process
        # only: refused here, before any training
        self.report_neighbors = int(report_neighbors or 0)
        if group is not None and self.report_neighbors:
            raise NotImplementedError("SemanticIDTrainer: report_neighbors is single-process only (the multi-GPU "
                                      "neighbour report is not built)")
        # opt-in (a sample size): also write index_recall_report.json (HierarchicalRQKMeans.index_quality of the
        # training rows: what a search through the IDs finds of a row's exact nearest rows, per depth and number of
        # probed prefixes).  Single process only: refused here, before any training
        self.report_index = int(report_index or 0)
        if group is not None and self.report_index:
            raise NotImplementedError("SemanticIDTrainer: report_index is single-process only (the multi-GPU index "
                                      "search is not built)")
        # opt-in (a sample size, the reference's is 50000): also write cluster_quality_report.json
        # (HierarchicalRQKMeans.cluster_quality of the training rows: the three scores of the reference's
        # calculate_metrics.py per prefix depth).  Single process only: refused here, before any training
        self.report_clusters = int(report_clusters or 0)
        if group is not None and self.report_clusters:
            raise NotImplementedError("SemanticIDTrainer: report_clusters is single-process only (the multi-GPU "
                                      "cluster report is not built)")
        # opt-in (a beam width 1..8): also write beam_report.json (HierarchicalRQKMeans.beam_report of the training
        # rows: what a beam-search encode of that width would change and gain); the IDs written stay greedy
        self.report_beam = int(report_beam or 0)
        # opt-in: also write assignment_margin_report.json (HierarchicalRQKMeans.assignment_margins of the training
        # rows) next to the other side files
        self.report_margins = report_margins
        # opt-in: also write quantization_report.json (HierarchicalRQKMeans.quantization_error of the training
        # rows) next to training_statistics.json; the reference has no such file
        self.report_quantization = report_quantization
        self.use_test_config = use_test_config
        self.rqkmeans_config = config.h_rqkmeans_test if use_test_config else config.h_rqkmeans
        self.device = device
        self.group = group
        self.rank = 0
        if group is not None:
            import torch.distributed as dist
            self.rank = dist.get_rank(group)
        self.output_dir = Path(config.output_dir) / "semantic_id"
        self.model_dir = Path(config.model_dir) / "semantic_id"
        self.checkpoint_dir = self.output_dir / "checkpoints"
        if self.rank == 0:
            for d in (self.output_dir, self.model_dir, self.checkpoint_dir):
                d.mkdir(parents=True, exist_ok=True)

    def load_song_vectors(self, max_samples: int = None) -> Tuple[List[str], np.ndarray]:
        """:72-131 (native reader, the reference's skip rules and fp16 rule)."""
        path = self.config.data.song_vectors_file
        if not os.path.isfile(path):
            raise FileNotFoundError(f"Song vector file not found: {path}")
        ids, x = rq_io.load_song_vectors(path, self.rqkmeans_config.embedding_dim, self.rqkmeans_config.layer_clusters,
                                         limit=max_samples)
        logger.info("Successfully loaded %d song vectors", len(ids))
        return ids, x

    def train(self, resume: bool = True) -> Dict:
        """:133-207."""
        max_samples = 100000 if self.use_test_config else None
        song_ids, vectors = self.load_song_vectors(max_samples=max_samples)
        vectors_np = np.asarray(vectors, dtype=np.float32) if vectors.dtype != np.float32 else vectors
        # every rank reads the checkpoints on resume; only rank 0 writes them
        model = HierarchicalRQKMeans(config=self.rqkmeans_config, checkpoint_dir=str(self.checkpoint_dir),
                                     device=self.device, group=self.group)
        logger.info("Training status: %s", model.get_training_status())
        train_result = model.train(vectors_np, resume=resume)
        stats = None
        semantic_ids = None
        if self.rank == 0:
            model.save_model(str(self.model_dir))
            self._save_config(model)
            semantic_ids = self._generate_semantic_ids(song_ids, train_result)
            self._save_semantic_ids(semantic_ids)
            stats = self._generate_statistics(semantic_ids)
            self._save_statistics(stats)
        result = {"model": model, "semantic_ids": semantic_ids, "statistics": stats, "song_ids": song_ids}
        if self.report_quantization:
            # every rank takes part (sharded rows, all-reduced sums); fp16 rows cross to the device as they are
            report = model.quantization_error(vectors)
            if self.rank == 0:
                rq_io.write_json(str(self.output_dir / "quantization_report.json"), report)
            result["quantization_report"] = report
        if self.report_margins:
            margins = model.assignment_margins(vectors)  # every rank takes part, as above
            if self.rank == 0:
                rq_io.write_json(str(self.output_dir / "assignment_margin_report.json"), margins)
            result["assignment_margin_report"] = margins
        if self.report_beam:
            beam = model.beam_report(vectors, self.report_beam)  # every rank takes part, as above
            if self.rank == 0:
                rq_io.write_json(str(self.output_dir / "beam_report.json"), beam)
            result["beam_report"] = beam
        if self.report_clusters:
            clusters = model.cluster_quality(vectors, sample=self.report_clusters)
            rq_io.write_json(str(self.output_dir / "cluster_quality_report.json"), clusters)
            result["cluster_quality_report"] = clusters
        if self.report_neighbors:
            neighbors = model.neighbor_quality(vectors, sample=self.report_neighbors)
            rq_io.write_json(str(self.output_dir / "neighbor_report.json"), neighbors)
            result["neighbor_report"] = neighbors
        if self.report_index:
            index = model.index_quality(vectors, sample=self.report_index)
            rq_io.write_json(str(self.output_dir / "index_recall_report.json"), index)
            result["index_recall_report"] = index
        if self.report_collisions:
            collisions = model.collision_report(vectors)
            rq_io.write_json(str(self.output_dir / "collision_report.json"), collisions)
            result["collision_report"] = collisions
        if self.report_trie:
            trie = model.build_trie(vectors).report()
            rq_io.write_json(str(self.output_dir / "trie_report.json"), trie)
            result["trie_report"] = trie
        if self.dedup_token:
            # the trained IDs themselves (the tuples of song_semantic_ids.jsonl), each with its rank as one more token
            trained = np.stack([np.asarray(t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else t)
                                for t in train_result["cluster_ids"]], 1)
            unique = model.predict_unique(vectors, ids=trained)
            # the dict rule of _generate_semantic_ids: a song id repeated in the CSV keeps its last row's tuple
            unique_ids = {sid: [int(v) for v in row] for sid, row in zip(song_ids, unique)}
            path = Path(self.config.data.semantic_ids_file).with_name("song_semantic_ids_unique.jsonl")
            rq_io.write_semantic_ids(str(path), unique_ids)
            result["unique_semantic_ids"] = unique_ids
        return result

    def _generate_semantic_ids(self, song_ids: list, train_result: Dict) -> Dict:
        """:209-237 (one host copy per level instead of a per-element .item() loop; a song id repeated in
        the CSV keeps its last row's IDs, as the reference's dict assignment does)."""
        levels = [np.asarray(t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else t, dtype=np.int64)
                  for t in train_result["cluster_ids"]]
        ids = np.stack(levels, 1) if levels else np.zeros((len(song_ids), 0), dtype=np.int64)
        return {sid: [int(v) for v in row] for sid, row in zip(song_ids, ids)}

    def _save_semantic_ids(self, semantic_ids: Dict):
        """:239-264."""
        n_unique = rq_io.write_semantic_ids(self.config.data.semantic_ids_file, semantic_ids)
        logger.info("Saved %d total IDs, %d unique semantic IDs.", len(semantic_ids), n_unique)

    def _save_config(self, model: HierarchicalRQKMeans):
        """:266-288."""
        rq_io.write_json(str(self.output_dir / "training_config.json"),
                         rq_io.training_config(model.config, self.use_test_config))

    def _generate_statistics(self, semantic_ids: Dict) -> Dict:
        """:290-333."""
        return rq_io.semantic_id_statistics(semantic_ids, self.rqkmeans_config.need_clusters)

    def _save_statistics(self, stats: Dict):
        """:335-365."""
        rq_io.write_json(str(self.output_dir / "training_statistics.json"), stats)
