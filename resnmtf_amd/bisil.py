"""The bisilhouette score of a biclustering (``bisil`` in a ``res_nmtf_inner`` result, ``R/obtain_bicl.r:189-199``;
the score the k sweep of ``apply_resnmtf`` ranks, ``R/main.r:291-312``): the host half of the definition.

The per-member silhouettes come from the device (``Engine.bisil`` -> ``resnmtf_bisil``, for sparse views
``Engine.bisil_sparse`` -> ``resnmtf_bisil_sparse``; ``csrc/resnmtf_bisil.hip.inc``); this module combines them.  The
definition restates the published score, since the source of ``bisilhouette::bisilhouette`` is
not available: parity with the R package is unpinned.  With bicluster l = (rows I_l, columns J_l), active when both
are non-empty:

- sigma_l = (mean of the row silhouettes over I_l + mean of the column silhouettes over J_l) / 2;
- a view's score = the mean of sigma_l over the active biclusters, 0 with fewer than two;
- ``bisil`` = 0 if the view scores sum to 0, else the mean of the non-zero view scores (``R/obtain_bicl.r:198-199``).
"""
from __future__ import annotations

from typing import Callable, Optional, Sequence

import numpy as np

from . import device_views

METRICS = {"euclidean": 0, "manhattan": 1, "cosine": 2}     # resnmtf_bisil's metric codes (R/utils.r:424-427)


def active(rc, cc) -> np.ndarray:
    """The biclusters with at least one row and one column."""
    return (np.asarray(rc).sum(axis=0) > 0) & (np.asarray(cc).sum(axis=0) > 0)


def view_score(rc, cc, row_sil, col_sil) -> float:
    """One view's score from its cluster matrices (n x k, m x k, 0 / 1) and its per-member silhouettes (same shapes)."""
    rc = np.asarray(rc, dtype=np.float64); cc = np.asarray(cc, dtype=np.float64)
    row_sil = np.asarray(row_sil, dtype=np.float64); col_sil = np.asarray(col_sil, dtype=np.float64)
    if rc.shape != row_sil.shape or cc.shape != col_sil.shape or rc.shape[1] != cc.shape[1]:
        raise ValueError("silhouettes must have the shapes of the cluster matrices")
    act = np.flatnonzero(active(rc, cc))
    if len(act) < 2:
        return 0.0
    sigma = [0.5 * (row_sil[rc[:, l] != 0, l].mean() + col_sil[cc[:, l] != 0, l].mean()) for l in act]
    return float(np.mean(sigma))


def overall(view_scores: Sequence[float]) -> float:
    """``ifelse(sum(bisil) == 0, 0, mean(bisil[bisil != 0]))`` (``R/obtain_bicl.r:198``)."""
    s = np.asarray(view_scores, dtype=np.float64)
    if s.size == 0 or s.sum() == 0:
        return 0.0
    return float(s[s != 0].mean())


def score(row_clusters, col_clusters, distance: str = "euclidean", *,
          sil: Optional[Callable] = None, engine=None, sparse_views: bool = False) -> float:
    """``bisil`` of a result's cluster matrices (one per view).  The silhouettes of view v come from
    ``sil(v, rc, cc, distance)`` -> ``(row_sil, col_sil)``; by default ``engine.bisil`` (an ``Engine`` that holds the
    views' data).  ``sil`` is also the stand-in hook for tests without a device.  ``sparse_views=True`` (with
    ``engine``): a view with ``engine.sparse[v]`` goes through ``engine.bisil_sparse`` (``resnmtf_bisil_sparse``), the
    others through ``engine.bisil``; by default every view goes through ``engine.bisil``, which refuses a sparse one.
    A view whose two cluster matrices are ``torch`` tensors on the engine's GPU is scored there instead
    (``engine.bisil_device(..., silhouettes=False)``: the silhouettes and their combination stay on the device, dense
    and sparse views alike, and the returned score is ``view_score`` of them bit for bit); one tensor on the device
    paired with a host matrix is a ``ValueError``.  ``sparse_views`` keeps its meaning for host matrices only."""
    if distance not in METRICS:
        raise ValueError("distance must be one of 'euclidean', 'manhattan' or 'cosine'.")
    if len(row_clusters) != len(col_clusters):
        raise ValueError("row_clusters and col_clusters must hold one matrix per view")
    if sil is None:
        if engine is None:
            raise ValueError("pass engine (an Engine holding the views' data) or sil")
        sil = engine.bisil
        if sparse_views:
            def sil(v, rc, cc, distance):
                return (engine.bisil_sparse if engine.sparse[v] else engine.bisil)(v, rc, cc, distance)
    scores = []
    for v, (rc, cc) in enumerate(zip(row_clusters, col_clusters)):
        # both matrices tensors on the engine's GPU: scored and combined there, nothing is downloaded but the score
        if engine is not None and device_views.cluster_route(rc, cc, getattr(engine, "device_id", 0), f"view {v}"):
            scores.append(engine.bisil_device(v, rc, cc, distance, silhouettes=False)[2])
            continue
        rs, cs = sil(v, rc, cc, distance)
        scores.append(view_score(rc, cc, rs, cs))
    return overall(scores)
