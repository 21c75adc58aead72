"""Plain fp64 NumPy restatement of the bisilhouette definition, written from its text: the
yardstick of resnmtf_bisil and ``resnmtf_amd.bisil``.  Loops follow the definition literally; nothing is shared with
the package."""
from __future__ import annotations

import numpy as np


def dist(x, y, metric):
    x = np.asarray(x, dtype=np.float64); y = np.asarray(y, dtype=np.float64)
    if metric == "euclidean":
        return float(np.sqrt(np.sum((x - y) ** 2)))
    if metric == "manhattan":
        return float(np.sum(np.abs(x - y)))
    if metric == "cosine":
        nx, ny = float(np.dot(x, x)), float(np.dot(y, y))
        if nx == 0.0 and ny == 0.0:
            return 0.0
        if nx == 0.0 or ny == 0.0:
            return 1.0
        return float(1.0 - np.dot(x, y) / (np.sqrt(nx) * np.sqrt(ny)))
    raise ValueError(metric)


def distances_from(x, i, feats, metric):
    """Distances from point ``i`` to every point of ``x`` (points x features), on the features ``feats``."""
    sub = np.asarray(x[:, feats], dtype=np.float64)
    xi = sub[i]
    if metric == "euclidean":
        return np.sqrt(((sub - xi) ** 2).sum(1))
    if metric == "manhattan":
        return np.abs(sub - xi).sum(1)
    nrm, ni = (sub * sub).sum(1), float(xi @ xi)
    with np.errstate(divide="ignore", invalid="ignore"):
        d = 1.0 - (sub @ xi) / (np.sqrt(nrm) * np.sqrt(ni))
    d = np.where((nrm == 0.0) != (ni == 0.0), 1.0, d)      # exactly one norm 0
    return np.where((nrm == 0.0) & (ni == 0.0), 0.0, d)    # both 0


def member_silhouette(x, members, features, k, i, metric):
    """s of member ``i`` of bicluster ``k`` on one side (``x`` points x features; ``members[l]`` / ``features[l]``
    the index sets of bicluster l on this side / the other)."""
    K = len(members)
    act = [l for l in range(K) if len(members[l]) > 0 and len(features[l]) > 0]
    d = distances_from(x, i, features[k], metric)
    own = [p for p in members[k] if p != i]
    if not own:
        return 0.0                                         # |I_k| = 1
    a = d[own].mean()
    bs = []
    for l in act:
        if l == k:
            continue
        other = [p for p in members[l] if p != i]
        if other:                                          # empty sets are skipped
            bs.append(d[other].mean())
    if not bs:
        return 0.0
    b = min(bs)
    mx = max(a, b)
    return 0.0 if mx == 0.0 else float((b - a) / mx)


def side_silhouettes(x, members, features, metric):
    """Silhouettes of one side: n_points x K, 0 at non-members and inactive biclusters."""
    K = len(members)
    out = np.zeros((x.shape[0], K))
    for k in range(K):
        if len(members[k]) == 0 or len(features[k]) == 0:
            continue
        for i in members[k]:
            out[i, k] = member_silhouette(x, members, features, k, i, metric)
    return out


def index_sets(rc, cc):
    K = rc.shape[1]
    return [list(np.flatnonzero(rc[:, k])) for k in range(K)], [list(np.flatnonzero(cc[:, k])) for k in range(K)]


def silhouettes(x, rc, cc, metric="euclidean"):
    """(row_sil, col_sil) of one view: ``x`` n x m, ``rc`` n x K and ``cc`` m x K 0 / 1."""
    x = np.asarray(x, dtype=np.float64)
    rows, cols = index_sets(rc, cc)
    return side_silhouettes(x, rows, cols, metric), side_silhouettes(x.T, cols, rows, metric)


def view_score(rc, cc, row_sil, col_sil):
    K = rc.shape[1]
    act = [k for k in range(K) if rc[:, k].sum() > 0 and cc[:, k].sum() > 0]
    if len(act) < 2:
        return 0.0
    sig = [0.5 * (row_sil[rc[:, k] == 1, k].mean() + col_sil[cc[:, k] == 1, k].mean()) for k in act]
    return float(np.mean(sig))


def bisil(views, rcs, ccs, metric="euclidean"):
    scores = []
    for x, rc, cc in zip(views, rcs, ccs):
        rs, cs = silhouettes(x, rc, cc, metric)
        scores.append(view_score(rc, cc, rs, cs))
    scores = np.asarray(scores)
    if scores.sum() == 0:
        return 0.0
    return float(scores[scores != 0].mean())
