"""Plain fp64 NumPy restatement of the bisilhouette definition, written from its text: the
yardstick of resnmtf_bisil and ``resnmtf_amd.bisil``.  Loops follow the definition literally; nothing is shared with
the package.  ``side_silhouettes_allpairs`` states the same definition a second time by full distance matrices, for the
shapes the loops do not scale to; tests/test_gpu_bisil_forms.py holds the two together."""
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


def pairwise(a, b, metric):
    """The |a| x |b| fp64 distance matrix between the rows of ``a`` and of ``b`` (points x features), accumulated one
    feature at a time."""
    a = np.asarray(a, dtype=np.float64); b = np.asarray(b, dtype=np.float64)
    d = np.zeros((a.shape[0], b.shape[0]))
    if metric == "euclidean":
        for f in range(a.shape[1]):
            d += (a[:, f, None] - b[None, :, f]) ** 2
        return np.sqrt(d)
    if metric == "manhattan":
        for f in range(a.shape[1]):
            d += np.abs(a[:, f, None] - b[None, :, f])
        return d
    if metric != "cosine":
        raise ValueError(metric)
    na, nb = np.zeros(a.shape[0]), np.zeros(b.shape[0])
    for f in range(a.shape[1]):
        d += a[:, f, None] * b[None, :, f]
        na += a[:, f] ** 2
        nb += b[:, f] ** 2
    za, zb = (na == 0.0)[:, None], (nb == 0.0)[None, :]
    with np.errstate(divide="ignore", invalid="ignore"):
        d = 1.0 - d / (np.sqrt(na)[:, None] * np.sqrt(nb)[None, :])
    return np.where(za & zb, 0.0, np.where(za | zb, 1.0, d))


def side_silhouettes_allpairs(x, members, features, metric, block=512):
    """``side_silhouettes`` stated a second time, from DESIGN.md section 13 and not from the loops above: per active
    bicluster k the full distance matrix from I_k (in row blocks) to U, the union of the active biclusters' members, on
    J_k; the diagonal leaves with its member; a, b and s by masked means over the 0 / 1 membership of U.  It shares
    nothing with ``member_silhouette`` but the definition, scales to thousands of points, and sums in another order."""
    K = len(members)
    out = np.zeros((x.shape[0], K))
    act = [l for l in range(K) if len(members[l]) > 0 and len(features[l]) > 0]
    if not act:
        return out
    union = np.array(sorted(set().union(*[set(int(p) for p in members[l]) for l in act])), dtype=np.int64)
    pos = {int(p): u for u, p in enumerate(union)}
    memb = np.zeros((union.size, K))
    for l in act:
        memb[[pos[int(p)] for p in members[l]], l] = 1.0
    for k in act:
        sub = np.asarray(x[np.ix_(union, np.asarray(features[k], dtype=np.int64))], dtype=np.float64)
        own = np.array([pos[int(p)] for p in members[k]], dtype=np.int64)
        others = np.array([l for l in act if l != k], dtype=np.int64)
        for r0 in range(0, own.size, block):
            me = own[r0:r0 + block]
            d = pairwise(sub[me], sub, metric)
            d[np.arange(me.size), me] = 0.0                          # a point is no neighbour of itself
            count = memb.sum(0)[None, :] - memb[me]                  # |I_l \ {i}|
            with np.errstate(divide="ignore", invalid="ignore"):
                mean = np.where(count > 0, (d @ memb) / count, np.inf)
            a = mean[:, k]
            b = mean[:, others].min(axis=1) if others.size else np.full(me.size, np.inf)
            mx = np.maximum(a, b)
            ok = np.isfinite(a) & np.isfinite(b) & (mx != 0.0)
            with np.errstate(divide="ignore", invalid="ignore"):
                out[union[me], k] = np.where(ok, (b - a) / mx, 0.0)
    return out


def silhouettes_allpairs(x, rc, cc, metric="euclidean"):
    """``silhouettes`` through ``side_silhouettes_allpairs``."""
    x = np.asarray(x, dtype=np.float64)
    rows, cols = index_sets(rc, cc)
    return side_silhouettes_allpairs(x, rows, cols, metric), side_silhouettes_allpairs(x.T, cols, rows, metric)


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
