"""Literal restatements of the reference's relevance scoring (test infrastructure).

``relevance_sets`` follows ``relevance_results`` / ``jaccard_main`` (``R/stability_analysis.r:16-67``) with
``cart_prod`` / ``jaccard_func`` (``R/utils.r:117-145``) word for word: biclusters as Python sets of (row, col)
pairs.  ``relevance_counts`` is the closed integer form the device kernel evaluates; both divide the same two
integers once in fp64, so they agree bitwise.
"""
from __future__ import annotations

import numpy as np


def _members(col) -> list:
    return [i for i, x in enumerate(col) if x == 1]


def cart_prod(a, b):
    """R/utils.r:133-145 (NULL for an empty side)."""
    if len(a) == 0 or len(b) == 0:
        return set()
    return {(x, y) for x in a for y in b}


def jaccard_func(a: set, b: set) -> float:
    """R/utils.r:117-126."""
    inter = len(a & b)
    union = len(a) + len(b) - inter
    return 0.0 if union == 0 else inter / union


def relevance_sets(row_c, col_c, true_r, true_c) -> np.ndarray:
    """relevance_results (R/stability_analysis.r:45-67); the scalar edge returns broadcast over the k columns."""
    row_c, col_c, true_r, true_c = (np.asarray(a) for a in (row_c, col_c, true_r, true_c))
    m, n = row_c.shape[1], true_r.shape[1]
    m_0 = int((row_c.sum(axis=0) != 0).sum())
    n_0 = int((true_r.sum(axis=0) != 0).sum())
    if (m_0 == 0 and n_0 != 0) or (n_0 == 0 and m_0 != 0):
        return np.zeros(n)
    if m_0 == 0 and n_0 == 0:
        return np.ones(n)
    jac = np.zeros((m, n))
    for i in range(m):
        m_i = cart_prod(_members(row_c[:, i]), _members(col_c[:, i]))
        for j in range(n):
            m_j = cart_prod(_members(true_r[:, j]), _members(true_c[:, j]))
            jac[i, j] = jaccard_func(m_i, m_j)
    return jac.max(axis=0)


def relevance_counts(row_c, col_c, true_r, true_c) -> np.ndarray:
    """The same from integer counts: I = |R_i ^ TR_j| |C_i ^ TC_j|, U = |R_i| |C_i| + |TR_j| |TC_j| - I."""
    rc, cc, tr, tc = (np.asarray(a).astype(np.int64) for a in (row_c, col_c, true_r, true_c))
    n = tr.shape[1]
    ra, rb, ca, cb = rc.sum(0), tr.sum(0), cc.sum(0), tc.sum(0)
    m_0, n_0 = int((ra != 0).sum()), int((rb != 0).sum())
    if (m_0 == 0) != (n_0 == 0):
        return np.zeros(n)
    if m_0 == 0:
        return np.ones(n)
    ri, ci = rc.T @ tr, cc.T @ tc                      # [i, j] intersections
    out = np.zeros(n)
    for j in range(n):
        best = 0.0
        for i in range(rc.shape[1]):
            inter = int(ri[i, j]) * int(ci[i, j])
            union = int(ra[i]) * int(ca[i]) + int(rb[j]) * int(cb[j]) - inter
            jac = 0.0 if union == 0 else inter / union
            if i == 0 or jac > best:
                best = jac
        out[j] = best
    return out


# ---- stand-ins for the CPU tests of api.stability_check (no device) ----
def fake_results(seed: int = 3, n_views: int = 2, k: int = 4):
    """A results dict with binary clusters (every cluster non-empty) and the views it came from."""
    rng = np.random.default_rng(seed)
    shapes = [(30, 20), (25, 20)][:n_views]
    data = [rng.random(s) for s in shapes]
    res = {"output_f": [rng.random((n, k)) for n, _ in shapes], "output_s": [rng.random((k, k)) for _ in shapes],
           "output_g": [rng.random((m, k)) for _, m in shapes], "Error": 0.5, "All_Error": np.array([1.0, 0.5]),
           "row_clusters": [], "col_clusters": []}
    for n, m in shapes:
        rc = (rng.random((n, k)) < 0.4).astype(np.float64); rc[0] = 1.0
        cc = (rng.random((m, k)) < 0.4).astype(np.float64); cc[0] = 1.0
        res["row_clusters"].append(rc); res["col_clusters"].append(cc)
    return res, data


def fake_relevance(r: int, n_views: int = 2, k: int = 4) -> np.ndarray:
    """Repeat r's n_views x k relevance: arbitrary fp64 values in [0, 1] (sums of them depend on the order)."""
    return np.random.default_rng(1000 + r).random((n_views, k))


def fake_runner(n_views: int = 2, k: int = 4, fail_at=None):
    def runner(r):
        if r == fail_at:
            return {"stability_performed": False, "tag": f"stability={r}"}
        return {"stability_performed": True, "relevance": fake_relevance(r, n_views, k), "tag": f"stability={r}"}
    return runner
