"""Host reference of the device SVD initialisation, stage by stage (test infrastructure; plain fp64 NumPy).

``resnmtf_init_svd`` is a randomized subspace iteration: a Gaussian sketch, per half step one streaming product and a
CholeskyQR2, an L x L eigenproblem at the end, then ``init_mats_inner``'s arithmetic on the k leading triplets.  The
statistics below take the device's signed basis (``Engine.init_svd(return_basis=True)``) and check ONE stage each:

* ``orth_stat``: U = Q Ut is orthonormal -- the Gram, the Cholesky and the applies (fp64 throughout, rounding only);
* ``product_stat``: V diag(d) = X^T U entry by entry -- the last streaming product and the slab sum, row by row;
* ``residual_stat`` / ``sv_stat``: the triplets are singular triplets of X -- the iteration as a whole;
* ``finish``: F0, S0, G0, lambda, mu from U, V, d (R/update_steps.r:93-115 without the noise).

``sketch_svd`` is the same algorithm in fp64 with replaceable products: the yardstick for what the algorithm itself
reaches, and the place where tests/test_init_ref_host.py plants the bugs each statistic exists to catch.
"""
from __future__ import annotations

import numpy as np

RIDGE = 1e-14          # orthonormalise(): times trace(Gram), round 0 only
RANK_CUT = 2e-14       # kRankCut: a Cholesky pivot not above this times trace(Gram) zeroes its column
GRAM_BLOCKS = 256      # kGramBlocks


def sketch_width(k: int) -> int:
    """L = min(64, 16 ceil((k + 8) / 16)) (resnmtf_init_svd)."""
    return min(64, 16 * ((k + 8 + 15) // 16))


def takes_sketch(n: int, m: int, k: int) -> bool:
    """False: the view takes the thin route (exact Gram of the short side)."""
    return min(n, m) >= sketch_width(k)


def gram_rows_per_block(length: int) -> int:
    """ts_gram_host: rows of one workgroup of ts_gram_kernel."""
    return 16 * ((-(-length // GRAM_BLOCKS) + 15) // 16)


# ---------------------------------------------------------------------------------------------------------------------
# finish_init
# ---------------------------------------------------------------------------------------------------------------------
def finish(U, V, d, k):
    """R/update_steps.r:93-115 with sigma = 0 on the k leading triplets: ``(F0, S0, G0, lambda, mu)``.  A zero vector
    (a triplet past the rank of X, where svd() returns some unit vector) is replaced by the constant unit vector, as
    finish_init does."""
    f = np.abs(np.asarray(U, dtype=np.float64)[:, :k])                               # :93
    g = np.abs(np.asarray(V, dtype=np.float64)[:, :k])                               # :94
    for w in (f, g):
        zero = w.sum(axis=0) == 0
        w[:, zero] = 1.0 / np.sqrt(w.shape[0])
    s = np.abs(np.diag(np.asarray(d, dtype=np.float64)[:k]))                         # :95
    cf, cg = f.sum(axis=0), g.sum(axis=0)                                            # :100-101
    s = s * (cf * cg)[None, :]                                                       # :102-105
    f = f / cf[None, :]                                                              # :106-109
    g = g / cg[None, :]                                                              # :110-113
    return f, s, g, f.sum(axis=0), g.sum(axis=0)                                     # :114-115


def half_normal_z(noise, sigma):
    """z scores of the mean and of the second moment of ``noise`` against |N(0, sd^2)|, sd = sqrt(sigma) (mvrnorm's
    sigma I is a covariance, R/update_steps.r:96-99): mean sd sqrt(2 / pi) with variance sd^2 (1 - 2 / pi), second
    moment sd^2 with variance 2 sd^4."""
    x = np.asarray(noise, dtype=np.float64).ravel()
    sd = np.sqrt(sigma)
    z_mean = (x.mean() - sd * np.sqrt(2.0 / np.pi)) / (sd * np.sqrt((1.0 - 2.0 / np.pi) / x.size))
    z_m2 = (np.mean(x * x) - sd * sd) / (sd * sd * np.sqrt(2.0 / x.size))
    return float(z_mean), float(z_m2)


# ---------------------------------------------------------------------------------------------------------------------
# the algorithm in fp64
# ---------------------------------------------------------------------------------------------------------------------
def cholesky_cut(C, cut):
    """cholesky_upper: C = R^T R with the columns whose pivot is not above ``cut`` left out (zero row, R[j, j] = 0)."""
    L = C.shape[0]
    R = np.zeros((L, L))
    for j in range(L):
        d = C[j, j] - R[:j, j] @ R[:j, j]
        if not d > cut:
            continue
        R[j, j] = np.sqrt(d)
        R[j, j + 1:] = (C[j, j + 1:] - R[:j, j] @ R[:j, j + 1:]) / R[j, j]
    return R


def invert_cut(R):
    """invert_upper: the inverse of R on the columns kept, zero rows and columns elsewhere."""
    keep = np.flatnonzero(np.diag(R) != 0)
    Ri = np.zeros_like(R)
    Ri[np.ix_(keep, keep)] = np.linalg.inv(R[np.ix_(keep, keep)])
    return Ri


def _gram(Y):
    return Y.T @ Y


def _apply(Y, M):
    return Y @ M


def orthonormalise(Y, gram=_gram, apply=_apply):
    """CholeskyQR2 as the device runs it: the ridge in round 0, the rank cut in both."""
    for rnd in range(2):
        C = gram(Y)
        tr = np.trace(C)
        if rnd == 0:
            C = C + RIDGE * tr * np.eye(C.shape[0])
        Y = apply(Y, invert_cut(cholesky_cut(C, RANK_CUT * tr)))
    return Y


def sketch_svd(x, L, n_power, rng, xg=None, xtq=None, gram=_gram, apply=_apply, q_perm=None):
    """``(U, V, d)`` (n x L, m x L, L descending) of the randomized subspace iteration of resnmtf_init_svd in fp64:
    Gaussian Omega (m x L), CholeskyQR2 after every product but the last, the L x L eigenproblem of Z^T Z, U = Q Ut,
    V = Z Ut / d.  The two products, the Gram and the apply can be replaced (``xg(x, Z)``, ``xtq(x, Q)``, ``gram(Y)``,
    ``apply(Y, M)``); ``q_perm`` permutes the columns of the f32 operand copy of Q that X^T Q reads."""
    x = np.asarray(x, dtype=np.float64)
    xg = xg or (lambda a, z: a @ z)
    xtq = xtq or (lambda a, q: a.T @ q)
    Z = rng.standard_normal((x.shape[1], L))
    for it in range(n_power):
        Q = orthonormalise(xg(x, Z), gram, apply)
        Z = xtq(x, Q if q_perm is None else Q[:, q_perm])
        if it + 1 < n_power:
            Z = orthonormalise(Z, gram, apply)
    lam, Ut = np.linalg.eigh(gram(Z))
    order = np.argsort(-lam, kind="stable")
    d = np.sqrt(np.maximum(lam[order], 0.0))
    Ut = Ut[:, order]
    inv = np.divide(1.0, d, out=np.zeros_like(d), where=d > 0)
    return apply(Q, Ut), apply(Z, Ut * inv[None, :]), d


def thin_svd(x):
    """The thin route in fp64: eigenvectors W of the Gram of the short side, the long side as Y W / d."""
    x = np.asarray(x, dtype=np.float64)
    tall = x.shape[1] <= x.shape[0]
    Y = x if tall else x.T
    lam, W = np.linalg.eigh(Y.T @ Y)
    order = np.argsort(-lam, kind="stable")
    d = np.sqrt(np.maximum(lam[order], 0.0))
    W = W[:, order]
    inv = np.divide(1.0, d, out=np.zeros_like(d), where=d > 0)
    long_side = Y @ (W * inv[None, :])
    return (long_side, W, d) if tall else (W, long_side, d)


# ---------------------------------------------------------------------------------------------------------------------
# the statistics
# ---------------------------------------------------------------------------------------------------------------------
def _worst(a):
    a = np.asarray(a, dtype=np.float64)
    if a.size == 0:
        return 0.0
    return float(np.max(np.where(np.isfinite(a), a, np.inf)))


def orth_stat(U, cols=None):
    """max |U^T U - I| over the leading ``cols`` columns (None: all)."""
    U = np.asarray(U, dtype=np.float64)[:, :cols]
    return _worst(np.abs(U.T @ U - np.eye(U.shape[1])))


def product_stat(x, U, V, d, L, cols):
    """``(worst, nz)``: max over rows i and the leading ``cols`` columns j of ``|X^T U - V diag(d)|[i, j] / (sqrt(L)
    ||X[:, i]||_2)`` (each entry of X^T U is a sum of n products bounded by ||X[:, i]|| ||u_j|| = ||X[:, i]||; V diag(d)
    is X^T Q, the f32 product, rotated by the L x L orthogonal Ut, which mixes L columns); ``nz`` counts the entries
    that are not exactly zero in rows where the column of X is all zero."""
    x = np.asarray(x, dtype=np.float64)
    U = np.asarray(U, dtype=np.float64)[:, :cols]; V = np.asarray(V, dtype=np.float64)[:, :cols]
    diff = np.abs(x.T @ U - V * np.asarray(d, dtype=np.float64)[None, :cols])
    norms = np.linalg.norm(x, axis=0)
    live = norms > 0
    worst = _worst(diff[live] / (np.sqrt(L) * norms[live, None]))
    return worst, int(np.count_nonzero(V[~live]))


def residual_stat(x, U, V, d, cols):
    """max over the leading ``cols`` triplets of ``||X v_j - d_j u_j||_2 / d_1``."""
    x = np.asarray(x, dtype=np.float64)
    U = np.asarray(U, dtype=np.float64)[:, :cols]; V = np.asarray(V, dtype=np.float64)[:, :cols]
    d = np.asarray(d, dtype=np.float64)
    return _worst(np.linalg.norm(x @ V - U * d[None, :cols], axis=0) / d[0])


def sv_stat(d, sigma, cols):
    """max over the leading ``cols`` values of ``|d_j - sigma_j| / sigma_1``."""
    d = np.asarray(d, dtype=np.float64); sigma = np.asarray(sigma, dtype=np.float64)
    return _worst(np.abs(d[:cols] - sigma[:cols]) / sigma[0])
