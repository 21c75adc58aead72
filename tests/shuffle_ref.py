"""NumPy restatement of the device shuffle (``feistel_perm``, ``csrc/resnmtf_kernels.hip.inc``; its inverse,
``csrc/resnmtf_sparse_shuffle.hip.inc``) in wrapping ``uint64`` arithmetic, and the shuffle of a sparse matrix built
from its stored entries only: ``shuffle_csc``.  The dense kernel computes ``staging[i] = X[pi(i)]`` with i column-major
in the destination and pi(i) row-major in the source, so a stored entry at (r, c) lands at ``i = pi^-1(r m + c)``."""
import numpy as np
import scipy.sparse as sp

_U = np.uint64
_GOLD, _M1, _M2 = _U(0x9E3779B97F4A7C15), _U(0xBF58476D1CE4E5B9), _U(0x94D049BB133111EB)


def half_bits(count: int) -> int:
    hb = 1
    while (1 << (2 * hb)) < count:
        hb += 1
    return hb


def _f(x, seed, rnd):
    with np.errstate(over="ignore"):
        f = x + _U(seed & 0xFFFFFFFFFFFFFFFF) + _GOLD * _U(rnd + 1)
        f ^= f >> _U(31); f *= _M1; f ^= f >> _U(29); f *= _M2; f ^= f >> _U(32)
    return f


def _once(i, hb, seed, inverse):
    mask, sh = _U((1 << hb) - 1), _U(hb)
    l, r = i >> sh, i & mask
    for rnd in (range(3, -1, -1) if inverse else range(4)):
        if inverse:
            l, r = (r ^ _f(l, seed, rnd)) & mask, l
        else:
            l, r = r, (l ^ _f(r, seed, rnd)) & mask
    return (l << sh) | r


def _walk(i, count, seed, inverse):
    i = np.array(i, dtype=_U, ndmin=1, copy=True)
    hb = half_bits(int(count))
    todo = np.ones(i.shape, dtype=bool)
    while todo.any():                                  # cycle walking: apply once more while the value is >= count
        i[todo] = _once(i[todo], hb, seed, inverse)
        todo &= i >= _U(count)
    return i


def feistel_perm(i, count: int, seed: int) -> np.ndarray:
    """pi(i) for every i (any integer array-like, values < count)."""
    return _walk(i, count, seed, False)


def feistel_perm_inverse(j, count: int, seed: int) -> np.ndarray:
    return _walk(j, count, seed, True)


def shuffle_dense(x: np.ndarray, seed: int) -> np.ndarray:
    """The dense formula entry for entry: staging[i] = X.flat[pi(i)], staging column-major n x m."""
    n, m = x.shape
    pi = feistel_perm(np.arange(n * m), n * m, seed).astype(np.int64)
    return np.ascontiguousarray(x).reshape(-1)[pi].reshape((n, m), order="F")


def shuffle_csc(csc, seed: int):
    """The shuffle of a CSC matrix from its stored entries alone (explicit zeros kept): the same stored values (rounded
    to fp32, as the device holds them) at their destination positions, row indices ascending within a column."""
    csc = sp.csc_matrix(csc)
    n, m = csc.shape
    col = np.repeat(np.arange(m, dtype=np.int64), np.diff(csc.indptr))
    src = csc.indices.astype(np.int64) * m + col
    dst = feistel_perm_inverse(src, n * m, seed).astype(np.int64) if len(src) else src
    order = np.argsort(dst, kind="stable")
    dst = dst[order]
    vals = csc.data.astype(np.float32).astype(np.float64)[order]
    indptr = np.searchsorted(dst // n, np.arange(m + 1), side="left").astype(np.int64)
    return sp.csc_matrix((vals, (dst % n).astype(np.int32), indptr), shape=(n, m))


def draw_seed(shuffle_seed: int, attempt: int, v: int) -> int:
    """The seed of ``problem._draw_shuffle``'s ``attempt``-th draw of view v."""
    return (shuffle_seed + 7919 * attempt) * 1000003 + v


def attempts_needed(csc, shuffle_seed: int, v: int = 0, bound: int = 64):
    """How many draws ``_draw_shuffle`` makes of this view until no row or column is left without a positive entry
    (``None``: the bound is exhausted)."""
    for attempt in range(bound):
        s = shuffle_csc(csc, draw_seed(shuffle_seed, attempt, v))
        positive = s.data > 0
        rows = np.bincount(s.indices[positive], minlength=s.shape[0])
        cols = np.bincount(np.repeat(np.arange(s.shape[1]), np.diff(s.indptr))[positive], minlength=s.shape[1])
        if (rows > 0).all() and (cols > 0).all():
            return attempt + 1
    return None
