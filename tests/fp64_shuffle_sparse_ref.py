"""The fp64 restatement of ``shuffle_ref.shuffle_csc`` -- the same function without its fp32 rounding -- with the redraw
condition and the column normalisation of ``resnmtf_fp64_shuffle_sparse``, in NumPy.  A stored
entry at (r, c) lands at ``i = pi^-1(r m + c)``, column ``i // n``, row ``i % n``; explicit zeros stay stored; a line is
empty when it holds no stored entry > 0; a column sum is taken in the dense route's order (lane t of 256 adds the rows
= t mod 256 ascending from 0.0, then the 256-wide tree)."""
import numpy as np
import scipy.sparse as sp

import shuffle_ref as S


def csc_parts(n, m, rows, cols, vals):
    """(indptr, indices, data) of the canonical CSC of the given positions, explicit zeros kept, no SciPy clean-up."""
    rows, cols, vals = np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64), np.asarray(vals, dtype=np.float64)
    order = np.lexsort((rows, cols))
    indptr = np.concatenate([[0], np.cumsum(np.bincount(cols, minlength=m))]).astype(np.int64)
    return indptr, rows[order].astype(np.int32), vals[order]


def raw_csc(n, m, indptr, indices, data):
    """A ``csc_matrix`` over the arrays as they are (no duplicates summed, no zero dropped)."""
    out = sp.csc_matrix((n, m), dtype=np.float64)
    out.indptr, out.indices, out.data = np.asarray(indptr, dtype=np.int64), np.asarray(indices, dtype=np.int32), np.asarray(data, dtype=np.float64)
    return out


def shuffle_csc64(csc, seed: int):
    """``shuffle_ref.shuffle_csc`` on the fp64 values as they are: (indptr, indices, data) of the draw's canonical CSC."""
    n, m = csc.shape
    col = np.repeat(np.arange(m, dtype=np.int64), np.diff(csc.indptr))
    src = csc.indices.astype(np.int64) * m + col
    dst = S.feistel_perm_inverse(src, n * m, seed).astype(np.int64) if len(src) else src
    order = np.argsort(dst, kind="stable")
    dst = dst[order]
    vals = np.asarray(csc.data, dtype=np.float64)[order]
    indptr = np.searchsorted(dst // n, np.arange(m + 1), side="left").astype(np.int64)
    return indptr, (dst % n).astype(np.int64), vals


def empty_lines(n, m, indptr, indices, data):
    """The boolean masks of the rows / columns without a stored entry > 0."""
    positive = data > 0
    col = np.repeat(np.arange(m), np.diff(indptr))
    rows = np.bincount(indices[positive], minlength=n) == 0
    cols = np.bincount(col[positive], minlength=m) == 0
    return rows, cols


def lane_colsums(m, indptr, indices, data):
    """Every column's sum in the 256-lane order over its stored entries (rows ascending): ``np.add.at`` adds one entry
    after the other in index order, so a residue's additions happen in ascending row order."""
    acc = np.zeros((m, 256))
    col = np.repeat(np.arange(m), np.diff(indptr))
    np.add.at(acc, (col, indices % 256), data + 0.0)
    s = 128
    while s > 0:
        acc[:, :s] += acc[:, s:2 * s]
        s >>= 1
    return acc[:, 0].copy()


def lane_colsums_sparse_cols(m, indptr, indices, data):
    """``lane_colsums`` for a very wide matrix: only the non-empty columns get an accumulator row."""
    lens = np.diff(indptr)
    live = np.flatnonzero(lens)
    sub = np.concatenate([[0], np.cumsum(lens[live])])
    out = np.zeros(m)
    out[live] = lane_colsums(len(live), sub, indices, data)
    return out


def normalised(m, indptr, indices, data):
    """``(x + 0.0) / colsum[c]`` per stored entry; 0 / 0 = NaN stays."""
    colsum = lane_colsums_sparse_cols(m, indptr, indices, data)
    with np.errstate(invalid="ignore", divide="ignore"):
        return (data + 0.0) / np.repeat(colsum, np.diff(indptr))


def draw(csc, seed: int, normalise: bool):
    """Everything ``engine.fp64_shuffle_sparse`` returns, from the helper: (indptr, indices, values, empty rows, empty cols)."""
    n, m = csc.shape
    indptr, indices, data = shuffle_csc64(csc, seed)
    er, ec = empty_lines(n, m, indptr, indices, data)
    return indptr, indices, (normalised(m, indptr, indices, data) if normalise else data), er, ec


def bits(a) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)
