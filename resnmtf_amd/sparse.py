"""Host side of sparse data views (``resnmtf_create_sparse`` / ``resnmtf_set_view_csc``).

A view given as a ``scipy.sparse`` matrix is factorised as the dense matrix it stands for -- what the reference does with
an R ``Matrix`` (``R/utils.r:416-419`` densifies it with ``as.matrix``) -- but it is stored and streamed on the device as
CSC + CSR.  ``scipy`` is imported only when such a matrix is seen.  Every function here works on a canonical COPY (CSC,
sorted indices, duplicates summed, explicit zeros dropped): the caller's matrix is never modified.
"""
from __future__ import annotations

import numpy as np


def is_sparse(x) -> bool:
    """True for a ``scipy.sparse`` matrix or array, without importing scipy."""
    return type(x).__module__.startswith("scipy.sparse")


def is_sparse_view(x) -> bool:
    """True for every view that is stored sparse on the device: a ``scipy.sparse`` matrix, or a sparse ``torch`` tensor in
    device memory / its ``device_views.SparseDeviceView`` (no host copy exists of those: ``validate`` and the host
    sub-samples do not apply, the device checks and the device routes stand in)."""
    from . import device_views
    return is_sparse(x) or device_views.is_sparse_device_view(x)


def canonical_csc(x):
    """A canonical fp64 CSC copy of ``x``: sorted row indices, duplicates summed, explicit zeros dropped."""
    import scipy.sparse as sp
    c = sp.csc_matrix(x, dtype=np.float64, copy=True)
    c.sum_duplicates()          # (also sorts the indices)
    c.eliminate_zeros()
    c.sort_indices()
    return c


def validate(x, what: str = "view") -> None:
    """The checks of ``resnmtf_set_view_csc`` on the host, before any device work: no negative or non-finite entry (the
    per-column shift of ``make_non_neg``, ``R/utils.r:20-27``, would turn every implicit zero positive) and no all-zero
    column (``matrix_normalisation``, ``R/utils.r:86-88``, would divide it by zero: a NaN column in the reference)."""
    validate_values(x, what)
    if (np.diff(x.indptr) == 0).any():
        raise ValueError(f"sparse {what} has an all-zero column: matrix_normalisation (R/utils.r:86-88) would divide it "
                         "by zero.")


def validate_values(x, what: str = "view") -> None:
    """The part of ``validate`` that holds for a view that is already pre-processed (a sub-sample, a view to be scored):
    no negative or non-finite entry; an all-zero column is fine there."""
    if not np.isfinite(x.data).all():
        raise ValueError(f"sparse {what} has a non-finite entry.")
    if (x.data < 0).any():
        raise ValueError(f"sparse {what} has a negative entry: the non-negativity shift of make_non_neg (R/utils.r:20-27) "
                         "would turn every implicit zero positive; shift the data and pass it dense.")


def check_data_one(x):
    """``check_inputs`` (``R/utils.r:416,422``) of one sparse view: validated, then divided by its column sums (fp64).
    Returns a new canonical CSC matrix, equal to ``naming.check_data`` on ``x.toarray()``."""
    c = canonical_csc(x)
    validate(c)
    colsum = np.add.reduceat(c.data, c.indptr[:-1]) if c.nnz else np.zeros(c.shape[1])
    c.data = c.data / np.repeat(colsum, np.diff(c.indptr))
    return c


def subsample(x, rows, cols):
    """``X[rows, cols]`` of a canonical CSC matrix (a stability sub-sample, not re-normalised) and the masks of its
    all-zero rows / columns (the condition under which ``stability_repeat`` trims, ``R/stability_analysis.r:165-190``)."""
    sub = canonical_csc(x[np.asarray(rows)][:, np.asarray(cols)])
    er = np.bincount(sub.indices, minlength=sub.shape[0]) == 0
    ec = np.diff(sub.indptr) == 0
    return sub, er, ec
