"""Host restatement of a sparse sub-sample (``resnmtf_subsample_view_sparse``, DESIGN.md section 10 "Device copies and
sub-samples") and the helpers the sparse-view tests share: the source matrices, an upload that keeps stored zeros, the
bitwise comparison of two CSC matrices and the empty-line masks.  NumPy / SciPy only; no device."""
import ctypes as C

import numpy as np
import scipy.sparse as sp


def f32(a):
    return np.asarray(a).astype(np.float32).astype(np.float64)


def random_csc(n, m, density, seed):
    x = sp.random(n, m, density=density, random_state=seed, format="csc")
    x.data = f32(x.data + 0.05)
    return x


def case(name):
    """(source CSC, k, run sweeps): the sources of tests/test_gpu_sparse_shuffle.py, plus 130 x 5.  Values are
    fp32-representable, so a dense engine can hold the same matrix."""
    if name == "37x23":                 # 50 %, one stored entry whose fp32 value is an explicit zero on the device
        x = random_csc(37, 23, 0.5, 1)
        x.data[5] = 1.0e-60
        return x, 3, True
    if name == "64x64":                 # fully stored: a column is exactly one trip of 64
        return sp.csc_matrix(f32(np.random.default_rng(2).random((64, 64)) + 0.1)), 4, True
    if name == "130x5":                 # fully stored, 130 entries per column: two full trips and a partial one
        return sp.csc_matrix(f32(np.random.default_rng(7).random((130, 5)) + 0.1)), 2, True
    if name == "300x200":               # 5 % plus one dense row and one dense column: a wide block in the plan
        d = random_csc(300, 200, 0.05, 3).toarray()
        rng = np.random.default_rng(4)
        d[17, :] = f32(rng.random(200) + 0.1); d[:, 31] = f32(rng.random(300) + 0.1)
        return sp.csc_matrix(d), 5, True
    if name == "300x200_1pct":          # sub-samples with empty lines
        return random_csc(300, 200, 0.01, 5), 3, False
    if name == "70000x70000":           # n' m' > 2^32: 64-bit keys; structure only
        rng = np.random.default_rng(6)
        pos = np.unique(rng.integers(0, 70000 * 70000, 2000, dtype=np.int64))
        return sp.csc_matrix((f32(rng.random(len(pos)) + 0.1), (pos // 70000, pos % 70000)), shape=(70000, 70000)), 2, False
    if name == "50x30_empty":
        return sp.csc_matrix((50, 30)), 2, False
    raise KeyError(name)


def subsample_csc(held, rows, cols):
    """``held[rows][:, cols]`` of a CSC matrix as canonical CSC (ascending rows within a column) with the stored zeros
    KEPT: destination row i is source row rows[i], destination column j is source column cols[j]; the lists are
    unsorted and free of repeats."""
    held = sp.csc_matrix(held)
    n, m = held.shape
    rows = np.asarray(rows, dtype=np.int64); cols = np.asarray(cols, dtype=np.int64)
    assert len(np.unique(rows)) == len(rows) and len(np.unique(cols)) == len(cols)
    inv_r = np.full(n, -1, dtype=np.int64); inv_r[rows] = np.arange(len(rows))
    inv_c = np.full(m, -1, dtype=np.int64); inv_c[cols] = np.arange(len(cols))
    r = inv_r[held.indices]
    c = inv_c[np.repeat(np.arange(m), np.diff(held.indptr))]
    keep = (r >= 0) & (c >= 0)
    r, c, val = r[keep], c[keep], held.data[keep]
    order = np.argsort(c * len(rows) + r, kind="stable")
    indptr = np.concatenate(([0], np.cumsum(np.bincount(c, minlength=len(cols))))).astype(np.int64)
    return sp.csc_matrix((val[order], r[order].astype(np.int32), indptr), shape=(len(rows), len(cols)))


def upload_csc(eng, v, c, pre_processed):
    """resnmtf_set_view_csc with the arrays as they are (Engine.set_view_sparse would drop the explicit zeros)."""
    col_ptr = np.ascontiguousarray(c.indptr, dtype=np.int64)
    row_idx = np.ascontiguousarray(c.indices, dtype=np.int32)
    vals = np.ascontiguousarray(c.data, dtype=np.float64)
    if row_idx.size == 0:
        row_idx = np.zeros(1, dtype=np.int32); vals = np.zeros(1)
    eng._check(eng._lib.resnmtf_set_view_csc(eng._h, v, col_ptr.ctypes.data_as(C.POINTER(C.c_longlong)),
                                             row_idx.ctypes.data_as(C.POINTER(C.c_int)),
                                             vals.ctypes.data_as(C.POINTER(C.c_double)), 1 if pre_processed else 0))


def same_csc(a, b):
    return (a.shape == b.shape and np.array_equal(a.indptr, b.indptr) and np.array_equal(a.indices, b.indices)
            and a.data.tobytes() == b.data.tobytes())


def host_masks(s):
    """(rows, cols) without a stored entry > 0."""
    positive = s.data > 0
    rows = np.bincount(s.indices[positive], minlength=s.shape[0]) == 0
    cols = np.bincount(np.repeat(np.arange(s.shape[1]), np.diff(s.indptr))[positive], minlength=s.shape[1]) == 0
    return rows, cols


def planted_sparse(seed):
    """The planted problem of tests/test_gpu_sparse.py (test-resnmtf.R:38-52 with the noise kept at 5 %): three 60 x 60
    blocks of height 10 in 180 x 180."""
    rng = np.random.default_rng(seed)
    rc = np.kron(np.eye(3), np.ones((60, 1)))
    x = rc @ np.diag([10.0, 10.0, 10.0]) @ rc.T + 0.1 * np.abs(rng.normal(size=(180, 180))) * (rng.random((180, 180)) < 0.05)
    return sp.csr_matrix(x), rc
