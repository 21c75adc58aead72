"""CPU tests of sparse data views: the new C entries are exported, declared and refuse a NULL handle
without touching a device; the host checks and canonicalisation of scipy.sparse views; the out-of-scope refusals; the
existing refusals also fire for sparse inputs; the host pre-processing equals naming.check_data on the dense matrix."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import resnmtf_amd
from resnmtf_amd import _lib, naming, sparse


def _raw(seed=0, n=30, m=12, density=0.3):
    x = sp.random(n, m, density=density, random_state=seed, format="csr")
    return x + sp.eye(n, m, format="csr")          # no empty column


def test_new_symbols_exported_and_declared():
    lib = _lib.load()
    for name in ("resnmtf_create_sparse", "resnmtf_set_view_csc", "resnmtf_view_storage"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)


def test_new_entries_refuse_null_handle():
    lib = _lib.load()
    cp = np.zeros(3, dtype=np.int64); ri = np.zeros(1, dtype=np.int32); vals = np.zeros(1)
    assert lib.resnmtf_set_view_csc(None, 0, cp.ctypes.data_as(C.POINTER(C.c_longlong)),
                                    ri.ctypes.data_as(C.POINTER(C.c_int)), vals.ctypes.data_as(C.POINTER(C.c_double)), 0) == 1
    assert lib.resnmtf_view_storage(None, 0, None, None, None) == 1
    h = C.c_void_p()
    nr = np.array([4], dtype=np.int32); kk = np.array([2], dtype=np.int32)
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
    assert lib.resnmtf_create_sparse(1, ip(nr), ip(nr), ip(kk), None, None, None, C.byref(h)) == 1     # NULL capacity
    assert h.value is None
    assert b"nnz_capacity" in lib.resnmtf_last_error(None)


def test_sparse_preprocessing_equals_check_data_and_leaves_input_alone():
    x = _raw(1) * 3.0
    x_before = x.copy()
    got = naming.check_data([x])[0]
    want = naming.check_data([x.toarray()])[0]
    assert sp.issparse(got) and got.format == "csc"
    np.testing.assert_allclose(got.toarray(), want, rtol=1e-14, atol=0)
    assert (x != x_before).nnz == 0 and x.format == "csr"


def test_canonicalisation_sorts_sums_duplicates_and_copies():
    rows = np.array([3, 1, 3, 0]); cols = np.array([0, 0, 0, 1]); vals = np.array([1.0, 2.0, 4.0, 0.0])
    coo = sp.coo_matrix((vals, (rows, cols)), shape=(5, 2))
    c = sparse.canonical_csc(coo)
    assert c.format == "csc" and c.has_canonical_format
    assert list(c.indptr) == [0, 2, 2] and list(c.indices) == [1, 3]         # explicit zero dropped
    np.testing.assert_array_equal(c.data, [2.0, 5.0])                         # duplicates summed
    assert list(coo.row) == [3, 1, 3, 0]                                      # caller's matrix untouched
    unsorted = sp.csc_matrix((np.array([1.0, 2.0]), np.array([2, 0]), np.array([0, 2])), shape=(3, 1))
    assert list(sparse.canonical_csc(unsorted).indices) == [0, 2] and list(unsorted.indices) == [2, 0]


def test_negative_entries_and_zero_columns_are_refused_before_device_work():
    neg = _raw(2).tolil(); neg[0, 0] = -1.0
    with pytest.raises(ValueError, match="negative"):
        naming.check_data([neg.tocsr()])
    zero = _raw(3).tolil(); zero[:, 4] = 0.0
    with pytest.raises(ValueError, match="all-zero column"):
        naming.check_data([zero.tocsr()])
    for bad in (neg.tocsr(), zero.tocsr()):
        with pytest.raises(ValueError):
            resnmtf_amd.apply_resnmtf([bad], k_val=3, spurious=False, stability=False)
        with pytest.raises(ValueError):
            resnmtf_amd.res_nmtf_inner([bad], None, None, k_vec=[3], spurious=False)


def test_out_of_scope_refusals():
    x = naming.check_data([_raw(4)])[0]
    with pytest.raises(NotImplementedError, match="host_init"):
        resnmtf_amd.res_nmtf_inner([x], None, None, k_vec=[3], spurious=False, host_init=True)
    from resnmtf_amd import sharded
    f, s, g = np.ones((30, 3)), np.eye(3), np.ones((12, 3))
    with pytest.raises(NotImplementedError, match="sparse"):
        sharded.res_nmtf_inner([x], init_f=[f], init_s=[s], init_g=[g], rank=0, world=1)


def test_existing_refusals_fire_for_sparse_inputs():
    x = [_raw(5)]
    with pytest.raises(NotImplementedError, match="stability"):
        resnmtf_amd.apply_resnmtf(x, k_val=3)
    with pytest.raises(NotImplementedError, match="k sweep"):
        resnmtf_amd.apply_resnmtf(x, stability=False, spurious=False)
    with pytest.raises(ValueError, match="ranks"):
        resnmtf_amd.apply_resnmtf(x, k_val=13, stability=False, spurious=False)
    with pytest.raises(NotImplementedError, match="spurious"):
        resnmtf_amd.apply_resnmtf(x, k_val=3, stability=False)
    with pytest.raises(NotImplementedError, match="spurious"):
        resnmtf_amd.res_nmtf_inner(x, None, None, k_vec=[3])
    with pytest.raises(ValueError, match="distance"):
        resnmtf_amd.res_nmtf_inner(x, None, None, k_vec=[3], spurious=False, distance="chebyshev")


def test_host_subsample_and_empty_lines():
    x = sparse.canonical_csc(np.array([[1.0, 0.0, 2.0], [0.0, 0.0, 3.0], [4.0, 0.0, 0.0]]))
    sub, er, ec = sparse.subsample(x, [1, 2], [0, 1, 2])
    np.testing.assert_array_equal(sub.toarray(), [[0.0, 0.0, 3.0], [4.0, 0.0, 0.0]])
    assert list(er) == [False, False] and list(ec) == [False, True, False]
