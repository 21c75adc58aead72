"""The bisilhouette of sparse views in double precision (resnmtf_fp64_bisil_sparse):
engine.fp64_bisil_sparse against engine.fp64_bisil on the densified matrix (bit for bit, compared as uint64 words),
against Engine.bisil_sparse on data fp32 holds (bit for bit), against the plain restatement (bisil_ref, 1e-9), twice
(equal bits), through every route a sparse view takes in, the guards of the C entry, and the API: a mixed view list
through res_nmtf_inner and the fp64 k sweep on sparse views.

Data: uniform doubles (not fp32-representable) thresholded to a stored share, as _data of test_gpu_bisil_sparse.py builds
them, with that file's clusters: an all-zero row that is a member, a dense row, an all-zero column that is a feature, an
empty and a singleton bicluster."""
import ctypes as C
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import bisil_ref as B
import resnmtf_amd
from resnmtf_amd import _lib, api, bisil, device_views, engine, naming
from resnmtf_amd._lib import ResnmtfError
from resnmtf_amd.engine import Engine
from test_gpu_bisil_forms import chunk2_ragged
from test_gpu_bisil_sparse import CONFIGS, ZERO_COL, ZERO_ROW, _blocks, _clusters, _data, planted

pytestmark = pytest.mark.gpu

METRICS = ("euclidean", "manhattan", "cosine")
ATOL = 1e-9            # the project's ceiling (test_gpu_bisil.py)
SENTINEL = -7.25


def same_bits(a, b):
    """Equal as 64-bit words: a NaN or a -0.0 is compared too."""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def assert_sparse_is_dense(x, rc, cc, metrics=METRICS, nonzero=True):
    """engine.fp64_bisil_sparse of csc(x) against engine.fp64_bisil of x, per metric; returns the sparse results."""
    xs = sp.csc_matrix(x)
    out = {}
    for metric in metrics:
        got = engine.fp64_bisil_sparse(xs, rc, cc, metric)
        want = engine.fp64_bisil(xs.toarray(), rc, cc, metric)
        assert same_bits(got[0], want[0]) and same_bits(got[1], want[1]), metric
        if nonzero:
            assert got[0].any() and got[1].any(), metric
        out[metric] = got
    return out


# ---- 1. bit for bit the dense fp64 scorer ----
@functools.lru_cache(maxsize=None)
def _case(ci):
    n, m, density, K, p = CONFIGS[ci]
    x = _data(n, m, density, 40 + ci)
    rc, cc = _clusters(n, m, K, 80 + ci, p)
    xs = sp.csc_matrix(x)
    out = {"x": x, "rc": rc, "cc": cc, "sparse": {}, "again": {}, "dense": {}}
    for metric in METRICS:
        out["sparse"][metric] = engine.fp64_bisil_sparse(xs, rc, cc, metric)
        out["again"][metric] = engine.fp64_bisil_sparse(xs, rc, cc, metric)
        out["dense"][metric] = engine.fp64_bisil(xs.toarray(), rc, cc, metric)
    return out


def test_data_is_not_fp32_representable_and_has_the_edge_lines():
    c = _case(0)
    x = c["x"]
    stored = x[x != 0]
    assert np.mean(stored.astype(np.float32).astype(np.float64) != stored) > 0.99
    assert not x[ZERO_ROW].any() and not x[:, ZERO_COL].any() and c["rc"][ZERO_ROW, 0] == 1 and c["cc"][ZERO_COL, 0] == 1
    assert c["rc"][:, 3].sum() == 0 and c["rc"][:, 2].sum() == 1


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("ci", range(len(CONFIGS)))
def test_bitwise_equal_to_the_dense_fp64_scorer(ci, metric):
    c = _case(ci)
    (rs, cs), (dr, dc) = c["sparse"][metric], c["dense"][metric]
    assert same_bits(rs, dr) and same_bits(cs, dc)
    if CONFIGS[ci][3] > 1:
        assert rs.any() and cs.any()


@pytest.mark.parametrize("ci", range(len(CONFIGS)))
def test_two_calls_give_equal_bits(ci):
    c = _case(ci)
    for metric in METRICS:
        a, b = c["sparse"][metric], c["again"][metric]
        assert same_bits(a[0], b[0]) and same_bits(a[1], b[1])


WORST = {metric: 0.0 for metric in METRICS}


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("ci", range(len(CONFIGS)))
def test_silhouettes_match_the_restatement(ci, metric):
    c = _case(ci)
    rs, cs = c["sparse"][metric]
    wr, wc = B.silhouettes(c["x"], c["rc"], c["cc"], metric)
    worst = max(np.abs(rs - wr).max(), np.abs(cs - wc).max())
    WORST[metric] = max(WORST[metric], worst)
    print(f"MEASURED config {CONFIGS[ci]} {metric}: max |d| {worst:.3e}; worst so far {WORST[metric]:.3e}")
    np.testing.assert_allclose(rs, wr, rtol=0, atol=ATOL)
    np.testing.assert_allclose(cs, wc, rtol=0, atol=ATOL)


def test_crafted_line_lengths():
    """Columns with exactly 0, 1, 63, 64, 65 and 129 stored entries as features of the row side, rows with 0, 1, 63, 64 and
    65 as features of the column side (one wave strides a line 64 entries at a time), and on either side a feature line
    whose entries all lie outside U."""
    n, m = 140, 80
    rng = np.random.default_rng(7)
    x = np.zeros((n, m))
    body = rng.random((n - 10, m - 10))
    x[10:, 10:] = np.where(body > 0.9, body, 0.0)
    col_len, row_len = (0, 1, 63, 64, 65, 129), (0, 1, 63, 64, 65)
    for c, l in enumerate(col_len):                        # columns 0 .. 5: entries in rows 10 .. 139 only
        x[10 + rng.choice(n - 10, l, replace=False), c] = rng.random(l) + 0.01
    for r, l in enumerate(row_len):                        # rows 0 .. 4: entries in columns 10 .. 79 only
        x[r, 10 + rng.choice(m - 10, l, replace=False)] = rng.random(l) + 0.01
    x[100:, 6] = 0.0; x[:100, 6] = 0.0
    x[100 + rng.choice(40, 7, replace=False), 6] = rng.random(7) + 0.01        # column 6: stored in rows outside U only
    x[5, :] = 0.0
    x[5, 70 + rng.choice(10, 4, replace=False)] = rng.random(4) + 0.01        # row 5: stored in columns outside U only
    rc, cc = np.zeros((n, 2)), np.zeros((m, 2))
    rc[:60, 0] = 1; rc[40:100, 1] = 1                      # U = rows 0 .. 99
    cc[:40, 0] = 1; cc[30:70, 1] = 1                       # U = columns 0 .. 69
    assert [np.count_nonzero(x[:, c]) for c in range(6)] == list(col_len)
    assert [np.count_nonzero(x[r]) for r in range(5)] == list(row_len)
    assert np.count_nonzero(x[:, 6]) == 7 and not x[:100, 6].any() and np.count_nonzero(x[5]) == 4 and not x[5, :70].any()
    assert_sparse_is_dense(x, rc, cc)


@pytest.mark.parametrize("n_u", (63, 64, 65))
def test_union_sizes_around_one_tile(n_u):
    n, m = 150, 90
    x = _data(n, m, 0.3, 11)
    rng = np.random.default_rng(n_u)
    rc, cc = np.zeros((n, 2)), np.zeros((m, 2))
    rows, cols = rng.permutation(n)[:n_u], rng.permutation(m)[:n_u]
    rc[rows[:40], 0] = 1; rc[rows[30:], 1] = 1
    cc[cols[:40], 0] = 1; cc[cols[30:], 1] = 1
    assert (rc.sum(1) > 0).sum() == n_u and (cc.sum(1) > 0).sum() == n_u
    assert_sparse_is_dense(x, rc, cc)


def test_many_feature_lines():
    """40 x 700, one bicluster with about 600 feature columns: many more lines than waves in a workgroup."""
    n, m = 40, 700
    rng = np.random.default_rng(3)
    u = rng.random((n, m))
    x = np.where(u > 0.9, u, 0.0)
    rc = (rng.random((n, 1)) < 0.6).astype(np.float64)
    cc = np.ones((m, 1)); cc[rng.choice(m, 100, replace=False), 0] = 0
    assert cc.sum() == 600
    got = assert_sparse_is_dense(x, rc, cc, nonzero=False)
    assert not got["euclidean"][0].any()                   # (K = 1: no other bicluster, every silhouette is 0)
    # the same 600 lines beside a second bicluster on the other rows and columns: silhouettes that are not 0
    assert_sparse_is_dense(x, np.hstack([rc, 1.0 - rc]), np.hstack([cc, 1.0 - cc]))


def test_chunked_distance_launch():
    """2950 x 60 at 10 % stored with chunk2_ragged's clusters: chunk_tiles 2, 24 chunks, the last one short."""
    c = chunk2_ragged()
    plan = engine.fp64_bisil_plan(2950, 2945, 3, 1, 2950)
    assert plan["chunk_tiles"] == 2 and plan["chunks"] == 24
    u = np.random.default_rng(5).random((2950, 60))
    x = np.where(u > 0.9, u, 0.0)
    assert_sparse_is_dense(x, c["rc"], c["cc"])


def test_view_without_a_stored_entry():
    rc, cc = _clusters(40, 30, 5, 2)
    for metric in METRICS:
        rs, cs = engine.fp64_bisil_sparse(sp.csc_matrix((40, 30)), rc, cc, metric)
        want = engine.fp64_bisil(np.zeros((40, 30)), rc, cc, metric)
        assert same_bits(rs, want[0]) and same_bits(cs, want[1])
        assert not rs.any() and not cs.any()


def test_cosine_member_without_restricted_features():
    """Row 11 stores entries, none of them in the columns of its bicluster: its restricted norm is 0 (distance 1 to every
    line that has one, 0 to another such line)."""
    n, m = 150, 90
    x = _data(n, m, 0.3, 13)
    rc, cc = _clusters(n, m, 3, 14)
    rc[11] = (1, 0, 0)
    x[11, cc[:, 0] > 0] = 0.0
    assert x[11].any() and rc[:, 0].sum() > 2
    got = assert_sparse_is_dense(x, rc, cc, metrics=("cosine",))["cosine"]
    wr, wc = B.silhouettes(x, rc, cc, "cosine")
    np.testing.assert_allclose(got[0], wr, rtol=0, atol=ATOL)
    np.testing.assert_allclose(got[1], wc, rtol=0, atol=ATOL)


# ---- 2. bit for bit Engine.bisil_sparse on data fp32 holds ----
@pytest.mark.parametrize("K", (3, 12, 17))
def test_bitwise_equal_to_the_f32_engine_on_fp32_data(K):
    n, m = 150, 90
    x = _data(n, m, 0.3, 20 + K).astype(np.float32).astype(np.float64)
    rc, cc = _clusters(n, m, K, 30 + K, 0.3)
    xs = sp.csc_matrix(x)
    with Engine([n], [m], [2], nnz=[xs.nnz]) as e:
        e.set_view_sparse(0, xs, pre_processed=True)
        for metric in METRICS:
            want = e.bisil_sparse(0, rc, cc, metric)
            got = engine.fp64_bisil_sparse(xs, rc, cc, metric)
            assert same_bits(got[0], want[0]) and same_bits(got[1], want[1]), metric
            assert got[0].any() and got[1].any()


# ---- 3. every route in ----
def _entries(n, m, density, seed, dtype):
    """(rows, cols, values in `dtype`, the same widened to fp64) in canonical CSC order; positive values `dtype` holds."""
    import torch
    from test_gpu_sparse_device_views import pattern, values
    rows, cols = pattern(n, m, density, seed, special=True)
    v, wide = values(len(rows), getattr(torch, dtype), seed + 1)
    return rows, cols, v, wide


def _c_call(n, m, rc, cc, metric=0, host=None, dev=None, stream=None, struct_size=None, null=(), device_id=0, k=None):
    """resnmtf_fp64_bisil_sparse through ctypes.  host: (col_ptr, row_idx, values); dev: (layout code, a, b, values, nnz[,
    index type[, dtype code]]) with device tensors, addresses or None.  Returns (code, text, row_sil, col_sil), the outputs
    pre-filled with SENTINEL."""
    import torch
    from test_gpu_sparse_device_views import CODES
    lib = _lib.load()
    rc, cc = np.asfortranarray(rc, dtype=np.float64), np.asfortranarray(cc, dtype=np.float64)
    K = rc.shape[1]
    rs, cs = np.full((max(n, 1), K), SENTINEL, order="F"), np.full((max(m, 1), K), SENTINEL, order="F")
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))                  # noqa: E731
    job = _lib.Fp64BisilSparseJob()
    job.struct_size = C.sizeof(job) if struct_size is None else struct_size
    job.n, job.m, job.k, job.metric = n, m, K if k is None else k, metric
    keep = []
    if host is not None:
        keep = [np.ascontiguousarray(host[0], dtype=np.int64), np.ascontiguousarray(host[1], dtype=np.int32),
                np.ascontiguousarray(host[2], dtype=np.float64)]
        job.x.col_ptr = keep[0].ctypes.data_as(C.POINTER(C.c_longlong))
        job.x.row_idx, job.x.values = keep[1].ctypes.data_as(C.POINTER(C.c_int)), dp(keep[2])
    if dev is not None:
        layout, a, b, vals, nnz = dev[:5]
        ptr = lambda x: None if x is None else (x if isinstance(x, int) else x.data_ptr()) or None      # noqa: E731
        kinds = [x.dtype for x in (a, b) if torch.is_tensor(x)]
        c = job.x_dev
        c.layout = layout
        c.index_type = dev[5] if len(dev) > 5 else (_lib.INDEX_I32 if kinds and kinds[0] == torch.int32 else _lib.INDEX_I64)
        c.dtype = dev[6] if len(dev) > 6 else CODES[vals.dtype]
        c.ptr_or_rows, c.idx_or_cols, c.values, c.nnz = ptr(a), ptr(b), ptr(vals), nnz
        job.stream = stream
    job.row_clusters, job.col_clusters, job.row_sil, job.col_sil = dp(rc), dp(cc), dp(rs), dp(cs)
    for name in null:
        setattr(job, name, None)
    torch.cuda.synchronize()
    code = lib.resnmtf_fp64_bisil_sparse(device_id, C.byref(job))
    return code, (lib.resnmtf_last_error(None) or b"").decode(), rs, cs


N3, M3 = 33, 97


@functools.lru_cache(maxsize=None)
def _route_case(dtype):
    rows, cols, v, wide = _entries(N3, M3, 0.2, 50, dtype)
    rc, cc = _clusters(N3, M3, 3, 51)
    host = sp.csc_matrix((wide, (rows, cols)), shape=(N3, M3))
    want = {metric: engine.fp64_bisil_sparse(host, rc, cc, metric) for metric in ("euclidean", "cosine")}
    assert want["euclidean"][0].any() and want["euclidean"][1].any()
    return rows, cols, v, rc, cc, want


@pytest.mark.parametrize("index", ("int32", "int64"))
@pytest.mark.parametrize("layout", ("csc", "csc_perm", "csr", "coo"))
def test_layouts_and_index_types(layout, index):
    """A sparse_csc (rows in canonical order, and permuted within the columns), a sparse_csr (columns permuted within the
    rows) and a coalesced sparse_coo tensor (any order) on the GPU give the bits of the host route on the canonical CSC."""
    import torch
    from test_gpu_sparse_device_views import LAYOUT_CODE, arrays, as_tensor, on_device
    rows, cols, v, rc, cc, want = _route_case("float64")
    a, b, vals = on_device(*arrays(layout, rows, cols, v, N3, M3, 3), getattr(torch, index))
    for metric in want:
        if layout == "coo" and index == "int32":             # (torch's COO indices are int64 only: the C entry itself)
            code, text, rs, cs = _c_call(N3, M3, rc, cc, bisil.METRICS[metric], dev=(LAYOUT_CODE[layout], a, b, vals, len(rows)))
            assert code == 0, text
        else:
            rs, cs = engine.fp64_bisil_sparse(as_tensor(layout, a, b, vals, (N3, M3)), rc, cc, metric)
        assert same_bits(rs, want[metric][0]) and same_bits(cs, want[metric][1]), metric


@pytest.mark.parametrize("dtype", ("float64", "float32", "float16", "bfloat16"))
def test_value_types(dtype):
    import torch
    from test_gpu_sparse_device_views import arrays, as_tensor, on_device
    rows, cols, v, rc, cc, want = _route_case(dtype)
    assert v.dtype == getattr(torch, dtype)
    t = as_tensor("csr", *on_device(*arrays("csr", rows, cols, v, N3, M3, 4), torch.int64), (N3, M3))
    view = device_views.SparseDeviceView(t)                   # (the host layer's own wrapper is taken as the tensor)
    for metric in want:
        rs, cs = engine.fp64_bisil_sparse(view if metric == "cosine" else t, rc, cc, metric)
        assert same_bits(rs, want[metric][0]) and same_bits(cs, want[metric][1]), metric


def test_explicit_zero_stays_stored_and_scores_as_zero():
    import torch
    from test_gpu_sparse_device_views import arrays, as_tensor, on_device
    rows, cols, v, rc, cc, _ = _route_case("float64")
    v = v.clone(); v[17] = 0.0
    host = sp.csc_matrix((v.numpy(), (rows, cols)), shape=(N3, M3))
    t = as_tensor("csc", *on_device(*arrays("csc", rows, cols, v, N3, M3, 5), torch.int64), (N3, M3))
    assert t._nnz() == len(rows) and engine._sparse.canonical_csc(host).nnz == len(rows) - 1
    want = engine.fp64_bisil_sparse(host, rc, cc, "manhattan")
    got = engine.fp64_bisil_sparse(t, rc, cc, "manhattan")
    assert same_bits(got[0], want[0]) and same_bits(got[1], want[1])
    # the host entry itself with the zero kept in its CSC: the same bits again
    ccol = np.concatenate([[0], np.cumsum(np.bincount(cols, minlength=M3))])
    code, text, rs, cs = _c_call(N3, M3, rc, cc, 1, host=(ccol, rows, v.numpy()))
    assert code == 0 and same_bits(rs, want[0]) and same_bits(cs, want[1]), text


def test_device_view_is_read_where_it_lies(monkeypatch):
    """The route taken: the job names the tensor's own arrays and no host CSC, and nothing is downloaded during the call."""
    import torch
    from test_gpu_sparse_device_views import arrays, as_tensor, on_device
    rows, cols, v, rc, cc, want = _route_case("float64")
    t = as_tensor("csc", *on_device(*arrays("csc_perm", rows, cols, v, N3, M3, 6), torch.int64), (N3, M3))
    keep = []
    job = engine._fp64_bisil_sparse_job(device_views.SparseDeviceView(t), N3, M3, 0, keep)
    assert not job.x.col_ptr and not job.x.row_idx and not job.x.values
    assert (job.x_dev.ptr_or_rows, job.x_dev.idx_or_cols, job.x_dev.values) == (t.ccol_indices().data_ptr(), t.row_indices().data_ptr(),
                                                                               t.values().data_ptr())
    assert job.x_dev.nnz == len(rows) and job.x_dev.layout == _lib.SPARSE_CSC

    def refuse(*args, **kwargs):
        raise AssertionError("a tensor was brought to the host")
    for name in ("cpu", "numpy", "tolist", "to_dense"):
        monkeypatch.setattr(torch.Tensor, name, refuse)
    monkeypatch.setattr(device_views, "sparse_tensor_to_scipy", refuse)
    got = engine.fp64_bisil_sparse(t, rc, cc, "euclidean")
    monkeypatch.undo()
    assert same_bits(got[0], want["euclidean"][0]) and same_bits(got[1], want["euclidean"][1])


# ---- 4. the guards of the C entry ----
def _refused(result, want_code, match):
    code, text, rs, cs = result
    assert code == want_code and match in text, (code, text, match)
    assert (rs == SENTINEL).all() and (cs == SENTINEL).all()


def test_guards_of_the_c_entry():
    import torch
    from test_gpu_sparse_device_views import arrays, on_device
    rows, cols, v, rc, cc, want = _route_case("float64")
    nnz = len(rows)
    ccol = np.concatenate([[0], np.cumsum(np.bincount(cols, minlength=M3))])
    host = (ccol, rows, v.numpy())
    a, b, vals = on_device(*arrays("csc", rows, cols, v, N3, M3, 1), torch.int64)
    dev = (_lib.SPARSE_CSC, a, b, vals, nnz)
    call = functools.partial(_c_call, N3, M3, rc, cc)
    # what resnmtf_fp64_bisil refuses, with its texts
    for kw, match in ((dict(host=host, struct_size=8), "resnmtf_fp64_bisil_sparse_job struct_size mismatch"),
                      (dict(host=host, k=0), "k must be in [1, 64]"), (dict(host=host, k=65), "k must be in [1, 64]"),
                      (dict(host=host, metric=3), "metric must be 0 (euclidean), 1 (manhattan) or 2 (cosine)"),
                      (dict(host=host, dev=dev), "X is given in two places (job->x and job->x_dev)"),
                      (dict(), "X is given in no place (job->x or job->x_dev)"),
                      (dict(host=host, null=("col_sil",)), "row_clusters / col_clusters / row_sil / col_sil are NULL"),
                      (dict(dev=dev, null=("row_clusters",)), "row_clusters / col_clusters / row_sil / col_sil are NULL"),
                      (dict(host=host, device_id=99), "device_id out of range")):
        _refused(call(**kw), 1, match)
    _refused(_c_call(0, M3, rc, cc, host=host), 1, "view dimensions must be positive")
    bad_r, bad_c = rc.copy(), cc.copy()
    bad_r[5, 0], bad_c[2, 0] = 0.5, np.nan
    for route in (dict(host=host), dict(dev=dev)):
        _refused(_c_call(N3, M3, bad_r, bad_c, **route), 1, "row_clusters entries must be 0 or 1")
        _refused(_c_call(N3, M3, rc, bad_c, **route), 1, "col_clusters entries must be 0 or 1")
    # what resnmtf_fp64_run_sparse refuses of a host view
    p = ccol.copy(); p[3] = p[2] - 1
    i = rows.copy(); i[4] = N3
    w = v.numpy().copy(); w[6] = -1.0
    for bad, match in (((p, rows, v.numpy()), "view 0: col_ptr is not monotone (column 2)"),
                       ((ccol, i, v.numpy()), "view 0: row index out of range in column"),
                       ((ccol, rows, w), "view 0: negative entry in column")):
        _refused(call(host=bad), 1, match)
    # what resnmtf_fp64_run_sparse_device refuses of a device view: the struct, the pointers, then the device checks
    host_array = np.zeros(nnz)
    for bad, match in (((7, a, b, vals, nnz), "view 0: spd->view: unknown layout"),
                       ((_lib.SPARSE_CSC, a, b, vals, nnz, 9), "view 0: spd->view: unknown index type"),
                       ((_lib.SPARSE_CSC, a, b, vals, nnz, _lib.INDEX_I64, 11), "view 0: spd->view: unknown dtype"),
                       ((_lib.SPARSE_CSC, a, b, vals, -1), "view 0: spd->view: nnz is negative"),
                       ((_lib.SPARSE_CSC, a, None, vals, nnz), "view 0: spd->view: ptr_or_rows / idx_or_cols / values is NULL"),
                       ((_lib.SPARSE_CSC, a, b, host_array.ctypes.data, nnz, _lib.INDEX_I64, _lib.DTYPE_F64),
                        "view 0: spd->view.values is not device memory of device 0"),
                       # (2^20 indices of 8 bytes: beyond any block torch's allocator may have carved the array from)
                       ((_lib.SPARSE_CSC, a, b, vals, 1 << 20), "view 0: spd->view.idx_or_cols is shorter than its element count")):
        _refused(call(dev=bad), 1, match)
    i = b.clone(); i[4] = N3
    _refused(call(dev=(_lib.SPARSE_CSC, a, i, vals, nnz)), 1, "row index out of range (entry 4)")
    w = vals.clone(); w[6] = -1.0
    _refused(call(dev=(_lib.SPARSE_CSC, a, b, w, nnz)), 1, "negative")
    # a position stored twice in a device COO: the canonicaliser's refusal
    r, c, x = on_device(*arrays("coo", rows, cols, v, N3, M3, 2), torch.int64)
    r[9], c[9] = r[3], c[3]
    _refused(call(dev=(_lib.SPARSE_COO, r, c, x, nnz)), 1, "stored twice")
    # the job itself is fine: the same call without a fault runs on both routes and gives the bits of the engine function
    for route in (dict(host=host), dict(dev=dev)):
        code, text, rs, cs = call(**route)
        assert code == 0 and same_bits(rs, want["euclidean"][0]) and same_bits(cs, want["euclidean"][1]), text
    assert _lib.load().resnmtf_fp64_bisil_sparse(0, None) == 1


def test_no_active_bicluster_is_zero_without_device_work():
    rows, cols, v, rc, cc, _ = _route_case("float64")
    ccol = np.concatenate([[0], np.cumsum(np.bincount(cols, minlength=M3))])
    code, text, rs, cs = _c_call(N3, M3, rc, np.zeros_like(cc), host=(ccol, rows, v.numpy()), device_id=99)
    assert code == 0 and not rs.any() and not cs.any(), text          # (the device is never chosen: its id is not read)


def test_workspace_above_the_free_memory_is_refused_with_its_byte_count():
    """200000 x 200000 with a handful of entries, one bicluster holding every row and column: G alone is 200000 x 200000
    doubles = 320 GB, more than the device has.  Refused before anything is allocated, the outputs untouched."""
    n = 200000
    at = np.array([0, 17, 4096, 123456, n - 1])
    xs = sp.csc_matrix((np.arange(1.0, 6.0), (at, at[::-1])), shape=(n, n))
    ones = np.ones((n, 1))
    with pytest.raises(ResnmtfError, match=r"fp64_bisil_sparse workspace: \d+ bytes asked for \(320000000000 of them the restricted "
                                           r"block, features x padded members, \d+ the CSC and CSR copies of X\)") as e:
        engine.fp64_bisil_sparse(xs, ones, ones)
    assert e.value.code == 4
    asked = int(str(e.value).split(" bytes asked for")[0].split()[-1])
    assert asked >= 320_000_000_000
    c = xs.tocsc()
    _refused(_c_call(n, n, ones, ones, host=(c.indptr, c.indices, c.data)), 4, "bytes asked for")


# ---- 5. the API ----
def _mixed_problem():
    x1 = _blocks(1, 60, 40, 3); x1[x1 < 0.5] = 0.0          # sparse view: the blocks only
    x2 = _blocks(2, 60, 30, 3)                              # dense view, rows shared with view 0
    data = naming.check_data([sp.csc_matrix(x1), x2])
    rn, cn = naming.give_names(data, None, None, None, None)
    kw = dict(k_vec=[3, 3], spurious=False, row_names=rn, col_names=cn, seed=5, n_iters=30, precision="fp64", score_bisil=True,
              fp64_bisil=True)
    return data, naming.shared_names(rn), naming.shared_names(cn), kw


def _check_combination(res, views, dense_views, metric):
    """res["bisil"] is, exactly, the combination over the two engine functions on the returned clusters, and the same
    combination with engine.fp64_bisil on the densified views."""
    rcs = [device_views.to_numpy(r) for r in res["row_clusters"]]
    ccs = [device_views.to_numpy(c) for c in res["col_clusters"]]
    by_kind, densified = [], []
    for v, (x, d) in enumerate(zip(views, dense_views)):
        one = engine.fp64_bisil_sparse if resnmtf_amd.sparse.is_sparse_view(x) else engine.fp64_bisil
        by_kind.append(bisil.view_score(rcs[v], ccs[v], *one(x, rcs[v], ccs[v], metric)))
        densified.append(bisil.view_score(rcs[v], ccs[v], *engine.fp64_bisil(d, rcs[v], ccs[v], metric)))
    assert res["bisil"] == bisil.overall(by_kind) == bisil.overall(densified)
    assert res["bisil"] != 0.0


def test_res_nmtf_inner_scores_a_mixed_view_list():
    data, rs, cs, kw = _mixed_problem()
    dense = [data[0].toarray(), data[1]]
    with pytest.raises(NotImplementedError, match="scores dense views only; sparse views"):      # without the opt-in: as before
        api.res_nmtf_inner(data, rs, cs, fp64_sparse=True, **kw)
    for metric in ("euclidean", "cosine"):
        res = api.res_nmtf_inner(data, rs, cs, distance=metric, fp64_sparse=True, fp64_bisil_sparse=True, **kw)
        _check_combination(res, data, dense, metric)
        want = B.bisil(dense, res["row_clusters"], res["col_clusters"], metric)
        print(f"MEASURED api bisil {metric}: {res['bisil']!r}, restated {want!r}")
        assert res["bisil"] == pytest.approx(want, abs=ATOL)


def test_res_nmtf_inner_scores_a_device_sparse_view():
    import torch
    data, rs, cs, kw = _mixed_problem()
    dense = [data[0].toarray(), data[1]]
    dev = torch.device("cuda", 0)
    c = data[0]
    t = torch.sparse_csc_tensor(torch.as_tensor(c.indptr, dtype=torch.int64, device=dev),
                                torch.as_tensor(c.indices, dtype=torch.int64, device=dev), torch.as_tensor(c.data, device=dev), c.shape)
    there = [t, data[1]]
    res = api.res_nmtf_inner(there, rs, cs, fp64_sparse_device=True, fp64_bisil_sparse=True, **kw)
    _check_combination(res, there, dense, "euclidean")
    on_device = api.res_nmtf_inner(there, rs, cs, fp64_sparse_device=True, fp64_device=True, output="torch", fp64_bisil_sparse=True, **kw)
    assert isinstance(on_device["row_clusters"][0], torch.Tensor) and on_device["bisil"] == res["bisil"]
    _check_combination(on_device, there, dense, "euclidean")


def test_fp64_k_sweep_on_sparse_views():
    """The construction of test_gpu_bisil_sparse.py::test_k_sweep_on_sparse_views, through the fp64 path."""
    data, truth = [], planted_clusters()
    for seed in (1, 2):
        x = planted(seed)
        data.append(sp.csc_matrix(np.where(x > 0.2, x, 0.0)))        # the blocks and the noise above two sigma
    kw = dict(k_max=5, spurious=False, stability=False, k_sweep=True, return_sweep=True, seed=3, n_iters=40, precision="fp64",
              fp64_sparse=True)
    with pytest.raises(NotImplementedError, match="a sparse view in the k sweep is not supported"):      # without the opt-in: as before
        resnmtf_amd.apply_resnmtf(data, **kw)
    res = resnmtf_amd.apply_resnmtf(data, fp64_bisil_sparse=True, **kw)
    sweep = res["k_sweep"]
    print("MEASURED fp64 k sweep on sparse views:", sweep)
    assert sweep["k"][:3] == [3, 4, 5] and np.isfinite(sweep["bisil"]).all()
    assert sweep["k"][int(np.argmax(sweep["bisil"]))] == 3             # the planted k
    assert [f.shape[1] for f in res["output_f"]] == [3, 3] and res["bisil"] == max(sweep["bisil"])
    for v in range(2):                                                  # the planted clusters, in some order
        for got, want in ((res["row_clusters"][v], truth), (res["col_clusters"][v], truth)):
            assert sorted(map(tuple, got.T)) == sorted(map(tuple, want.T))
    p = api.prepare(api._views(data), None, None, None, None, None, normalise=True, symmetrise=True)
    one = api.res_nmtf_inner(p.data, p.row_shared, p.col_shared, None, None, None, [3, 3], p.phi, p.xi, p.psi, 40, spurious=False,
                             row_names=p.row_names, col_names=p.col_names, seed=3 + 3, precision="fp64", fp64_sparse=True,
                             score_bisil=True, fp64_bisil=True, fp64_bisil_sparse=True)
    assert one["bisil"] == res["bisil"]
    for key in ("output_f", "output_s", "output_g", "row_clusters", "col_clusters", "lambda", "mu"):
        for v in range(2):
            assert same_bits(one[key][v], res[key][v]), (key, v)
    assert same_bits(one["All_Error"], res["All_Error"])
    x64 = [d.toarray() for d in p.data]
    want = B.bisil(x64, res["row_clusters"], res["col_clusters"], "euclidean")
    print(f"MEASURED sweep bisil {res['bisil']!r}, restated {want!r}")
    assert res["bisil"] == pytest.approx(want, abs=ATOL)


def planted_clusters():
    """The three 60-row (and 60-column) blocks of `planted`."""
    c = np.zeros((180, 3))
    for i in range(3):
        c[i * 60:(i + 1) * 60, i] = 1
    return c


def test_refusals_that_remain_with_the_flag():
    import torch
    x = planted(1)
    xs = sp.csc_matrix(np.where(x > 0.2, x, 0.0))
    on = dict(precision="fp64", fp64_sparse=True, fp64_bisil=True, fp64_bisil_sparse=True)
    with pytest.raises(NotImplementedError, match="a sparse view with fp64_spurious is not supported"):
        resnmtf_amd.apply_resnmtf([xs], k_val=3, stability=False, spurious_on_device=True, fp64_spurious=True, **on)
    with pytest.raises(NotImplementedError, match="a sparse view with fp64_stability is not supported"):
        resnmtf_amd.apply_resnmtf([xs], k_val=3, spurious=False, fp64_stability=True, **on)
    t = torch.as_tensor(x, device=torch.device("cuda", 0))
    with pytest.raises(NotImplementedError, match="a view in device memory is not supported"):
        resnmtf_amd.apply_resnmtf([t], k_sweep=True, stability=False, spurious=False, fp64_device=True, **on)
