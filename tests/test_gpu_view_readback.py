"""Views out to device memory and reference clusters in from it (``resnmtf_get_view_device`` /
``resnmtf_get_view_sparse_device`` / ``resnmtf_set_reference_clusters_device``).  The yardstick is
the host route in the same process -- ``get_view``, ``get_view_sparse`` (converted by SciPy), ``set_reference_clusters`` --
and every comparison is on bits: no tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import resnmtf_amd
from resnmtf_amd import _lib, api, batched, naming
from resnmtf_amd._lib import ResnmtfError
from resnmtf_amd.engine import Engine, _dp, _ip
from resnmtf_amd.problem import prepare

import shuffle_ref

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
INVALID, STATE = 1, 5                                   # RESNMTF_ERR_*
CANARY = -7.0
# the issue's shapes (40 x 1024 and 1024 x 40: an fp32 pitch of 4 KiB, padded), then both sides of the copy kernel's own
# 32 x 32 tile and of the image's 64-row tile
DENSE_SHAPES = [(1, 1), (1, 70), (70, 1), (33, 65), (130, 31), (257, 70), (40, 1024), (1024, 40),
                (32, 32), (31, 33), (64, 64), (65, 63)]
INT_BITS = {torch.float32: torch.int32, torch.float64: torch.int64}


def bits_equal(a, b) -> bool:
    """Same shape, same dtype, same bits (NaN payloads and the sign of zero included), whatever the strides."""
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(INT_BITS[a.dtype]), b.view(INT_BITS[b.dtype]))


def view_data(n, m, seed):
    rng = np.random.default_rng(seed)
    x = rng.random((n, m)) + 0.05
    return x / x.sum(0, keepdims=True)


def raw_data(n, m, seed):
    """Data with negatives for ``set_view_raw`` (n = 1: a shifted single-entry column is 0 / 0 = NaN, compared on bits)."""
    return np.random.default_rng(seed).normal(size=(n, m))


def references(eng, v=0):
    """``get_view`` as an fp64 tensor and as its exact fp32 cast, on the device."""
    ref = eng.get_view(v)
    t64 = torch.from_numpy(np.ascontiguousarray(ref)).to(DEV)
    t32 = t64.float()
    assert bits_equal(t32.double(), t64)                # (the stored image is f32: the cast loses nothing)
    return {torch.float64: t64, torch.float32: t32}


def sliced_outputs(n, m, dtype):
    """(big, out, mask of big outside out) for ``big[1::2, 2::3]`` and for the transpose of such a slice: two non-unit
    strides either way."""
    big = torch.full((2 * n + 2, 3 * m + 4), CANARY, dtype=dtype, device=DEV)
    mask = torch.ones_like(big, dtype=torch.bool)
    mask[1:1 + 2 * n:2, 2:2 + 3 * m:3] = False
    big_t = torch.full((3 * m + 4, 2 * n + 2), CANARY, dtype=dtype, device=DEV)
    mask_t = torch.ones_like(big_t, dtype=torch.bool)
    mask_t[2:2 + 3 * m:3, 1:1 + 2 * n:2] = False
    return [(big, big[1:1 + 2 * n:2, 2:2 + 3 * m:3], mask), (big_t, big_t[2:2 + 3 * m:3, 1:1 + 2 * n:2].T, mask_t)]


def assert_dense_readback(eng, n, m, v=0):
    refs = references(eng, v)
    for dtype, ref in refs.items():
        for order in ("C", "F"):
            got = eng.get_view_device(v, dtype=dtype, order=order)
            assert got.device == torch.device(DEV) and got.dtype == dtype
            if n > 1 and m > 1:
                assert got.stride() == ((m, 1) if order == "C" else (1, n))
            assert bits_equal(got, ref), (dtype, order)
            if not torch.isnan(ref).any():
                assert torch.equal(got, ref)
        for big, out, mask in sliced_outputs(n, m, dtype):
            assert tuple(out.shape) == (n, m)
            if n > 1 and m > 1:
                assert 1 not in out.stride()
            assert eng.get_view_device(v, out=out) is out
            assert bits_equal(out, ref), (dtype, out.stride())
            assert bool((big[mask] == CANARY).all())    # nothing outside the slice was written


# ------------------------------------------------------------------------------------------------------ dense read-back
@pytest.mark.parametrize("shape", DENSE_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_dense_readback_equals_get_view(shape):
    n, m = shape
    with Engine([n], [m], [min(2, n, m)]) as eng:
        eng.set_view(0, view_data(n, m, 3))
        assert_dense_readback(eng, n, m)
        eng.set_view_raw(0, raw_data(n, m, 4))
        assert_dense_readback(eng, n, m)


def test_dense_readback_of_device_drawn_views():
    n, m = 70, 50
    rng = np.random.default_rng(5)
    rows, cols = rng.choice(n, 41, replace=False), rng.choice(m, 33, replace=False)
    with Engine([n], [m], [2]) as src, Engine([n], [m], [2]) as shuf, Engine([41], [33], [2]) as sub:
        src.set_view(0, view_data(n, m, 6))
        shuf.shuffle_view_from(0, src, 0, seed=11)
        assert_dense_readback(shuf, n, m)
        assert not bits_equal(shuf.get_view_device(0), src.get_view_device(0))
        sub.subsample_view_from(0, src, 0, rows, cols)
        assert_dense_readback(sub, 41, 33)
        assert bits_equal(sub.get_view_device(0, dtype=torch.float64), references(src)[torch.float64][rows][:, cols])


def test_dense_readback_is_ordered_with_the_callers_stream():
    n, m = 1024, 40
    with Engine([n], [m], [2]) as eng:
        eng.set_view(0, view_data(n, m, 7))
        ref = references(eng)[torch.float32]
        buf = torch.empty((n, m), dtype=torch.float32, device=DEV)
        a = torch.rand((2048, 2048), device=DEV)
        side = torch.cuda.Stream(device=DEV)
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            torch.mm(a, a)                              # (work in front of the fill)
            buf.fill_(float("nan"))
            eng.get_view_device(0, out=buf)
            buf.mul_(2.0)
        side.synchronize()
        assert not bool(torch.isnan(buf).any())
        assert bits_equal(buf, ref * 2.0)


def test_dense_readback_refusals_leave_out_untouched():
    n, m = 33, 65
    lib = _lib.load()
    vp = C.c_void_p
    with Engine([n], [m], [2]) as eng, Engine([n], [m], [2]) as bare, Engine([n], [m], [2], nnz=[40]) as sparse_eng:
        eng.set_view(0, view_data(n, m, 8))
        out = torch.full((n, m), CANARY, dtype=torch.float32, device=DEV)
        wide = torch.full((n, 2 * m), CANARY, dtype=torch.float32, device=DEV)
        half = torch.full((n, m), CANARY, dtype=torch.float16, device=DEV)
        host = np.full((n, m), CANARY, dtype=np.float32)

        def call(h=eng, ptr=out.data_ptr(), dtype=_lib.DTYPE_F32, rs=m, cs=1):
            return lib.resnmtf_get_view_device(h._h, 0, vp(ptr), dtype, rs, cs, None)

        sparse_eng.set_view_sparse(0, sp.csc_matrix(np.eye(n, m)), pre_processed=True)
        assert call(h=sparse_eng) == INVALID                                        # a sparse view
        with pytest.raises(ResnmtfError, match="INVALID.*sparse"):
            sparse_eng.get_view_device(0, out=out)
        assert call(ptr=half.data_ptr(), dtype=_lib.DTYPE_F16) == INVALID           # narrowing is not a copy
        assert call(ptr=half.data_ptr(), dtype=_lib.DTYPE_BF16) == INVALID
        assert call(dtype=9) == INVALID
        for bad in (half, half.to(torch.bfloat16)):
            with pytest.raises(ValueError, match="narrowing"):
                eng.get_view_device(0, out=bad)
        with pytest.raises(ValueError, match="narrowing"):
            eng.get_view_device(0, dtype=torch.float16)
        assert call(rs=1, cs=0) == INVALID                                          # an expand()ed tensor: stride 0
        assert call(rs=0, cs=1) == INVALID
        assert call(rs=-m, cs=1) == INVALID
        with pytest.raises(ValueError, match="positive"):
            eng.get_view_device(0, out=out[:, :1].expand(n, m))
        assert call(ptr=wide.data_ptr(), rs=1, cs=2) == INVALID                     # overlapping strides
        assert call(rs=m - 1, cs=1) == INVALID
        assert call(rs=1, cs=n - 1) == INVALID
        with pytest.raises(ValueError, match="share an address"):
            eng.get_view_device(0, out=torch.as_strided(wide, (n, m), (1, 2)))
        with pytest.raises(ValueError, match="shape"):
            eng.get_view_device(0, out=wide)
        with pytest.raises(ValueError, match="shape"):
            eng.get_view_device(0, out=out.T)
        with pytest.raises(ValueError, match="lives on"):
            eng.get_view_device(0, out=torch.zeros((n, m)))
        assert call(ptr=host.ctypes.data) == INVALID                                # a raw host pointer
        assert call(ptr=0) == INVALID
        assert call(h=bare) == STATE                                                # a view with no data
        with pytest.raises(ResnmtfError, match="STATE"):
            bare.get_view_device(0, out=out)
        for t in (out, wide, half.float()):
            assert bool((t == CANARY).all())
        assert (host == CANARY).all()
        assert bits_equal(eng.get_view_device(0, out=out), references(eng)[torch.float32])      # the handle is usable


# ----------------------------------------------------------------------------------------------------- sparse read-back
def _f32(a):
    return np.asarray(a).astype(np.float32).astype(np.float64)


def _upload_csc(eng, v, c, pre_processed):
    """resnmtf_set_view_csc with the arrays as they are (Engine.set_view_sparse would drop the explicit zeros)."""
    col_ptr = np.ascontiguousarray(c.indptr, dtype=np.int64)
    row_idx = np.ascontiguousarray(c.indices, dtype=np.int32)
    vals = np.ascontiguousarray(c.data, dtype=np.float64)
    if row_idx.size == 0:
        row_idx = np.zeros(1, dtype=np.int32); vals = np.zeros(1)
    eng._check(eng._lib.resnmtf_set_view_csc(eng._h, v, col_ptr.ctypes.data_as(C.POINTER(C.c_longlong)), _ip(row_idx), _dp(vals),
                                             1 if pre_processed else 0))


def _sparse_case(name):
    """(CSC with sorted indices and its explicit zeros kept, pre_processed)."""
    if name in ("150x90_3pct", "150x90_30pct"):
        density = 0.03 if name.endswith("3pct") else 0.3
        d = sp.random(150, 90, density=density, random_state=12, format="csc")
        d.data = _f32(d.data + 0.05)
        d = d.toarray()
        d[17, :] = _f32(np.random.default_rng(13).random(90) + 0.1)      # a dense row (every column has a positive entry)
        d[40, :] = 0.0                                                   # an all-zero row
        c = sp.csc_matrix(d)
        at = int(np.flatnonzero(c.indices != 17)[3])
        c.data[at] = 1.0e-60                                             # one stored entry that is an explicit zero in fp32
        return c, False
    if name == "40x30_zero_column":
        d = sp.random(40, 30, density=0.2, random_state=14, format="csc").toarray()
        d[:, 7] = 0.0
        return sp.csc_matrix(_f32(d)), True
    if name == "1x1":
        return sp.csc_matrix(np.array([[0.75]])), True
    if name == "50x30_empty":
        return sp.csc_matrix((50, 30)), True
    raise KeyError(name)


def _sparse_engine(shape, nnz):
    return Engine([shape[0]], [shape[1]], [min(2, *shape)], nnz=[nnz])


def _same_csc(a, b):
    return (np.array_equal(a.indptr, b.indptr) and np.array_equal(a.indices, b.indices) and a.data.tobytes() == b.data.tobytes())


def _np(t):
    return t.cpu().numpy()


def coo_int32_arrays(eng, v, nnz):
    """The int32 row and column indices of the COO read-back as the library writes them (no tensor in between)."""
    rows = torch.full((max(nnz, 1),), -1, dtype=torch.int32, device=DEV)
    cols = torch.full((max(nnz, 1),), -1, dtype=torch.int32, device=DEV)
    eng._check(eng._lib.resnmtf_get_view_sparse_device(eng._h, v, _lib.SPARSE_COO, C.c_void_p(rows.data_ptr()), C.c_void_p(cols.data_ptr()),
                                                       _lib.INDEX_I32, None, _lib.DTYPE_F32, None))
    return _np(rows)[:nnz], _np(cols)[:nnz]


def assert_sparse_readback(eng, second=None, combos=None, v=0):
    """Every layout x index dtype x value dtype of view v against ``get_view_sparse`` converted by SciPy; ``second``: the
    round trip through ``set_view_sparse_device(pre_processed=True)`` into that engine."""
    held = eng.get_view_sparse(v)
    held.has_sorted_indices = True                      # (canonical: nothing is re-sorted, explicit zeros stay)
    csr = held.tocsr()
    coo = csr.tocoo()
    assert csr.nnz == held.nnz == coo.nnz and csr.has_sorted_indices
    want = {"csc": (held.indptr, held.indices, held.data), "csr": (csr.indptr, csr.indices, csr.data),
            "coo": (coo.row, coo.col, coo.data)}
    combos = combos or [(lay, it, dt) for lay in ("csc", "csr", "coo") for it in (torch.int32, torch.int64)
                        for dt in (torch.float32, torch.float64)]
    for layout, index_dtype, dtype in combos:
        t = eng.get_view_sparse_device(v, layout=layout, index_dtype=index_dtype, dtype=dtype)
        assert t.device == torch.device(DEV) and tuple(t.shape) == held.shape and t.dtype == dtype
        if layout == "csc":
            assert t.layout == torch.sparse_csc
            a, b, vals = t.ccol_indices(), t.row_indices(), t.values()
        elif layout == "csr":
            assert t.layout == torch.sparse_csr
            a, b, vals = t.crow_indices(), t.col_indices(), t.values()
        else:
            assert t.layout == torch.sparse_coo and t.is_coalesced()
            a, b, vals = t._indices()[0], t._indices()[1], t._values()
        # (torch keeps the indices of a COO tensor as int64 whatever it is given: coo_int32_arrays reads the library's own)
        held_as = torch.int64 if layout == "coo" else index_dtype
        assert a.dtype == held_as and b.dtype == held_as and vals.dtype == dtype
        wa, wb, wv = want[layout]
        assert np.array_equal(_np(a), wa) and np.array_equal(_np(b), wb), (layout, index_dtype)
        np_dt = np.float32 if dtype == torch.float32 else np.float64
        assert _np(vals).tobytes() == np.asarray(wv).astype(np_dt).tobytes(), (layout, dtype)
        assert np.asarray(wv).astype(np_dt).astype(np.float64).tobytes() == np.asarray(wv, dtype=np.float64).tobytes()
        if layout == "coo" and index_dtype == torch.int32:
            rows, cols = coo_int32_arrays(eng, v, held.nnz)
            assert np.array_equal(rows, coo.row) and np.array_equal(cols, coo.col)
        if second is not None:
            second.set_view_sparse_device(0, t, pre_processed=True)
            assert _same_csc(second.get_view_sparse(0), held), (layout, index_dtype, dtype)


@pytest.mark.parametrize("name", ["150x90_3pct", "150x90_30pct", "40x30_zero_column", "1x1", "50x30_empty"])
def test_sparse_readback_equals_get_view_sparse(name):
    c, pre = _sparse_case(name)
    with _sparse_engine(c.shape, c.nnz) as eng, _sparse_engine(c.shape, c.nnz) as second:
        _upload_csc(eng, 0, c, pre)
        held = eng.get_view_sparse(0)
        assert held.nnz == c.nnz and np.array_equal(held.indices, c.indices)
        if name.startswith("150x90"):
            assert (held.data == 0).sum() == 1 and (np.diff(held.tocsr().indptr) == 0).sum() >= 1
        if name == "40x30_zero_column":
            assert (np.diff(held.indptr) == 0).sum() >= 1
        assert_sparse_readback(eng, second)


def test_sparse_readback_of_device_drawn_views():
    c, pre = _sparse_case("150x90_30pct")
    rng = np.random.default_rng(15)
    rows, cols = rng.choice(150, 120, replace=False), rng.choice(90, 61, replace=False)
    some = [("csc", torch.int64, torch.float32), ("csr", torch.int32, torch.float64), ("coo", torch.int64, torch.float64)]
    with _sparse_engine(c.shape, c.nnz) as src, _sparse_engine(c.shape, c.nnz) as shuf:
        _upload_csc(src, 0, c, pre)
        shuf.shuffle_view_sparse_from(0, src, 0, seed=1000003 * 3 + 1, normalise=False)
        assert not _same_csc(shuf.get_view_sparse(0), src.get_view_sparse(0))
        assert_sparse_readback(shuf, combos=some)
        count = src.subsample_count_sparse(0, rows, cols)
        with _sparse_engine((120, 61), count) as sub:
            sub.subsample_view_sparse_from(0, src, 0, rows, cols)
            assert sub.view_storage(0)[1] == count
            assert_sparse_readback(sub, combos=some)


def test_sparse_readback_refusals():
    lib = _lib.load()
    vp = C.c_void_p
    c, pre = _sparse_case("40x30_zero_column")
    with _sparse_engine(c.shape, c.nnz) as eng, Engine([40], [30], [2]) as dense, _sparse_engine(c.shape, c.nnz) as bare:
        _upload_csc(eng, 0, c, pre)
        dense.set_view(0, view_data(40, 30, 16))
        ptr = torch.full((31,), -1, dtype=torch.int64, device=DEV)
        idx = torch.full((c.nnz,), -1, dtype=torch.int64, device=DEV)
        vals = torch.full((c.nnz,), CANARY, dtype=torch.float32, device=DEV)
        host_ptr = np.full(31, -1, dtype=np.int64)

        def call(h=eng, layout=_lib.SPARSE_CSC, a=ptr.data_ptr(), index_type=_lib.INDEX_I64, dtype=_lib.DTYPE_F32):
            return lib.resnmtf_get_view_sparse_device(h._h, 0, layout, vp(a), vp(idx.data_ptr()), index_type, vp(vals.data_ptr()),
                                                      dtype, None)

        assert call(h=dense) == INVALID
        with pytest.raises(ResnmtfError, match="INVALID.*dense"):
            dense.get_view_sparse_device(0)
        assert call(layout=7) == INVALID
        assert call(index_type=5) == INVALID
        assert call(dtype=9) == INVALID
        assert call(dtype=_lib.DTYPE_F16) == INVALID and call(dtype=_lib.DTYPE_BF16) == INVALID
        assert call(a=host_ptr.ctypes.data) == INVALID
        assert call(h=bare) == STATE
        for bad, kw in ((ValueError, dict(layout="bsr")), (ValueError, dict(index_dtype=torch.int16)),
                        (ValueError, dict(dtype=torch.float16))):
            with pytest.raises(bad):
                eng.get_view_sparse_device(0, **kw)
        assert bool((ptr == -1).all()) and bool((idx == -1).all()) and bool((vals == CANARY).all()) and (host_ptr == -1).all()
        assert call() == 0                              # the handle is usable, and NULL arrays are skipped
        assert np.array_equal(_np(ptr), c.indptr) and np.array_equal(_np(idx), c.indices)
        idx.fill_(-1)
        assert lib.resnmtf_get_view_sparse_device(eng._h, 0, _lib.SPARSE_CSC, None, None, _lib.INDEX_I64, vp(vals.data_ptr()),
                                                  _lib.DTYPE_F32, None) == 0
        assert bool((idx == -1).all()) and _np(vals).tobytes() == c.data.astype(np.float32).tobytes()


# --------------------------------------------------------------------------------------------------- reference clusters
def _factors(rng, n, m, k, power=3.0):
    f = rng.random((n, k)) ** power + 1e-3
    g = rng.random((m, k)) ** power + 1e-3
    s = rng.random((k, k)) + np.eye(k)
    return f, s, g


def cluster_forms(rc, cc):
    """The same 0 / 1 matrices as they come from ``finalise_device`` (fp64 column-major), as fp32 row-major, as bf16 and
    as a slice with two non-unit strides of a larger fp16 tensor."""
    def sliced(t):
        big = torch.full((2 * t.shape[0] + 2, 3 * t.shape[1] + 4), 0.5, dtype=torch.float16, device=DEV)
        big[1:1 + 2 * t.shape[0]:2, 2:2 + 3 * t.shape[1]:3] = t.to(torch.float16)
        return big[1:1 + 2 * t.shape[0]:2, 2:2 + 3 * t.shape[1]:3]
    forms = {"fp64_col": (rc, cc), "fp32_row": (rc.float().contiguous(), cc.float().contiguous()),
             "bf16": (rc.to(torch.bfloat16), cc.to(torch.bfloat16)), "slice": (sliced(rc), sliced(cc)),
             "minus_zero": (torch.where(rc == 0, -0.0, rc), torch.where(cc == 0, -0.0, cc))}
    assert forms["fp32_row"][0].is_contiguous() and bool(torch.signbit(forms["minus_zero"][0]).any())
    for a, b in forms.values():
        assert torch.equal(a.double(), rc.double()) and torch.equal(b.double(), cc.double())
    return forms


def relevance_bits(subs, base, v):
    """relevance and relevance_masked of every (sub-sample handle, rows, cols, flags) against base's view v, as bytes."""
    out = []
    for eng, rows, cols, flags in subs:
        out.append(eng.relevance(v, base, v, rows, cols).tobytes())
        out.append(eng.relevance_masked(v, base, v, rows, cols, flags).tobytes())
    return out


def sub_handles(rng, N, M, k, shapes, v=0, n_views=1):
    """Handles with random factors and index lists into an N x M reference view (repeats allowed: a handle may be wider
    than the reference view, which is how k = 64 meets a 47-column view -- a handle's own k cannot exceed its extents)."""
    subs = []
    for n, m in shapes:
        eng = Engine([n] * n_views, [m] * n_views, [k] * n_views)
        eng.set_factors(v, *_factors(rng, n, m, k))
        flags = rng.random(k) < 0.3
        flags[0] = True
        subs.append((eng, rng.choice(N, n, replace=n > N), rng.choice(M, m, replace=m > M), flags))
    return subs


def assert_device_route_equals_host_route(rc, cc, N, M, k, subs, host_base, dev_base, v=0):
    host_base.set_reference_clusters(v, _np(rc), _np(cc))
    want = relevance_bits(subs, host_base, v)
    for name, (a, b) in cluster_forms(rc, cc).items():
        dev_base.set_reference_clusters_device(v, a, b)
        assert relevance_bits(subs, dev_base, v) == want, name
        dev_base.set_reference_clusters_device(v, torch.zeros_like(a), torch.ones_like(b))      # (gone before the next form)
    dev_base.set_reference_clusters_device(v, rc, cc)
    return want


def assert_refusals_keep_the_clusters(rc, cc, k, subs, dev_base, want, v=0):
    for which in (0, 1):
        for bad in (0.5, 2.0, float("nan")):
            pair = [rc.clone(), cc.clone()]
            pair[which][pair[which].shape[0] // 2, k - 1] = bad
            with pytest.raises(ResnmtfError, match="INVALID.*" + ("row" if which == 0 else "col") + "_clusters entries must be 0 or 1"):
                dev_base.set_reference_clusters_device(v, *pair)
            assert relevance_bits(subs, dev_base, v) == want, (which, bad)
    both = [rc.clone(), cc.clone()]
    both[0][0, 0] = 3.0; both[1][0, 0] = 3.0
    with pytest.raises(ResnmtfError, match="row_clusters entries"):      # (the row matrix's message comes first)
        dev_base.set_reference_clusters_device(v, *both)
    for bad_k in (0, 65):
        with pytest.raises(ResnmtfError, match="INVALID"):
            dev_base.set_reference_clusters_device(v, torch.zeros((rc.shape[0], bad_k), dtype=torch.float64, device=DEV),
                                                   torch.zeros((cc.shape[0], bad_k), dtype=torch.float64, device=DEV))
    with pytest.raises(ValueError, match="lives on"):
        dev_base.set_reference_clusters_device(v, rc.cpu(), cc)
    lib = _lib.load()
    host = np.asfortranarray(_np(rc))
    descs = [_lib.DeviceMatrix(host.ctypes.data, _lib.DTYPE_F64, 1, rc.shape[0]),
             _lib.DeviceMatrix(cc.data_ptr(), _lib.DTYPE_F64, int(cc.stride(0)), int(cc.stride(1)))]
    assert lib.resnmtf_set_reference_clusters_device(dev_base._h, v, k, C.byref(descs[0]), C.byref(descs[1]), None) == INVALID
    descs[0] = _lib.DeviceMatrix(rc.data_ptr(), 9, int(rc.stride(0)), int(rc.stride(1)))
    assert lib.resnmtf_set_reference_clusters_device(dev_base._h, v, k, C.byref(descs[0]), C.byref(descs[1]), None) == INVALID
    descs[0] = _lib.DeviceMatrix(rc.data_ptr(), _lib.DTYPE_F64, -1, int(rc.stride(1)))
    assert lib.resnmtf_set_reference_clusters_device(dev_base._h, v, k, C.byref(descs[0]), C.byref(descs[1]), None) == INVALID
    assert lib.resnmtf_set_reference_clusters_device(dev_base._h, v, k, None, C.byref(descs[1]), None) == INVALID
    assert relevance_bits(subs, dev_base, v) == want


def test_reference_clusters_from_the_two_view_planted_problem():
    from test_gpu_stability import _two_view_problem
    data, rn, cn, phi, k = _two_view_problem()
    pre = naming.check_data(data)
    shapes = [d.shape for d in pre]
    rng = np.random.default_rng(22)
    with Engine([s[0] for s in shapes], [s[1] for s in shapes], [k, k]) as src, \
            Engine([s[0] for s in shapes], [s[1] for s in shapes], [2, 2]) as host_base, \
            Engine([s[0] for s in shapes], [s[1] for s in shapes], [2, 2]) as dev_base:
        for v in range(2):
            src.set_view(v, pre[v])
            src.init_svd(v, seed=4 + v)
        src.set_restrictions()
        src.run(60)
        for v in range(2):
            rc, cc = src.finalise_device(v)[3:]
            assert rc.stride() == (1, shapes[v][0]) and 0 < float(rc.sum()) < rc.numel()
            subs = sub_handles(rng, shapes[v][0], shapes[v][1], k, [(int(0.8 * shapes[v][0]), 80), (33, 65)], v=v, n_views=2)
            try:
                want = assert_device_route_equals_host_route(rc, cc, *shapes[v], k, subs, host_base, dev_base, v=v)
                if v == 0:
                    assert_refusals_keep_the_clusters(rc, cc, k, subs, dev_base, want, v=v)
            finally:
                for s in subs:
                    s[0].close()


@pytest.mark.parametrize("k", [1, 64])
def test_reference_clusters_of_a_130x47_view(k):
    """k = 64 exceeds the view's 47 columns, and a handle's own k cannot exceed its extents: the clusters then come from
    ``finalise_device`` of a 130 x 64 handle (its column clusters cut to their first 47 rows, a strided slice), and the
    sub-sample handles are 64 and 70 columns wide with repeated column indices (and at least 64 rows)."""
    N, M = 130, 47
    rng = np.random.default_rng(23 + k)
    m_src = max(M, k)
    with Engine([N], [m_src], [k]) as src, Engine([N], [M], [2]) as host_base, Engine([N], [M], [2]) as dev_base:
        src.set_factors(0, *_factors(rng, N, m_src, k, power=1.0))
        rc, cc = src.finalise_device(0)[3:]
        cc = cc[:M]
        assert tuple(rc.shape) == (N, k) and tuple(cc.shape) == (M, k) and float(rc.sum()) > 0
        subs = sub_handles(rng, N, M, k, [(100, max(40, k)), (130, 70), (max(33, k + 6), max(35, k))])
        try:
            want = assert_device_route_equals_host_route(rc, cc, N, M, k, subs, host_base, dev_base)
            assert_refusals_keep_the_clusters(rc, cc, k, subs, dev_base, want)
        finally:
            for s in subs:
                s[0].close()


# ----------------------------------------------------------------------------------------------- through the public layer
def test_stability_check_scores_device_clusters_from_the_device(monkeypatch):
    from test_gpu_stability import _two_view_problem
    data, rn, cn, phi, k = _two_view_problem()
    p = prepare(data, phi, None, None, rn, cn, normalise=True, symmetrise=True)
    kw = dict(k_vec=[k, k], phi=p.phi, xi=p.xi, psi=p.psi, n_iters=60, spurious=False, row_names=p.row_names,
              col_names=p.col_names, seed=4)
    res_np = resnmtf_amd.res_nmtf_inner(p.data, p.row_shared, p.col_shared, **kw)
    res_t = resnmtf_amd.res_nmtf_inner(p.data, p.row_shared, p.col_shared, output="torch", **kw)
    assert all(isinstance(t, torch.Tensor) and t.device == torch.device(DEV) for t in res_t["row_clusters"] + res_t["col_clusters"])
    host_calls, dev_calls = [], []
    real_host, real_dev = Engine.set_reference_clusters, Engine.set_reference_clusters_device
    monkeypatch.setattr(Engine, "set_reference_clusters", lambda self, *a: (host_calls.append(a), real_host(self, *a))[1])
    monkeypatch.setattr(Engine, "set_reference_clusters_device", lambda self, *a: (dev_calls.append(a), real_dev(self, *a))[1])
    skw = dict(row_names=p.row_names, col_names=p.col_names, seed=9, n_stability=2, sample_rate=0.8)
    args = (k, p.phi, p.xi, p.psi, 60, False, 5, False, "euclidean")
    rel_np = api.stability_check(p.data, res_np, *args, remove_unstable=False, **skw)
    assert len(host_calls) == 2 and not dev_calls
    del host_calls[:]
    rel_t = api.stability_check(p.data, res_t, *args, remove_unstable=False, output="torch", **skw)
    assert not host_calls and len(dev_calls) == 2
    assert rel_t["res"] is res_t and rel_t["relevance"].tobytes() == rel_np["relevance"].tobytes()
    vals = np.unique(rel_np["relevance"])
    thr = float((vals[0] + vals[1]) / 2) if len(vals) > 1 else float(vals[0]) + 1e-9
    out_np = api.stability_check(p.data, res_np, *args, stab_thres=thr, **skw)
    del host_calls[:]
    out_t = api.stability_check(p.data, res_t, *args, stab_thres=thr, output="torch", **skw)
    assert not host_calls and list(out_t) == list(out_np)
    assert any((rel_np["relevance"][v] < thr).any() for v in range(2))
    for key in out_np:
        if key in ("row_clusters", "col_clusters"):
            for t, a, given in zip(out_t[key], out_np[key], res_t[key]):
                assert isinstance(t, torch.Tensor) and t.device == torch.device(DEV) and t is not given
                assert t.dtype == torch.float64 and _np(t).tobytes() == np.ascontiguousarray(a).tobytes()
        elif isinstance(out_np[key], list) and out_np[key] and isinstance(out_np[key][0], np.ndarray):
            for t, a in zip(out_t[key], out_np[key]):
                assert _np(t).tobytes() == np.ascontiguousarray(a).tobytes() if isinstance(t, torch.Tensor) else np.array_equal(t, a)
    out_mixed = api.stability_check(p.data, res_t, *args, stab_thres=thr, **skw)      # device clusters, NumPy asked for
    for key in ("row_clusters", "col_clusters"):
        for a, b in zip(out_mixed[key], out_np[key]):
            assert isinstance(a, np.ndarray) and a.tobytes() == b.tobytes()


def test_factorise_returns_the_shuffled_sparse_view_on_the_device():
    from test_gpu_sparse_shuffle import planted_sparse
    data = [planted_sparse(1)[0], planted_sparse(2)[0]]
    pre = naming.check_data(data)
    rn, cn = naming.give_names(data, None, None, None, None)
    zero = np.zeros((2, 2))
    k, shuffle_seed = 3, 4 * 7919 + 1
    dev = batched.DeviceData(pre, zero, zero, zero, rn, cn, pre_processed=True)
    try:
        with pytest.raises(NotImplementedError, match=r"return_data of a shuffled sparse view is not supported \(it would densify the shuffle\)"):
            dev.factorise(k, 5, 1, shuffle_seed=shuffle_seed, shuffle_sparse=True, return_data=True, output="numpy")
        res = dev.factorise(k, 5, 1, shuffle_seed=shuffle_seed, shuffle_sparse=True, return_data=True, output="torch")
        assert res["data"] == [None, None] and len(res["device_data"]) == 2
        for v in range(2):
            t = res["device_data"][v]
            assert t.layout == torch.sparse_csc and t.device == torch.device(DEV) and t.dtype == torch.float32
            held = dev.base.get_view_sparse(v)
            assert shuffle_ref.attempts_needed(held, shuffle_seed, v) == 1
            want = shuffle_ref.shuffle_csc(held, shuffle_ref.draw_seed(shuffle_seed, 0, v))
            with _sparse_engine(want.shape, want.nnz) as ref:
                _upload_csc(ref, 0, want, False)        # (re-normalised, as the shuffle is: R/obtain_bicl.r:35)
                assert _np(t.to_dense().double()).tobytes() == np.ascontiguousarray(ref.get_view_sparse(0).toarray()).tobytes()
        plain = dev.factorise(k, 5, 1, return_data=True, output="torch")      # unshuffled: both forms, the same values
        dense_dev = batched.DeviceData([_f32(d.toarray()) for d in pre], zero, zero, zero, rn, cn, pre_processed=True)
        try:
            dd = dense_dev.factorise(k, 5, 1, return_data=True, output="torch")
        finally:
            dense_dev.close()
        for v in range(2):
            assert _np(plain["device_data"][v].to_dense().double()).tobytes() == np.ascontiguousarray(plain["data"][v]).tobytes()
            assert dd["device_data"][v].layout == torch.strided and dd["device_data"][v].dtype == torch.float32
            assert _np(dd["device_data"][v].double()).tobytes() == np.ascontiguousarray(dd["data"][v]).tobytes()
        assert "device_data" not in dev.factorise(k, 5, 1, return_data=True)
    finally:
        dev.close()
