"""The sub-sample of a sparse view in double precision (resnmtf_fp64_subsample_sparse):
engine.fp64_subsample_sparse bit for bit (as uint64 words) against subsample_ref.subsample_csc + host_masks of the source --
which does not round --, against engine.fp64_subsample of the densified view read at the stored positions (+0.0 everywhere
else), against the f32 sparse route on fp32-valued data, from every layout, index type and value type a device view may
have, in count mode, feeding engine.fp64_run, and the guards of the C entry.  Every comparison is bit for bit.

Values are uniform doubles that fp32 does not hold unless a test says otherwise.  The shapes are the smallest at which each
kernel can still go wrong: a column walk of 64 entries per trip (columns of 0, 1, 63, 64, 65, 129 and 130 stored entries),
a scan in blocks of 256 counts (m_sub = 1, 255, 256, 257, 1025), rows that arrive in the wrong order (a reversed list), and
positions beyond 32 bits."""
import ctypes as C
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import fp64_shuffle_sparse_ref as R
from subsample_ref import host_masks, subsample_csc
from resnmtf_amd import _lib, device_views, engine
from resnmtf_amd._lib import ResnmtfError
from resnmtf_amd.engine import Engine

gpu = pytest.mark.gpu
SENTINEL = -12345
SCAN_BLOCK = 256            # F64_SUBSAMPLE_SPARSE_SCAN_BLOCK (csrc/resnmtf_fp64_subsample_sparse_job.h)


def _torch_dev():
    import torch
    return torch, torch.device("cuda", 0)


def doubles(count, seed):
    v = np.random.default_rng(seed).random(count) + 0.25
    assert count < 2 or (v.astype(np.float32).astype(np.float64) != v).any()
    return v


def pattern(n, m, density, seed):
    mask = np.random.default_rng(seed).random((n, m)) < density
    cols, rows = np.nonzero(mask.T)
    return rows.astype(np.int64), cols.astype(np.int64)


def draw(extent, count, seed):
    return np.random.default_rng(seed).permutation(extent)[:count].astype(np.int64)


@functools.lru_cache(maxsize=None)
def case(name):
    """(n, m, rows, cols, values of the source in canonical CSC order -- explicit zeros in `values` --, row list, column list)."""
    if name == "1x1":
        return 1, 1, np.zeros(1, np.int64), np.zeros(1, np.int64), doubles(1, 1), np.zeros(1, np.int64), np.zeros(1, np.int64)
    if name == "6x4_of_7x5":
        n, m = 7, 5
        rows, cols = pattern(n, m, 0.6, 2)
        rs, cs = draw(n, 6, 3), draw(m, 4, 4)
    elif name == "37x23_zero":                          # 50 %, one explicitly stored zero that the sub-sample keeps
        n, m = 37, 23
        rows, cols = pattern(n, m, 0.5, 5)
        rs, cs = draw(n, 33, 6), draw(m, 20, 7)
    elif name == "64x64_reversed":                      # fully stored, a permutation with the rows reversed: every column
        n = m = 64                                      # arrives in exactly the wrong order
        rows, cols = pattern(n, m, 2.0, 0)
        rs, cs = np.arange(63, -1, -1, dtype=np.int64), draw(m, 64, 8)
    elif name == "130x5_full":                          # two full trips and a partial one
        n, m = 130, 5
        rows, cols = pattern(n, m, 2.0, 0)
        rs, cs = draw(n, 117, 9), draw(m, 5, 10)
    elif name == "300x6_trips":                         # columns of exactly 0, 1, 63, 64, 65 and 129 stored entries, all kept
        n, m = 300, 6
        rng = np.random.default_rng(11)
        counts = [0, 1, 63, 64, 65, 129]
        rows = np.concatenate([np.sort(rng.permutation(n)[:c]) for c in counts]).astype(np.int64)
        cols = np.repeat(np.arange(m), counts).astype(np.int64)
        rs, cs = draw(n, 300, 12), draw(m, 6, 13)
    elif name == "300x200_lines":                       # 5 % with one dense row and one dense column, both sampled
        n, m = 300, 200
        mask = np.random.default_rng(14).random((n, m)) < 0.05
        mask[17, :] = True; mask[:, 31] = True
        cols, rows = (x.astype(np.int64) for x in np.nonzero(mask.T))
        rs, cs = draw(n, 270, 15), draw(m, 180, 16)
        rs[0], cs[0] = 17, 31
        rs, cs = np.unique(rs)[np.random.default_rng(17).permutation(len(np.unique(rs)))], np.unique(cs)[::-1].copy()
    elif name == "300x200_1pct":                        # empty rows and columns occur
        n, m = 300, 200
        rows, cols = pattern(n, m, 0.01, 18)
        rs, cs = draw(n, 270, 19), draw(m, 180, 20)
    elif name == "70000x70000":                         # n_sub m_sub > 2^32
        n = m = 70000
        pos = np.unique(np.random.default_rng(21).integers(0, n * m, 2000, dtype=np.int64))
        order = np.lexsort((pos // m, pos % m))
        rows, cols = (pos // m)[order], (pos % m)[order]
        rs, cs = draw(n, 66500, 22), draw(m, 66500, 23)
    elif name == "50x30_empty":
        n, m = 50, 30
        rows = cols = np.zeros(0, dtype=np.int64)
        rs, cs = draw(n, 45, 24), draw(m, 27, 25)
    elif name == "keeps_nothing":                       # a non-empty source whose sampled rows hold no entry
        n, m = 40, 30
        rows, cols = pattern(10, m, 0.7, 26)
        rs, cs = 10 + draw(30, 25, 27), draw(m, 27, 28)
    elif name.startswith("3x1100_"):                    # m_sub around the scan's block edge
        n, m = 3, 1100
        rows, cols = pattern(n, m, 0.6, 29)
        rs, cs = np.array([2, 0, 1], dtype=np.int64), draw(m, int(name.split("_")[1]), 30)
    else:
        raise KeyError(name)
    vals = doubles(len(rows), 31)
    if name == "37x23_zero":
        inside = np.flatnonzero(np.isin(rows, rs) & np.isin(cols, cs))
        vals[inside[7]] = 0.0
    return n, m, rows, cols, vals, rs, cs


def host_matrix(n, m, rows, cols, vals):
    """The canonical CSC over the arrays as they are (an explicit zero stays)."""
    return R.raw_csc(n, m, *R.csc_parts(n, m, rows, cols, vals))


def device_csc(n, m, rows, cols, vals, index="int64", dtype="float64"):
    torch, dev = _torch_dev()
    indptr, indices, data = R.csc_parts(n, m, rows, cols, vals)
    idx = getattr(torch, index)
    return torch.sparse_csc_tensor(torch.as_tensor(indptr, dtype=idx, device=dev), torch.as_tensor(indices.astype(np.int64), dtype=idx, device=dev),
                                   torch.as_tensor(data, device=dev).to(getattr(torch, dtype)), size=(n, m))


def parts(t):
    """(indptr, indices, values) of a returned sparse_csc tensor on the host, with the layout checks."""
    torch, _ = _torch_dev()
    assert t.layout == torch.sparse_csc and t.dtype == torch.float64 and t.device.type == "cuda"
    assert t.ccol_indices().dtype == torch.int64 and t.row_indices().dtype == torch.int64
    return t.ccol_indices().cpu().numpy(), t.row_indices().cpu().numpy(), t.values().cpu().numpy()


def wanted(src, rs, cs):
    """(indptr, indices, data, empty rows, empty columns) from the helper: it does not round and keeps stored zeros."""
    want = subsample_csc(src, rs, cs)
    er, ec = host_masks(want)
    return want.indptr.astype(np.int64), want.indices.astype(np.int64), want.data, er, ec


def same_as(got, want, what=None):
    t, er, ec = got
    gp, gi, gv = parts(t)
    assert tuple(t.shape) == (len(want[3]), len(want[4])), what
    assert np.array_equal(gp, want[0]) and np.array_equal(gi, want[1]), what
    assert np.array_equal(R.bits(gv), R.bits(want[2])), what
    assert er.dtype == bool and ec.dtype == bool and np.array_equal(er, want[3]) and np.array_equal(ec, want[4]), what
    return gp, gi, gv


def check_against_dense(gp, gi, gv, er, ec, dense_x, rs, cs, what=None):
    """engine.fp64_subsample of the densified view: the values at the stored positions, +0.0 elsewhere, masks equal."""
    d, dr, dc = engine.fp64_subsample(dense_x, rs, cs)
    d = np.ascontiguousarray(d.cpu().numpy())
    col = np.repeat(np.arange(len(cs)), np.diff(gp))
    assert np.array_equal(R.bits(gv), R.bits(d[gi, col])), what
    d[gi, col] = 0.0
    assert not R.bits(d).any(), what
    assert np.array_equal(er, dr) and np.array_equal(ec, dc), what


# ---------------------------------------------------------------------------------------------------------------------
# 0. the shapes say what they claim, on the CPU
# ---------------------------------------------------------------------------------------------------------------------
def test_the_cases_reach_the_edges_they_name():
    n, m, rows, cols, vals, rs, cs = case("300x6_trips")
    w = wanted(host_matrix(n, m, rows, cols, vals), rs, cs)
    assert sorted(np.diff(w[0]).tolist()) == [0, 1, 63, 64, 65, 129]
    n, m, rows, cols, vals, rs, cs = case("64x64_reversed")
    src = host_matrix(n, m, rows, cols, vals)
    w = wanted(src, rs, cs)
    assert len(w[2]) == 64 * 64 and np.array_equal(subsample_csc(src, rs, cs).toarray(), src.toarray()[np.ix_(rs, cs)])
    unsorted = src.toarray()[:, cs].T.ravel()            # the kept entries of each column in SOURCE row order
    assert not np.array_equal(R.bits(unsorted), R.bits(w[2]))
    n, m, rows, cols, vals, rs, cs = case("37x23_zero")
    assert (wanted(host_matrix(n, m, rows, cols, vals), rs, cs)[2] == 0).sum() == 1
    n, m, rows, cols, vals, rs, cs = case("300x200_1pct")
    w = wanted(host_matrix(n, m, rows, cols, vals), rs, cs)
    assert w[3].any() and w[4].any() and not w[3].all()
    n, m, rows, cols, vals, rs, cs = case("keeps_nothing")
    assert len(vals) > 0 and len(wanted(host_matrix(n, m, rows, cols, vals), rs, cs)[2]) == 0
    n, m, rows, cols, vals, rs, cs = case("70000x70000")
    assert len(rs) * len(cs) > 2 ** 32 and len(wanted(host_matrix(n, m, rows, cols, vals), rs, cs)[2]) > 1000
    assert [c for c in (1, 255, 256, 257, 1025)] == [1, SCAN_BLOCK - 1, SCAN_BLOCK, SCAN_BLOCK + 1, 4 * SCAN_BLOCK + 1]


# ---------------------------------------------------------------------------------------------------------------------
# 1. structure, values, masks and counts: the helper and the dense route, host and device route in
# ---------------------------------------------------------------------------------------------------------------------
SMALL = ["1x1", "6x4_of_7x5", "37x23_zero", "64x64_reversed", "130x5_full", "300x6_trips", "300x200_lines", "300x200_1pct",
         "3x1100_1", "3x1100_255", "3x1100_256", "3x1100_257", "3x1100_1025", "50x30_empty", "keeps_nothing"]


@gpu
@pytest.mark.parametrize("name", SMALL)
def test_subsample_against_the_helper_and_the_dense_route(name):
    n, m, rows, cols, vals, rs, cs = case(name)
    src = host_matrix(n, m, rows, cols, vals)
    want = wanted(src, rs, cs)
    got = engine.fp64_subsample_sparse(device_csc(n, m, rows, cols, vals), rs, cs)
    gp, gi, gv = same_as(got, want, (name, "device"))
    check_against_dense(gp, gi, gv, got[1], got[2], src.toarray(), rs, cs, name)
    if name == "37x23_zero":                            # canonical_csc drops the stored zero: the host route of the C entry
        code, text, out = _call(n, m, rs, cs, host=R.csc_parts(n, m, rows, cols, vals))
        assert code == 0, text
        assert (out["vals"] == 0).sum() == 1 and out["nnz_sub"] == len(want[2])
        assert np.array_equal(out["ccol"], want[0]) and np.array_equal(out["rows"], want[1])
        assert np.array_equal(R.bits(out["vals"]), R.bits(want[2]))
        assert np.array_equal(out["row_mask"].astype(bool), want[3]) and np.array_equal(out["col_mask"].astype(bool), want[4])
    else:
        same_as(engine.fp64_subsample_sparse(src, rs, cs), want, (name, "host"))
    if name in ("50x30_empty", "keeps_nothing"):
        assert got[0]._nnz() == 0 and not gp.any() and got[1].all() and got[2].all()
    # count mode: the same number and the same masks
    for x in (src if name != "37x23_zero" else device_csc(n, m, rows, cols, vals), device_csc(n, m, rows, cols, vals)):
        count, cr, cc = engine.fp64_subsample_sparse(x, rs, cs, count_only=True)
        assert count == len(want[2]) and np.array_equal(cr, want[3]) and np.array_equal(cc, want[4]), name


@gpu
@pytest.mark.parametrize("route", ["host", "device"])
def test_beyond_32_bits_of_positions(route):
    n, m, rows, cols, vals, rs, cs = case("70000x70000")
    src = host_matrix(n, m, rows, cols, vals)
    x = src if route == "host" else device_csc(n, m, rows, cols, vals)
    same_as(engine.fp64_subsample_sparse(x, rs, cs), wanted(src, rs, cs), route)


# ---------------------------------------------------------------------------------------------------------------------
# 2. the f32 route on data fp32 holds; where fp32 does not hold the data; repeatability
# ---------------------------------------------------------------------------------------------------------------------
def _f32_route(src, rs, cs):
    """Engine.subsample_view_sparse_from + get_view_sparse + empty_lines: (CSC matrix, empty rows, empty columns)."""
    n, m = src.shape
    with Engine([n], [m], [1], nnz=[src.nnz]) as base:
        base.set_view_sparse(0, src, pre_processed=True)
        count = base.subsample_count_sparse(0, rs, cs)
        with Engine([len(rs)], [len(cs)], [1], nnz=[count]) as e:
            e.subsample_view_sparse_from(0, base, 0, rs, cs)
            er, ec = e.empty_lines(0, counts=True)[:2]
            return e.get_view_sparse(0), np.asarray(er, dtype=bool), np.asarray(ec, dtype=bool)


@gpu
@pytest.mark.parametrize("name", ["6x4_of_7x5", "130x5_full", "300x200_lines", "300x200_1pct"])
def test_equals_the_f32_sparse_route_on_data_fp32_holds(name):
    n, m, rows, cols, vals, rs, cs = case(name)
    src = host_matrix(n, m, rows, cols, vals.astype(np.float32).astype(np.float64))
    want, wr, wc = _f32_route(src, rs.astype(np.int32), cs.astype(np.int32))
    gp, gi, gv = parts(engine.fp64_subsample_sparse(src, rs, cs)[0])
    got = engine.fp64_subsample_sparse(src, rs, cs)
    assert np.array_equal(gp, want.indptr) and np.array_equal(gi, want.indices) and np.array_equal(R.bits(gv), R.bits(want.data))
    assert np.array_equal(got[1], wr) and np.array_equal(got[2], wc)


@gpu
def test_keeps_values_the_f32_route_rounds_to_one():
    n, m = 40, 30
    rows, cols = pattern(n, m, 0.5, 41)
    p = np.random.default_rng(42).random(len(rows))
    vals = 1.0 + 2.0 ** -30 * p
    src = host_matrix(n, m, rows, cols, vals)
    rs, cs = draw(n, 36, 43), draw(m, 27, 44)
    f32_sub = _f32_route(src, rs.astype(np.int32), cs.astype(np.int32))[0]
    assert f32_sub.nnz > 100 and (f32_sub.data == 1.0).all()
    want = wanted(src, rs, cs)
    gp, gi, gv = same_as(engine.fp64_subsample_sparse(src, rs, cs), want)
    assert len(np.unique(gv)) == len(gv) and (gv > 1.0).all()
    assert np.array_equal(gp, f32_sub.indptr) and np.array_equal(gi, f32_sub.indices)


@gpu
def test_two_calls_give_equal_bits_whatever_the_outputs_held():
    n, m, rows, cols, vals, rs, cs = case("300x200_lines")
    host = R.csc_parts(n, m, rows, cols, vals)
    res = []
    for fill in (0x7F, 0x00, 0xA5):
        code, text, out = _call(n, m, rs, cs, host=host, fill=fill)
        assert code == 0, text
        res.append(out)
    for other in res[1:]:
        for key in ("ccol", "rows", "vals", "row_mask", "col_mask"):
            assert res[0][key].tobytes() == other[key].tobytes(), key
        assert [res[0][k] for k in ("nnz_sub", "n_empty_rows", "n_empty_cols")] == [other[k] for k in ("nnz_sub", "n_empty_rows", "n_empty_cols")]
    want = wanted(host_matrix(n, m, rows, cols, vals), rs, cs)
    assert np.array_equal(res[0]["ccol"], want[0]) and np.array_equal(res[0]["rows"], want[1])
    assert np.array_equal(R.bits(res[0]["vals"]), R.bits(want[2]))
    assert (res[0]["n_empty_rows"], res[0]["n_empty_cols"]) == (int(want[3].sum()), int(want[4].sum()))


@gpu
def test_count_mode_writes_nothing_to_the_callers_device_memory():
    torch, dev = _torch_dev()
    n, m, rows, cols, vals, rs, cs = case("300x200_1pct")
    want = wanted(host_matrix(n, m, rows, cols, vals), rs, cs)
    t = device_csc(n, m, rows, cols, vals)
    a, b, v = t.ccol_indices(), t.row_indices(), t.values()
    before = [x.clone() for x in (a, b, v)]
    for route in (dict(host=R.csc_parts(n, m, rows, cols, vals)), dict(dev=(_lib.SPARSE_CSC, a, b, v, len(vals)))):
        code, text, out = _call(n, m, rs, cs, count=True, **route)
        assert code == 0, text
        assert out["outputs_untouched"] and out["nnz_sub"] == len(want[2])
        assert np.array_equal(out["row_mask"].astype(bool), want[3]) and np.array_equal(out["col_mask"].astype(bool), want[4])
        assert (out["n_empty_rows"], out["n_empty_cols"]) == (int(want[3].sum()), int(want[4].sum()))
    assert all(torch.equal(x, y) for x, y in zip((a, b, v), before))          # the source is what it was


# ---------------------------------------------------------------------------------------------------------------------
# 3. every route in: bitwise the host route on the canonical CSC of the same positions and widened values
# ---------------------------------------------------------------------------------------------------------------------
N3, M3 = 33, 97


@functools.lru_cache(maxsize=None)
def _route_case(dtype):
    import torch
    from test_gpu_sparse_device_views import pattern as device_pattern, values
    rows, cols = device_pattern(N3, M3, 0.2, 50)
    v, wide = values(len(rows), getattr(torch, dtype), 52)
    rs, cs = draw(N3, 29, 53), draw(M3, 80, 54)
    t, er, ec = engine.fp64_subsample_sparse(sp.csc_matrix((wide, (rows, cols)), shape=(N3, M3)), rs, cs)
    return rows, cols, v, rs, cs, (*parts(t), er, ec)


@gpu
@pytest.mark.parametrize("index", ("int32", "int64"))
@pytest.mark.parametrize("layout", ("csc", "csc_perm", "csr", "coo"))
def test_layouts_and_index_types(layout, index):
    import torch
    from test_gpu_sparse_device_views import LAYOUT_CODE, arrays, as_tensor, on_device
    rows, cols, v, rs, cs, want = _route_case("float64")
    a, b, vals = on_device(*arrays(layout, rows, cols, v, N3, M3, 3), getattr(torch, index))
    if layout == "coo" and index == "int32":             # (torch's COO indices are int64 only: the C entry itself)
        code, text, out = _call(N3, M3, rs, cs, dev=(LAYOUT_CODE[layout], a, b, vals, len(rows)))
        assert code == 0, text
        assert np.array_equal(out["ccol"], want[0]) and np.array_equal(out["rows"], want[1])
        assert np.array_equal(R.bits(out["vals"]), R.bits(want[2]))
        assert np.array_equal(out["row_mask"].astype(bool), want[3]) and np.array_equal(out["col_mask"].astype(bool), want[4])
    else:
        same_as(engine.fp64_subsample_sparse(as_tensor(layout, a, b, vals, (N3, M3)), rs, cs), want, (layout, index))


@gpu
@pytest.mark.parametrize("dtype", ("float64", "float32", "float16", "bfloat16"))
def test_value_types(dtype):
    import torch
    from test_gpu_sparse_device_views import arrays, as_tensor, on_device
    rows, cols, v, rs, cs, want = _route_case(dtype)
    assert v.dtype == getattr(torch, dtype)
    t = as_tensor("csr", *on_device(*arrays("csr", rows, cols, v, N3, M3, 4), torch.int64), (N3, M3))
    same_as(engine.fp64_subsample_sparse(t, rs, cs), want, dtype)
    same_as(engine.fp64_subsample_sparse(device_views.SparseDeviceView(t), rs, cs), want, dtype)      # (the host layer's own wrapper)


@gpu
@pytest.mark.parametrize("layout", ("csc_perm", "csr", "coo"))
def test_device_view_is_read_where_it_lies(monkeypatch, layout):
    import torch
    from test_gpu_sparse_device_views import arrays, as_tensor, on_device
    rows, cols, v, rs, cs, want = _route_case("float64")
    t = as_tensor(layout, *on_device(*arrays(layout, rows, cols, v, N3, M3, 6), torch.int64), (N3, M3))
    if layout == "csc_perm":
        keep = []
        job = _lib.Fp64SubsampleSparseJob()
        engine._fill_fp64_sparse_source(job, device_views.SparseDeviceView(t), 0, keep, "x")
        assert not job.x.col_ptr and not job.x.row_idx and not job.x.values
        assert (job.x_dev.ptr_or_rows, job.x_dev.idx_or_cols, job.x_dev.values) == (t.ccol_indices().data_ptr(), t.row_indices().data_ptr(),
                                                                                   t.values().data_ptr())

    def refuse(*args, **kwargs):
        raise AssertionError("a tensor was brought to the host")
    for name in ("cpu", "numpy", "tolist", "to_dense"):
        monkeypatch.setattr(torch.Tensor, name, refuse)
    monkeypatch.setattr(device_views, "sparse_tensor_to_scipy", refuse)
    got = engine.fp64_subsample_sparse(t, rs, cs)
    counted = engine.fp64_subsample_sparse(t, rs, cs, count_only=True)
    monkeypatch.undo()
    same_as(got, want, layout)
    assert counted[0] == len(want[2]) and np.array_equal(counted[1], want[3])


# ---------------------------------------------------------------------------------------------------------------------
# 4. feeding the run
# ---------------------------------------------------------------------------------------------------------------------
@gpu
def test_the_subsample_feeds_the_fp64_run_as_a_sparse_device_view():
    """40 x 30 from 50 x 36, k = 3, 3 sweeps: the returned tensor as a sparse device view gives bit for bit the run on the
    helper's SciPy matrix through the host sparse route."""
    from resnmtf_amd import synth
    n, m, k = 50, 36, 3
    rows, cols = pattern(n, m, 0.5, 61)
    src = host_matrix(n, m, rows, cols, doubles(len(rows), 62))
    rs, cs = draw(n, 40, 63), draw(m, 30, 64)
    t, er, ec = engine.fp64_subsample_sparse(src, rs, cs)
    assert not er.any() and not ec.any()
    ref = subsample_csc(src, rs, cs)
    f, s, g = synth.random_init(40, 30, k, 9)
    base = {"k": k, "init_f": [f], "init_s": [s], "init_g": [g], "init_lam": None, "init_mu": None, "phi": np.zeros((1, 1)),
            "xi": np.zeros((1, 1)), "psi": np.zeros((1, 1)), "row_pairs": [[None]], "col_pairs": [[None]], "n_iters": 3}
    a = engine.fp64_run(dict(base, data=[device_views.SparseDeviceView(t)]))
    b = engine.fp64_run(dict(base, data=[ref]))
    for key in ("f", "s", "g", "lambda", "mu"):
        assert np.asarray(a[key][0]).tobytes() == np.asarray(b[key][0]).tobytes(), key
    assert np.asarray(a["all_error"]).tobytes() == np.asarray(b["all_error"]).tobytes() and np.isfinite(a["all_error"]).all()


# ---------------------------------------------------------------------------------------------------------------------
# 5. the C entry: its guards
# ---------------------------------------------------------------------------------------------------------------------
def _call(n, m, rs, cs, host=None, dev=None, struct_size=None, null=(), device_id=0, fill=0x5A, capacity=None, outs=None,
          stream=None, count=False, n_sub=None, m_sub=None):
    """The C entry itself on outputs filled with a byte pattern: (code, text, the outputs and host results).  `count`:
    count mode (no outputs, capacity 0; pattern-filled arrays of the caller are still watched)."""
    import torch
    lib = _lib.load()
    where = torch.device("cuda", 0)
    rs, cs = np.ascontiguousarray(rs, dtype=np.int32), np.ascontiguousarray(cs, dtype=np.int32)
    ns, ms = (len(rs) if n_sub is None else n_sub), (len(cs) if m_sub is None else m_sub)
    nnz = len(host[1]) if host is not None else dev[4] if dev is not None else 0
    cap = max(int(nnz), 0) if capacity is None else capacity
    ccol = torch.empty(max(ms, 0) + 1, dtype=torch.int64, device=where).view(torch.uint8).fill_(fill).view(torch.int64)
    rows = torch.empty(max(cap, 1), dtype=torch.int64, device=where).view(torch.uint8).fill_(fill).view(torch.int64)
    vals = torch.empty(max(cap, 1), dtype=torch.float64, device=where).view(torch.uint8).fill_(fill).view(torch.float64)
    if outs is not None:
        ccol, rows, vals = outs
    tensors = [x for x in (ccol, rows, vals) if torch.is_tensor(x)]
    before = [x.clone() for x in tensors]
    kept, nr, nc = C.c_longlong(SENTINEL), C.c_int(SENTINEL), C.c_int(SENTINEL)
    rm = np.full(max(ns, 1), 7, dtype=np.uint8); cm = np.full(max(ms, 1), 7, dtype=np.uint8)
    job = _lib.Fp64SubsampleSparseJob()
    job.struct_size = C.sizeof(job) if struct_size is None else struct_size
    job.n, job.m, job.n_sub, job.m_sub = n, m, ns, ms
    job.rows, job.cols = rs.ctypes.data_as(C.POINTER(C.c_int)), cs.ctypes.data_as(C.POINTER(C.c_int))
    keep = []
    if host is not None:
        keep = [np.ascontiguousarray(host[0], dtype=np.int64), np.ascontiguousarray(host[1], dtype=np.int32),
                np.ascontiguousarray(host[2], dtype=np.float64)]
        job.x.col_ptr = keep[0].ctypes.data_as(C.POINTER(C.c_longlong))
        job.x.row_idx, job.x.values = keep[1].ctypes.data_as(C.POINTER(C.c_int)), keep[2].ctypes.data_as(C.POINTER(C.c_double))
    if dev is not None:
        layout, a, b, v, stored = dev[:5]
        ptr = lambda x: None if x is None else (x if isinstance(x, int) else x.data_ptr()) or None      # noqa: E731
        kinds = [x.dtype for x in (a, b) if torch.is_tensor(x)]
        c = job.x_dev
        c.layout = layout
        c.index_type = dev[5] if len(dev) > 5 else (_lib.INDEX_I32 if kinds and kinds[0] == torch.int32 else _lib.INDEX_I64)
        c.dtype = dev[6] if len(dev) > 6 else {torch.float64: 0, torch.float32: 1, torch.float16: 2, torch.bfloat16: 3}[v.dtype]
        c.ptr_or_rows, c.idx_or_cols, c.values, c.nnz = ptr(a), ptr(b), ptr(v), stored
    job.stream = stream
    if not count:
        as_ptr = lambda x: x if isinstance(x, int) else x.data_ptr()      # noqa: E731
        job.out_col_ptr, job.out_row_idx, job.out_values = as_ptr(ccol), as_ptr(rows), as_ptr(vals)
        job.out_capacity = cap
    job.nnz_sub = C.pointer(kept)
    job.n_empty_rows, job.n_empty_cols = C.pointer(nr), C.pointer(nc)
    job.row_mask, job.col_mask = rm.ctypes.data_as(C.POINTER(C.c_ubyte)), cm.ctypes.data_as(C.POINTER(C.c_ubyte))
    for name in null:
        setattr(job, name, None)
    torch.cuda.synchronize()
    code = lib.resnmtf_fp64_subsample_sparse(device_id, C.byref(job))
    text = (lib.resnmtf_last_error(None) or b"").decode()
    torch.cuda.synchronize()
    outputs_untouched = all(torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for x, y in zip(tensors, before))
    host_untouched = nr.value == SENTINEL and nc.value == SENTINEL and (rm == 7).all() and (cm == 7).all()
    out = {"outputs_untouched": outputs_untouched, "untouched": outputs_untouched and host_untouched and kept.value == SENTINEL,
           "all_but_nnz_sub_untouched": outputs_untouched and host_untouched, "nnz_sub": kept.value,
           "n_empty_rows": nr.value, "n_empty_cols": nc.value, "row_mask": rm[:max(ns, 0)].copy(), "col_mask": cm[:max(ms, 0)].copy()}
    if code == 0 and not count:
        k = kept.value
        out.update(ccol=ccol.cpu().numpy(), rows=rows[:k].cpu().numpy(), vals=vals[:k].cpu().numpy())
    return code, text, out


def _refused(result, match, code=1):
    got, text, out = result
    assert got == code and match in text, (got, text, match)
    assert out["untouched"], match


@gpu
def test_capacity_refusal_names_both_numbers_and_sets_nnz_sub():
    n, m, rows, cols, vals, rs, cs = case("300x200_lines")
    want = wanted(host_matrix(n, m, rows, cols, vals), rs, cs)
    kept = len(want[2])
    t = device_csc(n, m, rows, cols, vals)
    for route in (dict(host=R.csc_parts(n, m, rows, cols, vals)), dict(dev=(_lib.SPARSE_CSC, t.ccol_indices(), t.row_indices(), t.values(), len(vals)))):
        code, text, out = _call(n, m, rs, cs, capacity=kept - 1, **route)
        assert code == 1 and f"out_capacity = {kept - 1} is below nnz_sub = {kept}" in text
        assert out["nnz_sub"] == kept and out["all_but_nnz_sub_untouched"]
        code, text, out = _call(n, m, rs, cs, capacity=kept, **route)          # exactly enough
        assert code == 0, text
        assert np.array_equal(out["rows"], want[1]) and np.array_equal(R.bits(out["vals"]), R.bits(want[2]))
    # a capacity of 0 with the two arrays NULL is fill mode when the pointers are given: fine when nothing is kept
    n, m, rows, cols, vals, rs, cs = case("keeps_nothing")
    code, text, out = _call(n, m, rs, cs, host=R.csc_parts(n, m, rows, cols, vals), capacity=0, null=("out_row_idx", "out_values"))
    assert code == 0 and out["nnz_sub"] == 0 and not out["ccol"].any(), text


@gpu
def test_guards_of_the_c_entry():
    import torch
    from test_gpu_sparse_device_views import arrays, on_device
    rows, cols, v, rs, cs, want = _route_case("float64")
    nnz = len(rows)
    ccol = np.concatenate([[0], np.cumsum(np.bincount(cols, minlength=M3))])
    host = (ccol, rows, v.numpy())
    a, b, vals = on_device(*arrays("csc", rows, cols, v, N3, M3, 1), torch.int64)
    dev = (_lib.SPARSE_CSC, a, b, vals, nnz)
    call = functools.partial(_call, N3, M3, rs, cs)
    # what resnmtf_fp64_subsample refuses of the extents and the lists, what resnmtf_fp64_shuffle_sparse of source and outputs
    twice = rs.copy(); twice[5] = twice[2]
    high = cs.copy(); high[7] = M3
    for kw, match in ((dict(host=host, struct_size=8), "resnmtf_fp64_subsample_sparse_job struct_size mismatch"),
                      (dict(host=host, n_sub=0), "n_sub must be in [1, n]"),
                      (dict(host=host, n_sub=N3 + 1), "n_sub must be in [1, n]"),
                      (dict(dev=dev, m_sub=M3 + 1), "m_sub must be in [1, m]"),
                      (dict(host=host, null=("rows",)), "rows / cols are NULL"),
                      (dict(dev=dev, null=("cols",)), "rows / cols are NULL"),
                      (dict(host=host, dev=dev), "X is given in two places (job->x and job->x_dev)"),
                      (dict(), "X is given in no place (job->x or job->x_dev)"),
                      (dict(host=host, capacity=-1), "out_capacity is negative"),
                      (dict(host=host, null=("out_col_ptr",)), "out_col_ptr is NULL"),
                      (dict(host=host, null=("out_values",)), "out_row_idx / out_values are NULL"),
                      (dict(dev=dev, null=("out_row_idx",)), "out_row_idx / out_values are NULL"),
                      (dict(host=host, null=("nnz_sub",)), "nnz_sub is NULL"),
                      (dict(host=host, count=True, null=("nnz_sub",)), "nnz_sub is NULL"),
                      (dict(host=host, null=("n_empty_cols",)), "n_empty_rows / n_empty_cols are NULL"),
                      (dict(dev=dev, count=True, null=("n_empty_rows",)), "n_empty_rows / n_empty_cols are NULL"),
                      (dict(host=host, device_id=99), "device_id out of range"),
                      (dict(dev=dev, device_id=-1), "device_id out of range")):
        _refused(call(**kw), match)
    _refused(_call(N3, M3, twice, cs, host=host), f"rows[5] = {twice[5]} occurs twice")
    _refused(_call(N3, M3, rs, high, dev=dev), f"cols[7] = {M3} is out of range [0, {M3})")
    _refused(_call(N3, M3, rs, -1 - cs, host=host, count=True), "cols[0] = ")
    _refused(_call(0, M3, rs, cs, host=host), "view dimensions must be positive")
    _refused(_call(N3, -1, rs, cs, dev=dev), "view dimensions must be positive")
    assert _lib.load().resnmtf_fp64_subsample_sparse(0, None) == 1 and b"job is NULL" in _lib.load().resnmtf_last_error(None)
    # outputs that are not memory of the device, too short, or overlapping
    where = torch.device("cuda", 0)
    ms = len(cs)
    good = lambda: (torch.zeros(ms + 1, dtype=torch.int64, device=where), torch.zeros(nnz, dtype=torch.int64, device=where),      # noqa: E731
                    torch.zeros(nnz, dtype=torch.float64, device=where))
    on_host = np.zeros(max(nnz, ms + 1), dtype=np.int64)
    for at, name in enumerate(("out_col_ptr", "out_row_idx", "out_values")):
        outs = list(good()); outs[at] = on_host.ctypes.data
        _refused(call(host=host, outs=tuple(outs)), name + " is not device memory of device 0")
    # (16 MiB asked of an emptied cache: torch takes a block of exactly that size from the runtime, so the end of the
    # tensor is the end of an allocation)
    torch.cuda.empty_cache()
    big = torch.zeros(1 << 21, dtype=torch.float64, device=where)
    outs = list(good()); outs[2] = big[(1 << 21) - nnz + 1:]
    _refused(call(host=host, outs=tuple(outs)), "out_values reaches beyond its allocation (too short for out_capacity doubles)")
    both = torch.zeros(2 * nnz, dtype=torch.int64, device=where)
    outs = list(good()); outs[1] = both; outs[2] = both.view(torch.float64)[nnz - 1:]
    _refused(call(host=host, outs=tuple(outs)), "out_row_idx overlaps out_values")
    outs = list(good()); outs[2] = vals
    _refused(call(dev=dev, outs=tuple(outs)), "out_values overlaps x_dev.values")
    outs = list(good()); outs[0] = a
    _refused(call(dev=dev, outs=tuple(outs)), "out_col_ptr overlaps x_dev.ptr_or_rows")
    # what resnmtf_fp64_run_sparse refuses of a host view
    p = ccol.copy(); p[3] = p[2] - 1
    i = rows.copy(); i[4] = N3
    w = v.numpy().copy(); w[6] = -1.0
    z = v.numpy().copy(); z[2] = np.inf
    for bad, match in (((p, rows, v.numpy()), "view 0: col_ptr is not monotone (column 2)"),
                       ((ccol, i, v.numpy()), "view 0: row index out of range in column"),
                       ((ccol, rows, w), "view 0: negative entry in column"),
                       ((ccol, rows, z), "view 0: non-finite entry in column")):
        _refused(call(host=bad), match)
        _refused(call(host=bad, count=True), match)
    # what resnmtf_fp64_run_sparse_device refuses of a device view: the struct, the pointers, then the device checks --
    # every one of them refused on the host or by the canonicaliser's checked read, before any output is written
    host_array = np.zeros(nnz)
    for bad, match in (((7, a, b, vals, nnz), "view 0: spd->view: unknown layout"),
                       ((_lib.SPARSE_CSC, a, b, vals, nnz, 9), "view 0: spd->view: unknown index type"),
                       ((_lib.SPARSE_CSC, a, b, vals, nnz, _lib.INDEX_I64, 11), "view 0: spd->view: unknown dtype"),
                       ((_lib.SPARSE_CSC, a, b, vals, -1), "view 0: spd->view: nnz is negative"),
                       ((_lib.SPARSE_CSC, a, None, vals, nnz), "view 0: spd->view: ptr_or_rows / idx_or_cols / values is NULL"),
                       ((_lib.SPARSE_CSC, a, b, host_array.ctypes.data, nnz, _lib.INDEX_I64, _lib.DTYPE_F64),
                        "view 0: spd->view.values is not device memory of device 0")):
        _refused(call(dev=bad), match)
    i = b.clone(); i[4] = N3
    _refused(call(dev=(_lib.SPARSE_CSC, a, i, vals, nnz)), "row index out of range (entry 4)")
    w = vals.clone(); w[6] = -1.0
    _refused(call(dev=(_lib.SPARSE_CSC, a, b, w, nnz)), "negative")
    q = a.clone(); q[3] = q[2] - 1
    _refused(call(dev=(_lib.SPARSE_CSC, q, b, vals, nnz)), "col_ptr is not monotone")
    # a position stored twice in a device COO: the canonicaliser's refusal, in fill mode and in count mode
    r, c, x = on_device(*arrays("coo", rows, cols, v, N3, M3, 2), torch.int64)
    r[9], c[9] = r[3], c[3]
    _refused(call(dev=(_lib.SPARSE_COO, r, c, x, nnz)), "stored twice")
    _refused(call(dev=(_lib.SPARSE_COO, r, c, x, nnz), count=True), "stored twice")
    # the job itself is fine: the same call without a fault runs on both routes and gives the bits of the engine function
    for route in (dict(host=host), dict(dev=dev)):
        code, text, out = call(**route)
        assert code == 0, text
        assert np.array_equal(out["ccol"], want[0]) and np.array_equal(out["rows"], want[1]) and np.array_equal(R.bits(out["vals"]), R.bits(want[2]))
        assert np.array_equal(out["row_mask"].astype(bool), want[3]) and np.array_equal(out["col_mask"].astype(bool), want[4])
        assert (out["nnz_sub"], out["n_empty_rows"], out["n_empty_cols"]) == (len(want[2]), int(want[3].sum()), int(want[4].sum()))


@gpu
def test_dense_and_sparse_entries_keep_to_their_views():
    with pytest.raises(NotImplementedError, match="fp64_subsample gathers dense views"):
        engine.fp64_subsample(sp.csc_matrix(np.eye(3)), [0, 1], [0, 1])
    with pytest.raises(ValueError, match="fp64_subsample_sparse gathers sparse views .*fp64_subsample takes a dense one"):
        engine.fp64_subsample_sparse(np.eye(3), [0, 1], [0, 1])
    with pytest.raises(ResnmtfError, match="view 0: negative entry in column"):
        engine.fp64_subsample_sparse(sp.csc_matrix(-np.eye(3)), [0, 1], [0, 1])
    with pytest.raises(ResnmtfError, match=r"rows\[1\] = 0 occurs twice"):
        engine.fp64_subsample_sparse(sp.csc_matrix(np.eye(3)), [0, 0], [0, 1])


@gpu
def test_sparse_device_view_is_one_copy_read_by_every_call():
    torch, dev = _torch_dev()
    n, m, rows, cols, vals, rs, cs = case("300x200_lines")
    src = host_matrix(n, m, rows, cols, vals)
    t = engine.fp64_sparse_device_view(src)
    assert t.layout == torch.sparse_csc and t.device == dev and t.dtype == torch.float64 and t._nnz() == src.nnz
    assert engine.fp64_sparse_device_view(t) is t
    view = device_views.SparseDeviceView(t)
    assert engine.fp64_sparse_device_view(view) is view
    same_as(engine.fp64_subsample_sparse(t, rs, cs), wanted(src, rs, cs))
    with pytest.raises(ValueError, match="fp64_sparse_device_view takes sparse views"):
        engine.fp64_sparse_device_view(np.eye(3))
