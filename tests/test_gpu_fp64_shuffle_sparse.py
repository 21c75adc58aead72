"""shuffle_view of a sparse view in double precision (resnmtf_fp64_shuffle_sparse):
engine.fp64_shuffle_sparse bit for bit (as uint64 words) against the fp64 restatement of shuffle_ref.shuffle_csc
(fp64_shuffle_sparse_ref) and against engine.fp64_shuffle of the densified view read at the stored positions -- structure,
values with normalise off and on, masks and counts --, against the f32 route on fp32-valued data, from every layout, index
type and value type a device view may have, feeding engine.fp64_run, and the guards of the C entry.

Values are uniform doubles that fp32 does not hold unless a test says otherwise.  A NaN (0 / 0 in an empty column) is
compared as a NaN, not by its payload: NumPy and the device may spell it differently.

On the four kinds of draws (empty rows only, empty columns only, both, neither): at 300 x 200 with 1 % stored, 600 entries
over 500 lines, every draw has both (about 300 e^-2 = 40 empty rows are expected), so that shape checks the masks of draws
with both; the seeds of the other three kinds are searched on the CPU at 12 x 9 with 30 % stored, where all four occur."""
import ctypes as C
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import fp64_shuffle_sparse_ref as R
import shuffle_ref as S
from resnmtf_amd import _lib, device_views, engine, problem
from resnmtf_amd._lib import ResnmtfError
from resnmtf_amd.engine import Engine

gpu = pytest.mark.gpu
SEEDS = [0, 1, 2 ** 64 - 1]
SENTINEL = -12345


def _torch_dev():
    import torch
    return torch, torch.device("cuda", 0)


def same(a, b) -> bool:
    """Equal bits, a NaN matching any NaN."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(R.bits(a[~na]), R.bits(b[~nb]))


def pattern(n, m, density, seed):
    rng = np.random.default_rng(seed)
    mask = rng.random((n, m)) < density
    cols, rows = np.nonzero(mask.T)
    return rows.astype(np.int64), cols.astype(np.int64)


def doubles(count, seed):
    v = np.random.default_rng(seed).random(count) + 0.25
    assert count < 2 or (v.astype(np.float32).astype(np.float64) != v).any()
    return v


def full(n, m):
    cols, rows = np.nonzero(np.ones((m, n), dtype=bool))
    return rows.astype(np.int64), cols.astype(np.int64)


@functools.lru_cache(maxsize=None)
def case(name):
    """(n, m, rows, cols, values) in canonical CSC order; explicit zeros are in `values`."""
    if name in ("1x1", "1x7", "7x1", "64x64_full"):
        n, m = (int(x) for x in name.split("_")[0].split("x"))
        rows, cols = full(n, m)
    elif name == "37x23_zero":
        n, m = 37, 23
        rows, cols = pattern(n, m, 0.3, 1)
    elif name == "33x31":
        n, m = 33, 31
        rows, cols = pattern(n, m, 0.4, 2)
    elif name == "300x200_lines":                       # one dense row and one dense column
        n, m = 300, 200
        mask = np.random.default_rng(3).random((n, m)) < 0.05
        mask[17, :] = True; mask[:, 31] = True
        cols, rows = (x.astype(np.int64) for x in np.nonzero(mask.T))
    elif name == "300x200_1pct":
        n, m = 300, 200
        rows, cols = pattern(n, m, 0.01, 5)
    elif name in ("257x3", "513x2", "600x5"):           # rows r and r + 256 in one column: what the lane order exists for
        n, m = (int(x) for x in name.split("x"))
        rows, cols = pattern(n, m, 0.6, 6 + n)
    elif name == "70000x70000":                         # n m > 2^32
        n = m = 70000
        pos = np.unique(np.random.default_rng(6).integers(0, n * m, 5000, dtype=np.int64))
        order = np.lexsort((pos // m, pos % m))
        rows, cols = (pos // m)[order], (pos % m)[order]
    elif name == "5x4_empty":
        n, m = 5, 4
        rows = cols = np.zeros(0, dtype=np.int64)
    else:
        raise KeyError(name)
    vals = doubles(len(rows), 11)
    if name == "37x23_zero":
        vals[7] = 0.0
    return n, m, rows, cols, vals


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


def check_against_helper(got, src, seed, normalise, what):
    t, er, ec = got
    n, m = src.shape
    indptr, indices, vals, wr, wc = R.draw(src, seed, normalise)
    gp, gi, gv = parts(t)
    assert tuple(t.shape) == (n, m) and len(gv) == src.nnz, what
    assert np.array_equal(gp, indptr) and np.array_equal(gi, indices), what
    assert same(gv, vals), what
    assert er.dtype == bool and np.array_equal(er, wr) and np.array_equal(ec, wc), what
    return gp, gi, gv


def check_against_dense(gp, gi, gv, er, ec, dense_x, seed, normalise, what):
    """engine.fp64_shuffle of the densified view, read at the stored positions; its masks."""
    n, m = dense_x.shape
    d, _, dr, dc = engine.fp64_shuffle(dense_x, seed, normalise=normalise)
    d = d.cpu().numpy()
    col = np.repeat(np.arange(m), np.diff(gp))
    assert same(gv, d[gi, col]), what
    assert np.array_equal(er, dr) and np.array_equal(ec, dc), what
    if not normalise:                                   # the dense draw is +0.0 everywhere else
        rest = d.copy(); rest[gi, col] = 0.0
        assert not R.bits(rest).any(), what


# ---------------------------------------------------------------------------------------------------------------------
# 0. the helper itself, on the CPU: the dense formula of shuffle_ref at the stored positions
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["1x7", "37x23_zero", "33x31", "64x64_full", "257x3"])
def test_helper_is_the_dense_formula_at_the_stored_positions(name):
    n, m, rows, cols, vals = case(name)
    src = host_matrix(n, m, rows, cols, vals)
    for seed in SEEDS:
        indptr, indices, data = R.shuffle_csc64(src, seed)
        d = S.shuffle_dense(src.toarray(), seed)
        col = np.repeat(np.arange(m), np.diff(indptr))
        assert len(data) == len(vals) and np.array_equal(R.bits(d[indices, col]), R.bits(data))
        assert np.count_nonzero(d) == np.count_nonzero(vals)
        assert all((np.diff(indices[indptr[c]:indptr[c + 1]]) > 0).all() for c in range(m))
        # the 256-lane column sum of the stored entries is that of the dense column (absent +0.0 entries change no bit)
        lanes = np.zeros((m, 256))
        for r in range(n):
            lanes[:, r % 256] += d[r, :] + 0.0
        s = 128
        while s:
            lanes[:, :s] += lanes[:, s:2 * s]; s >>= 1
        assert np.array_equal(R.bits(lanes[:, 0]), R.bits(R.lane_colsums(m, indptr, indices, data)))


def test_the_shapes_exercise_the_cycle_walk_and_its_absence():
    assert 4 ** S.half_bits(64 * 64) == 64 * 64                  # no walk
    assert 4 ** S.half_bits(33 * 31) > 33 * 31                   # the walk runs
    assert 70000 * 70000 > 2 ** 32


# ---------------------------------------------------------------------------------------------------------------------
# 1. structure, values, masks and counts: the helper and the dense route, host and device route in
# ---------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name", ["1x1", "1x7", "7x1", "37x23_zero", "64x64_full", "33x31", "300x200_lines", "300x200_1pct", "257x3",
                                  "513x2", "600x5"])
def test_draw_against_the_helper_and_the_dense_route(name):
    n, m, rows, cols, vals = case(name)
    src = host_matrix(n, m, rows, cols, vals)
    dense_x = src.toarray()
    t = device_csc(n, m, rows, cols, vals)
    has_zero = bool((vals == 0).any())
    for seed in SEEDS:
        for normalise in (False, True):
            got = engine.fp64_shuffle_sparse(t, seed, normalise=normalise)
            gp, gi, gv = check_against_helper(got, src, seed, normalise, (name, seed, normalise, "device"))
            check_against_dense(gp, gi, gv, got[1], got[2], dense_x, seed, normalise, (name, seed, normalise))
            if not has_zero:                            # (canonical_csc drops an explicit zero: the host route of the C entry below)
                hot = engine.fp64_shuffle_sparse(src, seed, normalise=normalise)
                check_against_helper(hot, src, seed, normalise, (name, seed, normalise, "host"))
    if name == "300x200_1pct":
        assert got[1].any() and got[2].any()
    if name == "37x23_zero":
        assert t._nnz() == len(vals) and (parts(got[0])[2] == 0).sum() == 1          # the explicit zero stays stored
        indptr, indices, data = R.csc_parts(n, m, rows, cols, vals)
        code, text, out = _call(n, m, host=(indptr, indices, data), seed=1, normalise=1)
        assert code == 0, text
        want = R.draw(src, 1, True)
        assert np.array_equal(out["ccol"], want[0]) and np.array_equal(out["rows"], want[1]) and same(out["vals"], want[2])


def _inverse_image(n, m, dest_rows, dest_cols, seed):
    """The source positions (canonical order) whose shuffle with `seed` lands on the given destination positions, and
    for each of them the index of its destination in the given lists."""
    i = np.asarray(dest_cols, dtype=np.int64) * n + np.asarray(dest_rows, dtype=np.int64)
    j = S.feistel_perm(i, n * m, seed).astype(np.int64)
    rows, cols = j // m, j % m
    order = np.lexsort((rows, cols))
    return rows[order], cols[order], order


@gpu
@pytest.mark.parametrize("seed", SEEDS)
def test_columns_of_0_1_255_256_and_257_entries_in_the_draw(seed):
    """600 x 5 whose DRAW has a column with exactly 0, 1, 255, 256 and 257 stored entries (the source is the inverse
    image of that pattern): one trip of the column walk short of full, full, and one entry into the next block."""
    n, m = 600, 5
    rng = np.random.default_rng(21)
    counts = [0, 1, 255, 256, 257]
    dr = np.concatenate([np.sort(rng.permutation(n)[:c]) for c in counts]).astype(np.int64)
    dc = np.repeat(np.arange(m), counts)
    rows, cols, _ = _inverse_image(n, m, dr, dc, seed)
    vals = doubles(len(rows), 22)
    src = host_matrix(n, m, rows, cols, vals)
    for route in (src, device_csc(n, m, rows, cols, vals)):
        got = engine.fp64_shuffle_sparse(route, seed, normalise=True)
        gp, gi, gv = check_against_helper(got, src, seed, True, seed)
        assert np.diff(gp).tolist() == counts and got[2].tolist() == [True, False, False, False, False]
    check_against_dense(gp, gi, gv, got[1], got[2], src.toarray(), seed, True, seed)


@functools.lru_cache(maxsize=None)
def _kinds_of_draws():
    """12 x 9 at 30 %: the first seed of each kind of draw, searched on the CPU."""
    n, m = 12, 9
    rows, cols = pattern(n, m, 0.3, 31)
    src = host_matrix(n, m, rows, cols, doubles(len(rows), 32))
    found = {}
    for seed in range(4000):
        indptr, indices, data = R.shuffle_csc64(src, seed)
        er, ec = R.empty_lines(n, m, indptr, indices, data)
        found.setdefault((bool(er.any()), bool(ec.any())), seed)
        if len(found) == 4:
            break
    return src, found


def test_all_four_kinds_of_draws_exist_at_the_small_shape():
    assert len(_kinds_of_draws()[1]) == 4


@gpu
def test_masks_of_draws_with_empty_rows_only_columns_only_both_and_neither():
    src, found = _kinds_of_draws()
    for (rows_empty, cols_empty), seed in sorted(found.items()):
        got = engine.fp64_shuffle_sparse(src, seed, normalise=False)
        check_against_helper(got, src, seed, False, seed)
        assert bool(got[1].any()) == rows_empty and bool(got[2].any()) == cols_empty
        check_against_dense(*parts(got[0]), got[1], got[2], src.toarray(), seed, False, seed)


@gpu
@pytest.mark.parametrize("route", ["host", "device"])
def test_beyond_32_bits_of_positions(route):
    n, m, rows, cols, vals = case("70000x70000")
    src = host_matrix(n, m, rows, cols, vals)
    x = src if route == "host" else device_csc(n, m, rows, cols, vals)
    for seed in (1, 2 ** 64 - 1):
        got = engine.fp64_shuffle_sparse(x, seed, normalise=True)
        check_against_helper(got, src, seed, True, seed)
        assert got[1].sum() >= n - len(vals) and got[2].sum() >= m - len(vals)


@gpu
def test_view_without_a_stored_entry():
    n, m, rows, cols, vals = case("5x4_empty")
    for x in (sp.csc_matrix((n, m)), device_csc(n, m, rows, cols, vals)):
        for normalise in (False, True):
            t, er, ec = engine.fp64_shuffle_sparse(x, 3, normalise=normalise)
            gp, gi, gv = parts(t)
            assert not gp.any() and len(gp) == m + 1 and len(gi) == 0 and len(gv) == 0 and er.all() and ec.all()


@gpu
def test_stored_zero_in_an_empty_column_gives_nan_exactly_there():
    """The draw's column 2 holds one stored entry, an explicit zero: 0 / 0 there, as the dense route's whole column."""
    n, m, seed = 9, 4, 5
    dr = np.array([0, 3, 8, 4, 1, 2, 7, 5])
    dc = np.array([0, 0, 0, 1, 1, 2, 3, 3])
    rows, cols, order = _inverse_image(n, m, dr, dc, seed)
    vals = doubles(len(dr), 41)
    vals[np.flatnonzero(order == 5)[0]] = 0.0            # the entry that lands at (2, 2)
    src = host_matrix(n, m, rows, cols, vals)
    t, er, ec = engine.fp64_shuffle_sparse(device_csc(n, m, rows, cols, vals), seed, normalise=True)
    gp, gi, gv = check_against_helper((t, er, ec), src, seed, True, "nan")
    col = np.repeat(np.arange(m), np.diff(gp))
    assert np.isnan(gv).sum() == 1 and col[np.isnan(gv)][0] == 2 and gi[np.isnan(gv)][0] == 2
    assert ec.tolist() == [False, False, True, False]
    d = engine.fp64_shuffle(src.toarray(), seed, normalise=True)[0].cpu().numpy()
    assert np.isnan(d[:, 2]).all() and same(gv, d[gi, col])


# ---------------------------------------------------------------------------------------------------------------------
# 2. the f32 route on data fp32 holds; repeatability
# ---------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name", ["37x23_zero", "300x200_lines", "257x3"])
def test_equals_the_f32_sparse_route_on_data_fp32_holds(name):
    """Un-normalised: bit for bit Engine.shuffle_view_sparse_from + get_view_sparse.  (Normalised the f32 route sums a
    column in plain entry order, csc_normalise_kernel, and rounds to fp32: agreement to f32 rounding only, DESIGN.md
    section 10; no bits are asserted there.)"""
    n, m, rows, cols, vals = case(name)
    vals = vals.astype(np.float32).astype(np.float64)
    src = sp.csc_matrix((vals[vals != 0], (rows[vals != 0], cols[vals != 0])), shape=(n, m))
    src.sort_indices()
    with Engine([n], [m], [1], nnz=[src.nnz]) as base, Engine([n], [m], [1], nnz=[src.nnz]) as e:
        base.set_view_sparse(0, src, pre_processed=True)
        for seed in SEEDS:
            e.shuffle_view_sparse_from(0, base, 0, seed=seed, normalise=False)
            want = e.get_view_sparse(0)
            gp, gi, gv = parts(engine.fp64_shuffle_sparse(src, seed, normalise=False)[0])
            assert np.array_equal(gp, want.indptr) and np.array_equal(gi, want.indices)
            assert np.array_equal(R.bits(gv), R.bits(want.data)), (name, seed)


@gpu
def test_two_calls_give_equal_bits_whatever_the_outputs_held():
    n, m, rows, cols, vals = case("300x200_lines")
    indptr, indices, data = R.csc_parts(n, m, rows, cols, vals)
    res = []
    for fill in (0x7F, 0x00, 0xA5):
        code, text, out = _call(n, m, host=(indptr, indices, data), seed=9, normalise=1, fill=fill)
        assert code == 0, text
        res.append(out)
    for other in res[1:]:
        for key in ("ccol", "rows", "vals", "row_mask", "col_mask"):
            assert res[0][key].tobytes() == other[key].tobytes(), key
        assert (res[0]["n_empty_rows"], res[0]["n_empty_cols"]) == (other["n_empty_rows"], other["n_empty_cols"])
    src = host_matrix(n, m, rows, cols, vals)
    want = R.draw(src, 9, True)
    assert np.array_equal(res[0]["ccol"], want[0]) and np.array_equal(res[0]["rows"], want[1]) and same(res[0]["vals"], want[2])
    assert (res[0]["n_empty_rows"], res[0]["n_empty_cols"]) == (int(want[3].sum()), int(want[4].sum()))


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
    host = sp.csc_matrix((wide, (rows, cols)), shape=(N3, M3))
    want = {normalise: engine.fp64_shuffle_sparse(host, 4, normalise=normalise) for normalise in (False, True)}
    return rows, cols, v, {k: (*parts(t), er, ec) for k, (t, er, ec) in want.items()}


def _same_draw(got, want):
    gp, gi, gv = parts(got[0])
    return (np.array_equal(gp, want[0]) and np.array_equal(gi, want[1]) and same(gv, want[2]) and np.array_equal(got[1], want[3])
            and np.array_equal(got[2], want[4]))


@gpu
@pytest.mark.parametrize("index", ("int32", "int64"))
@pytest.mark.parametrize("layout", ("csc", "csc_perm", "csr", "coo"))
def test_layouts_and_index_types(layout, index):
    import torch
    from test_gpu_sparse_device_views import LAYOUT_CODE, arrays, as_tensor, on_device
    rows, cols, v, want = _route_case("float64")
    a, b, vals = on_device(*arrays(layout, rows, cols, v, N3, M3, 3), getattr(torch, index))
    for normalise in (False, True):
        if layout == "coo" and index == "int32":             # (torch's COO indices are int64 only: the C entry itself)
            code, text, out = _call(N3, M3, dev=(LAYOUT_CODE[layout], a, b, vals, len(rows)), seed=4, normalise=int(normalise))
            assert code == 0, text
            assert np.array_equal(out["ccol"], want[normalise][0]) and np.array_equal(out["rows"], want[normalise][1])
            assert same(out["vals"], want[normalise][2])
        else:
            assert _same_draw(engine.fp64_shuffle_sparse(as_tensor(layout, a, b, vals, (N3, M3)), 4, normalise=normalise), want[normalise])


@gpu
@pytest.mark.parametrize("dtype", ("float64", "float32", "float16", "bfloat16"))
def test_value_types(dtype):
    import torch
    from test_gpu_sparse_device_views import arrays, as_tensor, on_device
    rows, cols, v, want = _route_case(dtype)
    assert v.dtype == getattr(torch, dtype)
    t = as_tensor("csr", *on_device(*arrays("csr", rows, cols, v, N3, M3, 4), torch.int64), (N3, M3))
    view = device_views.SparseDeviceView(t)                   # (the host layer's own wrapper is taken as the tensor)
    for normalise in (False, True):
        assert _same_draw(engine.fp64_shuffle_sparse(view if normalise else t, 4, normalise=normalise), want[normalise])


@gpu
def test_device_view_is_read_where_it_lies(monkeypatch):
    import torch
    from test_gpu_sparse_device_views import arrays, as_tensor, on_device
    rows, cols, v, want = _route_case("float64")
    t = as_tensor("csc", *on_device(*arrays("csc_perm", rows, cols, v, N3, M3, 6), torch.int64), (N3, M3))
    keep = []
    job = _lib.Fp64ShuffleSparseJob()
    engine._fill_fp64_sparse_source(job, device_views.SparseDeviceView(t), 0, keep, "x")
    assert not job.x.col_ptr and not job.x.row_idx and not job.x.values
    assert (job.x_dev.ptr_or_rows, job.x_dev.idx_or_cols, job.x_dev.values) == (t.ccol_indices().data_ptr(), t.row_indices().data_ptr(),
                                                                               t.values().data_ptr())

    def refuse(*args, **kwargs):
        raise AssertionError("a tensor was brought to the host")
    for name in ("cpu", "numpy", "tolist", "to_dense"):
        monkeypatch.setattr(torch.Tensor, name, refuse)
    monkeypatch.setattr(device_views, "sparse_tensor_to_scipy", refuse)
    got = engine.fp64_shuffle_sparse(t, 4, normalise=True)
    monkeypatch.undo()
    assert _same_draw(got, want[True])


# ---------------------------------------------------------------------------------------------------------------------
# 4. feeding the run
# ---------------------------------------------------------------------------------------------------------------------
@gpu
def test_the_draw_feeds_the_fp64_run_as_a_sparse_device_view():
    """40 x 30, k = 3, 3 sweeps: the returned tensor as a sparse device view gives bit for bit the run on the helper's
    SciPy matrix through the host sparse route."""
    from resnmtf_amd import synth
    n, m, k = 40, 30, 3
    rows, cols = pattern(n, m, 0.5, 61)
    src = host_matrix(n, m, rows, cols, doubles(len(rows), 62))
    t, er, ec = engine.fp64_shuffle_sparse(src, 2, normalise=True)
    assert not er.any() and not ec.any()
    indptr, indices, vals, _, _ = R.draw(src, 2, True)
    ref = R.raw_csc(n, m, indptr, indices, vals)
    f, s, g = synth.random_init(n, m, k, 9)
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
def _call(n, m, host=None, dev=None, seed=0, normalise=0, struct_size=None, null=(), device_id=0, fill=0x5A, nnz_out=None,
          outs=None, stream=None):
    """The C entry itself on outputs filled with a byte pattern: (code, text, the outputs and host results)."""
    import torch
    lib = _lib.load()
    where = torch.device("cuda", 0)
    nnz = (len(host[1]) if host is not None else dev[4] if dev is not None else 0) if nnz_out is None else nnz_out
    nnz = max(int(nnz), 0)
    ccol = torch.full((m + 1,), 0, dtype=torch.int64, device=where).view(torch.uint8).fill_(fill).view(torch.int64)
    rows = torch.empty(max(nnz, 1), dtype=torch.int64, device=where).view(torch.uint8).fill_(fill).view(torch.int64)
    vals = torch.empty(max(nnz, 1), dtype=torch.float64, device=where).view(torch.uint8).fill_(fill).view(torch.float64)
    if outs is not None:
        ccol, rows, vals = outs
    tensors = [x for x in (ccol, rows, vals) if torch.is_tensor(x)]
    before = [x.clone() for x in tensors]
    nr, nc = C.c_int(SENTINEL), C.c_int(SENTINEL)
    rm = np.full(max(n, 1), 7, dtype=np.uint8); cm = np.full(max(m, 1), 7, dtype=np.uint8)
    job = _lib.Fp64ShuffleSparseJob()
    job.struct_size = C.sizeof(job) if struct_size is None else struct_size
    job.n, job.m, job.normalise, job.seed = n, m, normalise, seed & 0xFFFFFFFFFFFFFFFF
    keep = []
    if host is not None:
        keep = [np.ascontiguousarray(host[0], dtype=np.int64), np.ascontiguousarray(host[1], dtype=np.int32),
                np.ascontiguousarray(host[2], dtype=np.float64)]
        job.x.col_ptr = keep[0].ctypes.data_as(C.POINTER(C.c_longlong))
        job.x.row_idx, job.x.values = keep[1].ctypes.data_as(C.POINTER(C.c_int)), keep[2].ctypes.data_as(C.POINTER(C.c_double))
    if dev is not None:
        layout, a, b, v, count = dev[:5]
        ptr = lambda x: None if x is None else (x if isinstance(x, int) else x.data_ptr()) or None      # noqa: E731
        kinds = [x.dtype for x in (a, b) if torch.is_tensor(x)]
        c = job.x_dev
        c.layout = layout
        c.index_type = dev[5] if len(dev) > 5 else (_lib.INDEX_I32 if kinds and kinds[0] == torch.int32 else _lib.INDEX_I64)
        c.dtype = dev[6] if len(dev) > 6 else {torch.float64: 0, torch.float32: 1, torch.float16: 2, torch.bfloat16: 3}[v.dtype]
        c.ptr_or_rows, c.idx_or_cols, c.values, c.nnz = ptr(a), ptr(b), ptr(v), count
    job.stream = stream
    as_ptr = lambda x: x if isinstance(x, int) else x.data_ptr()      # noqa: E731
    job.out_col_ptr, job.out_row_idx, job.out_values = as_ptr(ccol), as_ptr(rows), as_ptr(vals)
    job.n_empty_rows, job.n_empty_cols = C.pointer(nr), C.pointer(nc)
    job.row_mask, job.col_mask = rm.ctypes.data_as(C.POINTER(C.c_ubyte)), cm.ctypes.data_as(C.POINTER(C.c_ubyte))
    for name in null:
        setattr(job, name, None)
    torch.cuda.synchronize()
    code = lib.resnmtf_fp64_shuffle_sparse(device_id, C.byref(job))
    text = (lib.resnmtf_last_error(None) or b"").decode()
    torch.cuda.synchronize()
    untouched = (all(torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for x, y in zip(tensors, before)) and nr.value == SENTINEL
                 and nc.value == SENTINEL and (rm == 7).all() and (cm == 7).all())
    out = {"untouched": untouched, "n_empty_rows": nr.value, "n_empty_cols": nc.value, "row_mask": rm[:n].copy(), "col_mask": cm[:m].copy()}
    if code == 0:
        out.update(ccol=ccol.cpu().numpy(), rows=rows[:nnz].cpu().numpy(), vals=vals[:nnz].cpu().numpy())
    return code, text, out


def _refused(result, match, code=1):
    got, text, out = result
    assert got == code and match in text, (got, text, match)
    assert out["untouched"], match


@gpu
def test_guards_of_the_c_entry():
    import torch
    from test_gpu_sparse_device_views import arrays, on_device
    rows, cols, v, want = _route_case("float64")
    nnz = len(rows)
    ccol = np.concatenate([[0], np.cumsum(np.bincount(cols, minlength=M3))])
    host = (ccol, rows, v.numpy())
    a, b, vals = on_device(*arrays("csc", rows, cols, v, N3, M3, 1), torch.int64)
    dev = (_lib.SPARSE_CSC, a, b, vals, nnz)
    call = functools.partial(_call, N3, M3, seed=4)
    # what resnmtf_fp64_shuffle refuses, with its texts where the condition is the same
    for kw, match in ((dict(host=host, struct_size=8), "resnmtf_fp64_shuffle_sparse_job struct_size mismatch"),
                      (dict(host=host, dev=dev), "X is given in two places (job->x and job->x_dev)"),
                      (dict(), "X is given in no place (job->x or job->x_dev)"),
                      (dict(host=host, null=("out_col_ptr",)), "out_col_ptr is NULL"),
                      (dict(host=host, null=("out_values",)), "out_row_idx / out_values are NULL"),
                      (dict(dev=dev, null=("out_row_idx",)), "out_row_idx / out_values are NULL"),
                      (dict(host=host, null=("n_empty_cols",)), "n_empty_rows / n_empty_cols are NULL"),
                      (dict(host=host, device_id=99), "device_id out of range"),
                      (dict(dev=dev, device_id=-1), "device_id out of range")):
        _refused(call(**kw), match)
    _refused(_call(0, M3, host=host), "view dimensions must be positive")
    _refused(_call(N3, -1, dev=dev), "view dimensions must be positive")
    # (n * m above 2^62 cannot be stated with two ints: the check is exercised by the stand-alone host program)
    assert _lib.load().resnmtf_fp64_shuffle_sparse(0, None) == 1 and b"job is NULL" in _lib.load().resnmtf_last_error(None)
    # outputs that are not memory of the device, too short, or overlapping
    where = torch.device("cuda", 0)
    good = lambda: (torch.zeros(M3 + 1, dtype=torch.int64, device=where), torch.zeros(nnz, dtype=torch.int64, device=where),      # noqa: E731
                    torch.zeros(nnz, dtype=torch.float64, device=where))
    on_host = np.zeros(max(nnz, M3 + 1), dtype=np.int64)
    for at, name in enumerate(("out_col_ptr", "out_row_idx", "out_values")):
        outs = list(good()); outs[at] = on_host.ctypes.data
        _refused(call(host=host, outs=tuple(outs)), name + " is not device memory of device 0")
    # (16 MiB asked of an emptied cache: torch takes a block of exactly that size from the runtime, so the end of the
    # tensor is the end of an allocation)
    torch.cuda.empty_cache()
    big = torch.zeros(1 << 21, dtype=torch.float64, device=where)
    outs = list(good()); outs[2] = big[(1 << 21) - nnz + 1:]
    _refused(call(host=host, outs=tuple(outs)), "out_values reaches beyond its allocation (too short for nnz doubles)")
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
                       ((ccol, rows[::-1].copy(), v.numpy()), "view 0: row ind"),
                       ((ccol, rows, w), "view 0: negative entry in column"),
                       ((ccol, rows, z), "view 0: non-finite entry in column")):
        _refused(call(host=bad), match)
    # what resnmtf_fp64_run_sparse_device refuses of a device view: the struct, the pointers, then the device checks
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
    # a position stored twice in a device COO: the canonicaliser's refusal
    r, c, x = on_device(*arrays("coo", rows, cols, v, N3, M3, 2), torch.int64)
    r[9], c[9] = r[3], c[3]
    _refused(call(dev=(_lib.SPARSE_COO, r, c, x, nnz)), "stored twice")
    # the job itself is fine: the same call without a fault runs on both routes and gives the bits of the engine function
    for route in (dict(host=host), dict(dev=dev)):
        code, text, out = call(normalise=1, **route)
        assert code == 0, text
        assert np.array_equal(out["ccol"], want[True][0]) and np.array_equal(out["rows"], want[True][1]) and same(out["vals"], want[True][2])
        assert np.array_equal(out["row_mask"].astype(bool), want[True][3]) and np.array_equal(out["col_mask"].astype(bool), want[True][4])
        assert (out["n_empty_rows"], out["n_empty_cols"]) == (int(want[True][3].sum()), int(want[True][4].sum()))


def test_early_refusal_of_a_view_with_fewer_entries_than_lines():
    x = sp.csc_matrix((np.array([1.0, 2.0]), (np.array([0, 3]), np.array([1, 2]))), shape=(5, 4))

    def never(*a, **k):
        raise AssertionError("a draw was made")
    with pytest.raises(ValueError, match=r"shuffle_view: view 1 stores 2 entries, fewer than max\(n, m\) = 5"):
        problem._draw_shuffle_fp64(x, 1, 3, shuffle_sparse=never)


@gpu
def test_dense_and_sparse_entries_keep_to_their_views():
    with pytest.raises(NotImplementedError, match="fp64_shuffle draws dense views"):
        engine.fp64_shuffle(sp.csc_matrix(np.eye(3)), 0)
    with pytest.raises(ValueError, match="fp64_shuffle_sparse draws sparse views"):
        engine.fp64_shuffle_sparse(np.eye(3), 0)
    with pytest.raises(ResnmtfError, match="view 0: negative entry in column"):
        engine.fp64_shuffle_sparse(sp.csc_matrix(-np.eye(3)), 0)
