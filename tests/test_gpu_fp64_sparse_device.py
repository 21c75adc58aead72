"""GPU tests of sparse views of the device-wide fp64 path taken from device memory (resnmtf_fp64_run_sparse_device, DESIGN.md
section 24): torch CSC / CSR / COO tensors, int32 / int64 indices, four value types, entries in any order.  The yardstick
is the host route in the same process -- ``engine.fp64_run`` on the ``scipy.sparse`` canonical CSC of the same values --
and every comparison is on BYTES: F, S, G, lambda, mu, All_Error and the sweep count, no tolerance (the one exception
is the explicit-zeros case, whose host route drops the zeros).  Values are multiples of 2^-10 that every one of the four
types holds exactly (at most 8 significant bits), no explicit zeros; at most 5 fixed sweeps unless a test says otherwise.
Cases are built as tests/test_gpu_sparse_device_views.py and tests/test_gpu_fp64_sparse.py build theirs."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import helpers
from resnmtf_amd import _lib, api, naming, synth
from resnmtf_amd._lib import ResnmtfError
from resnmtf_amd.engine import fp64_run, fp64_sparse_plan
from resnmtf_amd.problem import pair_table
from test_gpu_fp64 import COUPLED, MAX_ITERS, _check_api, _oracle_from_init, _same_bits
from test_gpu_fp64_sparse import _c_job, _skewed, sparsify
from test_gpu_sparse_device_views import CODES, DEV, DTYPES, LAYOUT_CODE, _device_refusals, arrays, as_tensor, on_device

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

SWEEPS = 5
_DP = C.POINTER(C.c_double)


# ---- building blocks ----
def quantised(x):
    """x with every non-zero entry rounded up to a multiple of 2^-10 (a stored entry stays one)."""
    return np.where(x > 0, np.ceil(x * 1024.0) / 1024.0, 0.0)


def entries(n, m, density, seed, edit=None):
    """(rows, cols, values) of the stored positions in canonical CSC order; values k / 1024, 1 <= k <= 255.  `edit` works
    on the mask before the positions are read."""
    rng = np.random.default_rng(seed)
    mask = rng.random((n, m)) < density
    mask[rng.integers(0, n, m), np.arange(m)] = True
    if edit is not None:
        edit(mask, rng)
    cols, rows = np.nonzero(mask.T)
    vals = rng.integers(1, 256, len(rows)) / 1024.0
    return rows.astype(np.int64), cols.astype(np.int64), vals


def of_matrix(x):
    """(rows, cols, values) of a dense matrix's non-zeros, canonical CSC order."""
    cols, rows = np.nonzero(x.T)
    return rows.astype(np.int64), cols.astype(np.int64), x[rows, cols]


def host_view(rows, cols, vals, shape):
    return sp.csc_matrix((vals, (rows, cols)), shape=shape)


def device_view(layout, rows, cols, vals, shape, index_dtype=torch.int64, dtype=torch.float64, seed=1):
    """The torch tensor of `layout` ("csc", "csc_perm": rows shuffled inside columns, "csr": columns shuffled inside rows,
    "coo": random order) on the GPU."""
    a, b, v = arrays(layout, rows, cols, torch.as_tensor(vals).to(dtype), shape[0], shape[1], seed)
    return as_tensor(layout, *on_device(a, b, v, index_dtype), shape)


def problem(data, k, init, n_iters=SWEEPS, **more):
    f, s, g = init
    return dict({"data": [data], "k": k, "init_f": [f], "init_s": [s], "init_g": [g], "n_iters": n_iters}, **more)


def assert_same_bits(got, ref, what):
    assert got["iters"] == ref["iters"], what
    assert np.asarray(got["all_error"]).tobytes() == np.asarray(ref["all_error"]).tobytes(), what
    for key in ("f", "s", "g", "lambda", "mu"):
        for v, (x, y) in enumerate(zip(got[key], ref[key])):
            x = x.cpu().numpy() if torch.is_tensor(x) else np.asarray(x)
            assert np.array_equal(x, np.asarray(y), equal_nan=True) and x.tobytes() == np.asarray(y).tobytes(), (what, key, v)


def one_case(n, m, k, density, seed, edit=None, layouts=("csc", "coo"), n_iters=SWEEPS):
    rows, cols, vals = entries(n, m, density, seed, edit)
    init = synth.random_init(n, m, k, seed + 1)
    ref = fp64_run(problem(host_view(rows, cols, vals, (n, m)), k, init, n_iters))
    assert ref["iters"] == n_iters
    for layout in layouts:
        got = fp64_run(problem(device_view(layout, rows, cols, vals, (n, m)), k, init, n_iters))
        assert_same_bits(got, ref, (n, m, k, layout))
    return rows, cols, vals


# ---- the C entry itself, one view ----
def c_run(shape, k, init, n_iters, spd=None, host=None, stream=None):
    """resnmtf_fp64_run_sparse_device with one view.  spd: (layout code, a, b, values, nnz) -- device tensors, None or an
    address --; host: (col_ptr, row_idx, values), the view as host CSC arrays exactly as given (resnmtf_fp64_run_sparse's
    route, explicit zeros kept).  Returns (code, message, outputs); the outputs start as -7."""
    lib = _lib.load()
    n, m = shape
    keep = [np.asfortranarray(a, dtype=np.float64) for a in init]
    outs = {"f": np.full((n, k), -7.0, order="F"), "s": np.full((k, k), -7.0, order="F"), "g": np.full((m, k), -7.0, order="F"),
            "lambda": np.full(k, -7.0), "mu": np.full(k, -7.0), "all_error": np.full(max(n_iters, 1), -7.0),
            "iters": np.full(1, -7, dtype=np.int32)}
    j = _lib.GroupJob()
    j.struct_size = C.sizeof(_lib.GroupJob)
    j.n_views, j.k, j.n_iters = 1, k, n_iters
    j.n_rows[0], j.n_cols[0] = n, m
    j.f0[0], j.s0[0], j.g0[0] = (a.ctypes.data_as(_DP) for a in keep)
    j.f_out[0], j.s_out[0], j.g_out[0], j.lambda_out[0], j.mu_out[0] = (outs[key].ctypes.data_as(_DP) for key in ("f", "s", "g", "lambda", "mu"))
    j.row_count[0][0] = j.col_count[0][0] = -1
    j.all_error, j.err_capacity, j.iters_done = outs["all_error"].ctypes.data_as(_DP), len(outs["all_error"]), outs["iters"].ctypes.data_as(C.POINTER(C.c_int))
    s = d = None
    if host is not None:
        s = _lib.Fp64Sparse()
        s.struct_size = C.sizeof(_lib.Fp64Sparse)
        csc = [np.ascontiguousarray(host[0], dtype=np.int64), np.ascontiguousarray(host[1], dtype=np.int32),
               np.ascontiguousarray(host[2], dtype=np.float64)]
        if csc[1].size == 0:
            csc[1], csc[2] = np.zeros(1, np.int32), np.zeros(1)
        keep += csc
        s.view[0].col_ptr = csc[0].ctypes.data_as(C.POINTER(C.c_longlong))
        s.view[0].row_idx, s.view[0].values = csc[1].ctypes.data_as(C.POINTER(C.c_int)), csc[2].ctypes.data_as(_DP)
    if spd is not None:
        layout, a, b, vals, nnz = spd
        d = _lib.Fp64SparseDevice()
        d.struct_size = C.sizeof(_lib.Fp64SparseDevice)
        d.stream = stream
        c = d.view[0]
        ptr = lambda x: None if x is None else (x if isinstance(x, int) else x.data_ptr()) or None
        kinds = [x.dtype for x in (a, b) if torch.is_tensor(x)]
        c.layout, c.index_type = layout, _lib.INDEX_I32 if kinds and kinds[0] == torch.int32 else _lib.INDEX_I64
        c.dtype, c.ptr_or_rows, c.idx_or_cols, c.values, c.nnz = CODES[vals.dtype], ptr(a), ptr(b), ptr(vals), nnz
    torch.cuda.synchronize()
    rc = lib.resnmtf_fp64_run_sparse_device(0, C.byref(j), None if s is None else C.byref(s), None, None if d is None else C.byref(d),
                                            1e-6, 100)
    outs["iters"] = int(outs["iters"][0])
    return rc, (lib.resnmtf_last_error(None) or b"").decode(), outs


def listed(outs):
    """c_run's outputs in the shape of an fp64_run result."""
    return {"f": [outs["f"]], "s": [outs["s"]], "g": [outs["g"]], "lambda": [outs["lambda"]], "mu": [outs["mu"]],
            "all_error": outs["all_error"][:max(outs["iters"], 0)], "iters": outs["iters"]}


def untouched(outs):
    return all(np.all(np.asarray(o) == -7) for o in outs.values())


# ---- 1. layouts and types on 129 x 127 at 10 %, k = 16 ----
N1, M1, K1 = 129, 127, 16


@pytest.fixture(scope="module")
def base():
    rows, cols, vals = entries(N1, M1, 0.10, 21)
    init = synth.random_init(N1, M1, K1, 22)
    ref = fp64_run(problem(host_view(rows, cols, vals, (N1, M1)), K1, init))
    assert ref["iters"] == SWEEPS and np.isfinite(ref["all_error"]).all()
    return rows, cols, vals, init, ref


@pytest.mark.parametrize("index", ["int32", "int64"])
@pytest.mark.parametrize("layout", ["csc", "csr", "coo"])
def test_layouts_and_index_types(base, layout, index):
    rows, cols, vals, init, ref = base
    index_dtype = getattr(torch, index)
    if layout == "coo" and index == "int32":             # (torch's COO indices are int64 only: the C entry itself)
        a, b, v = on_device(*arrays("coo", rows, cols, torch.as_tensor(vals), N1, M1, 3), index_dtype)
        rc, text, outs = c_run((N1, M1), K1, init, SWEEPS, spd=(_lib.SPARSE_COO, a, b, v, len(rows)))
        assert rc == _lib.OK, text
        got = listed(outs)
    else:
        got = fp64_run(problem(device_view(layout, rows, cols, vals, (N1, M1), index_dtype, seed=3), K1, init))
    assert_same_bits(got, ref, (layout, index))


@pytest.mark.parametrize("dtype", list(DTYPES))
def test_value_types(base, dtype):
    rows, cols, vals, init, ref = base
    t = device_view("csc", rows, cols, vals, (N1, M1), torch.int64, DTYPES[dtype])
    assert t.values().dtype == DTYPES[dtype] and np.array_equal(t.values().double().cpu().numpy(), vals)       # held exactly
    assert_same_bits(fp64_run(problem(t, K1, init)), ref, dtype)


def test_one_sort_and_two_sorts_agree(base):
    """Canonical CSC (its keys ascend strictly: the first sort and the duplicates check are skipped), the same matrix with
    the rows shuffled inside the columns and as COO in random order."""
    rows, cols, vals, init, ref = base
    for layout in ("csc", "csc_perm", "coo"):
        t = device_view(layout, rows, cols, vals, (N1, M1), seed=7)
        if layout == "csc_perm":
            assert not np.array_equal(t.row_indices().cpu().numpy(), rows)
        assert_same_bits(fp64_run(problem(t, K1, init)), ref, layout)
    view = api.device_views.SparseDeviceView(device_view("csr", rows, cols, vals, (N1, M1), seed=8))      # the host layer's own wrapper
    assert_same_bits(fp64_run(problem(view, K1, init)), ref, "SparseDeviceView")


# ---- 2. edges ----
def test_two_by_two():
    rows, cols, vals = np.array([0, 1, 0, 1]), np.array([0, 0, 1, 1]), np.array([0.25, 0.75, 0.5, 0.125])
    init = synth.random_init(2, 2, 1, 3)
    ref = fp64_run(problem(host_view(rows, cols, vals, (2, 2)), 1, init))
    for layout in ("csc", "csr", "coo"):
        assert_same_bits(fp64_run(problem(device_view(layout, rows, cols, vals, (2, 2)), 1, init)), ref, layout)


@pytest.mark.parametrize("n,m", [(33, 257), (257, 33)])
def test_ragged_shapes(n, m):
    one_case(n, m, 5, 0.10, 30 + n, layouts=("csc_perm", "csr"))


@pytest.mark.parametrize("k", [17, 33, 49, 64])
def test_every_padded_k_class(k):
    one_case(400, 300, k, 0.05, 40 + k)


def _empty_rows(mask, rng):
    mask[rng.choice(mask.shape[0], 40, replace=False), :] = False


def _one_entry_row(mask, rng):
    mask[17, :] = False
    mask[17, 23] = True


def _last_row_empty_last_col_full(mask, rng):
    mask[:, -1] = True
    mask[-1, :] = False


def _last_row_full_last_col_empty(mask, rng):
    mask[-1, :] = True
    mask[:, -1] = False


@pytest.mark.parametrize("edit", [_empty_rows, _one_entry_row, _last_row_empty_last_col_full, _last_row_full_last_col_empty],
                         ids=lambda f: f.__name__.strip("_"))
def test_special_lines(edit):
    n, m = 200, 150
    rows, cols, _ = one_case(n, m, 4, 0.2, 50, edit, layouts=("csc", "csr", "coo"))
    per_row, per_col = np.bincount(rows, minlength=n), np.bincount(cols, minlength=m)
    if edit is _empty_rows:
        assert (per_row == 0).sum() >= 40
    if edit is _one_entry_row:
        assert per_row[17] == 1
    if edit is _last_row_empty_last_col_full:
        assert per_row[-1] == 0 and per_col[-1] == n - 1
    if edit is _last_row_full_last_col_empty:
        assert per_row[-1] == m - 1 and per_col[-1] == 0


# ---- 3. the skewed view of section 22: the longest lines are reduced on the device ----
def test_skewed_view_takes_the_host_plan():
    x = quantised(_skewed().data[0])
    n, m, k = x.shape[0], x.shape[1], 6
    rows, cols, vals = of_matrix(x)
    host = host_view(rows, cols, vals, (n, m))
    plan = fp64_sparse_plan(host, k)
    assert plan["xg"][0] == 3 and plan["xtf"][0] == 6, plan                # a row in 3 pieces, a column in 6
    assert plan["xg"][2] == np.bincount(rows, minlength=n).max() and plan["xtf"][2] == np.bincount(cols, minlength=m).max()
    init = synth.random_init(n, m, k, 6)
    ref = fp64_run(problem(host, k, init))
    # (a piece count other than the host's would sum the long lines in another order: the bytes are the plan's witness)
    for layout in ("csc", "coo"):
        assert_same_bits(fp64_run(problem(device_view(layout, rows, cols, vals, (n, m)), k, init)), ref, layout)


# ---- 4. all four kinds of view in one job (g3), the factors on the device ----
def test_mixed_job():
    prob = helpers.golden_problem(helpers.load_golden("g3_three_views_phi_psi_xi"))
    data = [quantised(sparsify(x, 0.3, 70 + v)) for v, x in enumerate(prob.data)]
    k = prob.init_f[0].shape[1]
    common = {"k": k, "phi": prob.phi, "xi": prob.xi, "psi": prob.psi, "row_pairs": pair_table(prob.row_names),
              "col_pairs": pair_table(prob.col_names), "n_iters": SWEEPS}
    host = dict(common, data=[sp.csc_matrix(data[0]), data[1], sp.csc_matrix(data[2])], init_f=prob.init_f, init_s=prob.init_s,
                init_g=prob.init_g)
    ref = fp64_run(host)
    there = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float64, device=DEV)
    mixed = dict(common, data=[device_view("coo", *of_matrix(data[0]), data[0].shape), there(data[1]), sp.csc_matrix(data[2])],
                 init_f=[there(a) for a in prob.init_f], init_s=[there(a) for a in prob.init_s], init_g=[there(a) for a in prob.init_g])
    assert_same_bits(fp64_run(mixed), ref, "numpy out")
    got = fp64_run(mixed, output="torch", return_state=True)
    assert all(torch.is_tensor(t) and t.device.type == "cuda" for t in got["f"]) and len(got["state"]) == 3
    assert_same_bits(got, ref, "torch out")
    four = dict(host, data=[device_view("csr", *of_matrix(data[0]), data[0].shape), data[1], sp.csc_matrix(data[2])])
    four["data"][1] = there(data[1].T.copy()).T                            # (a column-major device matrix beside host factors)
    assert_same_bits(fp64_run(four), ref, "host factors")


# ---- 5. to convergence: a coupled problem of section 21, sparsified at 30 % ----
def test_convergence_stops_on_the_host_routes_sweep():
    shapes, k, kw, _ = COUPLED[0]                                         # (the oracle takes 46 sweeps on this one)
    prob = helpers.coupled_problem(shapes, k, 100, **kw)
    data = [quantised(sparsify(x, 0.3, 80 + v)) for v, x in enumerate(prob.data)]
    common = {"k": k, "init_f": prob.init_f, "init_s": prob.init_s, "init_g": prob.init_g, "phi": prob.phi, "xi": prob.xi, "psi": prob.psi,
              "row_pairs": pair_table(prob.row_names), "col_pairs": pair_table(prob.col_names), "n_iters": None}
    ref = fp64_run(dict(common, data=[sp.csc_matrix(x) for x in data]), max_iters=MAX_ITERS)
    assert 5 < ref["iters"] < MAX_ITERS
    layouts = ("csc_perm", "csr", "coo")
    got = fp64_run(dict(common, data=[device_view(layouts[v], *of_matrix(x), x.shape, seed=v) for v, x in enumerate(data)]), max_iters=MAX_ITERS)
    assert got["iters"] == ref["iters"]
    assert_same_bits(got, ref, "convergence")


# ---- 6. spd == NULL is resnmtf_fp64_run_device; repeatability ----
@pytest.mark.parametrize("kind", ["dense", "sparse"])
def test_without_the_struct_the_call_is_the_device_entry(kind):
    lib = _lib.load()
    rows, cols, vals = entries(60, 41, 0.3, 5)
    x = host_view(rows, cols, vals, (60, 41)).toarray()
    f, s, g = synth.random_init(60, 41, 3, 6)
    z = np.zeros((1, 1))
    prob = synth.Problem([x], [f], [s], [g], z, z, z, 3, "p", row_names=[[f"r{i}" for i in range(60)]], col_names=[[f"c{i}" for i in range(41)]])
    views = (0,) if kind == "sparse" else ()
    ja, sa, keep_a, outs_a = _c_job(prob, SWEEPS, sparse_views=views)
    jb, sb, keep_b, outs_b = _c_job(prob, SWEEPS, sparse_views=views)
    assert lib.resnmtf_fp64_run_device(0, C.byref(ja), C.byref(sa), None, 1e-6, 100) == _lib.OK
    assert lib.resnmtf_fp64_run_sparse_device(0, C.byref(jb), C.byref(sb), None, None, 1e-6, 100) == _lib.OK
    for a, b in zip(outs_a, outs_b):
        assert not np.any(a == -7) and a.tobytes() == b.tobytes()


def test_two_calls_give_the_same_bits(base):
    rows, cols, vals, init, ref = base
    t = device_view("coo", rows, cols, vals, (N1, M1), seed=11)
    a, b = fp64_run(problem(t, K1, init)), fp64_run(problem(t, K1, init))
    _same_bits(a, b)
    assert_same_bits(a, ref, "first of two")


# ---- 7. ordering: the values are produced on a side stream immediately before the call ----
def test_the_run_is_ordered_after_the_producer_stream():
    n, m, k = 300, 200, 3
    rows, cols, _ = entries(n, m, 0.3, 41)
    nnz = len(rows)
    ccol = np.concatenate([[0], np.cumsum(np.bincount(cols, minlength=m))])
    a, b, _ = on_device(ccol, rows, torch.zeros(1), torch.int64)
    base_t = torch.rand(1500, 1100, device=DEV, dtype=torch.float32)
    init = synth.random_init(n, m, k, 16)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(side):
        t = base_t
        for _ in range(200):                           # a queue of work the run has to wait for
            t = t * 1.0009765625 + 0.03125
        vals = t.reshape(-1)[:nnz] + 0.5               # the producer, enqueued immediately before the call
        got = fp64_run(problem(torch.sparse_csc_tensor(a, b, vals, (n, m)), k, init))      # (no synchronisation by the test)
    torch.cuda.synchronize()
    ref = fp64_run(problem(host_view(rows, cols, vals.double().cpu().numpy(), (n, m)), k, init))
    assert_same_bits(got, ref, "side stream")


# ---- 8. api.res_nmtf_inner(precision="fp64", fp64_sparse_device=True) from the device's own initialisation ----
@pytest.mark.parametrize("fp64_device", [False, True])
def test_api_route(fp64_device):
    prob = helpers.coupled_problem([(120, 90), (100, 90)], 4, 5, phi_w=1.0, psi_w=0.5)
    prob.data = [quantised(sparsify(x, 0.3, 50 + v)) for v, x in enumerate(prob.data)]
    k_vec, rs, cs = [4, 4], naming.shared_names(prob.row_names), naming.shared_names(prob.col_names)
    common = dict(spurious=False, row_names=prob.row_names, col_names=prob.col_names, precision="fp64", return_init=True, seed=3)
    there = [device_view("csr", *of_matrix(prob.data[0]), prob.data[0].shape), sp.coo_matrix(prob.data[1])]
    res = api.res_nmtf_inner(there, rs, cs, None, None, None, k_vec, prob.phi, prob.xi, prob.psi, SWEEPS, fp64_sparse_device=True,
                             fp64_sparse=True, fp64_device=fp64_device, **common)
    init = res["init"]
    assert len(init) == 2 and len(init[0]) == 5 and len(res["All_Error"]) == SWEEPS
    # the same start and the same data through the host route: the same bytes
    host = api.res_nmtf_inner([sp.csc_matrix(x) for x in prob.data], rs, cs, [i[0] for i in init], [i[1] for i in init],
                              [i[2] for i in init], k_vec, prob.phi, prob.xi, prob.psi, SWEEPS, fp64_sparse=True,
                              init_lm=([i[3] for i in init], [i[4] for i in init]), **common)
    assert list(res) == list(host)
    assert res["All_Error"].tobytes() == host["All_Error"].tobytes()
    for key in ("output_f", "output_s", "output_g", "lambda", "mu", "row_clusters", "col_clusters"):
        for v in range(2):
            assert np.asarray(res[key][v]).tobytes() == np.asarray(host[key][v]).tobytes(), (key, v)
    # ... and the oracle on the densified matrices, from that start, at section 21's bars (F, G, S 1e-11, All_Error 1e-13)
    _check_api(res, _oracle_from_init(prob, init, SWEEPS), 2, ("api", fp64_device))


# ---- 9. explicit zeros stay stored ----
def test_explicit_zeros_stay_stored():
    n, m, k = 70, 45, 3
    rows, cols, vals = entries(n, m, 0.2, 31)
    nnz = len(rows)
    ccol = np.concatenate([[0], np.cumsum(np.bincount(cols, minlength=m))])
    zeros = np.array([ccol[4], ccol[10] + 1, nnz - 1])                     # first of a column, inside one, the last entry
    assert ccol[11] - ccol[10] > 2 and ccol[5] - ccol[4] > 1
    vals = vals.copy()
    vals[zeros] = 0.0
    init = synth.random_init(n, m, k, 13)
    rc, text, kept = c_run((n, m), k, init, SWEEPS, host=(ccol, rows, vals))                # the zero-keeping canonical arrays
    assert rc == _lib.OK, text
    dropped = fp64_run(problem(host_view(rows, cols, vals, (n, m)), k, init))               # (sparse.canonical_csc drops them)
    for layout in ("csc", "csc_perm", "csr", "coo"):
        t = device_view(layout, rows, cols, vals, (n, m), seed=6)
        assert t._nnz() == nnz
        got = fp64_run(problem(t, k, init))
        assert_same_bits(got, listed(kept), layout)
        # against the host route without them: the same sums with some zero terms, grouped otherwise at most
        for key in ("f", "s", "g"):
            d = helpers.rel_fro(got[key][0], dropped[key][0])
            print(f"{layout} {key}: {d:.2e} from the host route that drops the zeros")
            assert d <= 1e-13, (layout, key, d)
        e = float(np.max(np.abs(got["all_error"] - dropped["all_error"])))
        assert e <= 1e-13, (layout, e)
        for key in ("lambda", "mu"):
            np.testing.assert_allclose(got[key][0], dropped[key][0], rtol=1e-13, atol=0)


# ---- 10. a view without a stored entry does what the host route does with the empty CSC ----
def test_no_stored_entry():
    n, m, k = 12, 7, 3
    init = synth.random_init(n, m, k, 15)
    rc_h, text_h, ref = c_run((n, m), k, init, SWEEPS, host=(np.zeros(m + 1, np.int64), np.zeros(0, np.int32), np.zeros(0)))
    no_values = torch.zeros(0, dtype=torch.float32, device=DEV)
    for layout, ptr_len in ((_lib.SPARSE_CSC, m + 1), (_lib.SPARSE_CSR, n + 1), (_lib.SPARSE_COO, 0)):
        ptr = torch.zeros(ptr_len, dtype=torch.int64, device=DEV) if ptr_len else None
        rc, text, got = c_run((n, m), k, init, SWEEPS, spd=(layout, ptr, None, no_values, 0))
        assert rc == rc_h, (layout, text, text_h)
        for key in ref:
            assert np.asarray(got[key]).tobytes() == np.asarray(ref[key]).tobytes(), (layout, key)
    # a pointer array that claims an entry is still judged
    bad = torch.zeros(m + 1, dtype=torch.int64, device=DEV)
    bad[-1] = 1
    rc, text, got = c_run((n, m), k, init, SWEEPS, spd=(_lib.SPARSE_CSC, bad, None, no_values, 0))
    assert rc == 1 and f"col_ptr[{m}] must equal nnz = 0" in text and untouched(got), text


# ---- 11. the device checks: each refusal by text, the lowest offender named, the outputs untouched ----
N_R, M_R = 12, 7
REFUSALS = {name: case for name, case in _device_refusals().items() if case[5]}      # (the all-zero-column kind: not pre-processed)


def test_the_refusal_cases_cover_the_device_checks():
    assert sorted(REFUSALS) == sorted(["ptr[0] != 0", "non-monotone pointer", "non-monotone row pointer", "ptr[last] < nnz", "ptr[last] > nnz",
                                       "row index -1", "row index n", "column index m, CSR", "column index m, COO", "NaN", "+inf", "negative",
                                       "duplicate, COO", "duplicate, CSC"])


@pytest.mark.parametrize("index", ["int32", "int64"])
@pytest.mark.parametrize("name", list(REFUSALS))
def test_device_refusals_write_no_output(name, index):
    layout, a, b, v, count, _, words = REFUSALS[name]
    init = synth.random_init(N_R, M_R, 3, 14)
    da, db, dv = on_device(a, b, v, getattr(torch, index))
    rc, text, outs = c_run((N_R, M_R), 3, init, SWEEPS, spd=(LAYOUT_CODE[layout], da, db, dv, count))
    assert rc == 1, (name, text)
    assert text.startswith("view 0: "), text
    for w in words:
        assert w in text, (name, text)
    assert untouched(outs), name


def test_a_refusal_reaches_python_and_the_next_call_runs():
    layout, a, b, v, count, _, words = REFUSALS["duplicate, CSC"]
    init = synth.random_init(N_R, M_R, 3, 14)
    bad = torch.sparse_csc_tensor(*on_device(a, b, v, torch.int64), (N_R, M_R))
    with pytest.raises(ResnmtfError, match="is stored twice"):
        fp64_run(problem(bad, 3, init))
    layout, a, b, v, count, _, words = REFUSALS["negative"]
    with pytest.raises(ResnmtfError, match=r"view 0: negative entry \(entry 3\)"):
        fp64_run(problem(torch.sparse_csc_tensor(*on_device(a, b, v, torch.int64), (N_R, M_R)), 3, init))
    rows, cols, vals = entries(N_R, M_R, 0.4, 77)
    ref = fp64_run(problem(host_view(rows, cols, vals, (N_R, M_R)), 3, init))
    assert_same_bits(fp64_run(problem(device_view("csc", rows, cols, vals, (N_R, M_R)), 3, init)), ref, "after a refusal")


def test_a_short_array_is_refused_before_any_launch():
    """An index array far shorter than nnz says (128 bytes described as 2^20 indices: beyond any block torch's allocator
    may have carved it from): refused on its size, never read."""
    n = m = 1024
    nnz = 1 << 20
    ptr = torch.zeros(m + 1, dtype=torch.int64, device=DEV)
    short = torch.zeros(16, dtype=torch.int64, device=DEV)
    vals = torch.zeros(16, dtype=torch.float64, device=DEV)
    rc, text, outs = c_run((n, m), 2, synth.random_init(n, m, 2, 14), SWEEPS, spd=(_lib.SPARSE_CSC, ptr, short, vals, nnz))
    assert rc == 1 and untouched(outs), text
    assert f"view 0: spd->view.idx_or_cols is shorter than its element count ({nnz} elements of 8 bytes)" in text, text
