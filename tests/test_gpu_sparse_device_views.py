"""Sparse views taken from device memory (``resnmtf_set_view_sparse_device``): torch CSC / CSR / COO
tensors, int32 / int64 indices, four value types, entries in any order.  The yardstick is the host route
(``resnmtf_set_view_csc``) in the same process; every comparison is on bits (``same`` of ``test_gpu_device_views.py``, NaN
positions included), no tolerance anywhere.  The shapes are the smallest at which each piece can go wrong: a 3-bit key,
ragged 256-thread blocks, a dense row / an empty row / a one-entry column, and some 39 000 entries (many blocks, more than
one radix-sort tile).  The 3 x 2 case runs at k = 2 (an engine refuses k above a view dimension), the others at k = 3, one
of them at k = 17 too (8 lines per wave instead of 16 in the sparse passes)."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import resnmtf_amd
from resnmtf_amd import _lib, api, batched, naming, sharded, synth
from resnmtf_amd._lib import ResnmtfError
from resnmtf_amd.engine import Engine
from resnmtf_amd.problem import prepare
from test_gpu_device_views import assert_same_results, same

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DTYPES = {"fp64": torch.float64, "fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}
CODES = {torch.float64: _lib.DTYPE_F64, torch.float32: _lib.DTYPE_F32, torch.float16: _lib.DTYPE_F16, torch.bfloat16: _lib.DTYPE_BF16}
LAYOUT_CODE = {"csc": _lib.SPARSE_CSC, "csc_perm": _lib.SPARSE_CSC, "csr": _lib.SPARSE_CSR, "coo": _lib.SPARSE_COO}
LAYOUTS = tuple(LAYOUT_CODE)
# (n, m, stored fraction, special lines, the k values)
CASES = {"3x2": (3, 2, 1.0, False, (2,)), "70x45": (70, 45, 0.2, False, (3, 17)), "33x97": (33, 97, 0.05, True, (3,)),
         "257x31": (257, 31, 0.3, False, (3,)), "500x260": (500, 260, 0.3, False, (3,))}


def pattern(n, m, density, seed, special=False):
    """(rows, cols) of the stored positions in canonical CSC order; every column holds an entry.  `special`: row 5 is
    dense, row 9 empty and column 3 holds one entry."""
    rng = np.random.default_rng(seed)
    mask = rng.random((n, m)) < density
    mask[rng.integers(0, n, m), np.arange(m)] = True
    if special:
        mask[5, :] = True
        mask[9, :] = False
        mask[:, 3] = False
        mask[5, 3] = True
    cols, rows = np.nonzero(mask.T)
    return rows.astype(np.int64), cols.astype(np.int64)


def values(nnz, dtype, seed):
    """Positive values in `dtype` and the same values widened to fp64 (exact)."""
    g = torch.Generator().manual_seed(seed)
    v = (torch.rand(nnz, generator=g, dtype=torch.float64) + 0.05).to(dtype)
    return v, v.double().numpy()


def arrays(layout, rows, cols, vals, n, m, seed):
    """(pointers or row indices, indices or column indices, values) of `layout` from canonical-order entries (NumPy index
    arrays, `vals` indexable by a NumPy permutation)."""
    rng = np.random.default_rng(seed)
    nnz = len(rows)
    ccol = np.concatenate([[0], np.cumsum(np.bincount(cols, minlength=m))])
    if layout == "csc":
        return ccol, rows, vals
    if layout == "csc_perm":                              # the rows of every column in random order
        order = np.lexsort((rng.random(nnz), cols))
        return ccol, rows[order], vals[order]
    if layout == "csr":
        order = np.lexsort((rng.random(nnz), rows))      # the columns of every row in random order
        crow = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))])
        return crow, cols[order], vals[order]
    perm = rng.permutation(nnz)
    return rows[perm], cols[perm], vals[perm]


def on_device(a, b, vals, index_dtype):
    return (torch.as_tensor(np.ascontiguousarray(a), dtype=index_dtype, device=DEV),
            torch.as_tensor(np.ascontiguousarray(b), dtype=index_dtype, device=DEV), vals.to(DEV))


def as_tensor(layout, a, b, vals, shape):
    if LAYOUT_CODE[layout] == _lib.SPARSE_CSC:
        return torch.sparse_csc_tensor(a, b, vals, shape)
    if layout == "csr":
        return torch.sparse_csr_tensor(a, b, vals, shape)
    return torch.sparse_coo_tensor(torch.stack([a, b]), vals, shape, is_coalesced=True)     # (distinct positions, any order)


def raw_call(eng, v, layout, a, b, vals, nnz, pre, index_type=None, dtype=None, stream=None):
    """The C entry itself; returns (code, message)."""
    lib = _lib.load()
    ptr = lambda x: None if x is None else C.c_void_p(x if isinstance(x, int) else x.data_ptr())
    if index_type is None:
        kinds = [x.dtype for x in (a, b) if x is not None and not isinstance(x, int)]
        index_type = _lib.INDEX_I32 if kinds and kinds[0] == torch.int32 else _lib.INDEX_I64
    rc = lib.resnmtf_set_view_sparse_device(eng._h, v, layout, ptr(a), ptr(b), index_type, ptr(vals),
                                            CODES[vals.dtype] if dtype is None else dtype, nnz, 1 if pre else 0, stream)
    return rc, (lib.resnmtf_last_error(eng._h) or b"").decode()


def upload(eng, layout, a, b, vals, shape, pre):
    """Through Engine.set_view_sparse_device wherever torch can hold the tensor (its COO indices are int64 only)."""
    if layout == "coo" and a.dtype == torch.int32:
        rc, text = raw_call(eng, 0, _lib.SPARSE_COO, a, b, vals, vals.numel(), pre)
        assert rc == 0, text
    else:
        eng.set_view_sparse_device(0, as_tensor(layout, a, b, vals, shape), pre_processed=pre)


def host_csc(eng, v, ccol, rows, vals64, pre):
    """resnmtf_set_view_csc with exactly these arrays (explicit zeros stay; Engine.set_view_sparse would drop them)."""
    lib = _lib.load()
    cp = np.ascontiguousarray(ccol, dtype=np.int64); ri = np.ascontiguousarray(rows, dtype=np.int32)
    vv = np.ascontiguousarray(vals64, dtype=np.float64)
    if ri.size == 0:
        ri = np.zeros(1, np.int32); vv = np.zeros(1)
    rc = lib.resnmtf_set_view_csc(eng._h, v, cp.ctypes.data_as(C.POINTER(C.c_longlong)), ri.ctypes.data_as(C.POINTER(C.c_int)),
                                  vv.ctypes.data_as(C.POINTER(C.c_double)), 1 if pre else 0)
    return rc, (lib.resnmtf_last_error(eng._h) or b"").decode()


def state(eng, init, v=0, others=()):
    """Everything a sparse upload leaves: the CSC read-back, the plan, the storage, the empty-line report, and -- through
    one sweep from `init` -- the CSR copy and data_norms (F, S, G, lambda, mu and the sweep's error)."""
    c = eng.get_view_sparse(v)
    out = {"arrays": [c.indptr, c.indices, c.data], "storage": eng.view_storage(v), "empty": eng.empty_lines(v, counts=True)}
    for w in (v, *others):                              # (`others`: the engine's further views start over too -- the error sums all)
        eng.set_factors(w, *init)
    errs = eng.run(n_iters=1)
    out["arrays"] += [errs, *eng.get_factors(v)]
    out["plan"] = eng.view_plan(v)                     # (after the sweep: the fields of the latest prepare are this upload's)
    return out


def assert_same_state(got, ref, what):
    assert len(got["arrays"]) == len(ref["arrays"]) == 9
    for i, (a, b) in enumerate(zip(got["arrays"], ref["arrays"])):
        assert same(a, b), (what, i)
    assert got["plan"] == ref["plan"], what
    assert got["storage"] == ref["storage"], what
    er, ec, n_er, n_ec = got["empty"]
    assert not er.any() and not ec.any() and n_er == 0 and n_ec == 0, what


# ---------------------------------------------------------------------------------------------- a. equal the host route
@pytest.mark.parametrize("name", list(CASES))
def test_arrays_plan_and_a_sweep_equal_the_host_route(name):
    n, m, density, special, ks = CASES[name]
    rows, cols = pattern(n, m, density, 7 * n + m, special)
    nnz = len(rows)
    if name == "500x260":
        assert nnz > 35000
    if special:
        per_row = np.bincount(rows, minlength=n); per_col = np.bincount(cols, minlength=m)
        assert per_row[5] == m and per_row[9] == 0 and per_col[3] == 1
    ccol = np.concatenate([[0], np.cumsum(np.bincount(cols, minlength=m))])
    for k in ks:
        init = synth.random_init(n, m, k, 11)
        with Engine([n], [m], [k], nnz=[nnz]) as eng:
            for dname in (DTYPES if name == "70x45" and k == 3 else ["fp32"]):
                vals, vals64 = values(nnz, DTYPES[dname], n + m)
                x = sp.csc_matrix((vals64, rows, ccol), shape=(n, m))
                for pre in (False, True):
                    eng.set_view_sparse(0, x, pre_processed=pre)
                    ref = state(eng, init)
                    assert ref["storage"] == (True, nnz, nnz) and np.isfinite(ref["arrays"][3]).all()
                    for layout in LAYOUTS:
                        for index_dtype in (torch.int32, torch.int64):
                            a, b, v = on_device(*arrays(layout, rows, cols, vals, n, m, 3), index_dtype)
                            eng.set_view_sparse(0, sp.csc_matrix(([1.0], ([0], [0])), shape=(n, m)), pre_processed=True)   # (the last upload is gone)
                            upload(eng, layout, a, b, v, (n, m), pre)
                            assert_same_state(state(eng, init), ref, (name, k, dname, pre, layout, str(index_dtype)))


# ------------------------------------------------------------------------------------- b. the fast path is the slow path
@pytest.mark.parametrize("name", ["500x260", "70x45"])
def test_canonical_csc_and_shuffled_coo_leave_the_same_view(name):
    n, m, density, special, _ = CASES[name]
    rows, cols = pattern(n, m, density, 5 * n + m)
    vals, _ = values(len(rows), torch.float32, 21)
    init = synth.random_init(n, m, 3, 12)
    out = []
    with Engine([n], [m], [3], nnz=[len(rows)]) as fast, Engine([n], [m], [3], nnz=[len(rows)]) as slow:
        for eng, layout in ((fast, "csc"), (slow, "coo")):
            a, b, v = on_device(*arrays(layout, rows, cols, vals, n, m, 4), torch.int64)
            if layout == "coo":
                assert not np.array_equal(a.cpu().numpy(), rows)           # (really out of order)
            for pre in (False, True):
                upload(eng, layout, a, b, v, (n, m), pre)
                out.append(state(eng, init))
    assert_same_state(out[0], out[2], "normalised")
    assert_same_state(out[1], out[3], "as given")


# ------------------------------------------------------------------------------------------------------ c. explicit zeros
def test_explicit_zeros_stay_stored():
    n, m = 70, 45
    rows, cols = pattern(n, m, 0.2, 31)
    nnz = len(rows)
    ccol = np.concatenate([[0], np.cumsum(np.bincount(cols, minlength=m))])
    vals, vals64 = values(nnz, torch.float32, 5)
    zeros = np.array([ccol[4], ccol[10] + 1, nnz - 1])                      # first of a column, inside one, the last entry
    assert ccol[11] - ccol[10] > 2 and ccol[5] - ccol[4] > 1
    vals[zeros] = 0.0; vals64[zeros] = 0.0
    init = synth.random_init(n, m, 3, 13)
    with Engine([n], [m], [3], nnz=[nnz]) as eng:
        for pre in (False, True):
            rc, text = host_csc(eng, 0, ccol, rows, vals64, pre)
            assert rc == 0, text
            ref = state(eng, init)
            assert ref["storage"] == (True, nnz, nnz)                       # the zeros counted
            assert (ref["arrays"][2][zeros] == 0.0).all()
            for layout in LAYOUTS:
                a, b, v = on_device(*arrays(layout, rows, cols, vals, n, m, 6), torch.int64)
                upload(eng, layout, a, b, v, (n, m), pre)
                assert_same_state(state(eng, init), ref, (pre, layout))
        # a column whose only entries are stored zeros
        vals[ccol[7]:ccol[8]] = 0.0; vals64[ccol[7]:ccol[8]] = 0.0
        for layout in LAYOUTS:
            a, b, v = on_device(*arrays(layout, rows, cols, vals, n, m, 6), torch.int64)
            with pytest.raises(ResnmtfError, match="column 7 is all zero"):
                upload(eng, layout, a, b, v, (n, m), False)
            upload(eng, layout, a, b, v, (n, m), True)
            assert eng.view_storage(0) == (True, nnz, nnz)
        rc, text = host_csc(eng, 0, ccol, rows, vals64, False)
        assert rc == 1 and "column 7 is all zero" in text                   # (the host route's own words)


# ------------------------------------------------------------------------------------------------------------ d. refusals
N_R, M_R = 12, 7


def _refusal_base():
    rows, cols = pattern(N_R, M_R, 0.4, 77)
    ccol = np.concatenate([[0], np.cumsum(np.bincount(cols, minlength=M_R))])
    assert (np.diff(ccol) >= 2).all() and ccol[2] >= 1
    vals, vals64 = values(len(rows), torch.float32, 8)
    return rows, cols, ccol, vals, vals64


def _device_refusals():
    """name -> (layout, arrays as NumPy / torch values, nnz handed over, pre_processed, words of the message)."""
    rows, cols, ccol, vals, _ = _refusal_base()
    nnz = len(rows)
    crow, ccols, cvals = arrays("csr", rows, cols, vals, N_R, M_R, 1)
    out = {}

    def csc(name, words, ptr=ccol, idx=rows, v=vals, count=nnz, pre=True):
        out[name] = ("csc", np.array(ptr), np.array(idx), v.clone(), count, pre, words)

    p = ccol.copy(); p[0] = 1
    csc("ptr[0] != 0", ["col_ptr[0] must be 0"], ptr=p)
    p = ccol.copy(); p[3] = p[2] - 1; p[6] = p[5] - 1                      # two offenders: the lower one is named
    csc("non-monotone pointer", ["col_ptr is not monotone (column 2)"], ptr=p)
    p = crow.copy(); p[4] = p[3] - 1
    out["non-monotone row pointer"] = ("csr", p, ccols.copy(), cvals.clone(), nnz, True, ["row_ptr is not monotone (row 3)"])
    p = ccol.copy(); p[-1] = nnz - 1
    csc("ptr[last] < nnz", [f"col_ptr[{M_R}] must equal nnz = {nnz}"], ptr=p)
    p = ccol.copy(); p[-1] = nnz + 1
    csc("ptr[last] > nnz", [f"col_ptr[{M_R}] must equal nnz = {nnz}"], ptr=p)
    i = rows.copy(); i[9] = -1; i[4] = -1
    csc("row index -1", ["row index out of range (entry 4)"], idx=i)
    i = rows.copy(); i[6] = N_R
    csc("row index n", ["row index out of range (entry 6)"], idx=i)
    i = ccols.copy(); i[5] = M_R; i[11] = M_R + 3
    out["column index m, CSR"] = ("csr", crow.copy(), i, cvals.clone(), nnz, True, ["column index out of range (entry 5)"])
    r, c, v = arrays("coo", rows, cols, vals, N_R, M_R, 2)
    c = c.copy(); c[8] = M_R
    out["column index m, COO"] = ("coo", r.copy(), c, v.clone(), nnz, True, ["column index out of range (entry 8)"])
    for name, bad, words in (("NaN", float("nan"), "non-finite entry (entry 3)"), ("+inf", float("inf"), "non-finite entry (entry 3)"),
                             ("negative", -0.25, "negative entry (entry 3)")):
        v = vals.clone(); v[3] = bad; v[10] = bad
        csc(name, [words], v=v)
    r, c, v = arrays("coo", rows, cols, vals, N_R, M_R, 2)
    r = r.copy(); c = c.copy(); r[0], c[0] = r[5], c[5]
    out["duplicate, COO"] = ("coo", r, c, v.clone(), nnz, True, [f"(row {r[5]}, column {c[5]}) is stored twice"])
    i = rows.copy(); i[ccol[2] + 1] = i[ccol[2]]
    csc("duplicate, CSC", [f"(row {i[ccol[2]]}, column 2) is stored twice"], idx=i)
    v = vals.clone(); v[ccol[5]:ccol[6]] = 0.0; v[ccol[3]:ccol[4]] = 0.0
    csc("all-zero column", ["column 3 is all zero"], v=v, pre=False)
    csc("nnz = 0, not pre-processed", ["is all zero"], ptr=np.zeros(M_R + 1, np.int64), idx=rows[:0], v=vals[:0], count=0, pre=False)
    return out


DEVICE_REFUSALS = list(_device_refusals())
HOST_REFUSALS = ["capacity", "negative nnz", "dense view", "NULL pointers", "NULL values", "layout", "index type", "dtype",
                 "host pointer", "host values"]


@pytest.mark.parametrize("name", DEVICE_REFUSALS + HOST_REFUSALS)
def test_refusals_leave_the_view_as_it_was(name):
    rows, cols, ccol, vals, vals64 = _refusal_base()
    nnz = len(rows)
    init = synth.random_init(N_R, M_R, 3, 14)
    x = sp.csc_matrix((vals64, rows, ccol), shape=(N_R, M_R))
    with Engine([N_R, N_R], [M_R, M_R], [3, 3], nnz=[nnz, None]) as eng:
        eng.set_view(1, np.full((N_R, M_R), 1.0 / N_R))
        eng.set_view_sparse(0, x, pre_processed=False)
        before = state(eng, init, others=(1,))
        eng.set_view_sparse(0, x, pre_processed=False)                     # (state() ran a sweep: the same starting point again)
        if name in DEVICE_REFUSALS:
            layout, a, b, v, count, pre, words = _device_refusals()[name]
            for index_dtype in (torch.int32, torch.int64):
                da, db, dv = on_device(a, b, v, index_dtype)
                rc, text = raw_call(eng, 0, LAYOUT_CODE[layout], da, db, dv, count, pre)
                assert rc == 1, (name, text)
                for w in words:
                    assert w in text, (name, text)
        else:
            a, b, v = on_device(ccol, rows, vals, torch.int64)
            host_rows = np.ascontiguousarray(rows)
            host_vals = np.ascontiguousarray(vals64)
            view, code = 0, 1
            if name == "capacity":
                call = lambda: raw_call(eng, 0, _lib.SPARSE_CSC, a, b, v, nnz + 1, True)
                words = f"nnz = {nnz + 1} exceeds the view's nnz capacity {nnz}"
            elif name == "negative nnz":
                call, words = (lambda: raw_call(eng, 0, _lib.SPARSE_CSC, a, b, v, -1, True)), "negative"
            elif name == "dense view":
                call, words = (lambda: raw_call(eng, 1, _lib.SPARSE_CSC, a, b, v, nnz, True)), "dense"
            elif name == "NULL pointers":
                call, words = (lambda: raw_call(eng, 0, _lib.SPARSE_CSC, None, b, v, nnz, True)), "NULL"
            elif name == "NULL values":
                call, words = (lambda: raw_call(eng, 0, _lib.SPARSE_CSC, a, b, None, nnz, True, dtype=_lib.DTYPE_F32)), "NULL"
            elif name == "layout":
                call, words = (lambda: raw_call(eng, 0, 7, a, b, v, nnz, True)), "layout"
            elif name == "index type":
                call, words = (lambda: raw_call(eng, 0, _lib.SPARSE_CSC, a, b, v, nnz, True, index_type=5)), "index type"
            elif name == "dtype":
                call, words = (lambda: raw_call(eng, 0, _lib.SPARSE_CSC, a, b, v, nnz, True, dtype=9)), "dtype"
            elif name == "host pointer":
                call, words = (lambda: raw_call(eng, 0, _lib.SPARSE_CSC, a, int(host_rows.ctypes.data), v, nnz, True)), "device memory"
            else:
                call = lambda: raw_call(eng, 0, _lib.SPARSE_CSC, a, b, int(host_vals.ctypes.data), nnz, True, dtype=_lib.DTYPE_F64)
                words = "device memory"
            rc, text = call()
            assert rc == code and words in text, (name, rc, text)
        assert_same_state(state(eng, init, others=(1,)), before, name)
        # and the handle takes the next good upload
        a, b, v = on_device(ccol, rows, vals, torch.int64)
        rc, text = raw_call(eng, 0, _lib.SPARSE_CSC, a, b, v, nnz, False)
        assert rc == 0, text
        assert_same_state(state(eng, init, others=(1,)), before, name + ": after")


def test_no_stored_entry_is_a_view_when_pre_processed():
    n, m = N_R, M_R
    init = synth.random_init(n, m, 3, 15)
    with Engine([n], [m], [3], nnz=[4]) as eng:
        for layout, ptr_len in ((_lib.SPARSE_CSC, m + 1), (_lib.SPARSE_CSR, n + 1), (_lib.SPARSE_COO, 0)):
            ptr = torch.zeros(ptr_len, dtype=torch.int64, device=DEV)
            rc, text = raw_call(eng, 0, layout, ptr if ptr_len else None, None, torch.zeros(0, dtype=torch.float32, device=DEV), 0, True)
            assert rc == 0, text
            assert eng.view_storage(0) == (True, 0, 4)
            c = eng.get_view_sparse(0)
            assert c.nnz == 0 and not c.indptr.any()
            eng.set_factors(0, *init)
            assert len(eng.run(n_iters=1)) == 1                             # a sweep runs
        t = torch.sparse_csc_tensor(torch.zeros(m + 1, dtype=torch.int64), torch.zeros(0, dtype=torch.int64), torch.zeros(0), (n, m)).to(DEV)
        eng.set_view_sparse_device(0, t, pre_processed=True)
        with pytest.raises(ResnmtfError, match="all zero"):
            eng.set_view_sparse_device(0, t, pre_processed=False)


# ------------------------------------------------------------------------------------------------------------ e. ordering
def test_upload_is_ordered_after_the_producer_stream():
    n, m = 300, 200
    rows, cols = pattern(n, m, 0.3, 41)
    nnz = len(rows)
    ccol = np.concatenate([[0], np.cumsum(np.bincount(cols, minlength=m))])
    a, b, _ = on_device(ccol, rows, torch.zeros(1), torch.int64)
    base = torch.rand(1500, 1100, device=DEV, dtype=torch.float32)
    init = synth.random_init(n, m, 3, 16)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=DEV)
    with Engine([n], [m], [3], nnz=[nnz]) as eng:
        with torch.cuda.stream(side):
            t = base
            for _ in range(200):                       # a queue of work the upload has to wait for
                t = t * 1.0009765625 + 0.03125
            vals = t.reshape(-1)[:nnz] + 0.5           # the producer, enqueued immediately before the call
            eng.set_view_sparse_device(0, torch.sparse_csc_tensor(a, b, vals, (n, m)), pre_processed=False)   # (no synchronisation by the test)
        got = state(eng, init)
        torch.cuda.synchronize()
        eng.set_view_sparse(0, sp.csc_matrix((vals.double().cpu().numpy(), rows, ccol), shape=(n, m)), pre_processed=False)
        assert_same_state(got, state(eng, init), "side stream")


# --------------------------------------------------------------------------------------------------- f. the Python routes
def planted_q(seed):
    """The planted problem of test_gpu_sparse.py (three 60 x 60 blocks of height 10 in 180 x 180, 5 % noise) with every
    entry rounded to a multiple of 2^-10: every fp64 column sum is exact in any order, so the host's and the device's
    normalisation agree bitwise by construction."""
    rng = np.random.default_rng(seed)
    rc = np.kron(np.eye(3), np.ones((60, 1)))
    x = rc @ np.diag([10.0, 10.0, 10.0]) @ rc.T + 0.1 * np.abs(rng.normal(size=(180, 180))) * (rng.random((180, 180)) < 0.05)
    return np.round(x * 1024.0) / 1024.0


def sparse_tensor(x, layout="csc"):
    t = torch.tensor(x, dtype=torch.float64, device=DEV)
    return {"csc": t.to_sparse_csc, "csr": t.to_sparse_csr, "coo": lambda: t.to_sparse_coo().coalesce()}[layout]()


def assert_equal_results(got, ref, keys):
    for key in keys:
        a, b = got[key], ref[key]
        if isinstance(b, list):
            assert len(a) == len(b), key
            for u, w in zip(a, b):
                assert same(u, w), key
        else:
            assert same(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)), key


LIST_KEYS = ("output_f", "output_s", "output_g", "row_clusters", "col_clusters")


def test_res_nmtf_inner_on_a_sparse_tensor_and_an_array():
    x1, x2 = planted_q(1), planted_q(2)
    rn, cn = naming.give_names([x1, x2], None, None, None, None)
    rs, cs = naming.shared_names(rn), naming.shared_names(cn)
    kw = dict(k_vec=[3, 3], n_iters=100, spurious=False, row_names=rn, col_names=cn, seed=5)
    ref = resnmtf_amd.res_nmtf_inner([sp.csr_matrix(x1), x2], rs, cs, **kw)
    for layout in ("csc", "csr", "coo"):
        res = resnmtf_amd.res_nmtf_inner([sparse_tensor(x1, layout), x2], rs, cs, **kw)
        assert list(res) == list(ref)
        assert_equal_results(res, ref, LIST_KEYS + ("lambda", "mu", "All_Error", "Error"))
        assert res["bisil"] is None and ref["bisil"] is None
    assert np.isfinite(ref["All_Error"]).all() and len(ref["All_Error"]) == 100
    # output="torch": device tensors equal to the NumPy results
    res = resnmtf_amd.res_nmtf_inner([sparse_tensor(x1), x2], rs, cs, output="torch", **kw)
    assert_same_results(res, ref, True)


def test_apply_resnmtf_with_stability_on_sparse_tensors():
    x1, x2 = planted_q(1), planted_q(2)
    kw = dict(k_val=3, spurious=False, stability=True, n_stability=3, n_iters=100, seed=7)
    ref = resnmtf_amd.apply_resnmtf([sp.csr_matrix(x1), sp.csr_matrix(x2)], sparse_on_device=True, **kw)
    res = resnmtf_amd.apply_resnmtf([sparse_tensor(x1, "csc"), sparse_tensor(x2, "coo")], **kw)
    assert list(res) == list(ref)
    assert sum(rc.sum() for rc in ref["row_clusters"]) > 0
    assert_equal_results(res, ref, LIST_KEYS + ("All_Error", "Error"))

    def relevance(data, **opt):                       # the relevance itself: apply_resnmtf's steps, the unstable clusters kept
        p = prepare(api._views(data), None, None, None, None, None, normalise=True, symmetrise=True)
        inner = resnmtf_amd.res_nmtf_inner(p.data, p.row_shared, p.col_shared, k_vec=[3, 3], phi=p.phi, xi=p.xi, psi=p.psi, n_iters=100,
                                           spurious=False, row_names=p.row_names, col_names=p.col_names, seed=7)
        return api.stability_check(p.data, inner, 3, p.phi, p.xi, p.psi, 100, False, 5, False, "euclidean", row_names=p.row_names,
                                   col_names=p.col_names, seed=7, n_stability=3, remove_unstable=False, **opt)["relevance"]

    rel_ref = relevance([sp.csr_matrix(x1), sp.csr_matrix(x2)], sparse_on_device=True)
    rel = relevance([sparse_tensor(x1, "csr"), sparse_tensor(x2, "csc")])
    assert rel_ref.shape == (2, 3) and np.isfinite(rel_ref).all() and same(rel, rel_ref)


def test_k_sweep_with_removal_on_sparse_tensors():
    x1, x2 = planted_q(1), planted_q(2)
    kw = dict(k_min=3, k_max=4, k_sweep=True, n_iters=50, seed=7, num_repeats=2, n_stability=2, spurious_on_device=True, bisil_sparse=True,
              shuffle_sparse=True, return_sweep=True)
    ref = resnmtf_amd.apply_resnmtf([sp.csr_matrix(x1), sp.csr_matrix(x2)], sparse_on_device=True, **kw)
    res = resnmtf_amd.apply_resnmtf([sparse_tensor(x1, "csc"), sparse_tensor(x2, "csr")], **kw)
    assert list(res) == list(ref) and res["k_sweep"] == ref["k_sweep"]
    assert_equal_results(res, ref, LIST_KEYS + ("All_Error", "Error", "lambda", "mu"))
    assert res["bisil"] == ref["bisil"]
    assert same(np.asarray(res["spurious"]["removed"], dtype=np.float64), np.asarray(ref["spurious"]["removed"], dtype=np.float64))


def test_python_refusals_keep_their_messages():
    x = planted_q(1)
    t = sparse_tensor(x)
    kw = dict(k_vec=[3], n_iters=5, seed=1)
    with pytest.raises(NotImplementedError, match="host_init=True .* is not available for sparse views"):
        resnmtf_amd.res_nmtf_inner([t], None, None, spurious=False, host_init=True, **kw)
    with pytest.raises(NotImplementedError, match="the grouped path takes dense views only"):
        batched.run_jobs_grouped([batched.Job(data=[t], k_val=3)])
    with pytest.raises(NotImplementedError, match="sparse views are not supported by the view-sharded driver"):
        f, s_, g = synth.random_init(180, 180, 3, 2)
        sharded.res_nmtf_inner([t], init_f=[f], init_s=[s_], init_g=[g], k_vec=[3], n_iters=5, rank=0, world=1)
    with pytest.raises(NotImplementedError, match="device shuffles of sparse views are not supported"):
        resnmtf_amd.res_nmtf_inner([t], None, None, spurious=True, spurious_on_device=True, num_repeats=2, **kw)
    with pytest.raises(NotImplementedError, match="the bisilhouette score of sparse views is not supported"):
        resnmtf_amd.res_nmtf_inner([t], None, None, spurious=False, score_bisil=True, **kw)
    idx = torch.tensor([[0, 0, 1], [1, 1, 2]], device=DEV)
    uncoalesced = torch.sparse_coo_tensor(idx, torch.ones(3, device=DEV), (180, 180))
    assert not uncoalesced.is_coalesced()
    bsr = torch.tensor(x, device=DEV).to_sparse_bsr((2, 2))
    with Engine([180], [180], [3], nnz=[t._nnz()]) as eng:
        with pytest.raises(ValueError, match="coalesce"):
            eng.set_view_sparse_device(0, uncoalesced)
        with pytest.raises(ValueError, match="sparse_bsr"):
            eng.set_view_sparse_device(0, bsr)
        with pytest.raises(ValueError, match="lives on"):
            eng.set_view_sparse_device(0, t.cpu())
        with pytest.raises(ValueError, match="shape"):
            eng.set_view_sparse_device(0, sparse_tensor(x[:, :100]))
    with pytest.raises(ValueError, match="coalesce"):
        resnmtf_amd.res_nmtf_inner([uncoalesced], None, None, spurious=False, **kw)
    with pytest.raises(ValueError, match="sparse_bsr"):
        resnmtf_amd.res_nmtf_inner(bsr, None, None, spurious=False, **kw)
    # the device checks surface as the engine's error
    bad = torch.sparse_csc_tensor(t.ccol_indices(), t.row_indices(), -t.values(), (180, 180))
    with pytest.raises(ResnmtfError, match="negative entry"):
        resnmtf_amd.res_nmtf_inner([bad], None, None, spurious=False, **kw)
    # a CPU sparse tensor takes the host route
    ref = resnmtf_amd.res_nmtf_inner([sp.csc_matrix(x)], None, None, spurious=False, **kw)
    res = resnmtf_amd.res_nmtf_inner(t.cpu(), None, None, spurious=False, **kw)
    assert_equal_results(res, ref, LIST_KEYS + ("All_Error",))


# ------------------------------------------------------------------------------------------------------- g. free memory
def test_free_device_memory_is_the_same_after_every_round():
    dev = torch.device("cuda", 0)
    n, m = 70, 45
    rows, cols = pattern(n, m, 0.2, 51)
    nnz = len(rows)
    vals, _ = values(nnz, torch.float32, 9)
    good = {layout: on_device(*arrays(layout, rows, cols, vals, n, m, 8), torch.int64) for layout in LAYOUTS}
    r, c, v = arrays("coo", rows, cols, vals, n, m, 8)
    r = r.copy(); c = c.copy(); r[1], c[1] = r[20], c[20]
    duplicate = on_device(r, c, v, torch.int64)                            # refused after the sort storage was taken
    i = rows.copy(); i[7] = n
    out_of_range = on_device(arrays("csc", rows, cols, vals, n, m, 8)[0], i, vals, torch.int64)
    p = arrays("csc", rows, cols, vals, n, m, 8)[0].copy(); p[0] = 2
    bad_ptr = on_device(p, rows, vals, torch.int64)
    with Engine([n], [m], [3], nnz=[nnz]) as eng:

        def one_round():
            for layout in LAYOUTS:
                for pre in (False, True):
                    rc, text = raw_call(eng, 0, LAYOUT_CODE[layout], *good[layout], nnz, pre)
                    assert rc == 0, text
            for what, (layout, arrs) in {"stored twice": (_lib.SPARSE_COO, duplicate), "out of range": (_lib.SPARSE_CSC, out_of_range),
                                         "must be 0": (_lib.SPARSE_CSC, bad_ptr)}.items():
                rc, text = raw_call(eng, 0, layout, *arrs, nnz, True)
                assert rc == 1 and what in text, text
            rc, text = raw_call(eng, 0, _lib.SPARSE_CSC, *good["csc"], nnz + 1, True)
            assert rc == 1 and "capacity" in text

        one_round()                                                        # warm-up
        free = []
        for _ in range(3):
            one_round()
            free.append(torch.cuda.mem_get_info(dev)[0])
        print("free device memory after the three rounds:", free)
        assert max(free) - min(free) == 0, free
