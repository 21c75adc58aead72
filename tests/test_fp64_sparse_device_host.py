"""Host side of sparse views of the fp64 path taken from device memory (resnmtf_fp64_run_sparse_device, engine.fp64_run,
api.res_nmtf_inner(precision="fp64", fp64_sparse_device=True); no GPU): the symbol and the structs are
bound, the flag is keyword-only and opt-in -- without it the refusals of tests/test_fp64_host.py, test_fp64_sparse_host.py
and test_fp64_device_host.py still fire, the one of sparse tensors under fp64_device=True included --, with it the tensor
reaches the problem untouched, precision="f32" ignores it, and the C entry refuses a malformed
resnmtf_fp64_sparse_device before it touches a device, by text."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

from resnmtf_amd import _lib, api, device_views, engine
from test_fp64_device_host import THERE, _CallLog, _c_job, _dev, _inner_args, _mat, _never, _null

torch = pytest.importorskip("torch")

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "resnmtf_hip.h")


def _sparse_there(layout="csc", shape=(12, 9)):
    """A sparse tensor that is not on the CPU (the meta device stands for device memory) without a stored entry."""
    z = lambda count, dtype=torch.int64: torch.zeros(count, dtype=dtype, device="meta")
    if layout == "csc":
        return torch.sparse_csc_tensor(z(shape[1] + 1), z(0), z(0, torch.float64), size=shape, check_invariants=False)
    if layout == "csr":
        return torch.sparse_csr_tensor(z(shape[0] + 1), z(0), z(0, torch.float64), size=shape, check_invariants=False)
    return torch.sparse_coo_tensor(torch.zeros((2, 0), dtype=torch.int64, device="meta"), z(0, torch.float64), size=shape,
                                   is_coalesced=True)


# ---- the binding ----
def test_symbol_and_structs_are_bound():
    restype, argtypes = _lib.SIGNATURES["resnmtf_fp64_run_sparse_device"]
    assert restype is C.c_int
    assert argtypes == [C.c_int, C.POINTER(_lib.GroupJob), C.POINTER(_lib.Fp64Sparse), C.POINTER(_lib.Fp64Device),
                        C.POINTER(_lib.Fp64SparseDevice), C.c_double, C.c_int]
    lib = _lib.load()                                                      # (load() binds every name of SIGNATURES: it is exported)
    assert lib.resnmtf_fp64_run_sparse_device.argtypes == argtypes
    assert lib.resnmtf_abi_version() == _lib.ABI_VERSION == 2
    assert [f[0] for f in _lib.Fp64SparseDeviceView._fields_] == ["layout", "index_type", "dtype", "ptr_or_rows", "idx_or_cols",
                                                                  "values", "nnz"]
    assert [f[0] for f in _lib.Fp64SparseDevice._fields_] == ["struct_size", "stream", "view"]


def test_structs_follow_the_header():
    """The fields of the two structs, in the header's order and with its types; the sizes those give on an LP64 target (three
    ints + padding, three pointers and a long long; an int + padding, a pointer, eight views)."""
    text = open(HEADER).read()
    kinds = {"int": C.c_int, "const void*": C.c_void_p, "void*": C.c_void_p, "long long": C.c_longlong}
    view = re.search(r"typedef struct resnmtf_fp64_sparse_device_view \{(.*?)\} resnmtf_fp64_sparse_device_view;", text, re.S).group(1)
    fields = [(m.group(2), kinds[m.group(1)]) for m in re.finditer(r"^\s*(int|const void\*|long long) (\w+);", view, re.M)]
    assert fields == list(_lib.Fp64SparseDeviceView._fields_)
    whole = re.search(r"typedef struct resnmtf_fp64_sparse_device \{(.*?)\} resnmtf_fp64_sparse_device;", text, re.S).group(1)
    assert re.findall(r"^\s*(\S.*?);", whole, re.M) == ["int struct_size", "void* stream",
                                                       "resnmtf_fp64_sparse_device_view view[RESNMTF_GROUP_MAX_VIEWS]"]
    assert C.sizeof(_lib.Fp64SparseDeviceView) == 48
    assert C.sizeof(_lib.Fp64SparseDevice) == 16 + _lib.GROUP_MAX_VIEWS * 48
    assert re.search(r"int resnmtf_fp64_run_sparse_device\(int device_id, const resnmtf_group_job\* job, const resnmtf_fp64_sparse\* sp,\s*"
                     r"const resnmtf_fp64_device\* dev, const resnmtf_fp64_sparse_device\* spd, double tol,\s*int max_iters\);", text)


# ---- api.res_nmtf_inner: the flag ----
def test_the_flag_is_keyword_only(monkeypatch):
    monkeypatch.setattr(api, "Engine", _never)
    monkeypatch.setattr(engine, "fp64_run", _never)
    with pytest.raises(TypeError):
        api.res_nmtf_inner(*_inner_args(), 5, False, "euclidean", False, "fp64", False, False, True)


@pytest.mark.parametrize("layout", ["csc", "csr", "coo"])
@pytest.mark.parametrize("others", [dict(), dict(fp64_device=True), dict(fp64_sparse=True), dict(fp64_device=True, fp64_sparse=True)])
@pytest.mark.parametrize("spelled", [False, True])
def test_flag_off_keeps_the_refusal_of_sparse_tensors_in_device_memory(monkeypatch, layout, others, spelled):
    monkeypatch.setattr(api, "Engine", _never)
    monkeypatch.setattr(engine, "fp64_run", _never)
    args = list(_inner_args())
    more = {"fp64_sparse_device": False} if spelled else {}
    with pytest.raises(NotImplementedError, match=r'precision="fp64": sparse views \(view 0\) needs a live engine handle'):
        api.res_nmtf_inner(*([[_sparse_there(layout)]] + args[1:]), spurious=False, precision="fp64", **others, **more)
    with pytest.raises(NotImplementedError, match=r"sparse views \(view 0\)"):
        api.res_nmtf_inner(*([[device_views.SparseDeviceView(_sparse_there(layout))]] + args[1:]), spurious=False,
                           precision="fp64", **others, **more)


def test_flag_off_keeps_the_other_pinned_refusals(monkeypatch):
    monkeypatch.setattr(api, "Engine", _never)
    monkeypatch.setattr(engine, "fp64_run", _never)
    args = list(_inner_args())
    with pytest.raises(NotImplementedError, match="sparse views"):                       # a scipy.sparse view without fp64_sparse
        api.res_nmtf_inner(*([[sp.csc_matrix(args[0][0])]] + args[1:]), spurious=False, precision="fp64", fp64_sparse_device=True)
    there = torch.empty((12, 9), dtype=torch.float64, device="meta")
    with pytest.raises(NotImplementedError, match="views in device memory"):              # a dense tensor without fp64_device
        api.res_nmtf_inner(*([[there]] + args[1:]), spurious=False, precision="fp64", fp64_sparse_device=True)
    for flag, kwargs in (("score_bisil", dict(score_bisil=True)), ("post_on_device", dict(output="torch", post_on_device=True)),
                         ('output="torch"', dict(output="torch")), ("return_state", dict(return_state=True))):
        with pytest.raises(NotImplementedError, match=flag):
            api.res_nmtf_inner(*args, spurious=False, precision="fp64", fp64_sparse_device=True, **kwargs)
    with pytest.raises(NotImplementedError, match="spurious_on_device"):
        api.res_nmtf_inner(*args, spurious=True, spurious_on_device=True, precision="fp64", fp64_sparse_device=True)


def test_flag_on_checks_the_tensor_and_its_device(monkeypatch):
    """The new route is taken: what refuses now is device_views' own check, not the live-handle refusal."""
    monkeypatch.setattr(api, "Engine", _never)
    monkeypatch.setattr(engine, "fp64_run", _never)
    args = list(_inner_args())
    with pytest.raises(ValueError, match="view 0: the tensor lives on meta, the engine on cuda:0"):
        api.res_nmtf_inner(*([[_sparse_there()]] + args[1:]), spurious=False, precision="fp64", fp64_sparse_device=True)
    bsr = torch.sparse_bsr_tensor(torch.zeros(7, dtype=torch.int64, device="meta"), torch.zeros(0, dtype=torch.int64, device="meta"),
                                  torch.zeros((0, 2, 3), dtype=torch.float64, device="meta"), size=(12, 9), check_invariants=False)
    with pytest.raises(ValueError, match="must be sparse_csc, sparse_csr or sparse_coo"):
        api.res_nmtf_inner(*([[bsr]] + args[1:]), spurious=False, precision="fp64", fp64_sparse_device=True)


def _accept_meta(monkeypatch):
    """device_views.as_sparse_view with the one check a machine without a GPU cannot pass (the tensor is on cuda:device_id)
    taken out; everything else of it runs."""
    def as_sparse_view(x, device_id=0, what="view"):
        t = x.tensor if isinstance(x, device_views.SparseDeviceView) else x
        device_views.check_sparse_tensor(t, what)
        return x if isinstance(x, device_views.SparseDeviceView) else device_views.SparseDeviceView(t)
    monkeypatch.setattr(device_views, "as_sparse_view", as_sparse_view)


def _echo(seen):
    def runner(problem, tol, max_iters, device_id, **more):
        seen.update(problem=problem, more=more)
        n_v, k = len(problem["data"]), problem["k"]
        return {"f": problem["init_f"], "s": problem["init_s"], "g": problem["init_g"], "lambda": [np.ones(k)] * n_v,
                "mu": [np.ones(k)] * n_v, "all_error": np.array([0.3, 0.2]), "iters": 2}
    return runner


@pytest.mark.parametrize("wrapped", [False, True])
def test_flag_on_the_tensor_reaches_the_problem_untouched(monkeypatch, wrapped):
    monkeypatch.setattr(api, "Engine", _never)
    _accept_meta(monkeypatch)
    seen = {}
    monkeypatch.setattr(engine, "fp64_run", _echo(seen))
    args = list(_inner_args(2))
    there = _sparse_there("csr")
    given = device_views.SparseDeviceView(there) if wrapped else there
    res = api.res_nmtf_inner(*([[given, args[0][1]]] + args[1:]), spurious=False, precision="fp64", fp64_sparse_device=True)
    data = seen["problem"]["data"]
    assert isinstance(data[0], device_views.SparseDeviceView) and data[0].tensor is there and not data[0].raw
    assert (data[0] is given) == wrapped
    np.testing.assert_array_equal(data[1], args[0][1])
    assert seen["more"] == {}                                              # (output / return_state go with fp64_device alone)
    assert list(res) == ["output_f", "output_s", "output_g", "Error", "All_Error", "bisil", "row_clusters", "col_clusters",
                         "lambda", "mu"]
    # ... beside a host scipy.sparse view and with the device flags: the runner gets them as section 23 hands them over
    seen.clear()
    mixed = [[there, sp.csc_matrix(args[0][1])]] + args[1:]
    api.res_nmtf_inner(*mixed, spurious=False, precision="fp64", fp64_sparse_device=True, fp64_sparse=True, fp64_device=True)
    assert seen["problem"]["data"][0].tensor is there and sp.issparse(seen["problem"]["data"][1])
    assert seen["more"] == {"output": "numpy", "return_state": False}


def test_flag_on_host_init_keeps_the_sparse_views_refusal(monkeypatch):
    monkeypatch.setattr(api, "Engine", _never)
    monkeypatch.setattr(engine, "fp64_run", _never)
    _accept_meta(monkeypatch)
    args = list(_inner_args())
    with pytest.raises(NotImplementedError, match="not available for sparse views"):
        api.res_nmtf_inner([_sparse_there()], args[1], args[2], None, None, None, *args[6:], spurious=False, precision="fp64",
                           fp64_sparse_device=True, host_init=True)


class _SparseCallLog(_CallLog):
    """_CallLog with what a sparse engine is built and loaded with."""
    made = {}

    def __init__(self, n_rows, n_cols, k, device_id=0, **kw):
        super().__init__(n_rows, n_cols, k, device_id=device_id, **kw)
        _SparseCallLog.made = dict(kw)

    def set_view_sparse_device(self, v, tensor, pre_processed=False):
        _CallLog.calls.append(("set_view_sparse_device", tensor, pre_processed))


@pytest.mark.parametrize("fp64_device", [False, True])
def test_device_initialisation_uses_a_short_lived_sparse_engine(monkeypatch, fp64_device):
    monkeypatch.setattr(api, "Engine", _SparseCallLog)
    _accept_meta(monkeypatch)
    seen = {}
    monkeypatch.setattr(engine, "fp64_run", lambda problem, **kw: seen.update(problem=problem) or {
        "f": problem["init_f"], "s": problem["init_s"], "g": problem["init_g"], "lambda": problem["init_lam"],
        "mu": problem["init_mu"], "all_error": np.array([0.3]), "iters": 1})
    args = _inner_args(2)
    there = _sparse_there("coo")
    api.res_nmtf_inner([there, args[0][1]], args[1], args[2], None, None, None, *args[6:], spurious=False, precision="fp64", seed=4,
                       fp64_sparse_device=True, fp64_device=fp64_device)
    assert _SparseCallLog.made["nnz"] == [0, None]                         # view 0 is a sparse view of the engine
    read = "get_factors_device" if fp64_device else "get_factors"
    assert _CallLog.calls == (["create", ("set_view_sparse_device", there, True), "init_svd", "set_view", "init_svd", "set_restrictions"] +
                              ["set_shared_rows", "set_shared_cols"] * 2 + [read] * 2 + ["close"])
    assert seen["problem"]["data"][0].tensor is there


def test_f32_ignores_the_flag(monkeypatch):
    """The call sequence test_default_precision_leaves_the_call_sequence_as_it_is (tests/test_fp64_host.py) records."""
    monkeypatch.setattr(api, "Engine", _CallLog)
    monkeypatch.setattr(engine, "fp64_run", _never)
    args = _inner_args(2)
    want = (["create"] + ["set_view", "set_factors"] * 2 + ["set_restrictions"] + ["set_shared_rows", "set_shared_cols"] * 2 +
            ["run"] + ["finalise", "get_factors"] * 2 + ["close"])
    plain = api.res_nmtf_inner(*args, spurious=False)
    assert _CallLog.calls == want
    flagged = api.res_nmtf_inner(*args, spurious=False, precision="f32", fp64_sparse_device=True)
    assert _CallLog.calls == want and list(plain) == list(flagged)


# ---- engine.fp64_run ----
def test_fp64_run_checks_a_sparse_tensor_before_the_library(monkeypatch):
    monkeypatch.setattr(_lib, "load", lambda: None)                       # (a library call would fail on None)
    rng = np.random.default_rng(2)
    p = {"data": [_sparse_there("csc", (10, 8))], "k": 2, "init_f": [rng.random((10, 2))], "init_s": [rng.random((2, 2))],
         "init_g": [rng.random((8, 2))], "n_iters": 3}
    with pytest.raises(ValueError, match="problem 0, view 0: the tensor lives on meta, the engine on cuda:0"):
        engine.fp64_run(p)


def test_fp64_run_without_a_sparse_tensor_makes_the_calls_it_made(monkeypatch):
    """Nothing on the device: resnmtf_fp64_run / _run_sparse, never the device entries."""
    class Lib:
        calls = []

        def __getattr__(self, name):
            def call(*args):
                Lib.calls.append(name)
                return _lib.OK
            return call
    monkeypatch.setattr(_lib, "load", lambda: Lib())
    rng = np.random.default_rng(2)
    p = {"data": [rng.random((10, 8)) + 0.1], "k": 2, "init_f": [rng.random((10, 2))], "init_s": [rng.random((2, 2))],
         "init_g": [rng.random((8, 2))], "n_iters": 3}
    engine.fp64_run(p)
    engine.fp64_run(dict(p, data=[sp.csc_matrix(p["data"][0])]))
    assert Lib.calls == ["resnmtf_fp64_run", "resnmtf_fp64_run_sparse"]


# ---- the C entry: what it refuses before it touches a device ----
def _spd():
    d = _lib.Fp64SparseDevice()
    d.struct_size = C.sizeof(_lib.Fp64SparseDevice)
    return d


def _view(d, v=0, layout=_lib.SPARSE_CSC, index_type=_lib.INDEX_I64, dtype=_lib.DTYPE_F64, ptr=THERE, idx=THERE, values=THERE, nnz=5):
    c = d.view[v]
    c.layout, c.index_type, c.dtype, c.ptr_or_rows, c.idx_or_cols, c.values, c.nnz = layout, index_type, dtype, ptr, idx, values, nnz


def _host_sparse(j):
    """(sp, keep): view 0 as host CSC arrays."""
    s = _lib.Fp64Sparse()
    s.struct_size = C.sizeof(_lib.Fp64Sparse)
    n, m = j.n_rows[0], j.n_cols[0]
    csc = [np.arange(m + 1, dtype=np.int64), np.zeros(m, np.int32), np.ones(m)]
    s.view[0].col_ptr = csc[0].ctypes.data_as(C.POINTER(C.c_longlong))
    s.view[0].row_idx = csc[1].ctypes.data_as(C.POINTER(C.c_int))
    s.view[0].values = csc[2].ctypes.data_as(C.POINTER(C.c_double))
    return s, csc


def _cases():
    """(name, edit of (job, spd) returning (job, sp, dev), the text expected)."""
    def plain(edit_view):
        def edit(j, d):
            edit_view(d)
            return _null(j, "x"), None, None
        return edit

    def in_job_too(j, d):
        _view(d)
        return j, None, None

    def in_sp_too(j, d):
        _view(d)
        s, keep = _host_sparse(j)
        d._keep = keep
        return _null(j, "x"), s, None

    def in_dev_too(j, d):
        _view(d)
        dev = _dev()
        dev.x[0] = _mat()
        return _null(j, "x"), None, dev

    def nowhere(j, d):
        return _null(j, "x"), None, None

    def nowhere_beside_dev(j, d):
        return _null(j, "x"), None, _dev()

    def bad_size(j, d):
        _view(d)
        d.struct_size -= 8
        return _null(j, "x"), None, None

    def streams(j, d):
        _view(d)
        dev = _dev()
        dev.stream, d.stream = THERE, THERE + 64
        return _null(j, "x"), None, dev

    return [
        ("struct_size", bad_size, b"resnmtf_fp64_sparse_device struct_size mismatch"),
        ("beyond n_views", plain(lambda d: (_view(d), _view(d, v=1))), b"view 1: spd->view is given beyond n_views"),
        ("beyond n_views, nnz alone", plain(lambda d: (_view(d), _view(d, v=3, ptr=None, idx=None, values=None, nnz=1))),
         b"view 3: spd->view is given beyond n_views"),
        ("job->x too", in_job_too, b"view 0: x is given in two places, in sparse device arrays (spd->view) and in the job (job->x)"),
        ("sp too", in_sp_too, b"view 0: x is given in two places, in sparse device arrays (spd->view) and as host CSC arrays (sp->view)"),
        ("dev->x too", in_dev_too, b"view 0: x is given in two places, in sparse device arrays (spd->view) and as a device matrix (dev->x)"),
        ("nowhere", nowhere, b"view 0: x is given in none of job->x, sp, dev->x and spd"),
        ("nowhere, beside dev", nowhere_beside_dev, b"view 0: x is given in none of job->x, sp, dev->x and spd"),
        ("layout", plain(lambda d: _view(d, layout=3)), b"view 0: spd->view: unknown layout"),
        ("negative layout", plain(lambda d: _view(d, layout=-1)), b"view 0: spd->view: unknown layout"),
        ("index type", plain(lambda d: _view(d, index_type=2)), b"view 0: spd->view: unknown index type"),
        ("dtype", plain(lambda d: _view(d, dtype=4)), b"view 0: spd->view: unknown dtype"),
        ("negative nnz", plain(lambda d: _view(d, nnz=-1)), b"view 0: spd->view: nnz is negative"),
        ("NULL pointers", plain(lambda d: _view(d, ptr=None)), b"view 0: spd->view: ptr_or_rows / idx_or_cols / values is NULL"),
        ("NULL pointers at nnz = 0, CSR", plain(lambda d: _view(d, layout=_lib.SPARSE_CSR, ptr=None, idx=None, nnz=0)),
         b"view 0: spd->view: ptr_or_rows / idx_or_cols / values is NULL"),
        ("NULL indices", plain(lambda d: _view(d, idx=None)), b"view 0: spd->view: ptr_or_rows / idx_or_cols / values is NULL"),
        ("NULL values", plain(lambda d: _view(d, values=None)), b"view 0: spd->view: ptr_or_rows / idx_or_cols / values is NULL"),
        ("NULL rows, COO", plain(lambda d: _view(d, layout=_lib.SPARSE_COO, ptr=None)),
         b"view 0: spd->view: ptr_or_rows / idx_or_cols / values is NULL"),
        ("streams", streams, b"dev->stream and spd->stream differ"),
    ]


@pytest.mark.parametrize("case", _cases(), ids=lambda c: c[0])
def test_c_entry_refuses_a_malformed_struct(case):
    _, edit, text = case
    lib = _lib.load()
    invalid = {name: c for c, name in _lib.ERR_NAMES.items()}["INVALID"]
    j, keep, outs = _c_job()
    d = _spd()
    j, s, dev = edit(j, d)
    rc = lib.resnmtf_fp64_run_sparse_device(0, C.byref(j), None if s is None else C.byref(s), None if dev is None else C.byref(dev),
                                            C.byref(d), 1e-6, 100)
    assert rc == invalid, lib.resnmtf_last_error(None)
    assert text in lib.resnmtf_last_error(None), lib.resnmtf_last_error(None)
    assert all(np.all(o == -7) for o in outs)                             # a refusal writes no output


def test_c_entry_refuses_a_view_in_no_place_beside_a_sparse_device_view():
    """Two views, the first in spd, the second nowhere: the second is named."""
    lib = _lib.load()
    j, keep, outs = _c_job(V=2)
    d = _spd()
    _view(d)
    j = _null(_null(j, "x"), "x", v=1)
    assert lib.resnmtf_fp64_run_sparse_device(0, C.byref(j), None, None, C.byref(d), 1e-6, 100) != _lib.OK
    assert b"view 1: x is given in none of job->x, sp, dev->x and spd" in lib.resnmtf_last_error(None)
    assert all(np.all(o == -7) for o in outs)


@pytest.mark.parametrize("which", ["ptr_or_rows", "idx_or_cols", "values"])
def test_c_entry_refuses_host_memory_given_as_device_memory(which):
    """The arrays are looked at after the structure and before any allocation; host memory is not device memory (without a
    device the runtime knows no pointer at all, and the refusal is the same)."""
    lib = _lib.load()
    j, keep, outs = _c_job()
    n, m = j.n_rows[0], j.n_cols[0]
    host = {"ptr_or_rows": np.arange(m + 1, dtype=np.int64), "idx_or_cols": np.zeros(m, np.int64), "values": np.ones(m)}
    d = _spd()
    order = ["ptr_or_rows", "idx_or_cols", "values"]
    # (the arrays are judged in order: the ones before `which` are not given as host memory -- a COO view without entries
    # has none to judge -- so `which` is the first the runtime is asked about)
    if which == "ptr_or_rows":
        _view(d, ptr=host[which].ctypes.data, idx=host["idx_or_cols"].ctypes.data, values=host["values"].ctypes.data, nnz=m)
    else:
        _view(d, layout=_lib.SPARSE_COO, ptr=None, idx=None, values=None, nnz=0)
        setattr(d.view[0], which, host[which].ctypes.data)
    j = _null(j, "x")
    assert lib.resnmtf_fp64_run_sparse_device(0, C.byref(j), None, None, C.byref(d), 1e-6, 100) != _lib.OK
    assert f"view 0: spd->view.{which} is not device memory of device 0".encode() in lib.resnmtf_last_error(None), order
    assert all(np.all(o == -7) for o in outs)


def test_c_entry_without_the_struct_is_the_device_entry():
    """spd == NULL: resnmtf_fp64_run_device's refusals, word for word."""
    lib = _lib.load()
    for edit, text in ((lambda j, d: (d.x.__setitem__(0, _mat()), j)[1],
                        b"view 0: x is given both in the job (job->x) and in device memory (dev->x)"),
                       (lambda j, d: _null(j, "x"), b"view 0: x is given neither in the job (job->x) nor in device memory (dev->x)")):
        j, keep, outs = _c_job()
        d = _dev()
        j = edit(j, d)
        assert lib.resnmtf_fp64_run_sparse_device(0, C.byref(j), None, C.byref(d), None, 1e-6, 100) != _lib.OK
        assert text in lib.resnmtf_last_error(None)
    j, keep, outs = _c_job()
    j = _null(j, "x")
    assert lib.resnmtf_fp64_run_sparse_device(0, C.byref(j), None, None, None, 1e-6, 100) != _lib.OK
    assert b"x / f0 / s0 / g0 is NULL" in lib.resnmtf_last_error(None)
