"""Sparse views from device memory without a device: the C entry is declared, bound and exported, the
host layer tells sparse tensors from dense ones without importing torch, CPU sparse tensors take the host route as
``scipy.sparse`` matrices, the refusals that need no device, and the routing of a sparse-tensor marker through
``DeviceData`` with stand-in engines."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp

from resnmtf_amd import _lib, api, batched, device_views, problem, sparse
from resnmtf_amd.engine import Engine
from test_sparse_subsample_host import StubEngine, _names

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "resnmtf_set_view_sparse_device"


def _dense(n=6, m=5, seed=0):
    rng = np.random.default_rng(seed)
    x = np.round(rng.random((n, m)) * 16) / 16 * (rng.random((n, m)) < 0.5)
    x[0, :] = 0.5                                        # no all-zero column
    return x


def _layouts(x, dtype=torch.float64):
    t = torch.tensor(x, dtype=dtype)
    return {"coo": t.to_sparse_coo().coalesce(), "csr": t.to_sparse_csr(), "csc": t.to_sparse_csc()}


def test_entry_is_declared_bound_and_exported():
    with open(os.path.join(ROOT, "include", "resnmtf_hip.h")) as f:
        header = f.read()
    decl = re.search(r"\bint\s+" + NAME + r"\s*\(([^)]*)\)", header)
    assert decl and len(decl.group(1).split(",")) == 11
    assert re.search(r"#define\s+RESNMTF_ABI_VERSION\s+2\b", header) and _lib.ABI_VERSION == 2      # additions only
    res, args = _lib.SIGNATURES[NAME]
    assert res is C.c_int and len(args) == 11
    for name, value in (("SPARSE_CSC", 0), ("SPARSE_CSR", 1), ("SPARSE_COO", 2), ("INDEX_I32", 0), ("INDEX_I64", 1)):
        assert getattr(_lib, name) == value
        assert re.search(r"\bRESNMTF_" + name + r"\s*=\s*" + str(value) + r"\b", header)
    lib = _lib.load()                                    # (AttributeError if the built library lacks the symbol)
    assert getattr(lib, NAME).argtypes == args
    assert lib.resnmtf_set_view_sparse_device(None, 0, 0, None, None, 0, None, 0, 0, 1, None) == 1       # RESNMTF_ERR_INVALID
    assert callable(Engine.set_view_sparse_device)


def test_is_sparse_tensor_on_every_layout():
    x = _dense(6, 4)
    for t in _layouts(x).values():
        assert device_views.is_sparse_tensor(t) and device_views.is_tensor(t)
        assert not device_views.is_sparse_device_view(t)           # (on the CPU: it takes the host route)
    t = torch.tensor(x)
    for blocked in (t.to_sparse_bsr((2, 2)), t.to_sparse_bsc((2, 2))):
        assert device_views.is_sparse_tensor(blocked)
    for other in (t, x, sp.csc_matrix(x), sp.coo_matrix(x), [x], None, device_views.RawDeviceView(t)):
        assert not device_views.is_sparse_tensor(other)
    assert sparse.is_sparse_view(sp.csr_matrix(x)) and not sparse.is_sparse_view(x) and not sparse.is_sparse_view(t)


def test_is_sparse_tensor_does_not_import_torch():
    code = ("import sys, numpy as np\n"
            "from resnmtf_amd import device_views, sparse\n"
            "assert not device_views.is_sparse_tensor(np.zeros((2, 2))) and not sparse.is_sparse_view(np.zeros((2, 2)))\n"
            "assert 'torch' not in sys.modules\n")
    subprocess.run([sys.executable, "-c", code], check=True, cwd=ROOT)


@pytest.mark.parametrize("index_dtype", [torch.int32, torch.int64])
def test_cpu_sparse_tensor_becomes_the_scipy_matrix_of_its_values(index_dtype):
    x = _dense(9, 7, 3)
    ref = sp.csc_matrix(torch.tensor(x, dtype=torch.bfloat16).double().numpy())
    for name, t in _layouts(x, torch.bfloat16).items():
        if name == "csr":
            t = torch.sparse_csr_tensor(t.crow_indices().to(index_dtype), t.col_indices().to(index_dtype), t.values(), t.shape)
        elif name == "csc":
            t = torch.sparse_csc_tensor(t.ccol_indices().to(index_dtype), t.row_indices().to(index_dtype), t.values(), t.shape)
        got = device_views.host_or_device(t, "view 0")
        assert sparse.is_sparse(got) and got.format == "csc" and got.dtype == np.float64, name
        assert got.shape == ref.shape and (got != ref).nnz == 0 and got.nnz == ref.nnz, name
        assert sparse.is_sparse(device_views.as_view(t, 0))                     # never taken for a dense view
        (view,) = api._views(t)
        assert sparse.is_sparse(view) and (view != ref).nnz == 0
        p = problem.prepare([t], None, None, None, None, None, normalise=True, symmetrise=True)
        assert sparse.is_sparse(p.data[0]) and np.allclose(np.asarray(p.data[0].sum(0)), 1.0)


def test_refusals_that_need_no_device():
    x = _dense(6, 4)
    t = torch.tensor(x)
    idx = torch.tensor([[0, 0, 1], [1, 1, 2]])
    bad = {"sparse_bsr": t.to_sparse_bsr((2, 2)),
           "hybrid": torch.sparse_coo_tensor(idx[:, :2], torch.ones(2, 3), (6, 4, 3)).coalesce(),
           "floating": torch.tensor(x * 16).to(torch.int32).to_sparse_csc(),
           "2-D": torch.zeros(2, 6, 4).to_sparse_coo().coalesce(),
           "coalesce": torch.sparse_coo_tensor(idx, torch.ones(3), (6, 4))}
    assert not bad["coalesce"].is_coalesced() and bad["hybrid"].dense_dim() == 1
    for words, tensor in bad.items():
        with pytest.raises(ValueError, match=words):
            device_views.check_sparse_tensor(tensor)
        with pytest.raises(ValueError, match=words):
            api.res_nmtf_inner([tensor], None, None, k_vec=[2], n_iters=2, spurious=False)
        with pytest.raises(ValueError, match=words):
            device_views.as_view(tensor, 0)
    with pytest.raises(ValueError, match="batched|2-D"):
        device_views.check_sparse_tensor(torch.zeros(2, 6, 4).to_sparse_csr())


class Marker(device_views.SparseDeviceView):
    """What DeviceData keeps of a sparse CUDA tensor, made without a device."""

    def __init__(self, shape, nnz, raw=False):
        self.tensor, self.shape, self.nnz, self.raw, self.ndim = None, tuple(shape), int(nnz), raw, 2


def _device_data(monkeypatch):
    """A DeviceData over stand-in engines: a sparse view from device memory, a scipy.sparse view and a dense one."""
    monkeypatch.setattr(batched, "Engine", StubEngine)
    x = sp.csc_matrix(sp.random(20, 12, density=0.6, random_state=0, format="csc") + sp.csc_matrix(np.full((20, 12), 1e-3)))
    dev = object.__new__(batched.DeviceData)
    dev.sp = [Marker((20, 12), 150), x, None]
    dev.data_shapes = [(20, 12)] * 3
    rn, cn = _names(20, 12)
    dev.rn, dev.cn = rn + [rn[0]], cn + [[f"c{j}" for j in range(12)]]
    dev.phi = dev.xi = dev.psi = np.zeros((3, 3))
    dev.device_id = 0
    dev.base = StubEngine([20] * 3, [12] * 3, [2] * 3, nnz=[150, x.nnz, None], stored=[150, x.nnz, 0])
    StubEngine.made = []
    return dev, x


def test_a_marker_takes_the_device_routes_and_a_scipy_view_keeps_the_host_route(monkeypatch):
    dev, x = _device_data(monkeypatch)
    assert dev._sp_device(0) and not dev._sp_device(1) and not dev._sp_device(2)
    samples = ([np.arange(2, 20)] * 3, [np.arange(1, 11)] * 3)
    sub = x[2:20][:, 1:11]
    with dev.child(3, seed=5, samples=samples, sparse_on_device=False) as ch:
        probe, dense_probe, eng = StubEngine.made          # the marker's probe on the device, none for the scipy view
        assert probe.nnz_cap == [7 * 18 + 10] and probe.calls == [("sub_sparse", 0, 0, 18, 10)]
        assert dense_probe.nnz_cap == [None] and dense_probe.calls == [("sub", 0, 2, 18, 10)]
        assert eng.nnz_cap == [7 * 18 + 10, sub.nnz, None]
        assert ch.host_views[0] is None and ch.host_views[1].nnz == sub.nnz and ch.host_views[2] is None
        assert [c for c in eng.calls if c[0] != "init"] == [("sub_sparse", 0, 0, 18, 10), ("upload", 1, sub.nnz, True),
                                                            ("sub", 2, 2, 18, 10), ("restrictions",)]
    assert [c for c in dev.base.calls if c[0] == "count"] == [("count", 0, 18, 10)]
    StubEngine.made = []
    with dev.child(4, seed=5) as ch:                        # copies
        (eng,) = StubEngine.made
        assert eng.nnz_cap == [150, x.nnz, None] and ch.host_views[0] is None and ch.host_views[1].nnz == x.nnz
        assert [c for c in eng.calls if c[0] != "init"] == [("copy_sparse", 0, 0), ("upload", 1, x.nnz, True), ("copy", 2, 2),
                                                            ("restrictions",)]
    StubEngine.made = []
    with dev.child(4, seed=5, sparse_on_device=True):       # the opt-in still moves the scipy view to the device routes
        (eng,) = StubEngine.made
        assert [c for c in eng.calls if c[0] != "init"] == [("copy_sparse", 0, 0), ("copy_sparse", 1, 1), ("copy", 2, 2),
                                                            ("restrictions",)]
    with pytest.raises(NotImplementedError, match="device shuffles of sparse views are not supported"):
        with dev.child(3, seed=5, shuffle_seed=1):
            pass


def test_scipy_views_alone_make_exactly_the_earlier_calls(monkeypatch):
    dev, x = _device_data(monkeypatch)
    dev.sp, dev.data_shapes = dev.sp[1:], dev.data_shapes[1:]
    dev.rn, dev.cn = _names(20, 12)
    dev.phi = dev.xi = dev.psi = np.zeros((2, 2))
    dev.base = StubEngine([20, 20], [12, 12], [2, 2], nnz=[x.nnz, None], stored=[x.nnz, 0])
    StubEngine.made = []
    seen = {}
    real = problem.load_child
    monkeypatch.setattr(batched, "load_child", lambda *a, **kw: (seen.update(kw), real(*a, **kw))[1])
    with dev.child(4, seed=5):
        (eng,) = StubEngine.made
        assert [c for c in eng.calls if c[0] != "init"] == [("upload", 0, x.nnz, True), ("copy", 1, 1), ("restrictions",)]
    assert "sparse_on_device" not in seen and dev.base.calls == []
    with dev.child(4, seed=5, sparse_on_device=True):
        pass
    assert seen["sparse_on_device"] is True


def test_prepare_leaves_a_marker_to_its_upload():
    m = Marker((20, 12), 150)
    p = problem.prepare([m, np.full((20, 5), 0.5)], None, None, None, None, None, normalise=True, symmetrise=True)
    assert isinstance(p.data[0], device_views.SparseDeviceView) and p.data[0].raw and p.data[0].nnz == 150 and not m.raw
    assert np.allclose(p.data[1].sum(0), 1.0)
    calls = []

    class Eng:
        def set_view_sparse_device(self, v, tensor, pre_processed=False):
            calls.append((v, pre_processed))

    device_views.upload_sparse(Eng(), 0, m, pre_processed=True)
    device_views.upload_sparse(Eng(), 1, p.data[0], pre_processed=True)      # raw: normalised whatever the caller says
    device_views.upload_sparse(Eng(), 2, m, pre_processed=False)
    assert calls == [(0, True), (1, False), (2, False)]
    assert sparse.is_sparse_view(m) and device_views.is_device_view(m) and not sparse.is_sparse(m)
