"""Views out to device memory and reference clusters in from it: what can be checked without a
GPU -- the three entries are declared, bound and exported; the stride rule of ``Engine.get_view_device`` is a pure
function; ``stability_check`` hands cluster matrices that live on the engine's device to
``set_reference_clusters_device`` without turning them into NumPy, and everything else to ``set_reference_clusters`` as
before; ``DeviceData.factorise`` adds ``"device_data"`` and keeps its refusal, word for word, for ``output="numpy"``."""
import contextlib
import ctypes as C
import os
import re
import warnings

import numpy as np
import pytest
import scipy.sparse as sp

from resnmtf_amd import _lib, api, batched, device_views
from resnmtf_amd.engine import Engine
from stability_ref import fake_relevance, fake_results, fake_runner

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("resnmtf_get_view_device", "resnmtf_get_view_sparse_device", "resnmtf_set_reference_clusters_device")


def test_entries_declared_bound_and_exported():
    with open(os.path.join(ROOT, "include", "resnmtf_hip.h")) as f:
        header = f.read()
    lib = _lib.load()
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header)
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1] and getattr(lib, name).restype is C.c_int
    assert re.search(r"#define\s+RESNMTF_ABI_VERSION\s+2\b", header) and lib.resnmtf_abi_version() == 2      # additions only
    dm = C.POINTER(_lib.DeviceMatrix)
    assert _lib.SIGNATURES[NEW[0]][1] == [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_longlong, C.c_longlong, C.c_void_p]
    assert _lib.SIGNATURES[NEW[1]][1] == [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
    assert _lib.SIGNATURES[NEW[2]][1] == [C.c_void_p, C.c_int, C.c_int, dm, dm, C.c_void_p]
    for method in ("get_view_device", "get_view_sparse_device", "set_reference_clusters_device"):
        assert callable(getattr(Engine, method))


def test_a_null_handle_is_invalid():
    lib = _lib.load()
    one = _lib.DeviceMatrix(None, _lib.DTYPE_F64, 1, 1)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert lib.resnmtf_get_view_device(None, 0, None, _lib.DTYPE_F32, 1, 1, None) == 1       # RESNMTF_ERR_INVALID
        assert lib.resnmtf_get_view_sparse_device(None, 0, _lib.SPARSE_CSC, None, None, _lib.INDEX_I64, None, _lib.DTYPE_F32, None) == 1
        assert lib.resnmtf_set_reference_clusters_device(None, 0, 3, C.byref(one), C.byref(one), None) == 1


# ---------------------------------------------------------------------------------------------------------- the stride rule
def _strides(t):
    return tuple(t.shape), tuple(t.stride())


@pytest.mark.parametrize("make", [
    lambda: torch.empty((33, 65)),                                  # contiguous, row-major
    lambda: torch.empty((65, 33)).T,                                # transposed: column-major
    lambda: torch.empty((70, 200))[1::2, 2::3][:33, :65],           # sliced: two non-unit strides
    lambda: torch.empty((200, 70))[2::3, 1::2][:65, :33].T,         # ... and its transpose
    lambda: torch.empty((40, 65))[3:36],                            # a block of rows
    lambda: torch.empty((33, 70))[:, 2:67],                         # a block of columns
], ids=["contiguous", "transposed", "sliced", "sliced_transposed", "rows", "columns"])
def test_the_stride_rule_accepts_slices_and_transposes(make):
    t = make()
    assert tuple(t.shape) == (33, 65)
    device_views.check_readback_strides(*_strides(t))


@pytest.mark.parametrize("shape, strides", [((1, 70), (0, 1)), ((1, 70), (-5, 1)), ((1, 70), (1, 1)), ((1, 70), (7, 3)),
                                             ((70, 1), (1, 0)), ((70, 1), (1, 1)), ((70, 1), (2, -9)), ((1, 1), (0, 0)),
                                             ((1, 1), (-1, -1))])
def test_the_stride_of_an_extent_1_axis_is_not_read(shape, strides):
    device_views.check_readback_strides(shape, strides)


@pytest.mark.parametrize("shape, strides, text", [
    ((33, 65), (1, 2), "share an address"),          # overlapping: a (e - 1) = 32 >= 2
    ((33, 65), (1, 32), "share an address"),         # one short of a column: 32 >= 32
    ((33, 65), (64, 1), "share an address"),         # one short of a row: 64 >= 64
    ((33, 65), (5, 5), "share an address"),          # equal strides
    ((33, 65), (65, 0), "positive"),                 # expand()ed along the columns
    ((33, 65), (0, 1), "positive"),                  # ... along the rows
    ((33, 65), (0, 0), "positive"),
    ((33, 65), (-65, 1), "positive"),                # negative
    ((33, 65), (65, -1), "positive"),
    ((1, 70), (70, 0), "positive"),                  # an extent-1 axis does not excuse the other one
    ((70, 1), (-1, 1), "positive"),
])
def test_the_stride_rule_refuses_overlap_zero_and_negative_strides(shape, strides, text):
    with pytest.raises(ValueError, match=text):
        device_views.check_readback_strides(shape, strides)
    if strides in ((1, 32), (64, 1)):                 # the boundary: one element more of stride and the layout is fine
        rs, cs = strides
        device_views.check_readback_strides(shape, (rs, cs + 1) if rs <= cs else (rs + 1, cs))


def test_an_expanded_tensor_is_refused_by_its_strides():
    t = torch.zeros((33, 1)).expand(33, 65)
    with pytest.raises(ValueError, match="positive"):
        device_views.check_readback_strides(*_strides(t))
    with pytest.raises(ValueError, match="share an address"):
        device_views.check_readback_strides(*_strides(torch.as_strided(torch.zeros(200), (33, 65), (1, 2))))


# ------------------------------------------------------------------------------------- the routing of stability_check
class _BaseEngine:
    def __init__(self):
        self.host_calls, self.device_calls = [], []

    def set_reference_clusters(self, v, rc, cc):
        assert isinstance(rc, np.ndarray) and isinstance(cc, np.ndarray)
        self.host_calls.append((v, rc, cc))

    def set_reference_clusters_device(self, v, rc, cc):
        self.device_calls.append((v, rc, cc))


class _DeviceData:
    made = []

    def __init__(self, data, *args, device_id=0, pre_processed=False):
        self.data_shapes = [tuple(d.shape) for d in data]
        self.device_id = device_id
        self.base = _BaseEngine()
        self.closed = False
        _DeviceData.made.append(self)

    def stability_repeat(self, k, n_iters, seed, samples, tag="", **kw):
        return fake_runner(len(self.data_shapes), k)(int(tag.split("=")[1]))

    def close(self):
        self.closed = True


@pytest.fixture
def stand_ins(monkeypatch):
    """A stand-in ``DeviceData``; CPU tensors stand in for tensors on the engine's device, and ``to_numpy`` of one is an
    error."""
    _DeviceData.made = []
    monkeypatch.setattr(batched, "DeviceData", _DeviceData)
    monkeypatch.setattr(device_views, "on_engine_device", lambda x, device_id=0: isinstance(x, torch.Tensor))
    monkeypatch.setattr(device_views, "is_device_tensor", lambda x: isinstance(x, torch.Tensor))
    real = device_views.to_numpy

    def to_numpy(x):
        assert not isinstance(x, torch.Tensor), "a cluster matrix on the device was turned into NumPy"
        return real(x)
    monkeypatch.setattr(device_views, "to_numpy", to_numpy)
    return _DeviceData


def _stability(results, data, **kw):
    args = dict(n_stability=5, stab_thres=0.5, remove_unstable=True)
    args.update(kw)
    return api.stability_check(data, results, 4, None, None, None, 20, False, 5, False, "euclidean", **args)


def _as_tensors(results):
    """The clusters as fp64 column-major tensors, as ``finalise_device`` leaves them."""
    return dict(results, row_clusters=[torch.from_numpy(np.asfortranarray(a).T.copy()).T for a in results["row_clusters"]],
                col_clusters=[torch.from_numpy(np.asfortranarray(a).T.copy()).T for a in results["col_clusters"]])


def test_device_clusters_go_to_the_device_entry_and_never_to_numpy(stand_ins):
    results, data = fake_results()
    rel = sum(fake_relevance(r) for r in range(5)) / 5
    thr = float(np.median(rel))
    want = _stability(results, data, stab_thres=thr)                       # the route of today
    dev = stand_ins.made[-1]
    assert [c[0] for c in dev.base.host_calls] == [0, 1] and not dev.base.device_calls and dev.closed
    for (v, rc, cc) in dev.base.host_calls:
        assert np.array_equal(rc, results["row_clusters"][v]) and np.array_equal(cc, results["col_clusters"][v])
    on_device = _as_tensors(results)
    got = _stability(on_device, data, stab_thres=thr, output="torch")
    dev = stand_ins.made[-1]
    assert not dev.base.host_calls and [c[0] for c in dev.base.device_calls] == [0, 1] and dev.closed
    for (v, rc, cc) in dev.base.device_calls:                                # the caller's own tensors, read in place
        assert rc is on_device["row_clusters"][v] and cc is on_device["col_clusters"][v]
    assert list(got) == list(want) and got["output_f"] is on_device["output_f"]
    for key in ("row_clusters", "col_clusters"):
        for v, (t, a) in enumerate(zip(got[key], want[key])):
            assert isinstance(t, torch.Tensor) and t is not on_device[key][v] and t.dtype == torch.float64
            assert t.stride() == on_device[key][v].stride()
            assert t.numpy().tobytes() == np.ascontiguousarray(a).tobytes()
            assert np.array_equal(on_device[key][v].numpy(), results[key][v])      # the caller's tensors are not written
    assert any((rel[v] < thr).any() for v in range(2))
    plain = _stability(on_device, data, remove_unstable=False, output="torch")
    assert plain["res"] is on_device and plain["relevance"].tobytes() == rel.tobytes()


def test_a_view_with_one_host_matrix_takes_the_host_route(monkeypatch):
    _DeviceData.made = []
    monkeypatch.setattr(batched, "DeviceData", _DeviceData)
    monkeypatch.setattr(device_views, "on_engine_device", lambda x, device_id=0: isinstance(x, torch.Tensor))
    results, data = fake_results()
    mixed = _as_tensors(results)
    mixed["col_clusters"][1] = results["col_clusters"][1]                     # view 1: a tensor and an array
    out = _stability(mixed, data, remove_unstable=False)
    dev = _DeviceData.made[-1]
    assert [c[0] for c in dev.base.device_calls] == [0] and [c[0] for c in dev.base.host_calls] == [1]
    assert np.array_equal(dev.base.host_calls[0][1], results["row_clusters"][1])
    assert out["relevance"].tobytes() == (sum(fake_relevance(r) for r in range(5)) / 5).tobytes()


def test_number_biclusters_sums_device_tensors_on_the_device(stand_ins):
    results, _ = fake_results()
    want = float(sum(a.sum() for a in results["row_clusters"]))
    assert api._number_biclusters(results) == want
    assert api._number_biclusters(_as_tensors(results)) == want                # (to_numpy of a tensor raises here)
    halves = dict(results, row_clusters=[torch.from_numpy(a).to(torch.bfloat16) for a in results["row_clusters"]])
    assert api._number_biclusters(halves) == want                             # summed in fp64, whatever the dtype
    assert api._number_biclusters({}) == 0.0


# ----------------------------------------------------------------------------------------- the routing of factorise
class _ChildEngine:
    def __init__(self, shapes):
        self.shapes, self.calls = shapes, []

    def get_view(self, v):
        self.calls.append(("get_view", v))
        return np.full(self.shapes[v], float(v))

    def get_view_sparse(self, v):
        self.calls.append(("get_view_sparse", v))
        return sp.csc_matrix(np.full(self.shapes[v], float(v)))

    def get_view_device(self, v):
        self.calls.append(("get_view_device", v))
        return ("dense on the device", v)

    def get_view_sparse_device(self, v):
        self.calls.append(("get_view_sparse_device", v))
        return ("sparse_csc on the device", v)

    def run(self, n_iters=None, tol=0.0, max_iters=0):
        return np.array([1.0, 0.5])

    def finalise(self, v):
        n, m = self.shapes[v]
        return np.zeros((n, 2)), np.zeros((2, 2)), np.zeros((m, 2)), np.ones((n, 2)), np.ones((m, 2))

    def finalise_device(self, v):
        return ("finalise_device", v)


def _device_data(sparse_host_copy=True):
    """A ``DeviceData`` of one dense and one sparse view whose ``child`` yields a stand-in engine."""
    shapes = [(6, 5), (7, 4)]
    dev = object.__new__(batched.DeviceData)
    dev.sp = [None, sp.csc_matrix(np.ones(shapes[1]))]
    dev.data_shapes, dev.device_id = shapes, 0
    dev.entered = []

    @contextlib.contextmanager
    def child(k, seed=0, shuffle_seed=None, samples=None, **kw):
        eng = _ChildEngine(shapes)
        dev.entered.append(eng)
        host_views = [None, None if shuffle_seed is not None or not sparse_host_copy else dev.sp[1]]
        yield batched.Child(eng, [["r"] * s[0] for s in shapes], [["c"] * s[1] for s in shapes], samples, host_views)
    dev.child = child
    return dev


def test_factorise_adds_device_data_only_for_torch_output():
    dev = _device_data()
    res = dev.factorise(2, 5, return_data=True, output="torch")
    eng = dev.entered[-1]
    assert res["device_data"] == [("dense on the device", 0), ("sparse_csc on the device", 1)]
    assert isinstance(res["data"][0], np.ndarray) and isinstance(res["data"][1], np.ndarray)      # "data" is what it was
    assert list(res).index("device_data") == list(res).index("data") + 1
    assert res["device_out"] == [("finalise_device", 0), ("finalise_device", 1)]
    assert ("get_view_device", 0) in eng.calls and ("get_view_sparse_device", 1) in eng.calls
    host = dev.factorise(2, 5, return_data=True)
    assert "device_data" not in host and "device_out" not in host
    assert not any(name.endswith("_device") for name, _ in dev.entered[-1].calls)
    assert all(np.array_equal(a, b) for a, b in zip(host["data"], res["data"]))
    assert "device_data" not in dev.factorise(2, 5, output="torch") and "data" not in dev.factorise(2, 5, output="torch")


def test_a_shuffled_sparse_view_is_returned_on_the_device_and_refused_on_the_host():
    dev = _device_data()
    res = dev.factorise(2, 5, shuffle_seed=3, shuffle_sparse=True, return_data=True, output="torch")
    eng = dev.entered[-1]
    assert res["data"][1] is None and isinstance(res["data"][0], np.ndarray)
    assert res["device_data"] == [("dense on the device", 0), ("sparse_csc on the device", 1)]
    assert ("get_view_sparse", 1) not in eng.calls                           # nothing of the shuffle came to the host
    entered = len(dev.entered)
    for kw in (dict(output="numpy"), dict()):
        with pytest.raises(NotImplementedError) as info:
            dev.factorise(2, 5, shuffle_seed=3, shuffle_sparse=True, return_data=True, **kw)
        assert str(info.value) == "return_data of a shuffled sparse view is not supported (it would densify the shuffle)"
    assert len(dev.entered) == entered                                        # refused before any engine
