"""Factors in device memory (``resnmtf_set_factors_device`` / ``resnmtf_get_factors_device``): what
can be checked without a GPU -- the two entries are declared, bound and exported, the host layer decides per view between
the device and the host route and refuses a mix, another device and a wrong ``init_lm`` before any engine exists, and a
CPU tensor is taken as its fp64 array."""
import ctypes as C
import inspect
import os
import re
import warnings

import numpy as np
import pytest

from resnmtf_amd import _lib, api, device_views, problem
from resnmtf_amd.engine import Engine

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("resnmtf_set_factors_device", "resnmtf_get_factors_device")


def _header() -> str:
    with open(os.path.join(ROOT, "include", "resnmtf_hip.h")) as f:
        return f.read()


def test_entries_declared_bound_and_exported():
    header = _header()
    lib = _lib.load()
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header)
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1] and getattr(lib, name).restype is C.c_int
    assert re.search(r"#define\s+RESNMTF_ABI_VERSION\s+2\b", header) and _lib.ABI_VERSION == 2      # additions only
    assert lib.resnmtf_abi_version() == 2
    dm = C.POINTER(_lib.DeviceMatrix)
    assert _lib.SIGNATURES[NEW[0]][1] == [C.c_void_p, C.c_int, dm, dm, dm, dm, dm, C.c_void_p]
    assert _lib.SIGNATURES[NEW[1]][1] == [C.c_void_p, C.c_int] + [C.c_void_p] * 6
    assert callable(Engine.set_factors_device) and callable(Engine.get_factors_device)


def test_the_matrix_struct_matches_the_header():
    m = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*resnmtf_device_matrix\s*;", _header())
    assert m, "resnmtf_device_matrix is not declared"
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    assert re.findall(r"\b(ptr|dtype|row_stride|col_stride)\b", body) == [name for name, _ in _lib.DeviceMatrix._fields_]
    assert [t for _, t in _lib.DeviceMatrix._fields_] == [C.c_void_p, C.c_int, C.c_longlong, C.c_longlong]


def test_a_null_handle_is_invalid():
    lib = _lib.load()
    one = _lib.DeviceMatrix(None, _lib.DTYPE_F64, 1, 1)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert lib.resnmtf_set_factors_device(None, 0, None, None, None, None, None, None) == 1       # RESNMTF_ERR_INVALID
        assert lib.resnmtf_set_factors_device(None, 0, C.byref(one), C.byref(one), C.byref(one), None, None, None) == 1
        assert lib.resnmtf_get_factors_device(None, 0, None, None, None, None, None, None) == 1


class _Stub:
    def __init__(self, on_device):
        self.on_device = on_device


def test_the_route_is_a_pure_decision():
    on = lambda x: x.on_device       # noqa: E731
    d, h = _Stub(True), _Stub(False)
    assert device_views.factor_route(d, d, d, on_device=on) is True
    assert device_views.factor_route(h, h, h, on_device=on) is False
    for mix in ((d, h, h), (h, d, h), (h, h, d), (d, d, h), (d, h, d), (h, d, d)):
        with pytest.raises(ValueError, match="view 4.*mix"):
            device_views.factor_route(*mix, what="view 4", on_device=on)
    # the default predicate: NumPy arrays and CPU tensors are host objects
    assert device_views.factor_route(np.ones((3, 2)), torch.ones(2, 2), np.ones((4, 2))) is False
    assert not device_views.is_device_tensor(torch.ones(2, 2)) and not device_views.is_device_tensor(np.ones(2))
    assert device_views.is_device_tensor(torch.empty(2, 2, device="meta"))


def _problem(seed=0):
    rng = np.random.default_rng(seed)
    shapes, k = [(12, 7), (12, 9)], 2
    data = [rng.random(s) + 0.1 for s in shapes]
    data = [x / x.sum(0, keepdims=True) for x in data]
    init = ([rng.random((n, k)) for n, _ in shapes], [rng.random((k, k)) for _ in shapes], [rng.random((m, k)) for _, m in shapes])
    return data, init, k


def _inner(data, init, k, **kw):
    return api.res_nmtf_inner(data, None, None, init[0], init[1], init[2], k_vec=[k] * len(data), n_iters=1, spurious=False, **kw)


@pytest.mark.parametrize("which", [0, 1, 2])
def test_a_mixed_view_is_refused_before_any_engine(which, monkeypatch):
    data, init, k = _problem()
    made = []
    monkeypatch.setattr(api, "Engine", lambda *a, **kw: made.append(1) or (_ for _ in ()).throw(AssertionError("an engine was created")))
    init[which][1] = torch.empty(init[which][1].shape, dtype=torch.float64, device="meta")      # a device-type tensor: never read
    with pytest.raises(ValueError, match="view 1.*mix"):
        _inner(data, init, k)
    with pytest.raises(ValueError, match="view 1.*mix"):
        api.apply_resnmtf(data, init[0], init[1], init[2], k_val=k, n_iters=1, spurious=False, stability=False)
    assert not made


def test_another_device_is_refused_before_any_engine(monkeypatch):
    data, init, k = _problem()
    made = []
    monkeypatch.setattr(api, "Engine", lambda *a, **kw: made.append(1) or (_ for _ in ()).throw(AssertionError("an engine was created")))
    for part in init:
        part[0] = torch.empty(part[0].shape, dtype=torch.float32, device="meta")
    with pytest.raises(ValueError, match="view 0: init_f lives on meta.*cuda:0"):
        _inner(data, init, k)
    assert not made


@pytest.mark.parametrize("bad", [([np.ones(2)], [np.ones(2)]), ([np.ones(2)] * 2,), ([np.ones(2)] * 2, [np.ones(2)] * 3), 5])
def test_init_lm_of_the_wrong_length_is_refused_before_any_engine(bad, monkeypatch):
    data, init, k = _problem()
    made = []
    monkeypatch.setattr(api, "Engine", lambda *a, **kw: made.append(1) or (_ for _ in ()).throw(AssertionError("an engine was created")))
    with pytest.raises(ValueError, match="init_lm.*one entry per view.*2 views"):
        _inner(data, init, k, init_lm=bad)
    with pytest.raises(ValueError, match="init_lm needs explicit initial factors"):
        api.res_nmtf_inner(data, None, None, k_vec=[k, k], n_iters=1, spurious=False, init_lm=([np.ones(k)] * 2, [np.ones(k)] * 2))
    assert not made


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32, torch.float16, torch.bfloat16])
def test_cpu_tensor_factors_are_taken_as_their_fp64_arrays(dtype):
    _, init, _ = _problem(3)
    ts = [[torch.as_tensor(a).to(dtype) for a in part] for part in init]
    ts[2][1] = ts[2][1].T.contiguous().T                   # (any strides)
    routes, f, s, g = device_views.factor_routes(*ts, device_id=0)
    assert routes == [False, False]
    for got, part in zip((f, s, g), ts):
        for a, t in zip(got, part):
            assert isinstance(a, np.ndarray) and a.dtype == np.float64 and np.array_equal(a, t.double().numpy())
    same = device_views.factor_routes(*init, device_id=0)
    assert same[0] == [False, False] and all(a is b for got, part in zip(same[1:], init) for a, b in zip(got, part))


def test_the_new_keywords_and_the_state_key():
    sig = inspect.signature(api.res_nmtf_inner)
    for name, default in (("init_lm", None), ("return_state", False)):
        assert sig.parameters[name].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters[name].default is default
    assert "state" in problem._INNER_KEYS
    state = [tuple(np.ones(1) for _ in range(5))]
    res = problem.inner_result([1], [2], [3], np.ones(2), 2, state=state)
    assert res["state"] is state and "state" not in problem.inner_result([1], [2], [3], np.ones(2), 2)


def test_torch_stays_a_lazy_import():
    for name in ("engine.py", "device_views.py", "api.py"):
        with open(os.path.join(ROOT, "resnmtf_amd", name)) as f:
            assert not re.search(r"^(import|from)\s+torch\b", f.read(), re.M), name
