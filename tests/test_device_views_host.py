"""Dense views in device memory (``resnmtf_set_view_device`` / ``resnmtf_finalise_device``): what can
be checked without a GPU -- the two entries are declared, bound and exported, the dtype codes agree, the host layer
refuses bad tensors before it touches a device, and a CPU tensor is handled as its NumPy array."""
import ctypes as C
import os
import re
import warnings

import numpy as np
import pytest

from resnmtf_amd import _lib, api, device_views
from resnmtf_amd.engine import Engine
from resnmtf_amd.problem import prepare

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("resnmtf_set_view_device", "resnmtf_finalise_device")


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
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert lib.resnmtf_set_view_device(None, 0, None, 0, 1, 1, 0, None, None) == 1       # RESNMTF_ERR_INVALID
        assert lib.resnmtf_finalise_device(None, 0, None, None, None, None, None, None) == 1
    assert callable(Engine.set_view_device) and callable(Engine.finalise_device)


def test_dtype_codes_match_the_header():
    m = re.search(r"enum\s*\{([^}]*RESNMTF_DTYPE_F64[^}]*)\}", _header())
    assert m, "the dtype enum is not declared"
    codes = {name: int(val) for name, val in re.findall(r"RESNMTF_(DTYPE_[A-Z0-9]+)\s*=\s*(\d+)", m.group(1))}
    assert codes == {"DTYPE_F64": _lib.DTYPE_F64, "DTYPE_F32": _lib.DTYPE_F32, "DTYPE_F16": _lib.DTYPE_F16,
                     "DTYPE_BF16": _lib.DTYPE_BF16}
    assert len(set(codes.values())) == 4


def test_one_tensor_is_one_view():
    t = torch.rand(6, 4)
    views = api._as_list(t)
    assert len(views) == 1 and views[0] is t
    assert len(api._as_list([t, np.ones((6, 3))])) == 2


@pytest.mark.parametrize("bad, text", [(torch.ones(6, 4, dtype=torch.int32), "floating"),
                                       (torch.ones(2, 6, 4), "2-D"), (torch.ones(6), "2-D")])
def test_bad_tensors_are_refused_without_a_device(bad, text):
    if bad.ndim != 2:
        with pytest.raises(ValueError, match=text):
            api._as_list(bad)
    for call in (lambda: api._views([bad]),
                 lambda: prepare([bad], None, None, None, None, None, normalise=True, symmetrise=True),
                 lambda: api.res_nmtf_inner([bad], None, None, k_vec=[2], n_iters=1, spurious=False),
                 lambda: api.apply_resnmtf([bad], k_val=2, n_iters=1, spurious=False, stability=False)):
        with pytest.raises(ValueError, match=text):
            call()


def test_output_is_numpy_or_torch():
    for call in (lambda: api.res_nmtf_inner([np.ones((4, 3))], None, None, k_vec=[2], n_iters=1, spurious=False, output="cupy"),
                 lambda: api.apply_resnmtf([np.ones((4, 3))], k_val=2, n_iters=1, spurious=False, output="cupy")):
        with pytest.raises(ValueError, match="output"):
            call()


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32, torch.float16, torch.bfloat16])
def test_cpu_tensor_is_prepared_as_its_array(dtype):
    g = torch.Generator().manual_seed(3)
    ts = [(torch.rand(9, 5, generator=g) - 0.25).to(dtype), torch.rand(9, 7, generator=g).to(dtype).T.contiguous().T]
    arrays = [t.double().numpy() for t in ts]
    phi = np.array([[0.0, 1.5], [0.0, 0.0]])
    for normalise in (True, False):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            a = prepare(list(ts), phi, None, None, None, None, normalise=normalise, symmetrise=True)
            b = prepare(list(arrays), phi, None, None, None, None, normalise=normalise, symmetrise=True)
        assert a.row_names == b.row_names and a.col_names == b.col_names
        assert a.row_shared == b.row_shared and a.col_shared == b.col_shared
        for x, y in zip(a.data, b.data):
            assert isinstance(x, np.ndarray) and x.dtype == np.float64 and np.array_equal(x, y)
        for x, y in zip((a.phi, a.xi, a.psi), (b.phi, b.xi, b.psi)):
            assert np.array_equal(x, y)
    assert all(isinstance(v, np.ndarray) and np.array_equal(v, w) for v, w in zip(api._views(list(ts)), arrays))


def test_torch_stays_a_lazy_import_of_the_engine():
    """engine.py needs torch only inside the two device entry points."""
    with open(os.path.join(ROOT, "resnmtf_amd", "engine.py")) as f:
        text = f.read()
    top_level = [line for line in text.splitlines() if re.match(r"(import|from)\s+torch\b", line)]
    assert not top_level
    with open(os.path.join(ROOT, "resnmtf_amd", "device_views.py")) as f:
        assert not re.search(r"^\s*(import|from)\s+torch\b", f.read(), re.M)
    assert not device_views.is_tensor(np.ones((2, 2)))
