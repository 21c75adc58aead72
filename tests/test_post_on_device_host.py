"""The bisilhouette from device memory and the steps after the loop without downloads: what can be
checked without a GPU -- the entry is declared, bound and exported; ``bisil.score`` sends a view whose two cluster matrices
live on the engine's device to ``Engine.bisil_device`` and everything else where it went, and refuses a mix;
``spurious.apply_removal_device`` against ``spurious.apply_removal``; the argument check of ``post_on_device``; and the
summation order the device's combination follows, restated in NumPy scalars and pinned against ``bisil.view_score``."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import resnmtf_amd
from resnmtf_amd import _lib, api, batched, bisil, device_views, spurious
from resnmtf_amd.engine import Engine

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_declared_bound_and_exported():
    with open(os.path.join(ROOT, "include", "resnmtf_hip.h")) as f:
        header = f.read()
    lib = _lib.load()
    name = "resnmtf_bisil_device"
    assert re.search(r"\bint\s+" + name + r"\s*\(", header)
    assert name in _lib.SIGNATURES and hasattr(lib, name)
    dm = C.POINTER(_lib.DeviceMatrix)
    assert _lib.SIGNATURES[name][1] == [C.c_void_p, C.c_int, C.c_int, dm, dm, C.c_int, C.c_void_p, C.c_void_p,
                                        C.POINTER(C.c_double), C.c_void_p]
    assert re.search(r"#define\s+RESNMTF_ABI_VERSION\s+2\b", header) and lib.resnmtf_abi_version() == 2      # additions only
    assert callable(Engine.bisil_device)
    one = _lib.DeviceMatrix(None, _lib.DTYPE_F64, 1, 1)
    score = C.c_double(0.0)
    assert lib.resnmtf_bisil_device(None, 0, 3, C.byref(one), C.byref(one), 0, None, None, C.byref(score), None) == 1


# ---------------------------------------------------------------------------------------------------------- routing
class _Engine:
    """Records which entry scores which view; a tensor counts as living on its device (``on_device`` below)."""
    device_id = 0
    sparse = [False, True]

    def __init__(self):
        self.calls = []

    @staticmethod
    def _sil(rc, cc):
        return np.where(np.asarray(rc) != 0, 0.5, 0.0), np.where(np.asarray(cc) != 0, 0.25, 0.0)

    def bisil(self, v, rc, cc, distance):
        self.calls.append(("bisil", v))
        return self._sil(rc, cc)

    def bisil_sparse(self, v, rc, cc, distance):
        self.calls.append(("bisil_sparse", v))
        return self._sil(rc, cc)

    def bisil_device(self, v, rc, cc, distance="euclidean", *, silhouettes=True):
        assert isinstance(rc, torch.Tensor) and isinstance(cc, torch.Tensor) and not silhouettes
        self.calls.append(("bisil_device", v, distance))
        return None, None, 0.375


@pytest.fixture
def on_device(monkeypatch):
    monkeypatch.setattr(device_views, "on_engine_device", lambda x, device_id=0: isinstance(x, torch.Tensor))


def _clusters():
    rc = np.zeros((6, 2)); rc[:3, 0] = 1; rc[3:, 1] = 1
    cc = np.zeros((4, 2)); cc[:2, 0] = 1; cc[2:, 1] = 1
    return rc, cc


def test_score_routes_a_device_pair_to_the_device_entry(on_device):
    rc, cc = _clusters()
    eng = _Engine()
    got = bisil.score([torch.as_tensor(rc), rc], [torch.as_tensor(cc), cc], "cosine", engine=eng, sparse_views=True)
    assert eng.calls == [("bisil_device", 0, "cosine"), ("bisil_sparse", 1)]
    assert got == bisil.overall([0.375, bisil.view_score(rc, cc, *_Engine().bisil(1, rc, cc, "cosine"))])


def test_score_of_host_pairs_is_what_it_was(on_device):
    rc, cc = _clusters()
    eng = _Engine()
    assert bisil.score([rc, rc], [cc, cc], engine=eng) == 0.375
    assert eng.calls == [("bisil", 0), ("bisil", 1)]
    seen = []
    assert bisil.score([rc], [cc], sil=lambda v, a, b, d: (seen.append(v), _Engine().bisil(v, a, b, d))[1]) == 0.375
    assert seen == [0]


def test_score_refuses_a_mixed_pair(on_device):
    rc, cc = _clusters()
    eng = _Engine()
    with pytest.raises(ValueError, match=r"view 1: the cluster matrices mix a device tensor and a host matrix \(row_clusters on the "
                                         r"device, col_clusters on the host\)"):
        bisil.score([rc, torch.as_tensor(rc)], [cc, cc], engine=eng)
    assert device_views.cluster_route(rc, cc) is False                      # (pure: no device is asked)


def test_cluster_tensor_checks_need_no_device():
    rc, cc = _clusters()
    with pytest.raises(TypeError, match="rc is a ndarray"):
        device_views.check_cluster_tensors(rc, torch.as_tensor(cc), 6, 4)
    with pytest.raises(ValueError, match="lives on cpu"):
        device_views.check_cluster_tensors(torch.as_tensor(rc), torch.as_tensor(cc), 6, 4)
    with pytest.raises(ValueError, match="fp64, fp32, fp16 or bf16"):
        device_views.check_cluster_tensors(torch.as_tensor(rc).long(), torch.as_tensor(cc), 6, 4)


# ---------------------------------------------------------------------------------------------------------- the removal
def test_apply_removal_device_equals_apply_removal():
    rng = np.random.default_rng(5)
    K = 4
    res = {"output_s": [rng.random((K, K)), rng.random((K, K))],
           "row_clusters": [(rng.random((9, K)) < 0.5).astype(np.float64), (rng.random((7, K)) < 0.5).astype(np.float64)],
           "col_clusters": [(rng.random((5, K)) < 0.5).astype(np.float64), (rng.random((6, K)) < 0.5).astype(np.float64)]}
    check = {"score": np.array([[0.3, 0.0, 0.9, 0.1], [0.5, 0.6, 0.7, 0.8]]), "avg_threshold": np.array([0.2, 0.2]),
             "max_threshold": np.array([0.2, 0.4])}
    want = spurious.apply_removal(res, check)
    assert want["spurious"]["removed"].any() and not want["spurious"]["removed"].all()
    # column-major tensors, as finalise_device returns them
    as_t = lambda a: torch.as_tensor(np.ascontiguousarray(a.T)).T                                          # noqa: E731
    res_t = {key: [as_t(a) for a in vals] for key, vals in res.items()}
    before = {key: [t.clone() for t in vals] for key, vals in res_t.items()}
    got = spurious.apply_removal_device(res_t, check)
    assert list(got) == list(want)
    assert got["spurious"]["removed"].dtype == bool and got["spurious"]["removed"].tobytes() == want["spurious"]["removed"].tobytes()
    for key in ("score", "avg_threshold", "max_threshold"):
        assert got["spurious"][key].tobytes() == want["spurious"][key].tobytes()
    for key in ("row_clusters", "col_clusters"):
        for t, w, b, given in zip(got[key], want[key], before[key], res_t[key]):
            assert isinstance(t, torch.Tensor) and t.stride() == given.stride() and t.data_ptr() != given.data_ptr()
            assert np.array_equal(t.numpy(), w)
            assert torch.equal(given, b)                                    # the inputs are not written
    for t, b in zip(res_t["output_s"], before["output_s"]):
        assert torch.equal(t, b)


# ---------------------------------------------------------------------------------------------------------- the opt-in
def test_post_on_device_needs_torch_output():
    x = np.random.default_rng(0).random((12, 8))
    text = "post_on_device=True needs output='torch'"
    with pytest.raises(ValueError, match=text):
        api.res_nmtf_inner([x], None, None, k_vec=[2], spurious=False, post_on_device=True)
    with pytest.raises(ValueError, match=text):
        resnmtf_amd.apply_resnmtf([x], k_val=2, stability=False, spurious=False, post_on_device=True)
    with pytest.raises(ValueError, match=text):
        resnmtf_amd.apply_resnmtf([x], k_sweep=True, stability=False, spurious=False, post_on_device=True)
    dev = batched.DeviceData.__new__(batched.DeviceData)                    # (no engine: the check comes first)
    dev.data_shapes, dev.sp = [(12, 8)], [None]
    with pytest.raises(ValueError, match=text):
        dev.factorise(2, post_on_device=True)
    import inspect
    for fn in (api.res_nmtf_inner, api.apply_resnmtf, batched.DeviceData.factorise):
        p = inspect.signature(fn).parameters["post_on_device"]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is False


# ---------------------------------------------------------------------------------------------------------- the summation order
NP_BLOCK = 8192      # NumPy hands a long 1-D reduction to its inner loop in buffers of 8192 entries


def _pairwise(a):
    """``pairwise_sum`` of NumPy's add loop on Python floats: below 8 entries in order from 0.0; up to 128 eight strided
    accumulators that START as the first eight entries, combined as ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)),
    then the tail in order; above 128 split at n / 2 rounded down to a multiple of 8."""
    n = len(a)
    if n < 8:
        r = 0.0
        for x in a:
            r += x
        return r
    if n <= 128:
        r = list(a[:8])
        i = 8
        while i < n - (n % 8):
            for j in range(8):
                r[j] += a[i + j]
            i += 8
        res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
        for x in a[i:]:
            res += x
        return res
    n2 = n // 2
    n2 -= n2 % 8
    return _pairwise(a[:n2]) + _pairwise(a[n2:])


def np_sum(a):
    """``ndarray.sum()`` of a contiguous 1-D fp64 array: the first buffer of 8192 entries summed pairwise -- its first
    entry is part of the pairwise sum, not a separate start value --, every later buffer's pairwise sum added in order."""
    s = _pairwise(a[:NP_BLOCK])
    for i in range(NP_BLOCK, len(a), NP_BLOCK):
        s += _pairwise(a[i:i + NP_BLOCK])
    return s


def device_view_score(rc, cc, row_sil, col_sil):
    """The combination as bisil_member_mean_kernel and bisil_score_kernel form it (csrc/resnmtf_bisil.hip.inc), on Python
    floats: per active bicluster the members' silhouettes gathered in ascending index order, their mean = np_sum / count,
    sigma = 0.5 (row mean + column mean); then np_sum(sigma) / count, 0 with fewer than two active biclusters."""
    K = rc.shape[1]
    sigma = []
    for l in range(K):
        rows, cols = np.flatnonzero(rc[:, l]), np.flatnonzero(cc[:, l])
        if len(rows) == 0 or len(cols) == 0:
            continue
        mr = np_sum([float(row_sil[i, l]) for i in rows]) / float(len(rows))
        mc = np_sum([float(col_sil[i, l]) for i in cols]) / float(len(cols))
        sigma.append(0.5 * (mr + mc))
    return 0.0 if len(sigma) < 2 else np_sum(sigma) / float(len(sigma))


@pytest.mark.parametrize("count", [1, 7, 8, 9, 127, 128, 129, 1000, 5000, 8191, 8192, 8193, 20000])
def test_the_restated_summation_order_is_numpys(count):
    rng = np.random.default_rng(count)
    a = rng.standard_normal(count) * 10.0 ** rng.integers(-3, 3, count)
    assert np_sum([float(x) for x in a]) / float(count) == a.mean()
    col = np.asfortranarray(rng.standard_normal((count + 5, 2)))[:, 1]      # a strided column, gathered by a mask
    mask = np.ones(count + 5, dtype=bool); mask[:5] = False
    assert np_sum([float(x) for x in col[mask]]) / float(count) == col[mask].mean()


@pytest.mark.parametrize("count", [1, 7, 8, 9, 127, 128, 129, 1000, 5000])
def test_the_device_combination_order_equals_view_score_bitwise(count):
    """Member counts on both sides of NumPy's summation edges: bicluster 0 has ``count`` rows and bicluster 1 ``count``
    columns; silhouettes of mixed sign and magnitude, so that another order would show."""
    rng = np.random.default_rng(100 + count)
    n, m, K = count + 40, count + 30, 4
    rc = np.zeros((n, K)); cc = np.zeros((m, K))
    rc[rng.choice(n, count, replace=False), 0] = 1; cc[rng.choice(m, 11, replace=False), 0] = 1
    rc[rng.choice(n, 13, replace=False), 1] = 1; cc[rng.choice(m, count, replace=False), 1] = 1
    rc[rng.choice(n, 9, replace=False), 2] = 1                               # rows without columns: inactive
    rc[rng.choice(n, 30, replace=False), 3] = 1; cc[rng.choice(m, 20, replace=False), 3] = 1
    row_sil = np.asfortranarray(rng.uniform(-1, 1, (n, K)) * 10.0 ** rng.integers(-4, 1, (n, K)) * rc)
    col_sil = np.asfortranarray(rng.uniform(-1, 1, (m, K)) * 10.0 ** rng.integers(-4, 1, (m, K)) * cc)
    want = bisil.view_score(rc, cc, row_sil, col_sil)
    assert want != 0.0
    assert device_view_score(rc, cc, row_sil, col_sil) == want


def test_the_device_combination_with_fewer_than_two_active_is_zero():
    rc = np.zeros((5, 3)); cc = np.zeros((4, 3))
    assert device_view_score(rc, cc, rc, cc) == 0.0 == bisil.view_score(rc, cc, rc, cc)
    rc[:2, 1] = 1; cc[1:, 1] = 1; rc[3, 2] = 1
    sil_r, sil_c = rc * 0.5, cc * 0.25
    assert device_view_score(rc, cc, sil_r, sil_c) == 0.0 == bisil.view_score(rc, cc, sil_r, sil_c)
