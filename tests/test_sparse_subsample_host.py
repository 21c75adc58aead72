"""Device copies and sub-samples of sparse views without a device: the three C symbols, their bindings, the host
restatement of a sub-sample (subsample_ref) and the opt-in ``sparse_on_device`` plumbed through problem / batched / api
with stub engines."""
import ctypes as C
import inspect
import os
import re
import warnings

import numpy as np
import pytest
import scipy.sparse as sp

from resnmtf_amd import _lib, api, batched, problem
from resnmtf_amd.engine import Engine

import subsample_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("resnmtf_subsample_count_sparse", "resnmtf_subsample_view_sparse", "resnmtf_copy_view_sparse")


# ---------------------------------------------------------------------------------------------- the C-ABI
def test_new_symbols_are_declared_exported_and_bound():
    with open(os.path.join(ROOT, "include", "resnmtf_hip.h")) as f:
        header = f.read()
    lib = _lib.load()
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header)
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1] and getattr(lib, name).restype is C.c_int
    assert _lib.SIGNATURES["resnmtf_subsample_view_sparse"] == _lib.SIGNATURES["resnmtf_subsample_view"]
    assert _lib.SIGNATURES["resnmtf_copy_view_sparse"] == _lib.SIGNATURES["resnmtf_copy_view"]
    assert re.search(r"#define\s+RESNMTF_ABI_VERSION\s+2\b", header) and _lib.ABI_VERSION == 2      # additions only
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        nnz = C.c_longlong(-1)
        assert lib.resnmtf_subsample_count_sparse(None, 0, 0, None, 0, None, C.byref(nnz)) == 1       # RESNMTF_ERR_INVALID
        assert lib.resnmtf_subsample_view_sparse(None, 0, None, 0, None, None) == 1
        assert lib.resnmtf_copy_view_sparse(None, 0, None, 0) == 1
    for name in ("subsample_count_sparse", "subsample_view_sparse_from", "copy_view_sparse_from"):
        assert callable(getattr(Engine, name))


def test_restated_subsample_equals_dense_indexing_and_keeps_stored_zeros():
    x = sp.random(37, 23, density=0.5, random_state=3, format="csc")
    x.data[4] = 0.0
    rng = np.random.default_rng(1)
    rows, cols = rng.permutation(37)[:30], rng.permutation(23)[:20]
    got = subsample_ref.subsample_csc(x, rows, cols)
    assert got.has_sorted_indices and np.array_equal(got.toarray(), x.toarray()[np.ix_(rows, cols)])
    stored = np.zeros(x.shape, bool); stored[x.indices, np.repeat(np.arange(23), np.diff(x.indptr))] = True
    assert got.nnz == stored[np.ix_(rows, cols)].sum()              # zeros that were stored stay stored
    with pytest.raises(AssertionError):
        subsample_ref.subsample_csc(x, [1, 1], [0])


# ---------------------------------------------------------------------------------------------- plumbing, stub engines
class StubEngine:
    """What problem.load_child, DeviceData.child and DeviceData._trim_samples touch of an Engine."""
    made = []

    def __init__(self, n_rows, n_cols, k, device_id=0, nnz=None, stored=None):
        self.n_rows, self.n_cols, self.k, self.n_views = list(n_rows), list(n_cols), list(k), len(n_rows)
        self.sparse = [x is not None for x in (nnz or [None] * self.n_views)]
        self.nnz_cap = list(nnz or [None] * self.n_views)
        self.stored = list(stored) if stored is not None else [c or 0 for c in self.nnz_cap]
        self.calls = []
        StubEngine.made.append(self)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        pass

    def view_storage(self, v):
        self.calls.append(("storage", v))
        return self.sparse[v], self.stored[v], self.nnz_cap[v] if self.sparse[v] else -1

    def subsample_count_sparse(self, v, rows, cols):
        self.calls.append(("count", v, len(rows), len(cols)))
        return 7 * len(rows) + len(cols)

    def set_view_sparse(self, v, m, pre_processed=False):
        self.calls.append(("upload", v, m.nnz, pre_processed))

    def copy_view_from(self, v, other, v_src=0):
        self.calls.append(("copy", v, v_src))

    def copy_view_sparse_from(self, v, other, v_src=0):
        assert self.sparse[v] and other.sparse[v_src]
        self.calls.append(("copy_sparse", v, v_src))

    def subsample_view_from(self, v, other, v_src, rows, cols):
        self.calls.append(("sub", v, v_src, len(rows), len(cols)))

    def subsample_view_sparse_from(self, v, other, v_src, rows, cols):
        assert self.sparse[v] and other.sparse[v_src]
        self.calls.append(("sub_sparse", v, v_src, len(rows), len(cols)))

    def empty_lines(self, v):
        return np.zeros(self.n_rows[v], bool), np.zeros(self.n_cols[v], bool)

    def init_svd(self, v, seed=0):
        self.calls.append(("init", v, seed))

    def set_restrictions(self, *a):
        self.calls.append(("restrictions",))

    def set_shared_rows(self, *a):
        pass

    def set_shared_cols(self, *a):
        pass


def _names(n, m):
    return [[f"r{i}" for i in range(n)]] * 2, [[f"a{j}" for j in range(m)], [f"b{j}" for j in range(m)]]


def _load(samples, host_views, **kw):
    src = StubEngine([20, 20], [12, 12], [2, 2], nnz=[90, None], stored=[80, 0])
    shape = (20, 12) if samples is None else (len(samples[0][0]), len(samples[1][0]))
    eng = StubEngine([shape[0]] * 2, [shape[1]] * 2, [3, 3], nnz=[80, None])
    rn, cn = _names(*shape)
    problem.load_child(eng, src, 5, samples=samples, host_views=host_views, coupling=(None, None, None, rn, cn), **kw)
    return eng.calls


def test_load_child_calls_the_sparse_entries_for_sparse_views_and_the_dense_ones_for_dense():
    x = sp.random(20, 12, density=0.4, random_state=0, format="csc")
    samples = ([np.arange(18)] * 2, [np.arange(10)] * 2)
    sub = x[:18][:, :10]
    # sub-samples
    assert _load(samples, [None, None], sparse_on_device=True) == [
        ("sub_sparse", 0, 0, 18, 10), ("init", 0, 5), ("sub", 1, 1, 18, 10), ("init", 1, 6), ("restrictions",)]
    # copies
    assert _load(None, [None, None], sparse_on_device=True) == [
        ("copy_sparse", 0, 0), ("init", 0, 5), ("copy", 1, 1), ("init", 1, 6), ("restrictions",)]
    # off: exactly the earlier calls -- the sparse view uploaded from the host copy
    today_sub = [("upload", 0, sub.nnz, True), ("init", 0, 5), ("sub", 1, 1, 18, 10), ("init", 1, 6), ("restrictions",)]
    today_copy = [("upload", 0, x.nnz, True), ("init", 0, 5), ("copy", 1, 1), ("init", 1, 6), ("restrictions",)]
    assert _load(samples, [sub, None]) == today_sub and _load(samples, [sub, None], sparse_on_device=False) == today_sub
    assert _load(None, [x, None]) == today_copy


def _device_data(monkeypatch):
    """A DeviceData over stub engines: one sparse 20 x 12 view and one dense one sharing rows."""
    monkeypatch.setattr(batched, "Engine", StubEngine)
    x = sp.random(20, 12, density=0.6, random_state=0, format="csc")
    x = x + sp.csc_matrix(np.full((20, 12), 1e-3))            # fully stored: no sub-sample has an empty line
    dev = object.__new__(batched.DeviceData)
    dev.sp = [sp.csc_matrix(x), None]
    dev.data_shapes = [(20, 12), (20, 12)]
    dev.rn, dev.cn = _names(20, 12)
    dev.phi = dev.xi = dev.psi = np.zeros((2, 2))
    dev.device_id = 0
    dev.base = StubEngine([20, 20], [12, 12], [2, 2], nnz=[x.nnz, None], stored=[x.nnz, 0])
    StubEngine.made = []
    return dev, x


def test_child_sizes_the_engine_from_the_count_and_keeps_no_host_copy(monkeypatch):
    dev, x = _device_data(monkeypatch)
    samples = ([np.arange(2, 20)] * 2, [np.arange(1, 11)] * 2)
    with dev.child(3, seed=5, samples=samples, sparse_on_device=True) as ch:
        probe, dense_probe, eng = StubEngine.made
        assert probe.nnz_cap == [7 * 18 + 10] and probe.calls == [("sub_sparse", 0, 0, 18, 10)]      # the trimming probe
        assert dense_probe.nnz_cap == [None] and dense_probe.calls == [("sub", 0, 1, 18, 10)]
        assert eng.nnz_cap == [7 * 18 + 10, None] and eng.n_rows == [18, 18] and eng.k == [3, 3]
        assert ch.host_views == [None, None] and ch.eng is eng
        assert [c for c in eng.calls if c[0] != "init"] == [("sub_sparse", 0, 0, 18, 10), ("sub", 1, 1, 18, 10), ("restrictions",)]
    assert [c for c in dev.base.calls if c[0] == "count"] == [("count", 0, 18, 10)]       # the child re-uses the probe's count
    dev.base.calls = []
    with dev.child(3, seed=5, samples=samples, sparse_on_device=True):
        pass
    assert [c for c in dev.base.calls if c[0] == "count"] == [("count", 0, 18, 10)]       # per child, never a stale one
    seen = {0: (samples[0][0], samples[1][0], 99)}
    assert dev._subsample_count(0, samples[0][0], samples[1][0], seen) == 99             # the probe's lists: its count
    assert dev._subsample_count(0, samples[0][0][:-1], samples[1][0], seen) == 7 * 17 + 10     # other lists: counted again
    StubEngine.made = []
    with dev.child(4, seed=5, sparse_on_device=True) as ch:           # a copy: sized from base.view_storage
        (eng,) = StubEngine.made
        assert eng.nnz_cap == [x.nnz, None] and ch.host_views == [None, None]
        assert [c for c in eng.calls if c[0] != "init"] == [("copy_sparse", 0, 0), ("copy", 1, 1), ("restrictions",)]


def test_without_the_opt_in_child_makes_the_earlier_calls(monkeypatch):
    dev, x = _device_data(monkeypatch)
    samples = ([np.arange(2, 20)] * 2, [np.arange(1, 11)] * 2)
    sub = x[2:20][:, 1:11]
    dev.base.calls = []
    with dev.child(3, seed=5, samples=samples) as ch:
        probe, eng = StubEngine.made                                  # (the dense view's probe only)
        assert probe.nnz_cap == [None] and probe.calls == [("sub", 0, 1, 18, 10)]
        assert eng.nnz_cap == [sub.nnz, None] and ch.host_views[0].nnz == sub.nnz and ch.host_views[1] is None
        assert [c for c in eng.calls if c[0] != "init"] == [("upload", 0, sub.nnz, True), ("sub", 1, 1, 18, 10), ("restrictions",)]
    assert dev.base.calls == []                                       # no count, no storage query
    StubEngine.made = []
    with dev.child(4, seed=5, shuffle_seed=None) as ch:
        (eng,) = StubEngine.made
        assert eng.nnz_cap == [x.nnz, None] and ch.host_views[0].nnz == x.nnz
        assert [c for c in eng.calls if c[0] != "init"] == [("upload", 0, x.nnz, True), ("copy", 1, 1), ("restrictions",)]


@pytest.mark.parametrize("fn", [api.res_nmtf_inner, api.stability_check, api.apply_resnmtf, batched.DeviceData.child,
                                batched.DeviceData._trim_samples, batched.DeviceData.factorise,
                                batched.DeviceData.stability_repeat, batched.k_sweep_on_device,
                                batched.stability_relevance_on_device, batched.stability_on_device, problem.load_child])
def test_the_keyword_is_keyword_only_and_off_by_default(fn):
    fn = getattr(fn, "__wrapped__", fn)
    p = inspect.signature(fn).parameters["sparse_on_device"]
    assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is False


def test_the_drivers_forward_the_keyword_only_when_it_is_set():
    seen = []

    class Dev:
        data_shapes = [(20, 12)]

        class base:
            set_reference_clusters = staticmethod(lambda *a: None)

        def factorise(self, k, *a, **kw):
            seen.append(("factorise", k, kw.get("sparse_on_device")))
            return {}

        def stability_repeat(self, k, *a, **kw):
            seen.append(("repeat", k, kw.get("sparse_on_device")))
            return {"stability_performed": True, "relevance": np.ones((1, k))}

    res = {"row_clusters": [np.ones((20, 3))], "col_clusters": [np.ones((12, 3))]}
    batched.k_sweep_on_device(Dev(), 3, 4, 5, sparse_on_device=True)
    batched.k_sweep_on_device(Dev(), 3, 3, 5)
    batched.stability_relevance_on_device(Dev(), res, 3, 1, sparse_on_device=True)
    batched.stability_relevance_on_device(Dev(), res, 3, 1)
    assert seen == [("factorise", 3, True), ("factorise", 4, True), ("factorise", 3, None), ("repeat", 3, True), ("repeat", 3, None)]
    seen.clear()
    batched.stability_on_device(Dev(), 3, 1, sparse_on_device=True)
    batched.stability_on_device(Dev(), 3, 1)
    assert seen == [("factorise", 3, True), ("factorise", 3, None)]
