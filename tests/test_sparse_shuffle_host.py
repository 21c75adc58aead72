"""Sparse shuffles without a device: the NumPy restatement of the Feistel permutation and its inverse (shuffle_ref), the
shuffle of a sparse matrix from its stored entries against the dense formula, the opt-in ``shuffle_sparse`` plumbed
through problem / spurious / batched / api with stub engines, and the two new C symbols."""
import ctypes as C
import inspect
import os
import re
import warnings

import numpy as np
import pytest
import scipy.sparse as sp

import resnmtf_amd
from resnmtf_amd import _lib, api, batched, problem, spurious
from resnmtf_amd.engine import Engine

import shuffle_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTS = (1, 2, 37 * 23, 4096, 4097)


@pytest.mark.parametrize("count", COUNTS)
def test_restated_permutation_is_a_bijection_and_the_inverse_inverts_it(count):
    for seed in (0, 5, (7 + 7919 * 3) * 1000003 + 1):
        idx = np.arange(count)
        pi = shuffle_ref.feistel_perm(idx, count, seed)
        assert pi.dtype == np.uint64 and np.array_equal(np.sort(pi), idx.astype(np.uint64))
        assert np.array_equal(shuffle_ref.feistel_perm_inverse(pi, count, seed), idx.astype(np.uint64))
        assert np.array_equal(shuffle_ref.feistel_perm(shuffle_ref.feistel_perm_inverse(idx, count, seed), count, seed),
                              idx.astype(np.uint64))


def test_no_cycle_walking_at_an_even_power_of_two():
    assert shuffle_ref.half_bits(4096) == 6 and shuffle_ref.half_bits(4097) == 7 and shuffle_ref.half_bits(1) == 1


def test_shuffle_csc_equals_the_dense_formula_entry_for_entry():
    x = sp.random(37, 23, density=0.5, random_state=3, format="csc")
    x.data[4] = 0.0                                                     # a stored explicit zero travels with the rest
    x32 = x.toarray().astype(np.float32).astype(np.float64)
    for seed in (0, 11, 1000003 * 9):
        got = shuffle_ref.shuffle_csc(x, seed)
        assert got.nnz == x.nnz and got.has_sorted_indices
        assert np.array_equal(got.toarray(), shuffle_ref.shuffle_dense(x32, seed))
        assert np.array_equal(np.sort(got.data), np.sort(x.data.astype(np.float32).astype(np.float64)))
    assert not np.array_equal(shuffle_ref.shuffle_csc(x, 1).indices, shuffle_ref.shuffle_csc(x, 2).indices)
    empty = shuffle_ref.shuffle_csc(sp.csc_matrix((50, 30)), 4)
    assert empty.nnz == 0 and np.array_equal(empty.indptr, np.zeros(31))


# ---------------------------------------------------------------------------------------------- plumbing, stub engines
class StubEngine:
    """What problem.load_child / shuffled_engines touch of an Engine."""
    made = []

    def __init__(self, n_rows, n_cols, k, device_id=0, nnz=None, stored=None):
        self.n_rows, self.n_cols, self.k, self.n_views = list(n_rows), list(n_cols), list(k), len(n_rows)
        self.sparse = [x is not None for x in (nnz or [None] * self.n_views)]
        self.nnz_cap = list(nnz or [None] * self.n_views)
        self.stored = list(stored) if stored is not None else [c or 0 for c in self.nnz_cap]
        self.calls = []
        StubEngine.made.append(self)

    def view_storage(self, v):
        return self.sparse[v], self.stored[v], self.nnz_cap[v] if self.sparse[v] else -1

    def shuffle_view_from(self, v, other, v_src=0, seed=0, normalise=True):
        if self.sparse[v] or other.sparse[v_src]:
            raise _lib.ResnmtfError(1, "copy / shuffle of a sparse view is not supported (it would densify it)")
        self.calls.append(("dense", v, seed))

    def shuffle_view_sparse_from(self, v, other, v_src=0, seed=0, normalise=True):
        assert self.sparse[v] and other.sparse[v_src] and normalise
        self.calls.append(("sparse", v, seed))

    def empty_lines(self, v):
        return np.zeros(self.n_rows[v], bool), np.zeros(self.n_cols[v], bool)

    def init_svd(self, v, seed=0):
        self.calls.append(("init", v, seed))

    def set_restrictions(self, *a):
        pass

    def run(self, **kw):
        return np.zeros(1)

    def close(self):
        pass


def _mixed_source():
    return StubEngine([20, 20], [12, 12], [3, 3], nnz=[90, None], stored=[80, 0])


def test_opt_in_reaches_the_sparse_entry_for_sparse_views_and_the_dense_one_for_dense(monkeypatch):
    monkeypatch.setattr(problem, "Engine", StubEngine)
    src = _mixed_source()
    StubEngine.made = []
    engs = problem.shuffled_engines(src, 3, 2, seed=4, shuffle_sparse=True)
    assert len(engs) == 2 and StubEngine.made == engs
    for r, eng in enumerate(engs):
        assert eng.nnz_cap == [80, None]                       # capacity = the source's stored entries (view_storage)
        s = 4 * 7919 + r + 1
        assert [c for c in eng.calls if c[0] != "init"] == [("sparse", 0, shuffle_ref.draw_seed(s, 0, 0)),
                                                            ("dense", 1, shuffle_ref.draw_seed(s, 0, 1))]
        assert [c for c in eng.calls if c[0] == "init"] == [("init", 0, 4 + 1000 + r), ("init", 1, 4 + 1000 + r + 1)]


def test_without_the_opt_in_the_old_refusals_fire(monkeypatch):
    monkeypatch.setattr(problem, "Engine", StubEngine)
    with pytest.raises(_lib.ResnmtfError, match="shuffle of a sparse view is not supported"):
        problem.shuffled_engines(_mixed_source(), 3, 2, seed=4)                  # dense engines, the library's refusal
    x = sp.random(20, 12, density=0.6, random_state=0, format="csc")
    msg = "device shuffles of sparse views are not supported"
    with pytest.raises(NotImplementedError, match=msg):
        spurious.check_biclusters([x], [np.ones((20, 3))], 2)
    with pytest.raises(NotImplementedError, match=msg):
        resnmtf_amd.res_nmtf_inner([x], None, None, k_vec=[3], spurious=True, spurious_on_device=True)
    with pytest.raises(NotImplementedError, match=msg):
        resnmtf_amd.apply_resnmtf([x], spurious=True, spurious_on_device=True, stability=False, k_sweep=True,
                                  bisil_sparse=True)
    res = {"row_clusters": [np.ones((20, 3))], "col_clusters": [np.ones((12, 3))]}
    with pytest.raises(NotImplementedError, match=msg):
        api.stability_check([x], res, 3, None, None, None, None, True, 5, False, "euclidean", spurious_on_device=True)


def test_the_grouped_path_stays_refused_for_sparse_views():
    x = sp.random(20, 12, density=0.6, random_state=0, format="csc")
    with pytest.raises(NotImplementedError, match="grouped path takes dense views only"):
        spurious.check_biclusters([x], [np.ones((20, 3)) / 20], 2, grouped=True, shuffle_sparse=True)


def test_check_biclusters_takes_sparse_views_with_the_opt_in():
    """Through the stand-in hooks (no device): a sparse view is accepted for its shape, the scores come out."""
    rng = np.random.default_rng(0)
    x = sp.random(20, 12, density=0.6, random_state=0, format="csr")
    f = rng.random((20, 3))
    shuffled = [[rng.random((20, 3))] for _ in range(3)]
    jsd = lambda cols, pairs: np.abs(cols[:, pairs[:, 0]] - cols[:, pairs[:, 1]]).mean(0)   # noqa: E731
    got = spurious.check_biclusters([x], [f], 3, shuffled_f=shuffled, jsd=jsd, shuffle_sparse=True)
    want = spurious.check_biclusters([x.toarray()], [f], 3, shuffled_f=shuffled, jsd=jsd)
    assert got["score"].tobytes() == want["score"].tobytes() and got["max_threshold"] == want["max_threshold"]


def test_a_view_no_draw_can_fill_is_refused_before_the_first_draw():
    src = StubEngine([20], [12], [3], nnz=[30], stored=[19])            # 19 < max(20, 12)
    eng = StubEngine([20], [12], [3], nnz=[19])
    with pytest.raises(ValueError, match="would not terminate"):
        problem._draw_shuffle(eng, 0, src, 5, True)
    assert eng.calls == []
    src.stored = [20]
    problem._draw_shuffle(eng, 0, src, 5, True)
    assert eng.calls == [("sparse", 0, shuffle_ref.draw_seed(5, 0, 0))]


def test_exhausted_draws_raise_the_dense_path_error():
    class Never(StubEngine):
        def empty_lines(self, v):
            return np.ones(self.n_rows[v], bool), np.zeros(self.n_cols[v], bool)
    src = StubEngine([20], [12], [3], nnz=[30], stored=[30])
    eng = Never([20], [12], [3], nnz=[30])
    with pytest.raises(RuntimeError, match="shuffle_view: every draw left an all-zero row or column"):
        problem._draw_shuffle(eng, 0, src, 5, True)
    assert [c[2] for c in eng.calls] == [shuffle_ref.draw_seed(5, a, 0) for a in range(64)]


@pytest.mark.parametrize("fn", [api.res_nmtf_inner, api.stability_check, api.apply_resnmtf, api.check_biclusters,
                                spurious.check_biclusters, spurious.check_on_device, batched.DeviceData.child,
                                batched.DeviceData.factorise, batched.DeviceData.stability_repeat,
                                batched.shuffles_on_device, problem.shuffled_engines])
def test_the_keyword_is_keyword_only_and_off_by_default(fn):
    fn = getattr(fn, "__wrapped__", fn)
    p = inspect.signature(fn).parameters["shuffle_sparse"]
    assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is False


def test_remove_spurious_forwards_the_keyword(monkeypatch):
    seen = {}
    monkeypatch.setattr(spurious, "check_biclusters", lambda data, f, R, **kw: seen.update(kw) or
                        {"score": np.ones((1, 3)), "avg_threshold": np.zeros(1), "max_threshold": np.zeros(1)})
    res = {"output_f": [np.ones((4, 3))], "output_s": [np.eye(3)], "row_clusters": [np.ones((4, 3))],
           "col_clusters": [np.ones((5, 3))]}
    api.remove_spurious([np.ones((4, 5))], res, 2, shuffle_sparse=True, seed=3)
    assert seen == {"grouped": False, "shuffle_sparse": True, "seed": 3}


# ---------------------------------------------------------------------------------------------- the C-ABI
def test_new_symbols_are_declared_exported_and_bound():
    with open(os.path.join(ROOT, "include", "resnmtf_hip.h")) as f:
        header = f.read()
    lib = _lib.load()
    for name in ("resnmtf_shuffle_view_sparse", "resnmtf_get_view_csc"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", header)
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1] and getattr(lib, name).restype is C.c_int
    assert _lib.SIGNATURES["resnmtf_shuffle_view_sparse"] == _lib.SIGNATURES["resnmtf_shuffle_view"]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert lib.resnmtf_shuffle_view_sparse(None, 0, None, 0, 1, 1) == 1          # RESNMTF_ERR_INVALID
        assert lib.resnmtf_get_view_csc(None, 0, None, None, None) == 1
    assert callable(Engine.shuffle_view_sparse_from) and callable(Engine.get_view_sparse)
