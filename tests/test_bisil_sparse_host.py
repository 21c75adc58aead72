"""The bisilhouette of sparse views without a device: bisil.score(sparse_views=True) routes each view to the engine
method its storage needs, the opt-in bisil_sparse leaves spurious removal on sparse views refused, and the new C
symbol is in the header and in the binding."""
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

import resnmtf_amd
from resnmtf_amd import _lib, bisil

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class StubEngine:
    """What bisil.score reads of an Engine: ``sparse`` and the two silhouette methods (constant silhouettes)."""

    def __init__(self, sparse):
        self.sparse = list(sparse)
        self.calls = []

    def _sil(self, name, value, v, rc, cc, distance):
        self.calls.append((name, v, distance))
        return np.where(rc != 0, value, 0.0), np.where(cc != 0, value, 0.0)

    def bisil(self, v, rc, cc, distance="euclidean"):
        return self._sil("bisil", 0.25, v, rc, cc, distance)

    def bisil_sparse(self, v, rc, cc, distance="euclidean"):
        return self._sil("bisil_sparse", 0.75, v, rc, cc, distance)


RC = np.array([[1, 0], [1, 0], [0, 1], [0, 1]], dtype=np.float64)
CC = np.array([[1, 0], [0, 1], [0, 1]], dtype=np.float64)


def test_score_routes_each_view_by_its_storage():
    eng = StubEngine([True, False, True])
    got = bisil.score([RC] * 3, [CC] * 3, "manhattan", engine=eng, sparse_views=True)
    assert eng.calls == [("bisil_sparse", 0, "manhattan"), ("bisil", 1, "manhattan"), ("bisil_sparse", 2, "manhattan")]
    assert got == pytest.approx((0.75 + 0.25 + 0.75) / 3)          # constant silhouettes: a view scores its constant


def test_score_default_keeps_every_view_on_bisil():
    eng = StubEngine([True, False])
    bisil.score([RC] * 2, [CC] * 2, engine=eng)
    assert [c[0] for c in eng.calls] == ["bisil", "bisil"]
    eng = StubEngine([False, False])
    bisil.score([RC] * 2, [CC] * 2, engine=eng, sparse_views=True)   # no effect on dense views
    assert [c[0] for c in eng.calls] == ["bisil", "bisil"]


def _sparse_view():
    return sp.random(20, 12, density=0.5, random_state=0, format="csc")


def test_spurious_on_sparse_views_stays_refused_with_the_opt_in():
    msg = "device shuffles of sparse views are not supported"
    with pytest.raises(NotImplementedError, match=msg):
        resnmtf_amd.res_nmtf_inner([_sparse_view()], None, None, k_vec=[3], spurious=True, spurious_on_device=True,
                                   score_bisil=True, bisil_sparse=True)
    with pytest.raises(NotImplementedError, match=msg):
        resnmtf_amd.apply_resnmtf([_sparse_view()], spurious=True, spurious_on_device=True, stability=False,
                                  k_sweep=True, bisil_sparse=True)
    # without spurious_on_device: the entry points' own refusals, as before
    with pytest.raises(NotImplementedError, match="outside the accelerated path"):
        resnmtf_amd.res_nmtf_inner([_sparse_view()], None, None, k_vec=[3], spurious=True, score_bisil=True,
                                   bisil_sparse=True)
    with pytest.raises(NotImplementedError, match="outside the accelerated"):
        resnmtf_amd.apply_resnmtf([_sparse_view()], spurious=True, stability=False, k_sweep=True, bisil_sparse=True)


def test_without_the_opt_in_sparse_views_stay_refused():
    with pytest.raises(NotImplementedError, match=r"not supported \(dense views only\)"):
        resnmtf_amd.res_nmtf_inner([_sparse_view()], None, None, k_vec=[3], spurious=False, score_bisil=True)
    with pytest.raises(NotImplementedError, match="not supported for sparse views"):
        resnmtf_amd.apply_resnmtf([_sparse_view()], spurious=False, stability=False, k_sweep=True)


def test_symbol_in_header_and_binding():
    with open(os.path.join(ROOT, "include", "resnmtf_hip.h")) as f:
        header = f.read()
    assert re.search(r"\bint\s+resnmtf_bisil_sparse\s*\(", header)
    assert "resnmtf_bisil_sparse" in _lib.SIGNATURES
    assert _lib.SIGNATURES["resnmtf_bisil_sparse"] == _lib.SIGNATURES["resnmtf_bisil"]
