"""Stability selection on the device (R/stability_analysis.r:302-338): resnmtf_relevance bitwise against the literal
restatement of relevance_results applied to resnmtf_finalise's clusters, its refusals, and apply_resnmtf /
stability_check end to end -- including the reference's own test "resnmtf runs with stability and no spurious
removal" (tests/testthat/test-resnmtf.R:85-97)."""
import ctypes as C

import numpy as np
import pytest

import resnmtf_amd
from resnmtf_amd import api, naming
from resnmtf_amd.engine import Engine
from stability_ref import relevance_counts, relevance_sets

pytestmark = pytest.mark.gpu


def _factors(rng, n, m, k, power=3.0):
    f = rng.random((n, k)) ** power + 1e-3
    g = rng.random((m, k)) ** power + 1e-3
    s = rng.random((k, k)) + np.eye(k)
    return f, s, g


def _ref_engine(rng, N, M, k, p=0.35, empty=()):
    rc = (rng.random((N, k)) < p).astype(np.float64)
    cc = (rng.random((M, k)) < p).astype(np.float64)
    for j in empty:
        rc[:, j] = 0.0
    ref = Engine([N], [M], [2])
    ref.set_reference_clusters(0, rc, cc)
    return ref, rc, cc


def _restated(eng, v, rc_ref, cc_ref, rows, cols):
    _, _, _, rc, cc = eng.finalise(v)
    want = relevance_counts(rc, cc, rc_ref[rows], cc_ref[cols])
    return rc, cc, want


@pytest.mark.parametrize("k,n,m,N,M", [(1, 40, 30, 50, 40), (3, 150, 90, 170, 100), (3, 64, 65, 64, 65),
                                       (16, 700, 300, 800, 333), (64, 1000, 200, 1111, 222), (64, 129, 70, 129, 70)])
def test_relevance_bitwise_equals_restatement(k, n, m, N, M):
    rng = np.random.default_rng(1000 * k + n)
    ref, rc_ref, cc_ref = _ref_engine(rng, N, M, k, empty=(k - 1,) if k > 2 else ())
    eng = Engine([n], [m], [k])
    try:
        for trial in range(3):
            f, s, g = _factors(rng, n, m, k)
            if k > 2:
                f[:, 1] = 1.0                             # a uniform F column thresholds to an empty cluster
            eng.set_factors(0, f, s, g)
            rows = rng.choice(N, n, replace=trial > 0)
            cols = rng.choice(M, m, replace=False)
            got = eng.relevance(0, ref, 0, rows, cols)
            rc, cc, want = _restated(eng, 0, rc_ref, cc_ref, rows, cols)
            assert got.tobytes() == want.tobytes(), (got, want)
            if k <= 3 and n * m <= 4000:
                assert np.array_equal(want, relevance_sets(rc, cc, rc_ref[rows], cc_ref[cols]))
    finally:
        eng.close(); ref.close()


def test_relevance_after_a_run_and_finalise_unchanged():
    """On a handle that has run its loop: bitwise the restatement, and relevance leaves finalise's output as it was."""
    rng = np.random.default_rng(11)
    rc0 = np.kron(np.eye(3), np.ones((40, 1))); cc0 = np.kron(np.eye(3), np.ones((30, 1)))
    x = rc0 @ np.diag([10.0, 10.0, 10.0]) @ cc0.T + 0.1 * np.abs(rng.normal(size=(120, 90)))
    x = naming.check_data([x])[0]
    rows = np.sort(rng.choice(120, 108, replace=False)); cols = np.sort(rng.choice(90, 81, replace=False))
    ref, rc_ref, cc_ref = _ref_engine(rng, 120, 90, 3)
    ref.set_reference_clusters(0, rc0, cc0)
    eng = Engine([108], [81], [3])
    try:
        eng.set_view(0, x[np.ix_(rows, cols)])
        eng.init_svd(0, seed=5)
        eng.set_restrictions()
        eng.run(40)
        alone = eng.finalise(0)
        got = eng.relevance(0, ref, 0, rows, cols)
        after = eng.finalise(0)
        for a, b in zip(alone, after):
            assert a.tobytes() == b.tobytes()
        want = relevance_counts(alone[3], alone[4], rc0[rows], cc0[cols])
        assert got.tobytes() == want.tobytes()
        assert (got > 0.9).all()                          # the planted blocks are recovered
        eng.run(5)                                        # the loop resumes from the same state
        assert np.isfinite(eng.finalise(0)[0]).all()
    finally:
        eng.close(); ref.close()


def test_crafted_empty_sides_and_self_reference():
    rng = np.random.default_rng(3)
    n, m, k = 96, 80, 4
    eng = Engine([n], [m], [k])
    try:
        f, s, g = _factors(rng, n, m, k)
        eng.set_factors(0, np.ones((n, k)), s, g)         # every row cluster empty: m_0 = 0
        rows, cols = np.arange(n), np.arange(m)
        ref, rc_ref, cc_ref = _ref_engine(rng, n, m, k)
        assert np.array_equal(eng.relevance(0, ref, 0, rows, cols), np.zeros(k))       # n_0 != 0 -> 0
        ref.set_reference_clusters(0, np.zeros((n, k)), cc_ref)
        assert np.array_equal(eng.relevance(0, ref, 0, rows, cols), np.ones(k))        # both empty -> 1
        eng.set_factors(0, f, s, g)
        assert np.array_equal(eng.relevance(0, ref, 0, rows, cols), np.zeros(k))       # m_0 != 0, n_0 = 0 -> 0
        # reference = the sub-sample itself (same handle, identity draws): 1 for a non-empty bicluster
        f[:, 2] = 1.0
        eng.set_factors(0, f, s, g)
        _, _, _, rc, cc = eng.finalise(0)
        eng.set_reference_clusters(0, rc, cc)
        got = eng.relevance(0, eng, 0, rows, cols)
        want = relevance_counts(rc, cc, rc, cc)
        assert got.tobytes() == want.tobytes()
        nonempty = (rc.sum(0) > 0) & (cc.sum(0) > 0)
        assert not nonempty.all() and np.array_equal(got, np.where(nonempty, 1.0, 0.0))
        ref.close()
    finally:
        eng.close()


def test_refusals_return_their_codes():
    from resnmtf_amd import _lib
    lib = _lib.load()
    dp = C.POINTER(C.c_double); ip = C.POINTER(C.c_int)
    rng = np.random.default_rng(0)
    n, m, k, N, M = 20, 15, 3, 30, 25
    eng = Engine([n], [m], [k]); ref = Engine([N], [M], [2]); bare = Engine([n], [m], [k])
    try:
        f, s, g = _factors(rng, n, m, k)
        eng.set_factors(0, f, s, g)
        before = eng.finalise(0)
        rows = np.ascontiguousarray(rng.choice(N, n), dtype=np.int32)
        cols = np.ascontiguousarray(rng.choice(M, m), dtype=np.int32)
        out = np.zeros(k)
        rc = np.asfortranarray((rng.random((N, k)) < 0.5).astype(np.float64))
        cc = np.asfortranarray((rng.random((M, k)) < 0.5).astype(np.float64))

        def rel(h=eng._h, v=0, r=ref._h, vr=0, ro=rows, co=cols, o=out):
            return lib.resnmtf_relevance(h, v, r, vr, None if ro is None else ro.ctypes.data_as(ip),
                                         None if co is None else co.ctypes.data_as(ip), None if o is None else o.ctypes.data_as(dp))

        def setref(h=ref._h, v=0, kk=k, a=rc, b=cc):
            return lib.resnmtf_set_reference_clusters(h, v, kk, None if a is None else a.ctypes.data_as(dp),
                                                      None if b is None else b.ctypes.data_as(dp))

        assert rel() == 5                                 # no reference clusters set: RESNMTF_ERR_STATE
        assert setref(a=None) == 1 and setref(b=None) == 1
        assert setref(kk=0) == 1 and setref(kk=65) == 1 and setref(v=1) == 1
        half = rc.copy(order="F"); half[3, 1] = 0.5
        assert setref(a=half) == 1
        neg = cc.copy(order="F"); neg[0, 0] = -1.0
        assert setref(b=neg) == 1
        assert rel() == 5                                 # still nothing set after the refused calls
        assert setref() == 0
        assert rel(ro=None) == 1 and rel(co=None) == 1 and rel(o=None) == 1
        assert rel(r=None) == 1 and rel(vr=1) == 1 and rel(v=1) == 1
        assert rel(h=bare._h) == 5                        # the view has no factors
        bad = rows.copy(); bad[-1] = N
        assert rel(ro=bad) == 1
        bad[-1] = -1
        assert rel(ro=bad) == 1
        badc = cols.copy(); badc[0] = M
        assert rel(co=badc) == 1
        rc4 = np.asfortranarray(np.zeros((N, 4))); cc4 = np.asfortranarray(np.zeros((M, 4)))
        assert setref(kk=4, a=rc4, b=cc4) == 0
        assert rel() == 1                                 # reference k 4 != the view's k 3
        assert b"k" in lib.resnmtf_last_error(eng._h)
        if resnmtf_amd.device_count() > 1:                # handles on different devices
            other = Engine([N], [M], [2], device_id=1)
            try:
                assert lib.resnmtf_set_reference_clusters(other._h, 0, k, rc.ctypes.data_as(dp), cc.ctypes.data_as(dp)) == 0
                assert rel(r=other._h) == 1
            finally:
                other.close()
        assert setref() == 0
        assert rel() == 0
        after = eng.finalise(0)
        for a, b in zip(before, after):
            assert a.tobytes() == b.tobytes()
    finally:
        eng.close(); ref.close(); bare.close()


def planted(seed):
    """test-resnmtf.R:38-52: three 60 x 60 blocks of height 10 + 0.1 |N(0, 1)|."""
    rng = np.random.default_rng(seed)
    rc = np.kron(np.eye(3), np.ones((60, 1))); cc = np.kron(np.eye(3), np.ones((60, 1)))
    x = rc @ np.diag([10.0, 10.0, 10.0]) @ cc.T + 0.1 * np.abs(rng.normal(size=(180, 180)))
    return x, rc, cc


def test_reference_test_stability_without_spurious_removal():
    """test-resnmtf.R:85-97 ("resnmtf runs with stability and no spurious removal")."""
    x1, rc, cc = planted(1)
    x2, _, _ = planted(2)
    res = resnmtf_amd.apply_resnmtf([x1, x2], k_val=3, spurious=False, seed=7)
    assert len(res["output_f"]) == 2                                                   # :90
    assert res["output_f"][0].shape[0] == 180 and res["output_f"][0].shape[1] == 3       # :91-92
    for v in (1, 0):                                                                     # :93-96
        assert sorted(res["row_clusters"][v].sum(0)) == sorted(rc.sum(0))
        assert sorted(res["col_clusters"][v].sum(0)) == sorted(cc.sum(0))


def _two_view_problem():
    """Views of different extents (row draws independent, column draws shared) with partially shared row names."""
    rng = np.random.default_rng(21)
    n1, n2, m, k = 160, 120, 100, 4
    rc1 = np.zeros((n1, k)); rc2 = np.zeros((n2, k)); cc = np.zeros((m, k))
    for j in range(k):
        rc1[j * 40:(j + 1) * 40, j] = 1; rc2[j * 30:(j + 1) * 30, j] = 1; cc[j * 25:(j + 1) * 25, j] = 1
    heights = np.array([6.0, 4.0, 1.5, 0.8])
    x1 = rc1 @ np.diag(heights) @ cc.T + 0.6 * np.abs(rng.normal(size=(n1, m)))
    x2 = rc2 @ np.diag(heights) @ cc.T + 0.6 * np.abs(rng.normal(size=(n2, m)))
    rn = [[f"g{i}" for i in range(n1)], [f"g{i}" for i in range(80)] + [f"h{i}" for i in range(n2 - 80)]]
    cn = [[f"s{j}" for j in range(m)], [f"t{j}" for j in range(m)]]
    phi = np.zeros((2, 2)); phi[0, 1] = 0.5
    return [x1, x2], rn, cn, phi, k


def test_two_views_relevance_threshold_and_determinism():
    data, rn, cn, phi, k = _two_view_problem()
    res = resnmtf_amd.apply_resnmtf(data, k_val=k, phi=phi, spurious=False, stability=False, n_iters=60,
                                    row_names=rn, col_names=cn, seed=4)
    pre = naming.check_data(data)
    phi_m = naming.init_rest_mats(phi, 2); zero = np.zeros((2, 2))
    kw = dict(row_names=rn, col_names=cn, seed=9, n_stability=4, sample_rate=0.8)
    out = api.stability_check(pre, res, k, phi_m, zero, zero, 60, False, 5, False, "euclidean",
                              remove_unstable=False, return_repeats=True, **kw)
    rel = out["relevance"]
    assert out["res"] is res and rel.shape == (2, k)
    total = np.zeros((2, k))
    reps = out["stability"]["repeats"]
    assert len(reps) == 4
    for rep in reps:
        rows, cols = rep["extras"]["row_samples"], rep["extras"]["col_samples"]
        assert len(cols[0]) == len(cols[1]) and np.array_equal(cols[0], cols[1])      # equal extents share the draw
        assert len(rows[0]) != len(rows[1])                                              # different extents draw their own
        one = np.stack([relevance_counts(rep["row_clusters"][v], rep["col_clusters"][v],
                                         res["row_clusters"][v][rows[v]], res["col_clusters"][v][cols[v]])
                        for v in range(2)])
        assert one.tobytes() == np.asarray(rep["relevance"]).tobytes()
        total = total + one
    assert (total / 4).tobytes() == rel.tobytes()
    again = api.stability_check(pre, res, k, phi_m, zero, zero, 60, False, 5, False, "euclidean",
                                remove_unstable=False, **kw)
    assert again["relevance"].tobytes() == rel.tobytes()                                 # same seed, same bits
    vals = np.unique(rel)
    thr = float((vals[0] + vals[1]) / 2) if len(vals) > 1 else float(vals[0]) + 1e-9
    kept = api.stability_check(pre, res, k, phi_m, zero, zero, 60, False, 5, False, "euclidean",
                               stab_thres=thr, **kw)
    for v in range(2):
        drop = rel[v] < thr
        for key in ("row_clusters", "col_clusters"):
            assert np.array_equal(kept[key][v][:, drop], np.zeros_like(kept[key][v][:, drop]))
            assert np.array_equal(kept[key][v][:, ~drop], res[key][v][:, ~drop])
        assert kept["output_f"][v] is res["output_f"][v]
    assert any((rel[v] < thr).any() for v in range(2))
