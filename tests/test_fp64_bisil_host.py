"""Host side of the fp64 bisilhouette (api.res_nmtf_inner(precision="fp64", fp64_bisil=True), api.apply_resnmtf(precision=
"fp64"), engine.fp64_bisil; no GPU): the score is routed through ``bisil.score`` over a stand-in for
``engine.fp64_bisil`` on the views as the run received them, the flag does nothing under f32, the new refusals come before
any device work and carry their texts, ``apply_resnmtf`` validates ``precision`` and runs the fp64 sweep through
``sweep_runner``, and the built library exports the new symbols."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import helpers
from resnmtf_amd import _lib, api, bisil, build, engine, naming


def _never(*args, **kwargs):
    raise AssertionError("the device must not be reached")


def _inner_args(n_views=1, shape=(12, 9), k=2):
    rng = np.random.default_rng(1)
    data = naming.check_data([rng.random(shape) + 0.01 for _ in range(n_views)])
    rn, cn = naming.give_names(data)
    f, s, g, _, _ = api.svd_init(data, [k] * n_views, 0)
    z = np.zeros((n_views, n_views))
    return (data, naming.shared_names(rn), naming.shared_names(cn), f, s, g, [k] * n_views, z, z, z, 5)


def _echo(seen):
    """Stands in for engine.fp64_run: the initial factors come back as the result."""
    def runner(problem, tol, max_iters, device_id, **more):
        seen.update(problem=problem, more=more)
        n_v, k = len(problem["data"]), problem["k"]
        return {"f": problem["init_f"], "s": problem["init_s"], "g": problem["init_g"], "lambda": [np.ones(k)] * n_v,
                "mu": [np.ones(k)] * n_v, "all_error": np.array([0.3, 0.2]), "iters": 2}
    return runner


def _sil_log(calls):
    """Stands in for engine.fp64_bisil: silhouettes that depend on the view, so that the combination shows."""
    def sil(x, rc, cc, distance="euclidean", device_id=0):
        calls.append((x, np.array(rc), np.array(cc), distance, device_id))
        scale = 0.25 * len(calls)
        return scale * np.asarray(rc, dtype=np.float64), 2.0 * scale * np.asarray(cc, dtype=np.float64)
    return sil


def test_symbols_struct_and_export():
    assert "resnmtf_fp64_bisil" in _lib.SIGNATURES and "resnmtf_fp64_bisil_plan" in _lib.SIGNATURES
    names = [f[0] for f in _lib.Fp64BisilJob._fields_]
    assert names == ["struct_size", "n", "m", "k", "metric", "x", "x_dev", "stream", "row_clusters", "col_clusters",
                     "row_sil", "col_sil"]
    lib = C.CDLL(build.build(verbose=False))                              # the built library exports the new entries
    for name in ("resnmtf_fp64_bisil", "resnmtf_fp64_bisil_plan", "resnmtf_bisil"):
        assert hasattr(lib, name), name
    header = open(helpers.ROOT + "/include/resnmtf_hip.h").read()
    assert "int resnmtf_fp64_bisil(int device_id, const resnmtf_fp64_bisil_job* job);" in header
    assert "#define RESNMTF_ABI_VERSION 2 " in header                    # the ABI version does not move


def test_plan_query_needs_no_device():
    """The plan entry is host arithmetic: the kq table, the chunk rule (test_gpu_bisil_forms.py restates both) and the
    gather form from the strides."""
    assert engine.fp64_bisil_plan(2950, 2945, 3, 60, 1) == {"kq": 1, "chunk_tiles": 2, "chunks": 24, "gather": ("lds", "points")}
    assert engine.fp64_bisil_plan(5000, 4000, 17, 1, 5000) == {"kq": 8, "chunk_tiles": 3, "chunks": 27, "gather": ("points", "lds")}
    assert engine.fp64_bisil_plan(150, 20, 64, 0, 0)["gather"] == ("points", "points")       # a tie: along the points
    assert [engine.fp64_bisil_plan(64, 1, k)["kq"] for k in (4, 5, 8, 9, 16, 17, 32, 33, 64)] == [1, 2, 2, 4, 4, 8, 8, 16, 16]
    for bad in ((0, 1, 3, 1, 1), (10, 0, 3, 1, 1), (10, 5, 0, 1, 1), (10, 5, 65, 1, 1), (10, 5, 3, -1, 1)):
        with pytest.raises(_lib.ResnmtfError) as e:
            engine.fp64_bisil_plan(*bad)
        assert e.value.code == 1


def test_score_is_routed_through_fp64_bisil_on_the_views_as_received(monkeypatch):
    monkeypatch.setattr(api, "Engine", _never)
    seen, calls = {}, []
    monkeypatch.setattr(engine, "fp64_run", _echo(seen))
    monkeypatch.setattr(engine, "fp64_bisil", _sil_log(calls))
    args = _inner_args(2)
    res = api.res_nmtf_inner(*args, spurious=False, distance="manhattan", precision="fp64", score_bisil=True, fp64_bisil=True,
                             device_id=3)
    assert len(calls) == 2
    for v, (x, rc, cc, distance, device_id) in enumerate(calls):
        assert x is seen["problem"]["data"][v]                            # the view the run received, not a copy
        np.testing.assert_array_equal(x, args[0][v])
        np.testing.assert_array_equal(rc, res["row_clusters"][v])
        np.testing.assert_array_equal(cc, res["col_clusters"][v])
        assert distance == "manhattan" and device_id == 3
    want = bisil.overall([bisil.view_score(res["row_clusters"][v], res["col_clusters"][v],
                                           0.25 * (v + 1) * res["row_clusters"][v], 0.5 * (v + 1) * res["col_clusters"][v])
                          for v in range(2)])
    assert res["bisil"] == want and want != 0.0
    assert list(res) == ["output_f", "output_s", "output_g", "Error", "All_Error", "bisil", "row_clusters", "col_clusters",
                         "lambda", "mu"]


def test_sil_and_runner_hooks_of_the_inner_function():
    seen, calls = {}, []
    a = _inner_args(1)

    def sil(v, rc, cc, distance):
        calls.append((v, distance))
        return 0.5 * np.asarray(rc), 0.5 * np.asarray(cc)
    res = api._res_nmtf_inner_fp64(*a[:11], False, "cosine", False, row_names=None, col_names=None, device_id=0, max_iters=10,
                                   seed=None, engine_opts=None, host_init=False, return_init=False, score_bisil=True,
                                   spurious_on_device=False, output="numpy", init_lm=None, return_state=False,
                                   post_on_device=False, fp64_bisil=True, runner=_echo(seen), sil=sil)
    assert calls == [(0, "cosine")]
    assert res["bisil"] == bisil.score(res["row_clusters"], res["col_clusters"], "cosine", sil=sil)


def test_no_clusts_scores_nothing(monkeypatch):
    monkeypatch.setattr(api, "Engine", _never)
    monkeypatch.setattr(engine, "fp64_run", _echo({}))
    monkeypatch.setattr(engine, "fp64_bisil", _never)
    res = api.res_nmtf_inner(*_inner_args(), spurious=False, no_clusts=True, precision="fp64", score_bisil=True, fp64_bisil=True)
    assert "bisil" not in res or res["bisil"] is None


def test_flag_is_a_no_op_under_f32(monkeypatch):
    """precision="f32" with fp64_bisil=True makes the calls it makes without it and never reaches engine.fp64_bisil."""
    from test_fp64_host import _CallLog
    monkeypatch.setattr(api, "Engine", _CallLog)
    monkeypatch.setattr(engine, "fp64_run", _never)
    monkeypatch.setattr(engine, "fp64_bisil", _never)
    args = _inner_args(2)
    plain = api.res_nmtf_inner(*args, spurious=False)
    want = list(_CallLog.calls)
    flagged = api.res_nmtf_inner(*args, spurious=False, fp64_bisil=True)
    assert _CallLog.calls == want and list(plain) == list(flagged) and flagged["bisil"] is None


def test_without_the_flag_the_refusal_stands(monkeypatch):
    monkeypatch.setattr(api, "Engine", _never)
    monkeypatch.setattr(engine, "fp64_run", _never)
    monkeypatch.setattr(engine, "fp64_bisil", _never)
    with pytest.raises(NotImplementedError) as e:
        api.res_nmtf_inner(*_inner_args(), spurious=False, precision="fp64", score_bisil=True)
    assert str(e.value) == ('precision="fp64": score_bisil needs a live engine handle, which the fp64 path does not keep (it runs '
                            'through resnmtf_fp64_run); use precision="f32" for it')
    with pytest.raises(TypeError):                                       # keyword-only
        api.res_nmtf_inner(*_inner_args(), 5, False, "euclidean", False, True)


def test_sparse_view_with_score_bisil_is_refused_by_name(monkeypatch):
    monkeypatch.setattr(api, "Engine", _never)
    monkeypatch.setattr(engine, "fp64_run", _never)
    monkeypatch.setattr(engine, "fp64_bisil", _never)
    args = list(_inner_args(2))
    mixed = [[args[0][0], sp.csc_matrix(args[0][1])]] + args[1:]
    with pytest.raises(NotImplementedError, match=r"fp64_bisil=True scores dense views only; sparse views \(view 1\)"):
        api.res_nmtf_inner(*mixed, spurious=False, precision="fp64", fp64_sparse=True, score_bisil=True, fp64_bisil=True)
    with pytest.raises(NotImplementedError, match="sparse views"):       # without fp64_sparse: the earlier refusal, as before
        api.res_nmtf_inner(*mixed, spurious=False, precision="fp64", score_bisil=True, fp64_bisil=True)


def test_engine_fp64_bisil_refuses_before_the_library(monkeypatch):
    monkeypatch.setattr(_lib, "load", _never)
    x, rc, cc = np.ones((6, 4)), np.ones((6, 2)), np.ones((4, 2))
    with pytest.raises(ValueError, match="distance must be one of"):
        engine.fp64_bisil(x, rc, cc, "chebyshev")


def _raw_data(seed=0):
    rng = np.random.default_rng(seed)
    return [rng.random((30, 12)) + 0.01, rng.random((30, 10)) + 0.01]


def test_apply_resnmtf_precision_validation(monkeypatch):
    monkeypatch.setattr(api, "Engine", _never)
    monkeypatch.setattr(engine, "fp64_run", _never)
    data = _raw_data()
    with pytest.raises(ValueError, match="precision must be 'f32' or 'fp64'"):
        api.apply_resnmtf(data, k_val=3, precision="f64")
    with pytest.raises(TypeError):                                       # keyword-only
        api.apply_resnmtf(data, None, None, None, 3, None, None, None, 5, 3, 8, "euclidean", False, 5, False, 0.9, 5, False,
                          0.4, True, True, "fp64")
    with pytest.raises(NotImplementedError, match=r'precision="fp64"\): stability=True is not supported'):
        api.apply_resnmtf(data, k_val=3, spurious=False, precision="fp64")
    with pytest.raises(NotImplementedError, match=r'precision="fp64"\): spurious=True is not supported'):
        api.apply_resnmtf(data, k_val=3, stability=False, precision="fp64")
    with pytest.raises(NotImplementedError, match="pass k_val"):
        api.apply_resnmtf(data, stability=False, spurious=False, precision="fp64")
    with pytest.raises(NotImplementedError, match=r"a sparse view in the k sweep is not supported"):
        api.apply_resnmtf([sp.csc_matrix(data[0]), data[1]], stability=False, spurious=False, precision="fp64", k_sweep=True,
                          sweep_runner=_never)
    with pytest.raises(ValueError, match="k_max must be greater than k_min"):
        api.apply_resnmtf(data, stability=False, spurious=False, precision="fp64", k_sweep=True, k_min=4, k_max=4)
    with pytest.raises(ValueError, match="less than or equal to the ranks"):
        api.apply_resnmtf(data, stability=False, spurious=False, precision="fp64", k_sweep=True, k_min=3, k_max=11)
    with pytest.raises(NotImplementedError, match="explicit initial factors"):
        api.apply_resnmtf(data, np.ones((30, 3)), stability=False, spurious=False, precision="fp64", k_sweep=True)
    with pytest.raises(ValueError, match="no_clusts=True has none"):
        api.apply_resnmtf(data, stability=False, spurious=False, no_clusts=True, precision="fp64", k_sweep=True)


def test_apply_resnmtf_fp64_k_val_passes_the_flags_through(monkeypatch):
    seen = {}

    def inner(*args, **kw):
        seen.update(args=args, kw=kw)
        return {"bisil": 0.5}
    monkeypatch.setattr(api, "res_nmtf_inner", inner)
    data = _raw_data()
    out = api.apply_resnmtf(data, k_val=3, stability=False, spurious=False, n_iters=7, seed=11, precision="fp64", score_bisil=True,
                            fp64_bisil=True, fp64_sparse=True, fp64_device=True, fp64_sparse_device=True, device_id=1)
    assert out == {"bisil": 0.5}
    kw = seen["kw"]
    assert kw["precision"] == "fp64" and kw["score_bisil"] is True and kw["fp64_bisil"] is True and kw["seed"] == 11
    assert kw["fp64_sparse"] is True and kw["fp64_device"] is True and kw["fp64_sparse_device"] is True and kw["device_id"] == 1
    p = api.prepare(data, None, None, None, None, None, normalise=True, symmetrise=True)
    for got, want in zip(seen["args"][0], p.data):                        # the prepared data, k_vec, n_iters
        np.testing.assert_array_equal(got, want)
    assert seen["args"][6] == [3, 3] and seen["args"][10] == 7 and seen["args"][12] is False


def test_apply_resnmtf_fp64_sweep_runs_res_nmtf_inner_per_k(monkeypatch):
    """Without a sweep_runner every k goes to res_nmtf_inner(precision="fp64", score_bisil=True, fp64_bisil=True,
    seed=seed + k) on the prepared data with the shared maps; the pick is _sweep's (first maximum, extended while the
    largest k wins, capped at min(ncol, 64))."""
    calls = []
    scores = {3: 0.2, 4: 0.6, 5: 0.7, 6: 0.4}

    def inner(data, row_idx, col_idx, f, s, g, k_vec, phi, xi, psi, n_iters, num_repeats, spurious, distance, no_clusts, **kw):
        calls.append((list(k_vec), kw, row_idx, col_idx, spurious, no_clusts, distance))
        return {"bisil": scores[k_vec[0]], "k": k_vec[0]}
    monkeypatch.setattr(api, "res_nmtf_inner", inner)
    data = _raw_data()
    out = api.apply_resnmtf(data, stability=False, spurious=False, k_min=3, k_max=5, seed=100, distance="cosine", precision="fp64",
                            k_sweep=True, return_sweep=True)
    assert [c[0] for c in calls] == [[3, 3], [4, 4], [5, 5], [6, 6]]
    p = api.prepare(data, None, None, None, None, None, normalise=True, symmetrise=True)
    for k_vec, kw, row_idx, col_idx, spurious, no_clusts, distance in calls:
        assert kw["precision"] == "fp64" and kw["score_bisil"] is True and kw["fp64_bisil"] is True
        assert kw["seed"] == 100 + k_vec[0] and spurious is False and no_clusts is False and distance == "cosine"
        assert row_idx == p.row_shared and col_idx == p.col_shared
    assert out["k"] == 5 and out["k_sweep"] == {"k": [3, 4, 5, 6], "bisil": [0.2, 0.6, 0.7, 0.4]}


def test_apply_resnmtf_fp64_sweep_through_sweep_runner(monkeypatch):
    monkeypatch.setattr(api, "Engine", _never)
    monkeypatch.setattr(engine, "fp64_run", _never)
    ran = []

    def sweep_runner(k):
        ran.append(k)
        return {"bisil": {3: 0.1, 4: 0.9, 5: 0.3}[k], "k": k}
    out = api.apply_resnmtf(_raw_data(), stability=False, spurious=False, k_min=3, k_max=5, precision="fp64", k_sweep=True,
                            sweep_runner=sweep_runner, return_sweep=True)
    assert ran == [3, 4, 5] and out["k"] == 4 and out["k_sweep"]["bisil"] == [0.1, 0.9, 0.3]
    with pytest.warns(UserWarning, match="the k sweep stops at k = 10"):  # the cap: min(ncol) = 10
        out = api.apply_resnmtf(_raw_data(), stability=False, spurious=False, k_min=8, k_max=9, precision="fp64", k_sweep=True,
                                sweep_runner=lambda k: {"bisil": float(k), "k": k})
    assert out["k"] == 10


def test_default_precision_is_todays_function(monkeypatch):
    """apply_resnmtf without the keyword, and with precision="f32", never reaches the fp64 branch."""
    monkeypatch.setattr(api, "_apply_fp64", _never)
    with pytest.raises(NotImplementedError, match="pass k_val"):
        api.apply_resnmtf(_raw_data(), spurious=False)
    with pytest.raises(NotImplementedError, match="pass k_val"):
        api.apply_resnmtf(_raw_data(), spurious=False, precision="f32", fp64_bisil=True, score_bisil=True)
