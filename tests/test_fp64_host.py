"""Host side of the device-wide fp64 path (batched.run_job_fp64, api.res_nmtf_inner(precision="fp64"); no GPU): the
refusals come before the runner, the problem handed over is prepare_grouped_job's, the precision keyword is checked, what
needs a live handle is refused by name, and the default precision leaves res_nmtf_inner's calls as they are."""
import numpy as np
import pytest
import scipy.sparse as sp

import helpers
from resnmtf_amd import _lib, api, batched, engine, naming


def _never(*args, **kwargs):
    raise AssertionError("the device runner must not be reached")


def _job(shape=(30, 20), k=3, n_views=1, **kw):
    rng = np.random.default_rng(0)
    return batched.Job([rng.random(shape) + 0.01 for _ in range(n_views)], k, **kw)


def test_symbols_and_limits():
    assert "resnmtf_fp64_run" in _lib.SIGNATURES and "resnmtf_fp64_plan" in _lib.SIGNATURES
    assert batched.FP64_LIMITS.max_k == _lib.MAX_K == 64 and batched.FP64_LIMITS.max_view_entries is None
    assert batched.GROUPED_LIMITS == ("grouped", 8, 32, 1 << 22)


def test_refuses_sparse_views_before_the_runner():
    job = batched.Job([sp.random(30, 20, density=0.5, format="csc", random_state=1)], 3)
    with pytest.raises(NotImplementedError, match="fp64 path takes dense views only"):
        batched.run_job_fp64(job, runner=_never)


@pytest.mark.parametrize("k", [0, 65])
def test_refuses_k_outside_1_to_64(k):
    with pytest.raises(ValueError, match="fp64 path takes 1 <= k <= 64"):
        batched.run_job_fp64(_job(shape=(80, 80), k=k), runner=_never)


def test_refuses_more_than_8_views_and_k_above_a_dimension():
    with pytest.raises(ValueError, match="at most 8 views"):
        batched.run_job_fp64(_job(n_views=9), runner=_never)
    with pytest.raises(ValueError, match="exceeds a dimension"):
        batched.run_job_fp64(_job(shape=(30, 4), k=5), runner=_never)


def _echo(seen):
    def runner(problem, tol, max_iters, device_id):
        seen.update(problem=problem, tol=tol, max_iters=max_iters, device_id=device_id)
        n_v, k = len(problem["data"]), problem["k"]
        return {"f": problem["init_f"], "s": problem["init_s"], "g": problem["init_g"], "lambda": [np.ones(k)] * n_v,
                "mu": [np.ones(k)] * n_v, "all_error": np.array([0.3, 0.2]), "iters": 2}
    return runner


def test_takes_what_the_grouped_path_refuses():
    """k = 40 and 2049 x 2048 entries: over both grouped caps, prepared and handed to the runner here."""
    job = batched.Job([np.ones((2049, 2048))], 40, n_iters=2)
    init = ([np.ones((2049, 40))], [np.ones((40, 40))], [np.ones((2048, 40))])
    with pytest.raises(ValueError):
        batched.prepare_grouped_job(job, pre_processed=True, init=init)
    seen = {}
    res = batched.run_job_fp64(job, pre_processed=True, init=init, runner=_echo(seen))
    assert seen["problem"]["k"] == 40 and seen["problem"]["data"][0].shape == (2049, 2048)
    assert res["bisil"] is None and res["row_clusters"][0].shape == (2049, 40)


@pytest.mark.parametrize("pre_processed", [False, True])
def test_problem_equals_prepare_grouped_job(pre_processed):
    prob = helpers.coupled_problem([(40, 30), (36, 30), (44, 26)], 3, 3, phi_w=1.0, psi_w=0.5, xi_w=0.3, na_pairs=[(0, 2)])
    job = batched.Job(prob.data, 3, np.triu(prob.phi), np.triu(prob.xi), np.triu(prob.psi), 25, 3, prob.row_names,
                      prob.col_names, tag="coupled")
    want = batched.prepare_grouped_job(job, 0, pre_processed)
    seen = {}
    res = batched.run_job_fp64(job, device_id=2, pre_processed=pre_processed, max_iters=777, runner=_echo(seen))
    assert seen["tol"] == 1e-6 and seen["max_iters"] == 777 and seen["device_id"] == 2
    got = seen["problem"]
    assert set(got) == set(want)
    for key in want:
        a, b = got[key], want[key]
        if key in ("row_pairs", "col_pairs"):
            for ra, rb in zip(a, b):
                for pa, pb in zip(ra, rb):
                    assert (pa is None) == (pb is None)
                    if pa is not None:
                        for xa, xb in zip(pa, pb):
                            assert (xa is None and xb is None) or np.array_equal(xa, xb)
        elif key in ("row_names", "col_names", "k", "n_iters"):
            assert a == b
        elif isinstance(b, list):
            for xa, xb in zip(a, b):
                np.testing.assert_array_equal(xa, xb)
        else:
            np.testing.assert_array_equal(a, b)
    assert res["tag"] == "coupled" and res["bisil"] is None and res["Error"] == 0.2
    grouped = batched.run_jobs_grouped([job], pre_processed=pre_processed, group_runner=lambda ps, **kw: [_echo({})(ps[0], **kw)])[0]
    assert list(res) == list(grouped)                                   # run_job's keys, as the grouped path returns them


def _inner_args(n_views=1):
    rng = np.random.default_rng(1)
    data = naming.check_data([rng.random((12, 9)) + 0.01 for _ in range(n_views)])
    rn, cn = naming.give_names(data)
    f, s, g, _, _ = api.svd_init(data, [2] * n_views, 0)
    z = np.zeros((n_views, n_views))
    return (data, naming.shared_names(rn), naming.shared_names(cn), f, s, g, [2] * n_views, z, z, z, 5)


def test_precision_must_be_f32_or_fp64(monkeypatch):
    monkeypatch.setattr(api, "Engine", _never)
    with pytest.raises(ValueError, match="precision"):
        api.res_nmtf_inner(*_inner_args(), spurious=False, precision="bogus")
    with pytest.raises(TypeError):                                      # keyword-only
        api.res_nmtf_inner(*_inner_args(), 5, False, "euclidean", False, "fp64")


@pytest.mark.parametrize("flag,kwargs", [
    ("spurious_on_device", dict(spurious=True, spurious_on_device=True)),
    ("score_bisil", dict(spurious=False, score_bisil=True)),
    ("output=\"torch\"", dict(spurious=False, output="torch")),
    ("post_on_device", dict(spurious=False, output="torch", post_on_device=True)),
    ("return_state", dict(spurious=False, return_state=True)),
])
def test_fp64_refuses_what_needs_a_live_handle(monkeypatch, flag, kwargs):
    monkeypatch.setattr(api, "Engine", _never)
    monkeypatch.setattr(engine, "fp64_run", _never)
    with pytest.raises(NotImplementedError, match=flag):
        api.res_nmtf_inner(*_inner_args(), precision="fp64", **kwargs)


def test_fp64_refuses_sparse_and_device_memory(monkeypatch):
    import torch
    monkeypatch.setattr(api, "Engine", _never)
    monkeypatch.setattr(engine, "fp64_run", _never)
    args = list(_inner_args())
    sparse_args = [[sp.csc_matrix(args[0][0])]] + args[1:]
    with pytest.raises(NotImplementedError, match="sparse views"):
        api.res_nmtf_inner(*sparse_args, spurious=False, precision="fp64")
    there = torch.empty((12, 9), dtype=torch.float64, device="meta")       # (not on the CPU: stands for device memory)
    with pytest.raises(NotImplementedError, match="views in device memory"):
        api.res_nmtf_inner(*([[there]] + args[1:]), spurious=False, precision="fp64")
    f_there = [torch.empty((12, 2), dtype=torch.float64, device="meta")]
    with pytest.raises(NotImplementedError, match="factors in device memory"):
        api.res_nmtf_inner(*(args[:3] + [f_there] + args[4:]), spurious=False, precision="fp64")


def test_fp64_route_hands_the_explicit_start_to_the_runner(monkeypatch):
    monkeypatch.setattr(api, "Engine", _never)
    seen = {}
    monkeypatch.setattr(engine, "fp64_run", _echo(seen))
    args = _inner_args(2)
    lm = ([np.full(2, 2.0), np.full(2, 3.0)], [np.full(2, 4.0), np.full(2, 5.0)])
    res = api.res_nmtf_inner(*args, spurious=False, precision="fp64", init_lm=lm, return_init=True, max_iters=55)
    p = seen["problem"]
    assert seen["max_iters"] == 55 and p["k"] == 2 and p["n_iters"] == 5
    for v in range(2):
        np.testing.assert_array_equal(p["data"][v], args[0][v])
        np.testing.assert_array_equal(p["init_f"][v], args[3][v])
        np.testing.assert_array_equal(p["init_lam"][v], lm[0][v])
        np.testing.assert_array_equal(p["init_mu"][v], lm[1][v])
        np.testing.assert_array_equal(res["init"][v][4], lm[1][v])
    assert list(res) == ["output_f", "output_s", "output_g", "Error", "All_Error", "bisil", "row_clusters", "col_clusters",
                         "lambda", "mu", "init"]
    assert res["bisil"] is None and res["Error"] == 0.2


class _CallLog:
    """Stands in for engine.Engine inside api.res_nmtf_inner and records the order of the calls made on it."""
    calls = []

    def __init__(self, n_rows, n_cols, k, device_id=0, **kw):
        self.n_views, self.k, self.n_rows, self.n_cols = len(n_rows), list(k), list(n_rows), list(n_cols)
        self.owned = [True] * self.n_views
        _CallLog.calls = ["create"]

    def _log(name, result=None):
        def method(self, *args, **kwargs):
            _CallLog.calls.append(name)
            return result(self, *args) if result else None
        return method

    set_view = _log("set_view")
    init_svd = _log("init_svd")
    set_factors = _log("set_factors")
    set_restrictions = _log("set_restrictions")
    set_shared_rows = _log("set_shared_rows")
    set_shared_cols = _log("set_shared_cols")
    run = _log("run", lambda self, *a: np.array([0.5]))
    finalise = _log("finalise", lambda self, v: (np.ones((self.n_rows[v], self.k[v])), np.ones((self.k[v], self.k[v])),
                                                 np.ones((self.n_cols[v], self.k[v])), np.ones((self.n_rows[v], self.k[v])),
                                                 np.ones((self.n_cols[v], self.k[v]))))
    get_factors = _log("get_factors", lambda self, v: (np.ones((self.n_rows[v], self.k[v])), np.ones((self.k[v], self.k[v])),
                                                       np.ones((self.n_cols[v], self.k[v])), np.ones(self.k[v]), np.ones(self.k[v])))
    close = _log("close")


def test_default_precision_leaves_the_call_sequence_as_it_is(monkeypatch):
    monkeypatch.setattr(api, "Engine", _CallLog)
    monkeypatch.setattr(engine, "fp64_run", _never)
    args = _inner_args(2)
    want = (["create"] + ["set_view", "set_factors"] * 2 + ["set_restrictions"] + ["set_shared_rows", "set_shared_cols"] * 2 +
            ["run"] + ["finalise", "get_factors"] * 2 + ["close"])
    res_default = api.res_nmtf_inner(*args, spurious=False)
    assert _CallLog.calls == want
    res_f32 = api.res_nmtf_inner(*args, spurious=False, precision="f32")
    assert _CallLog.calls == want and list(res_default) == list(res_f32)
    # the device initialisation of the fp64 route: an engine is built, loaded, initialised, read and closed -- never run
    seen = {}
    monkeypatch.setattr(engine, "fp64_run", _echo(seen))
    api.res_nmtf_inner(*(args[:3] + (None, None, None) + args[6:]), spurious=False, precision="fp64", seed=4)
    assert _CallLog.calls == (["create"] + ["set_view", "init_svd"] * 2 + ["set_restrictions"] +
                              ["set_shared_rows", "set_shared_cols"] * 2 + ["get_factors"] * 2 + ["close"])
    assert seen["problem"]["init_lam"][0].shape == (2,)
