"""Host side of the grouped path (batched.run_jobs_grouped, no GPU): refusals before any device work, and job
preparation equal to what run_job / api.res_nmtf_inner load into the engine (captured through a recording stand-in
for the Engine and through the group_runner hook)."""
import contextlib

import numpy as np
import pytest
import scipy.sparse as sp

import helpers
from resnmtf_amd import api, batched, naming


def _never(*args, **kwargs):
    raise AssertionError("the device runner must not be reached")


def _job(shape=(30, 20), k=3, n_views=1, **kw):
    rng = np.random.default_rng(0)
    return batched.Job([rng.random(shape) + 0.01 for _ in range(n_views)], k, **kw)


def test_refuses_sparse_views():
    job = batched.Job([sp.random(30, 20, density=0.5, format="csc", random_state=1)], 3)
    with pytest.raises(NotImplementedError, match="dense views only"):
        batched.run_jobs_grouped([_job(), job], group_runner=_never)


@pytest.mark.parametrize("k", [0, 33])
def test_refuses_k_outside_1_to_32(k):
    with pytest.raises(ValueError, match="1 <= k <= 32"):
        batched.run_jobs_grouped([_job(), _job(shape=(40, 40), k=k)], group_runner=_never)


def test_refuses_more_than_8_views():
    with pytest.raises(ValueError, match="at most 8 views"):
        batched.run_jobs_grouped([_job(n_views=9)], group_runner=_never)


def test_refuses_oversize_view():
    big = batched.Job([np.ones((2049, 2048)) + 0.0, np.ones((10, 10))], 3)       # 2049 * 2048 > 2^22
    with pytest.raises(ValueError, match="2\\^22"):
        batched.run_jobs_grouped([_job(), big], group_runner=_never)


def test_refuses_k_above_a_dimension():
    with pytest.raises(ValueError, match="exceeds a dimension"):
        batched.run_jobs_grouped([_job(shape=(30, 4), k=5)], group_runner=_never)


def test_refuses_inits_of_wrong_length():
    with pytest.raises(ValueError, match="one initial state per job"):
        batched.run_jobs_grouped([_job(), _job()], inits=[None], group_runner=_never)


class _RecordingEngine:
    """Stands in for engine.Engine inside api.res_nmtf_inner and records what is loaded into it."""
    last = None

    def __init__(self, n_rows, n_cols, k, device_id=0, **kw):
        self.n_views, self.k = len(n_rows), list(k)
        self.n_rows, self.n_cols = list(n_rows), list(n_cols)
        self.owned = [True] * self.n_views
        self.views, self.factors, self.rows, self.cols, self.init_seeds = {}, {}, {}, {}, {}
        self.rest = None
        _RecordingEngine.last = self

    def set_view(self, v, x):
        self.views[v] = np.array(x, dtype=np.float64)

    def init_svd(self, v, seed=0):
        self.init_seeds[v] = seed

    def set_factors(self, v, f, s, g, lam=None, mu=None):
        self.factors[v] = (f, s, g, lam, mu)

    def set_restrictions(self, phi, xi, psi):
        self.rest = (np.array(phi), np.array(xi), np.array(psi))

    def set_shared_rows(self, v, w, iv, iw):
        self.rows[(v, w)] = (iv, iw)

    def set_shared_cols(self, v, w, iv, iw):
        self.cols[(v, w)] = (iv, iw)

    def run(self, n_iters=None, tol=1e-6, max_iters=100000):
        return np.array([0.5])

    def finalise(self, v):
        n, m, k = self.n_rows[v], self.n_cols[v], self.k[v]
        return np.ones((n, k)), np.ones((k, k)), np.ones((m, k)), np.ones((n, k)), np.ones((m, k))

    def get_factors(self, v):
        n, m, k = self.n_rows[v], self.n_cols[v], self.k[v]
        return np.ones((n, k)), np.ones((k, k)), np.ones((m, k)), np.ones(k), np.ones(k)

    def close(self):
        pass


def _coupled_job(seed, n_iters=None):
    prob = helpers.coupled_problem([(40, 30), (36, 30), (44, 26)], 3, seed, phi_w=1.0, psi_w=0.5, xi_w=0.3,
                                   na_pairs=[(0, 2)])
    raw = [x * 3.0 - 0.2 for x in prob.data]                  # negative entries: check_data shifts and normalises
    phi = np.triu(prob.phi)                                   # unsymmetrised, as a caller passes them
    return batched.Job(raw, 3, phi, np.triu(prob.xi), np.triu(prob.psi), n_iters, seed, prob.row_names,
                       prob.col_names, tag=f"coupled {seed}")


@pytest.mark.parametrize("pre_processed", [False, True])
def test_preparation_matches_what_run_job_loads(monkeypatch, pre_processed):
    jobs = [_coupled_job(3), _coupled_job(4, n_iters=25), _job(n_views=2)]
    captured = {}

    def runner(problems, tol, max_iters, device_id):
        captured["problems"], captured["tol"], captured["max_iters"] = problems, tol, max_iters
        return [{"f": p["init_f"], "s": p["init_s"], "g": p["init_g"], "lambda": [np.ones(p["k"])] * len(p["data"]),
                 "mu": [np.ones(p["k"])] * len(p["data"]), "all_error": np.array([0.3, 0.2]), "iters": 2}
                for p in problems]

    with pytest.warns(UserWarning, match="non-negative") if not pre_processed else contextlib.nullcontext():
        out = batched.run_jobs_grouped(jobs, pre_processed=pre_processed, max_iters=777, group_runner=runner)
    assert captured["tol"] == 1e-6 and captured["max_iters"] == 777
    monkeypatch.setattr(api, "Engine", _RecordingEngine)
    for job, prob, res in zip(jobs, captured["problems"], out):
        ref = batched.run_job(job, pre_processed=pre_processed)
        eng = _RecordingEngine.last
        n_v = len(job.data)
        assert prob["k"] == job.k_val and eng.k == [job.k_val] * n_v and prob["n_iters"] == job.n_iters
        for v in range(n_v):
            np.testing.assert_array_equal(prob["data"][v], eng.views[v])
        for got, want in zip((prob["phi"], prob["xi"], prob["psi"]), eng.rest):
            np.testing.assert_array_equal(got, want)
        for v in range(n_v):
            for w in range(n_v):
                if v == w:
                    continue
                for pairs, loaded in ((prob["row_pairs"], eng.rows), (prob["col_pairs"], eng.cols)):
                    iv, iw = pairs[v][w]
                    wv, ww = loaded[(v, w)]
                    if wv is None:
                        assert iv is None and iw is None
                    else:
                        np.testing.assert_array_equal(iv, wv)
                        np.testing.assert_array_equal(iw, ww)
        # run_job initialises on the device from job.seed; the grouped path runs init_mats_inner on the host instead
        assert eng.init_seeds == {v: job.seed + v for v in range(n_v)}
        want = api.svd_init(prob["data"], [job.k_val] * n_v, job.seed)
        for got, w in zip((prob["init_f"], prob["init_s"], prob["init_g"], prob["init_lam"], prob["init_mu"]), want):
            for a, b in zip(got, w):
                np.testing.assert_array_equal(a, b)
        assert set(res) == set(ref) and res["bisil"] is None and res["tag"] == job.tag
        assert res["Error"] == (0.25 if job.n_iters is None else 0.2)


def test_explicit_inits_are_passed_through_and_clusters_follow_the_rule():
    job = _job(shape=(12, 9), k=2)
    data = naming.check_data(job.data)
    f = np.full((12, 2), 1.0 / 12); f[0, 0] = 0.5; f[1, 1] = 0.5
    g = np.full((9, 2), 1.0 / 9); g[2, 1] = 0.4
    s = np.array([[1.0, 3.0], [2.0, 0.5]])
    lam, mu = np.array([1.0, 2.0]), np.array([3.0, 4.0])
    seen = {}

    def runner(problems, **kw):
        seen["p"] = problems[0]
        return [{"f": [f], "s": [s], "g": [g], "lambda": [lam], "mu": [mu], "all_error": np.array([0.1]), "iters": 1}]

    res = batched.run_jobs_grouped([job], inits=[([f], [s], [g], [lam], [mu])], group_runner=runner)[0]
    p = seen["p"]
    assert p["init_f"][0] is f and p["init_s"][0] is s and p["init_g"][0] is g
    assert p["init_lam"][0] is lam and p["init_mu"][0] is mu
    np.testing.assert_array_equal(p["data"][0], data[0])
    from oracle import resnmtf_oracle as O
    rc, cc = O.binary_clusters([f], [g], [s])
    np.testing.assert_array_equal(res["row_clusters"][0], rc[0])
    np.testing.assert_array_equal(res["col_clusters"][0], cc[0])



@pytest.mark.parametrize("bad", ["f_k", "s", "g_rows", "lam", "views"])
def test_refuses_mis_shaped_inits_before_the_device(bad):
    job = _job(shape=(12, 9), k=3, n_views=2)
    data = naming.check_data(job.data)
    f, s, g, lam, mu = (list(t) for t in api.svd_init(data, [3, 3], 0))
    if bad == "f_k":
        f[1] = api.svd_init(data, [2, 2], 0)[0][1]          # an F built for another k
    elif bad == "s":
        s[0] = s[0][:2, :2]
    elif bad == "g_rows":
        g[1] = g[1][:-1]
    elif bad == "lam":
        lam[0] = np.append(lam[0], 1.0)
    else:
        f = f[:1]
    with pytest.raises(ValueError, match="initial"):
        batched.run_jobs_grouped([job], inits=[(f, s, g, lam, mu)], group_runner=_never)


@pytest.mark.parametrize("bad", ["init_f", "init_s", "init_g", "init_lam", "init_mu"])
def test_group_run_refuses_mis_shaped_inits(bad):
    """engine.group_run checks every initial factor's shape before the library reads n k, k k, m k or k doubles."""
    from resnmtf_amd.engine import group_run
    rng = np.random.default_rng(1)
    p = {"data": [rng.random((12, 9))], "k": 3, "init_f": [rng.random((12, 3))], "init_s": [rng.random((3, 3))],
         "init_g": [rng.random((9, 3))], "init_lam": [np.ones(3)], "init_mu": [np.ones(3)], "n_iters": 5}
    shrink = {"init_f": (12, 2), "init_s": (2, 3), "init_g": (8, 3), "init_lam": (2,), "init_mu": (4,)}[bad]
    p[bad] = [rng.random(shrink)]
    with pytest.raises(ValueError):
        group_run([p])
