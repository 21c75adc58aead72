"""Host side of the SVD initialisation in double precision (no GPU): with ``Engine.__init__`` made to
raise and ``engine.fp64_init_svd`` / ``engine.fp64_run`` replaced by recording stand-ins, ``fp64_init=True`` builds no
engine in res_nmtf_inner, shuffled_fits_fp64, stability_repeat_fp64 or the k sweep and passes the seeds the f32 route
passes; it is a no-op with explicit factors, with ``host_init=True`` and under f32; without it the engine is still built.
Then the per-view seeds ``seed + v`` at the library boundary, the refusals of the C entry that need no device, and the
exported symbol."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import helpers
from resnmtf_amd import _lib, api, batched, build, engine, problem, spurious
from test_fp64_bisil_host import _inner_args, _never, _raw_data


class EngineBuilt(Exception):
    pass


def _no_engine(monkeypatch):
    def init(self, *args, **kwargs):
        raise EngineBuilt("an Engine was constructed")
    monkeypatch.setattr(engine.Engine, "__init__", init)
    monkeypatch.setattr(engine.Engine, "__del__", lambda self: None)


class _Start:
    """Stands in for engine.fp64_init_svd: logs every call and returns a start that depends on the seed."""

    def __init__(self):
        self.calls = []

    def __call__(self, views, k, seed=0, sigma=0.05, n_power=0, return_basis=False, output="numpy", device_id=0):
        self.calls.append(dict(views=views, k=k, seed=seed, sigma=sigma, n_power=n_power, return_basis=return_basis,
                               output=output, device_id=device_id))
        out = []
        for v, x in enumerate(views):
            n, m = x.shape
            rng = np.random.default_rng(int(seed) + v)
            five = [rng.random((n, k)) + 0.1, rng.random((k, k)) + 0.1, rng.random((m, k)) + 0.1, rng.random(k) + 0.5, rng.random(k) + 0.5]
            if output == "torch":
                import torch
                five = [torch.as_tensor(a) for a in five]
            out.append(tuple(five))
        return out


class _Run:
    """Stands in for engine.fp64_run: the initial factors come back as the result (tensors under output="torch")."""

    def __init__(self):
        self.calls = []

    def __call__(self, problem, tol=1.0e-6, max_iters=100000, device_id=0, output="numpy", return_state=False):
        self.calls.append(dict(problem=problem, output=output, device_id=device_id, max_iters=max_iters))
        n_v, k = len(problem["data"]), problem["k"]
        one = np.ones(k)
        if output == "torch":
            import torch
            one = torch.ones(k, dtype=torch.float64)
        return {"f": problem["init_f"], "s": problem["init_s"], "g": problem["init_g"], "lambda": [one] * n_v, "mu": [one] * n_v,
                "all_error": np.array([0.3, 0.2]), "iters": 2}


@pytest.fixture
def stubs(monkeypatch):
    _no_engine(monkeypatch)
    start, run = _Start(), _Run()
    monkeypatch.setattr(engine, "fp64_init_svd", start)
    monkeypatch.setattr(engine, "fp64_run", run)
    return start, run


# ---- res_nmtf_inner ---------------------------------------------------------------------------------------------------
def test_res_nmtf_inner_starts_from_fp64_init_svd_and_builds_no_engine(stubs):
    start, run = stubs
    a = _inner_args(2)
    args = (a[0], a[1], a[2], None, None, None) + a[6:]
    res = api.res_nmtf_inner(*args, spurious=False, seed=7, device_id=1, precision="fp64", fp64_init=True, return_init=True)
    assert len(start.calls) == 1 and len(run.calls) == 1
    call = start.calls[0]
    assert all(x is y for x, y in zip(call["views"], run.calls[0]["problem"]["data"]))      # the views the run receives
    assert (call["k"], call["seed"], call["output"], call["device_id"]) == (2, 7, "numpy", 1)      # seed: view v draws seed + v
    assert call["sigma"] == 0.05 and call["n_power"] == 0 and call["return_basis"] is False
    want = _Start()(a[0], 2, seed=7)
    p = run.calls[0]["problem"]
    for v in range(2):
        for key, i in (("init_f", 0), ("init_s", 1), ("init_g", 2), ("init_lam", 3), ("init_mu", 4)):
            assert np.array_equal(p[key][v], want[v][i])
        for got, ref in zip(res["init"][v], want[v]):                                       # return_init reports this start
            assert np.array_equal(got, ref)
    # seed=None is the f32 route's seed 0
    api.res_nmtf_inner(*args, spurious=False, precision="fp64", fp64_init=True)
    assert start.calls[-1]["seed"] == api._seed(None) == 0


def test_without_the_flag_the_engine_is_still_built(stubs):
    start, run = stubs
    a = _inner_args(2)
    with pytest.raises(EngineBuilt):
        api.res_nmtf_inner(a[0], a[1], a[2], None, None, None, *a[6:], spurious=False, seed=7, precision="fp64")
    assert start.calls == [] and run.calls == []


def test_the_flag_is_a_no_op_with_explicit_factors_host_init_and_f32(stubs, monkeypatch):
    start, run = stubs
    a = _inner_args(2)
    api.res_nmtf_inner(*a, spurious=False, precision="fp64", fp64_init=True)                      # explicit factors
    assert start.calls == [] and len(run.calls) == 1
    assert all(np.array_equal(x, y) for x, y in zip(run.calls[0]["problem"]["init_f"], a[3]))
    api.res_nmtf_inner(a[0], a[1], a[2], None, None, None, *a[6:], spurious=False, seed=3, precision="fp64", fp64_init=True,
                       host_init=True)                                                            # NumPy's SVD on the host
    assert start.calls == [] and len(run.calls) == 2
    f, s, g, lam, mu = api.svd_init(run.calls[1]["problem"]["data"], [2, 2], 3)
    assert all(np.array_equal(x, y) for x, y in zip(run.calls[1]["problem"]["init_f"], f))
    with pytest.raises(EngineBuilt):                                                              # f32: the engine, flag or not
        api.res_nmtf_inner(*a, spurious=False, fp64_init=True)
    assert start.calls == [] and len(run.calls) == 2
    with pytest.raises(TypeError):                                                                # keyword-only
        api.res_nmtf_inner(*a, 5, False, "euclidean", False, True)


def test_the_start_is_asked_for_on_the_device_under_fp64_device(stubs):
    start, run = stubs
    a = _inner_args(1)
    api.res_nmtf_inner(a[0], a[1], a[2], None, None, None, *a[6:], spurious=False, no_clusts=True, seed=2, precision="fp64",
                       fp64_device=True, output="torch", fp64_init=True)
    assert start.calls[0]["output"] == "torch" and run.calls[0]["output"] == "torch"
    start.calls.clear()
    xs = sp.csc_matrix(np.asarray(a[0][0]))
    api.res_nmtf_inner([xs], a[1], a[2], None, None, None, *a[6:], spurious=False, no_clusts=True, precision="fp64",
                       fp64_sparse=True, fp64_init=True)
    assert sp.issparse(start.calls[0]["views"][0]) and start.calls[0]["output"] == "numpy"      # from the sparse source


# ---- the shuffled fits ------------------------------------------------------------------------------------------------
def _draw(x, seed, normalise=True, device_id=0):
    return np.asarray(x) + 0.0, False, np.zeros(x.shape[0], dtype=bool), np.zeros(x.shape[1], dtype=bool)


def test_shuffled_fits_pass_the_flag_and_the_repeat_seeds(stubs):
    pytest.importorskip("torch")
    start, run = stubs
    data = list(_inner_args(2)[0])
    out = problem.shuffled_fits_fp64(data, 2, 3, seed=11, max_iters=40, device_id=0, shuffle=_draw, fp64_init=True)
    assert len(out) == 3 and [c["seed"] for c in start.calls] == [11 + 1000 + r for r in range(3)]      # the f32 fits' seeds
    assert all(c["output"] == "torch" and c["k"] == 2 for c in start.calls)
    with pytest.raises(EngineBuilt):                                                              # without it: today's engine
        problem.shuffled_fits_fp64(data, 2, 3, seed=11, shuffle=_draw)


def test_check_biclusters_passes_the_flag_only_when_set(monkeypatch):
    calls = []

    def fits(views, k, num_repeats, seed, max_iters, device_id, **kw):
        calls.append(kw)
        rng = np.random.default_rng(0)
        return [[rng.random((v.shape[0], k)) for v in views] for _ in range(num_repeats)]
    monkeypatch.setattr(spurious, "shuffled_fits_fp64", fits)
    rng = np.random.default_rng(1)
    data, F = [rng.random((8, 5))], [rng.random((8, 2))]
    jsd = lambda cols, pairs: np.full(len(pairs), 0.5)      # noqa: E731
    spurious.check_biclusters(data, F, 2, seed=1, jsd=jsd, precision="fp64", fp64_init=True)
    spurious.check_biclusters(data, F, 2, seed=1, jsd=jsd, precision="fp64")
    assert calls == [{"fp64_init": True}, {}]


def test_res_nmtf_inner_hands_the_flag_to_the_checker(stubs):
    seen = []

    def checker(data, output_f, num_repeats, **kw):
        seen.append(kw)
        return {"score": np.full((1, 2), 0.9), "avg_threshold": np.full(1, 0.2), "max_threshold": np.full(1, 0.3)}
    a = _inner_args(1)
    kw = dict(row_names=None, col_names=None, device_id=0, max_iters=10, seed=4, engine_opts=None, host_init=False,
              return_init=False, score_bisil=False, spurious_on_device=True, output="numpy", init_lm=None, return_state=False,
              post_on_device=False, fp64_spurious=True, num_repeats=3, checker=checker)
    api._res_nmtf_inner_fp64(a[0], a[1], a[2], None, None, None, *a[6:11], True, "euclidean", False, fp64_init=True, **kw)
    api._res_nmtf_inner_fp64(*a[:11], True, "euclidean", False, **kw)
    assert seen[0] == dict(seed=4, device_id=0, max_iters=10, precision="fp64", fp64_init=True)
    assert seen[1] == dict(seed=4, device_id=0, max_iters=10, precision="fp64")


# ---- the stability repeats --------------------------------------------------------------------------------------------
def test_stability_repeat_passes_the_flag_and_the_repeat_seed(stubs, monkeypatch):
    torch = pytest.importorskip("torch")
    start, run = stubs
    a = _inner_args(2, shape=(14, 10))
    data = [np.asarray(d) for d in a[0]]

    def gather(x, rows, cols, device_id=0):
        return torch.as_tensor(np.asarray(x)[np.ix_(rows, cols)]), np.zeros(len(rows), dtype=bool), np.zeros(len(cols), dtype=bool)
    monkeypatch.setattr(engine, "fp64_subsample", gather)
    monkeypatch.setattr(engine, "fp64_relevance", lambda rc, cc, tr, tc, rows, cols, device_id=0: np.ones(2))
    monkeypatch.setattr(engine, "fp64_device_view", lambda d, device_id=0: d)
    results = {"row_clusters": [np.ones((14, 2))] * 2, "col_clusters": [np.ones((10, 2))] * 2}
    rn, cn = [[f"r{i}" for i in range(14)]] * 2, [[f"c{v}_{i}" for i in range(10)] for v in range(2)]
    z = np.zeros((2, 2))
    out = batched.stability_relevance_fp64(data, results, 2, 2, 0.8, 5, 21, z, z, z, rn, cn, max_iters=30, fp64_init=True)
    assert out["stability_performed"] and [c["seed"] for c in start.calls] == [21 + 2000 + r for r in range(2)]
    assert all(c["output"] == "torch" for c in start.calls)
    assert all(v.shape[0] < 14 and v.shape[1] < 10 for v in start.calls[0]["views"])            # the sub-samples
    with pytest.raises(EngineBuilt):
        batched.stability_relevance_fp64(data, results, 2, 2, 0.8, 5, 21, z, z, z, rn, cn, max_iters=30)


def test_stability_check_passes_the_flag_only_when_set(monkeypatch):
    from stability_ref import fake_results
    calls = []

    def relevance(data, results, k, n_stability, sample_rate, n_iters, seed, phi, xi, psi, rn, cn, max_iters, device_id, **kw):
        calls.append(kw)
        return {"stability_performed": False, "relevance": None, "repeats": []}
    monkeypatch.setattr(batched, "stability_relevance_fp64", relevance)
    res, data = fake_results()
    for flag in ({"fp64_init": True}, {}):
        with pytest.warns(UserWarning):
            api.stability_check(data, res, 4, None, None, None, 5, False, 5, False, "euclidean", precision="fp64", **flag)
    assert "fp64_init" in calls[0] and calls[0]["fp64_init"] is True and "fp64_init" not in calls[1]


# ---- apply_resnmtf: the k_val fit, every k of the sweep, the stability check -----------------------------------------------
def test_apply_resnmtf_passes_the_flag_to_every_fit(monkeypatch):
    calls, stab = [], []
    scores = {3: 0.2, 4: 0.6, 5: 0.7, 6: 0.4}

    def inner(data, row_idx, col_idx, f, s, g, k_vec, phi, xi, psi, n_iters, num_repeats, spurious, distance, no_clusts, **kw):
        calls.append((list(k_vec), kw))
        return {"bisil": scores[k_vec[0]], "k": k_vec[0]}

    def check(data, results, k, *args, **kw):
        stab.append(kw)
        return results
    monkeypatch.setattr(api, "res_nmtf_inner", inner)
    monkeypatch.setattr(api, "stability_check", check)
    data = _raw_data()
    flags = dict(precision="fp64", spurious=True, spurious_on_device=True, fp64_spurious=True, fp64_stability=True)
    api.apply_resnmtf(data, k_val=3, seed=11, fp64_init=True, **flags)
    assert calls[-1][1]["fp64_init"] is True and calls[-1][1]["seed"] == 11 and stab[-1]["fp64_init"] is True and stab[-1]["seed"] == 11
    calls.clear()
    api.apply_resnmtf(data, k_min=3, k_max=5, seed=100, k_sweep=True, fp64_init=True, **flags)
    assert [c[0] for c in calls] == [[3, 3], [4, 4], [5, 5], [6, 6]]
    assert all(kw["fp64_init"] is True and kw["seed"] == 100 + k_vec[0] for k_vec, kw in calls) and stab[-1]["fp64_init"] is True
    calls.clear(); stab.clear()
    api.apply_resnmtf(data, k_min=3, k_max=4, seed=100, k_sweep=True, **flags)                  # without it: the calls of before
    assert all("fp64_init" not in kw for _, kw in calls) and "fp64_init" not in stab[-1]
    with pytest.raises(NotImplementedError, match="pass k_val"):                                  # f32: read by nobody
        api.apply_resnmtf(data, spurious=False, precision="f32", fp64_init=True)


# ---- the library boundary -----------------------------------------------------------------------------------------------
def test_symbol_struct_and_export():
    assert _lib.SIGNATURES["resnmtf_fp64_init_svd"] == (C.c_int, [C.c_int, C.POINTER(_lib.GroupJob), C.POINTER(_lib.Fp64Sparse),
                                                                  C.POINTER(_lib.Fp64Device), C.POINTER(_lib.Fp64SparseDevice),
                                                                  C.POINTER(_lib.Fp64Init)])
    assert [f[0] for f in _lib.Fp64Init._fields_] == [
        "struct_size", "n_power", "outputs_on_device", "sigma", "seed", "f0", "s0", "g0", "lambda0", "mu0", "singular_values",
        "basis_u", "basis_v", "basis_d", "basis_n_d"]
    lib = C.CDLL(build.build(verbose=False))
    assert hasattr(lib, "resnmtf_fp64_init_svd")
    header = open(helpers.ROOT + "/include/resnmtf_hip.h").read()
    assert "int resnmtf_fp64_init_svd(int device_id, const resnmtf_group_job* job, const resnmtf_fp64_sparse* sp," in header
    assert "R/update_steps.r:78-125" in header.split("typedef struct resnmtf_fp64_init {")[0][-4000:]
    assert "#define RESNMTF_ABI_VERSION 2 " in header                    # the ABI version does not move


class _FakeLib:
    """Stands in for the loaded library: records what resnmtf_fp64_init_svd is handed."""

    def __init__(self):
        self.seen = []

    def resnmtf_fp64_init_svd(self, device_id, job, sp_, dev, spd, init):
        j, i = job._obj, init._obj
        self.seen.append(dict(device_id=device_id, n_views=j.n_views, k=j.k, shapes=[(j.n_rows[v], j.n_cols[v]) for v in range(j.n_views)],
                              seeds=[int(i.seed[v]) for v in range(j.n_views)], sigma=i.sigma, n_power=i.n_power,
                              on_device=i.outputs_on_device, sparse=[bool(sp_ is not None and sp_._obj.view[v].col_ptr) for v in range(j.n_views)],
                              x=[bool(j.x[v]) for v in range(j.n_views)], basis=[bool(i.basis_u[v]) for v in range(j.n_views)],
                              factors=[bool(j.f0[v]) for v in range(j.n_views)], struct=i.struct_size))
        return 0


def test_engine_fills_the_structs_and_seeds_view_v_with_seed_plus_v(monkeypatch):
    fake = _FakeLib()
    monkeypatch.setattr(_lib, "load", lambda: fake)
    rng = np.random.default_rng(0)
    views = [rng.random((9, 7)), sp.csc_matrix(rng.random((9, 6))), rng.random((8, 7))]
    out = engine.fp64_init_svd(views, 3, seed=40, sigma=0.1, n_power=2, return_basis=True, device_id=1)
    s = fake.seen[0]
    assert s["seeds"] == [40, 41, 42] and s["shapes"] == [(9, 7), (9, 6), (8, 7)] and (s["n_views"], s["k"], s["device_id"]) == (3, 3, 1)
    assert s["sparse"] == [False, True, False] and s["x"] == [True, False, True] and s["factors"] == [False] * 3
    assert (s["sigma"], s["n_power"], s["on_device"], s["basis"]) == (0.1, 2, 0, [True] * 3) and s["struct"] == C.sizeof(_lib.Fp64Init)
    assert [tuple(a.shape) for a in out[1]] == [(9, 3), (3, 3), (6, 3), (3,), (3,), (3,), (9, 3), (6, 3), (0,)]
    engine.fp64_init_svd(views, 3, seed=[5, 9, 2])
    assert fake.seen[1]["seeds"] == [5, 9, 2] and fake.seen[1]["basis"] == [False] * 3
    with pytest.raises(ValueError, match="one seed per view"):
        engine.fp64_init_svd(views, 3, seed=[1, 2])
    with pytest.raises(ValueError, match="output"):
        engine.fp64_init_svd(views, 3, output="cupy")
    with pytest.raises(ValueError, match="every view must be a matrix"):
        engine.fp64_init_svd([np.ones(4)], 1)


# ---- the C entry's guards: refused before any device work -----------------------------------------------------------------
def _c_call(n=12, m=9, k=3, edit=None):
    """One host dense view; ``edit(job, init, sp)`` changes the structs before the call; returns (rc, text, outputs)."""
    lib = _lib.load()
    rng = np.random.default_rng(2)
    x = np.asfortranarray(rng.random((n, m)))
    outs = [np.full(s, -1.0, order="F") for s in ((n, k), (k, k), (m, k), (k,), (k,))]
    job, init, sp_ = _lib.GroupJob(), _lib.Fp64Init(), _lib.Fp64Sparse()
    job.struct_size, init.struct_size, sp_.struct_size = C.sizeof(job), C.sizeof(init), C.sizeof(sp_)
    job.n_views, job.k, job.n_rows[0], job.n_cols[0] = 1, k, n, m
    job.x[0] = x.ctypes.data_as(C.POINTER(C.c_double))
    init.sigma = 0.05
    for name, a in zip(("f0", "s0", "g0", "lambda0", "mu0"), outs):
        getattr(init, name)[0] = a.ctypes.data
    keep = [x]
    args = {"job": C.byref(job), "sp": None, "init": C.byref(init)}
    if edit is not None:
        edit(job, init, sp_, args, keep)
    rc = lib.resnmtf_fp64_init_svd(0, args["job"], args["sp"], None, None, args["init"])
    return rc, (lib.resnmtf_last_error(None) or b"").decode(), outs


GUARDS = {
    "job is NULL": lambda j, i, s, a, keep: a.update(job=None),
    "init is NULL": lambda j, i, s, a, keep: a.update(init=None),
    "resnmtf_fp64_init struct_size mismatch": lambda j, i, s, a, keep: setattr(i, "struct_size", 8),
    "resnmtf_group_job struct_size mismatch": lambda j, i, s, a, keep: setattr(j, "struct_size", 8),
    "resnmtf_fp64_sparse struct_size mismatch": lambda j, i, s, a, keep: (setattr(s, "struct_size", 4), a.update(sp=C.byref(s))),
    "k exceeds a view dimension": lambda j, i, s, a, keep: setattr(j, "k", 10),
    "k must be in [1, 64]": lambda j, i, s, a, keep: setattr(j, "k", 0),
    "sigma must be finite and >= 0": lambda j, i, s, a, keep: setattr(i, "sigma", -0.5),
    "sigma must be finite and >= 0 ": lambda j, i, s, a, keep: setattr(i, "sigma", float("nan")),
    "sigma must be finite and >= 0  ": lambda j, i, s, a, keep: setattr(i, "sigma", float("inf")),
    "view 0: an output is NULL": lambda j, i, s, a, keep: i.g0.__setitem__(0, None),
    "view 1: an output is given beyond n_views": lambda j, i, s, a, keep: i.mu0.__setitem__(1, i.mu0[0]),
    "view 0: the basis is given in part": lambda j, i, s, a, keep: (keep.append(np.zeros(64)),
                                                                   i.basis_d.__setitem__(0, keep[-1].ctypes.data_as(C.POINTER(C.c_double)))),
    "x / f0 / s0 / g0 is NULL": lambda j, i, s, a, keep: j.x.__setitem__(0, None),      # the view is given in no place
    "x has a non-finite entry": lambda j, i, s, a, keep: keep[0].__setitem__((3, 2), np.inf),
}


def _in_two_places(j, i, s, a, keep):
    ptr, idx, val = np.zeros(10, np.int64), np.zeros(1, np.int32), np.zeros(1)
    keep.extend([ptr, idx, val])
    s.view[0].col_ptr = ptr.ctypes.data_as(C.POINTER(C.c_longlong))
    s.view[0].row_idx = idx.ctypes.data_as(C.POINTER(C.c_int))
    s.view[0].values = val.ctypes.data_as(C.POINTER(C.c_double))
    a.update(sp=C.byref(s))


GUARDS["a view is given both dense (x) and sparse (col_ptr)"] = _in_two_places


@pytest.mark.parametrize("text", list(GUARDS))
def test_the_c_entry_refuses_before_any_device_work_and_writes_no_output(text):
    rc, said, outs = _c_call(edit=GUARDS[text])
    assert rc == 1, (rc, said)                                            # RESNMTF_ERR_INVALID
    assert text.strip() in said, said
    assert all((a == -1.0).all() for a in outs)
