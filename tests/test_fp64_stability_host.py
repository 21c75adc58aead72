"""Host side of stability selection in double precision (no GPU): the routing of
stability_check(precision="fp64") and apply_resnmtf(fp64_stability=True) through stand-ins (``repeat_runner``, ``runner``,
stand-in gathers, fits and scorings), the seeds and the draws, the shared trimming loop against a NumPy probe, the flag
as a no-op under f32, every earlier refusal word for word without the flag, the new refusals, and the exported symbols."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import helpers
from resnmtf_amd import _lib, api, batched, build, device_views, engine
from stability_ref import fake_relevance, fake_results, fake_runner
from test_fp64_bisil_host import _never, _raw_data

CHECK_ARGS = (None, None, None, 5, False, 5, False, "euclidean")          # phi, xi, psi, n_iters, spurious, num_repeats, no_clusts, distance


def test_symbols_structs_and_export():
    for name in ("resnmtf_fp64_subsample", "resnmtf_fp64_subsample_plan", "resnmtf_fp64_relevance"):
        assert name in _lib.SIGNATURES
    assert _lib.SIGNATURES["resnmtf_fp64_subsample"] == (C.c_int, [C.c_int, C.POINTER(_lib.Fp64SubsampleJob)])
    assert _lib.SIGNATURES["resnmtf_fp64_relevance"] == (C.c_int, [C.c_int, C.POINTER(_lib.Fp64RelevanceJob)])
    assert [f[0] for f in _lib.Fp64SubsampleJob._fields_] == [
        "struct_size", "n", "m", "n_sub", "m_sub", "rows", "cols", "x", "x_dev", "stream", "out", "n_empty_rows", "n_empty_cols",
        "row_mask", "col_mask"]
    assert [f[0] for f in _lib.Fp64RelevanceJob._fields_] == [
        "struct_size", "n", "m", "n_sub", "m_sub", "k", "k_ref", "row_c", "col_c", "true_r", "true_c", "true_r_dev", "true_c_dev",
        "rows", "cols", "stream", "relevance"]
    lib = C.CDLL(build.build(verbose=False))                              # the built library exports the new entries
    for name in ("resnmtf_fp64_subsample", "resnmtf_fp64_subsample_plan", "resnmtf_fp64_relevance"):
        assert hasattr(lib, name)
    header = open(helpers.ROOT + "/include/resnmtf_hip.h").read()
    assert "int resnmtf_fp64_subsample(int device_id, const resnmtf_fp64_subsample_job* job);" in header
    assert "int resnmtf_fp64_subsample_plan(long long row_stride, long long col_stride, int* out);" in header
    assert "int resnmtf_fp64_relevance(int device_id, const resnmtf_fp64_relevance_job* job);" in header
    assert "R/stability_analysis.r:124" in header.split("typedef struct resnmtf_fp64_subsample_job")[0][-3500:]
    assert "R/stability_analysis.r:45-67" in header.split("typedef struct resnmtf_fp64_relevance_job")[0][-3000:]
    assert f"#define RESNMTF_FP64_SUBSAMPLE_PLAN_INTS {_lib.FP64_SUBSAMPLE_PLAN_INTS}\n" in header
    assert "#define RESNMTF_ABI_VERSION 2 " in header                    # the ABI version does not move


def test_the_form_chooser_and_the_plan_need_no_device():
    assert engine.fp64_subsample_plan(1, 300)["gather"] == "rows" and engine.fp64_subsample_plan(70, 1)["gather"] == "lds"
    with pytest.raises(engine.ResnmtfError, match="strides must be >= 0"):
        engine.fp64_subsample_plan(1, -1)


def test_engine_entries_refuse_before_the_library(monkeypatch):
    monkeypatch.setattr(_lib, "load", lambda: None)
    with pytest.raises(NotImplementedError, match="a sparse view is not supported"):
        engine.fp64_subsample(sp.csc_matrix(np.eye(3)), [0], [0])
    with pytest.raises(ValueError, match="n x m matrix"):
        engine.fp64_subsample(np.ones(4), [0], [0])
    raw = device_views.RawDeviceView(np.ones((4, 3)))                      # (what it wraps is not looked at before the refusal)
    with pytest.raises(NotImplementedError, match="pre-processed dense views: a device tensor still to be shifted"):
        engine.fp64_subsample(raw, [0], [0])
    res, data = fake_results()
    with pytest.raises(NotImplementedError) as e:
        api.stability_check([data[0], device_views.RawDeviceView(data[1])], res, 4, *CHECK_ARGS, precision="fp64")
    assert str(e.value) == ('stability_check(precision="fp64"): a device tensor still to be shifted and column-normalised '
                            '(view 1) is not supported: the route takes pre-processed dense views')
    with pytest.raises(ValueError, match="rows must be a non-empty 1-D index list"):
        engine.fp64_subsample(np.ones((4, 3)), [], [0])
    with pytest.raises(ValueError, match="cols must hold integers"):
        engine.fp64_subsample(np.ones((4, 3)), [0], [0.5])


# ---- the shared trimming loop ---------------------------------------------------------------------------------------
def _numpy_probe(data, log=None):
    def probe(i, rows, cols):
        if log is not None:
            log.append((i, list(rows), list(cols)))
        sub = data[i][np.ix_(rows, cols)]
        return sub.sum(axis=1) == 0, sub.sum(axis=0) == 0
    return probe


def test_trim_samples_against_a_numpy_probe():
    rng = np.random.default_rng(0)
    a = rng.integers(1, 4, size=(12, 8)).astype(np.float64)
    b = rng.integers(1, 4, size=(12, 6)).astype(np.float64)          # shares the rows with view 0
    a[3, :] = 0.0                                                    # an empty row of view 0
    b[:, 2] = 0.0                                                    # an empty column of view 1
    b[7, :] = 0.0                                                    # an empty row of view 1
    shapes = [a.shape, b.shape]
    rows = [np.array([3, 0, 7, 5, 9]), None]; rows[1] = rows[0]
    cols = [np.array([1, 0, 6]), np.array([2, 4, 0])]
    log = []
    got = batched.trim_samples(shapes, (rows, cols), _numpy_probe([a, b], log))
    assert got is not None
    # view 0 drops its row 3 (no earlier view); view 1 then drops its row 7 -- and would drop it from view 0 too, were
    # view 0's list still as long as its own (R/stability_analysis.r:168-174 compares the lengths) -- and its column 2
    assert [list(r) for r in got[0]] == [[0, 7, 5, 9], [3, 0, 5, 9]] and [list(c) for c in got[1]] == [[1, 0, 6], [4, 0]]
    assert list(rows[0]) == [3, 0, 7, 5, 9] and list(cols[1]) == [2, 4, 0]        # the caller's draws are not modified
    # round 1: both views with their draws (every view has a list of its own); round 2: both at the fixed point
    assert log[:2] == [(0, [3, 0, 7, 5, 9], [1, 0, 6]), (1, [3, 0, 7, 5, 9], [2, 4, 0])]
    assert log[2:] == [(0, [0, 7, 5, 9], [1, 0, 6]), (1, [3, 0, 5, 9], [4, 0])]
    for v, d in enumerate((a, b)):
        sub = d[np.ix_(got[0][v], got[1][v])]
        assert (sub.sum(0) != 0).all() and (sub.sum(1) != 0).all()
    # an empty row of a later view leaves every earlier view that shares the rows while the lists are equally long
    a2 = a.copy(); a2[3, :] = 1.0
    shared = batched.trim_samples(shapes, (rows, cols), _numpy_probe([a2, b]))
    assert [list(r) for r in shared[0]] == [[3, 0, 5, 9], [3, 0, 5, 9]] and [list(c) for c in shared[1]] == [[1, 0, 6], [4, 0]]
    # nothing to trim: one round of probes, the draws come back equal
    full = batched.trim_samples(shapes, ([np.arange(3), np.arange(3)], [np.arange(2), np.array([0, 1])]), _numpy_probe([a, b]))
    assert [list(r) for r in full[0]] == [[0, 1, 2]] * 2
    # a view without shared extents trims alone
    c = np.ones((5, 6)); c[1, :] = 0.0
    alone = batched.trim_samples([a.shape, c.shape], ([np.array([0, 1, 2]), np.array([0, 1, 2])], [np.arange(3), np.arange(3)]),
                                 _numpy_probe([a, c]))
    assert list(alone[0][0]) == [0, 1, 2] and list(alone[0][1]) == [0, 2]


def test_trim_samples_returns_none_on_failure():
    a = np.zeros((6, 6)); a[0, 0] = 1.0
    assert batched.trim_samples([a.shape], ([np.arange(5)], [np.arange(5)]), _numpy_probe([a])) is None      # trims below 2 x 2
    assert batched.trim_samples([a.shape], ([np.arange(1)], [np.arange(5)]), _never) is None                 # too small to probe
    flip = {"n": 0}

    def never_settles(i, rows, cols):          # drops one row per round for ever: the loop is bounded
        flip["n"] += 1
        er = np.zeros(len(rows), dtype=bool); er[0] = True
        return er, np.zeros(len(cols), dtype=bool)
    assert batched.trim_samples([(100, 4)], ([np.arange(100)], [np.arange(4)]), never_settles, max_rounds=20) is None
    assert flip["n"] == 20


def test_the_f32_route_trims_through_the_same_loop(monkeypatch):
    seen = {}

    def fake(shapes, samples, probe, max_rounds=20):
        seen.update(shapes=shapes, samples=samples, max_rounds=max_rounds)
        return "trimmed"
    monkeypatch.setattr(batched, "trim_samples", fake)
    dev = batched.DeviceData.__new__(batched.DeviceData)
    dev.data_shapes, dev.sp = [(4, 3)], [None]
    assert dev._trim_samples(("r", "c")) == "trimmed"
    assert seen == {"shapes": [(4, 3)], "samples": ("r", "c"), "max_rounds": 20}


# ---- the fp64 repeats: seeds, draws, routing ------------------------------------------------------------------------
def test_repeat_seeds_draws_and_calls(monkeypatch):
    res, data = fake_results()
    n_v, k = 2, 4
    shapes = [d.shape for d in data]
    draws = batched.stability_draws(shapes, 3, 0.9, 7)
    gathers, fits, scored = [], [], []

    def subsample(x, rows, cols, device_id=0):
        gathers.append((x, np.array(rows), np.array(cols), device_id))
        return ("sub", id(x), len(rows), len(cols)), np.zeros(len(rows), dtype=bool), np.zeros(len(cols), dtype=bool)

    def inner(views, row_idx, col_idx, f, s, g, k_vec, phi, xi, psi, n_iters, num_repeats, spurious, **kw):
        fits.append((views, row_idx, col_idx, f, s, g, list(k_vec), n_iters, num_repeats, spurious, kw))
        return {"row_clusters": [("rc", v, kw["seed"]) for v in range(n_v)], "col_clusters": [("cc", v, kw["seed"]) for v in range(n_v)],
                "Error": 0.25, "All_Error": np.array([0.5, 0.25])}

    def relevance(row_c, col_c, true_r, true_c, rows, cols, device_id=0):
        scored.append((row_c, col_c, true_r, true_c, np.array(rows), np.array(cols), device_id))
        return fake_relevance(row_c[2], n_v, k)[row_c[1]]
    uploads = []

    def device_view(x, device_id=0):               # stands in for the one copy of a host view to the device
        uploads.append(x)
        return x
    monkeypatch.setattr(engine, "fp64_subsample", subsample)
    monkeypatch.setattr(engine, "fp64_relevance", relevance)
    monkeypatch.setattr(engine, "fp64_device_view", device_view)
    monkeypatch.setattr(api, "res_nmtf_inner", inner)
    rn = [[f"r{t}" for t in range(n)] for n, _ in shapes]
    cn = [[f"v{v}c{t}" for t in range(m)] for v, (_, m) in enumerate(shapes)]
    z = np.zeros((2, 2))
    out = batched.stability_relevance_fp64(data, res, k, 3, 0.9, 11, 7, z, z, z, rn, cn, max_iters=500, device_id=0)
    assert out["stability_performed"] and len(out["repeats"]) == 3 and len(fits) == 3
    total = np.zeros((n_v, k))
    for r, (rep, fit) in enumerate(zip(out["repeats"], fits)):
        views, row_idx, col_idx, f, s, g, k_vec, n_iters, num_repeats, spurious, kw = fit
        assert (row_idx, col_idx, f, s, g) == (None,) * 5 and k_vec == [k, k] and n_iters == 11 and spurious is False
        assert kw["seed"] == 7 + 2000 + r and kw["precision"] == "fp64" and kw["fp64_device"] is True and kw["output"] == "torch"
        assert kw["max_iters"] == 500 and "fp64_spurious" not in kw and "spurious_on_device" not in kw
        for v in range(n_v):                                       # the draws are the f32 route's; nothing was trimmed
            assert np.array_equal(rep["extras"]["row_samples"][v], draws[r][0][v])
            assert np.array_equal(rep["extras"]["col_samples"][v], draws[r][1][v])
            assert views[v] == ("sub", id(data[v]), len(draws[r][0][v]), len(draws[r][1][v]))
            assert kw["row_names"][v] == [rn[v][t] for t in draws[r][0][v]] and kw["col_names"][v] == [cn[v][t] for t in draws[r][1][v]]
        assert list(rep) == ["stability_performed", "relevance", "Error", "All_Error", "tag", "extras"] and rep["tag"] == f"stability={r}"
        want = np.stack([fake_relevance(7 + 2000 + r, n_v, k)[v] for v in range(n_v)])
        assert rep["relevance"].tobytes() == want.tobytes()
        total = total + want
    assert out["relevance"].tobytes() == (total / 3).tobytes()
    # every view is copied to the device once for all repeats; per repeat one sub-sample per view -- nothing is trimmed,
    # so the probe's tensor is the one factorised --, then one scoring per view against the reference's clusters as given
    assert len(uploads) == n_v and all(a is b for a, b in zip(uploads, data))
    assert len(gathers) == 3 * n_v and len(scored) == 3 * n_v
    for i, (row_c, col_c, true_r, true_c, rows, cols, device_id) in enumerate(scored):
        r, v = divmod(i, n_v)
        assert row_c == ("rc", v, 7 + 2000 + r) and col_c == ("cc", v, 7 + 2000 + r)
        assert true_r is res["row_clusters"][v] and true_c is res["col_clusters"][v]
        assert np.array_equal(rows, draws[r][0][v]) and np.array_equal(cols, draws[r][1][v])
    # with removal: the fp64 removal inside the fit, the repeat's own seed
    fits.clear()
    batched.stability_relevance_fp64(data, res, k, 1, 0.9, 11, 7, z, z, z, rn, cn, spurious_repeats=4, keep_clusters=False)
    kw = fits[0][-1]
    assert fits[0][8] == 4 and fits[0][9] is True and kw["spurious_on_device"] is True and kw["fp64_spurious"] is True and kw["seed"] == 2007


def test_a_repeat_that_cannot_be_sampled_is_not_performed(monkeypatch):
    res, data = fake_results()

    def all_empty(x, rows, cols, device_id=0):
        return "sub", np.ones(len(rows), dtype=bool), np.zeros(len(cols), dtype=bool)
    monkeypatch.setattr(engine, "fp64_subsample", all_empty)
    monkeypatch.setattr(engine, "fp64_device_view", lambda x, device_id=0: x)
    monkeypatch.setattr(api, "res_nmtf_inner", _never)
    monkeypatch.setattr(engine, "fp64_relevance", _never)
    z = np.zeros((2, 2))
    names = [[str(t) for t in range(40)]] * 2
    out = batched.stability_relevance_fp64(data, res, 4, 2, 0.9, 5, 0, z, z, z, names, names)
    assert out["stability_performed"] is False and out["relevance"] is None
    assert out["repeats"][0] == {"stability_performed": False, "tag": "stability=0"}


def test_stability_check_fp64_routes_through_the_runner_stand_in(monkeypatch):
    monkeypatch.setattr(batched, "DeviceData", _never)
    monkeypatch.setattr(engine, "fp64_subsample", _never)
    res, data = fake_results()
    f32 = api.stability_check(data, res, 4, *CHECK_ARGS, 0.9, 5, 0.6, False, repeat_runner=fake_runner(), seed=3)
    monkeypatch.setattr(batched, "stability_relevance_on_device", _never)          # the fp64 route does not pass through it
    kw = dict(repeat_runner=fake_runner(), seed=3, precision="fp64")
    out = api.stability_check(data, res, 4, *CHECK_ARGS, 0.9, 5, 0.6, False, **kw)
    total = np.zeros((2, 4))
    for r in range(5):
        total = total + fake_relevance(r)
    assert out["res"] is res and out["relevance"].tobytes() == (total / 5).tobytes()
    assert f32["relevance"].tobytes() == out["relevance"].tobytes()          # the same reduction
    cut = api.stability_check(data, res, 4, *CHECK_ARGS, 0.9, 5, 0.5, True, return_repeats=True, **kw)
    for i in range(2):
        drop = out["relevance"][i] < 0.5
        assert drop.any() and (cut["row_clusters"][i][:, drop] == 0).all() and (cut["col_clusters"][i][:, drop] == 0).all()
        assert np.array_equal(cut["row_clusters"][i][:, ~drop], res["row_clusters"][i][:, ~drop])
    assert len(cut["stability"]["repeats"]) == 5 and cut["output_f"] is res["output_f"]
    with pytest.warns(UserWarning, match="Unable to perform stability analysis"):
        same = api.stability_check(data, res, 4, *CHECK_ARGS, repeat_runner=fake_runner(fail_at=2), seed=3, precision="fp64")
    assert same is res


def test_stability_check_fp64_passes_its_arguments_on(monkeypatch):
    seen = {}

    def stand_in(data, results, k, n_stability, sample_rate, n_iters, seed, phi, xi, psi, row_names, col_names, max_iters, device_id,
                 keep_clusters=False, spurious_repeats=0, runner=None):
        seen.update(locals())
        return {"stability_performed": True, "relevance": np.full((2, 4), 0.7), "repeats": []}
    monkeypatch.setattr(batched, "stability_relevance_fp64", stand_in)
    monkeypatch.setattr(batched, "DeviceData", _never)
    res, data = fake_results()
    z = np.zeros((2, 2))
    api.stability_check(data, res, [4, 4], z, z, z, 9, True, 3, False, "euclidean", 0.8, 2, seed=5, max_iters=77, device_id=0,
                        spurious_on_device=True, return_repeats=True, precision="fp64")
    assert (seen["k"], seen["n_stability"], seen["sample_rate"], seen["n_iters"], seen["seed"]) == (4, 2, 0.8, 9, 5)
    assert (seen["max_iters"], seen["device_id"], seen["keep_clusters"], seen["spurious_repeats"], seen["runner"]) == (77, 0, True, 3, None)
    assert [len(r) for r in seen["row_names"]] == [30, 25] and seen["phi"] is z


# ---- refusals -------------------------------------------------------------------------------------------------------
def test_new_refusals_of_stability_check(monkeypatch):
    monkeypatch.setattr(batched, "DeviceData", _never)
    monkeypatch.setattr(engine, "fp64_subsample", _never)
    res, data = fake_results()
    with pytest.raises(ValueError, match="precision must be 'f32' or 'fp64'"):
        api.stability_check(data, res, 4, *CHECK_ARGS, precision="f64")
    with pytest.raises(TypeError):                                        # keyword-only
        api.stability_check(data, res, 4, *CHECK_ARGS, 0.9, 5, 0.6, True, "fp64")
    sparse_data = [data[0], sp.csc_matrix(data[1])]
    with pytest.raises(NotImplementedError) as e:
        api.stability_check(sparse_data, res, 4, *CHECK_ARGS, precision="fp64")
    assert str(e.value) == ('stability_check(precision="fp64"): a sparse view (view 1) is not supported: resnmtf_fp64_subsample '
                            'gathers dense views')
    for flag, kw in (("group", dict(group=object())), ("sparse_on_device", dict(sparse_on_device=True)),
                     ("shuffle_sparse", dict(shuffle_sparse=True))):
        with pytest.raises(NotImplementedError) as e:
            api.stability_check(data, res, 4, *CHECK_ARGS, precision="fp64", **kw)
        assert str(e.value) == (f'stability_check(precision="fp64"): {flag} is not supported: the fp64 repeats run one after the '
                                'other on dense views')
    with pytest.raises(NotImplementedError, match="outside the accelerated path; pass spurious=False"):
        api.stability_check(data, res, 4, None, None, None, 5, True, 5, False, "euclidean", precision="fp64")


def test_the_flag_is_a_no_op_under_f32(monkeypatch):
    calls = []

    def inner(*args, **kw):
        calls.append(("inner", sorted(kw)))
        return fake_results()[0]

    def check(*args, **kw):
        calls.append(("check", sorted(kw)))
        return "checked"
    monkeypatch.setattr(api, "res_nmtf_inner", inner)
    monkeypatch.setattr(api, "stability_check", check)
    data = _raw_data()
    plain = api.apply_resnmtf(data, k_val=3, spurious=False, seed=1)
    want = list(calls)
    calls.clear()
    flagged = api.apply_resnmtf(data, k_val=3, spurious=False, seed=1, fp64_stability=True)
    assert plain == flagged == "checked" and calls == want and "precision" not in dict(calls)["check"]
    with pytest.raises(TypeError):                                        # keyword-only
        api.apply_resnmtf(data, None, None, None, 3, None, None, None, 5, 3, 8, "euclidean", False, 5, False, 0.9, 5, True, 0.4,
                          True, True, True)


def test_without_the_flag_every_refusal_stands_word_for_word(monkeypatch):
    monkeypatch.setattr(api, "Engine", _never)
    monkeypatch.setattr(engine, "fp64_run", _never)
    monkeypatch.setattr(engine, "fp64_subsample", _never)
    data = _raw_data()
    text = ('apply_resnmtf(precision="fp64"): stability=True is not supported: the stability repeats run on the f32 engine; '
            'pass stability=False')
    for more in (dict(spurious=False), dict(spurious=False, k_val=None, k_sweep=True, sweep_runner=_never),
                 dict(spurious=True, spurious_on_device=True, fp64_spurious=True)):
        kw = dict(k_val=3, precision="fp64")
        kw.update(more)
        with pytest.raises(NotImplementedError) as e:
            api.apply_resnmtf(data, **kw)
        assert str(e.value) == text
    with pytest.raises(NotImplementedError) as e:                         # the flag does not replace fp64_spurious
        api.apply_resnmtf(data, k_val=3, precision="fp64", fp64_stability=True)
    assert str(e.value) == ('apply_resnmtf(precision="fp64"): spurious=True is not supported: spurious-bicluster removal runs '
                            'on the f32 engine; pass spurious=False')
    with pytest.raises(NotImplementedError, match="outside the accelerated path; pass spurious=False"):
        api.apply_resnmtf(data, k_val=3, precision="fp64", fp64_stability=True, fp64_spurious=True)
    with pytest.raises(NotImplementedError) as e:
        api.apply_resnmtf([sp.csc_matrix(data[0]), data[1]], k_val=3, spurious=False, precision="fp64", fp64_sparse=True,
                          fp64_stability=True)
    assert str(e.value) == ('apply_resnmtf(precision="fp64"): a sparse view with fp64_stability is not supported: '
                            'resnmtf_fp64_subsample gathers dense views; pass stability=False')


def test_apply_resnmtf_runs_the_fp64_check_after_the_fit_and_after_the_pick(monkeypatch):
    calls, checks = [], []
    scores = {3: 0.2, 4: 0.6, 5: 0.7, 6: 0.4}

    def inner(data, row_idx, col_idx, f, s, g, k_vec, *rest, **kw):
        calls.append(list(k_vec))
        return {"bisil": scores[k_vec[0]], "k": k_vec[0]}

    def check(data, results, k, phi, xi, psi, n_iters, spurious, num_repeats, no_clusts, distance, *rest, **kw):
        checks.append((data, results, list(k), spurious, num_repeats, rest, kw))
        return dict(results, checked=True)
    monkeypatch.setattr(api, "res_nmtf_inner", inner)
    monkeypatch.setattr(api, "stability_check", check)
    data = _raw_data()
    out = api.apply_resnmtf(data, k_val=3, spurious=False, seed=11, sample_rate=0.8, n_stability=3, stab_thres=0.3, remove_unstable=False,
                            precision="fp64", fp64_stability=True, max_iters=99)
    assert out == {"bisil": 0.2, "k": 3, "checked": True} and calls == [[3, 3]]
    views, results, k, spurious, num_repeats, rest, kw = checks.pop()
    assert k == [3, 3] and spurious is False and rest == (0.8, 3, 0.3)              # remove_unstable is NOT forwarded (main.r:255-262)
    assert kw["precision"] == "fp64" and kw["seed"] == 11 and kw["max_iters"] == 99 and kw["output"] == "numpy"
    assert kw["spurious_on_device"] is False and len(views) == 2 and abs(views[0].sum(0) - 1).max() < 1e-12     # the prepared data
    calls.clear()
    out = api.apply_resnmtf(data, k_min=3, k_max=5, seed=100, precision="fp64", k_sweep=True, return_sweep=True, num_repeats=4,
                            spurious=True, spurious_on_device=True, fp64_spurious=True, fp64_stability=True, remove_unstable=False)
    assert calls == [[3, 3], [4, 4], [5, 5], [6, 6]] and out["k"] == 5 and out["checked"] and out["k_sweep"]["k"] == [3, 4, 5, 6]
    views, results, k, spurious, num_repeats, rest, kw = checks.pop()
    assert results["k"] == 5 and k == [5, 5] and spurious is True and num_repeats == 4
    assert rest == (0.9, 5, 0.4, False)                                             # remove_unstable forwarded (main.r:324-332)
    assert kw["precision"] == "fp64" and kw["spurious_on_device"] is True and kw["seed"] == 100
    # stability=False: no check
    api.apply_resnmtf(data, k_val=3, spurious=False, stability=False, precision="fp64", fp64_stability=True)
    assert checks == []
