"""Host side of spurious-bicluster removal in double precision (no GPU): the routing of
res_nmtf_inner(precision="fp64", fp64_spurious=True) and apply_resnmtf through stand-ins (``runner``, ``checker``, a
stand-in shuffle, the ``shuffled_f`` / ``jsd`` hooks), the seeds of the driver, its redraw loop and the bound of 64, the
flag as a no-op under f32, every earlier refusal word for word without the flag, the new refusals, and the exported
symbol."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import helpers
import shuffle_ref as S
from resnmtf_amd import _lib, api, build, engine, problem, spurious
from test_fp64_bisil_host import _echo, _inner_args, _never, _raw_data

FLAGS = dict(spurious=True, spurious_on_device=True, fp64_spurious=True)


def test_symbol_struct_and_export():
    assert "resnmtf_fp64_shuffle" in _lib.SIGNATURES
    assert _lib.SIGNATURES["resnmtf_fp64_shuffle"] == (C.c_int, [C.c_int, C.POINTER(_lib.Fp64ShuffleJob)])
    names = [f[0] for f in _lib.Fp64ShuffleJob._fields_]
    assert names == ["struct_size", "n", "m", "normalise", "seed", "x", "x_dev", "stream", "out", "was_negative", "n_empty_rows",
                     "n_empty_cols", "row_mask", "col_mask"]
    lib = C.CDLL(build.build(verbose=False))                              # the built library exports the new entry
    assert hasattr(lib, "resnmtf_fp64_shuffle")
    header = open(helpers.ROOT + "/include/resnmtf_hip.h").read()
    assert "int resnmtf_fp64_shuffle(int device_id, const resnmtf_fp64_shuffle_job* job);" in header
    assert "R/obtain_bicl.r:11-22" in header.split("typedef struct resnmtf_fp64_shuffle_job")[0][-3500:]
    assert "#define RESNMTF_ABI_VERSION 2 " in header                    # the ABI version does not move


def test_engine_fp64_shuffle_refuses_before_the_library(monkeypatch):
    monkeypatch.setattr(_lib, "load", lambda: None)
    with pytest.raises(NotImplementedError, match="a sparse view is not supported"):
        engine.fp64_shuffle(sp.csc_matrix(np.eye(3)), 1)
    with pytest.raises(ValueError, match="n x m matrix"):
        engine.fp64_shuffle(np.ones(4), 1)


# ---- the driver: seeds, redraws, the bound ---------------------------------------------------------------------------
class _Shuffle:
    """Stands in for engine.fp64_shuffle: logs every call and reports an empty row for the first ``empty[(v, r)]`` draws."""

    def __init__(self, empty=None):
        self.calls, self.empty, self.count = [], empty or {}, {}

    def __call__(self, x, seed, normalise=True, device_id=0):
        self.calls.append((x, seed, normalise, device_id))
        n, m = x.shape
        key = id(x)
        self.count[key] = self.count.get(key, 0) + 1
        er = np.zeros(n, dtype=bool)
        er[0] = self.count[key] <= self.empty.get(key, 0)
        return ("draw", seed), False, er, np.zeros(m, dtype=bool)


def test_driver_seeds_are_those_of_the_f32_shuffles():
    data = [np.ones((6, 4)), np.ones((6, 5))]
    sh, fits, kept = _Shuffle(), [], []

    def fit(tensors, k, seed, max_iters, device_id):
        fits.append((tensors, k, seed, max_iters, device_id))
        return [np.full((6, k), float(seed)), np.full((6, k), float(seed) + 0.5)]
    out = problem.shuffled_fits_fp64(data, 3, 4, seed=11, max_iters=77, device_id=2, shuffle=sh, fit=fit,
                                     keep=lambda r, tensors, attempts: kept.append((r, attempts)))
    assert len(out) == 4 and all(len(fs) == 2 for fs in out)
    for r in range(4):
        shuffle_seed = 11 * 7919 + r + 1
        for v in range(2):
            x, seed, normalise, device_id = sh.calls[2 * r + v]
            assert x is data[v] and seed == S.draw_seed(shuffle_seed, 0, v) and normalise is True and device_id == 2
        tensors, k, seed, max_iters, device_id = fits[r]
        assert tensors == [("draw", S.draw_seed(shuffle_seed, 0, 0)), ("draw", S.draw_seed(shuffle_seed, 0, 1))]
        assert (k, seed, max_iters, device_id) == (3, 11 + 1000 + r, 77, 2)
        assert np.array_equal(out[r][0], np.full((6, 3), 11.0 + 1000 + r)) and out[r][0].dtype == np.float64
    assert kept == [(r, [1, 1]) for r in range(4)]


def test_redraw_loop_counts_attempts_and_is_bounded_at_64():
    x = np.ones((5, 4))
    sh = _Shuffle({id(x): 3})
    t, attempts = problem._draw_shuffle_fp64(x, 1, 500, device_id=0, shuffle=sh)
    assert attempts == 4 and t == ("draw", S.draw_seed(500, 3, 1))
    assert [c[1] for c in sh.calls] == [S.draw_seed(500, a, 1) for a in range(4)]
    sh = _Shuffle({id(x): 64})
    with pytest.raises(RuntimeError, match="shuffle_view: every draw left an all-zero row or column"):
        problem._draw_shuffle_fp64(x, 0, 9, shuffle=sh)
    assert len(sh.calls) == 64
    sh = _Shuffle({id(x): 63})
    assert problem._draw_shuffle_fp64(x, 0, 9, shuffle=sh)[1] == 64


def test_default_fit_is_the_fp64_path_from_device_memory(monkeypatch):
    seen = []

    def inner(data, row_idx, col_idx, f, s, g, k_vec, phi, xi, psi, n_iters, **kw):
        seen.append((data, row_idx, col_idx, f, s, g, k_vec, phi, xi, psi, n_iters, kw))
        return {"output_f": [np.ones((6, 2)), np.ones((6, 2))]}
    monkeypatch.setattr(api, "res_nmtf_inner", inner)
    data = [np.ones((6, 4)), np.ones((6, 5))]
    problem.shuffled_fits_fp64(data, 2, 2, seed=5, max_iters=40, device_id=1, shuffle=_Shuffle())
    assert len(seen) == 2
    for r, (tensors, row_idx, col_idx, f, s, g, k_vec, phi, xi, psi, n_iters, kw) in enumerate(seen):
        assert [t[0] for t in tensors] == ["draw", "draw"] and k_vec == [2, 2]
        assert (row_idx, col_idx, f, s, g, phi, xi, psi, n_iters) == (None,) * 9       # uncoupled, unrestricted, to convergence
        assert kw == dict(spurious=False, seed=5 + 1000 + r, max_iters=40, device_id=1, precision="fp64", fp64_device=True,
                          output="torch")


# ---- check_biclusters / remove_spurious with precision="fp64" --------------------------------------------------------
def _jsd(cols, pairs):
    cols, pairs = np.asarray(cols), np.asarray(pairs)
    return 0.1 + 0.01 * np.abs(cols[:, pairs[:, 0]] - cols[:, pairs[:, 1]]).sum(axis=0)


def test_check_biclusters_fp64_obtains_the_shuffled_f_from_the_driver(monkeypatch):
    rng = np.random.default_rng(0)
    data = [rng.random((8, 5)), rng.random((8, 6))]
    F = [rng.random((8, 2)), rng.random((8, 2))]
    shuffled = [[rng.random((8, 2)), rng.random((8, 2))] for _ in range(3)]
    calls = []

    def fits(views, k, num_repeats, seed, max_iters, device_id):
        calls.append((views, k, num_repeats, seed, max_iters, device_id))
        return shuffled
    monkeypatch.setattr(spurious, "shuffled_fits_fp64", fits)
    monkeypatch.setattr(spurious, "shuffled_engines", _never)
    got = spurious.check_biclusters(data, F, 3, seed=9, device_id=1, max_iters=50, jsd=_jsd, precision="fp64")
    views, k, num_repeats, seed, max_iters, device_id = calls[0]
    assert all(a is b or np.array_equal(a, b) for a, b in zip(views, data)) and (k, num_repeats, seed, max_iters, device_id) == (2, 3, 9, 50, 1)
    want = spurious.check_biclusters(data, F, 3, shuffled_f=shuffled, jsd=_jsd)
    for key in ("score", "avg_threshold", "max_threshold"):
        assert np.array_equal(got[key], want[key])
    assert len(calls) == 1
    spurious.check_biclusters(data, F, 3, jsd=_jsd, precision="fp64")
    assert calls[1][3] == 0                                               # seed None: 0, as the f32 route takes it
    # remove_spurious hands the keyword on
    res = {"output_f": F, "output_s": [np.eye(2), np.eye(2)], "row_clusters": [np.ones((8, 2)), np.ones((8, 2))],
           "col_clusters": [np.ones((5, 2)), np.ones((6, 2))]}
    out = spurious.remove_spurious(data, res, 3, seed=9, jsd=_jsd, precision="fp64")
    assert len(calls) == 3 and np.array_equal(out["spurious"]["score"], got["score"])
    # the refusals of the keyword
    with pytest.raises(ValueError, match="precision must be 'f32' or 'fp64'"):
        spurious.check_biclusters(data, F, 3, precision="f64")
    with pytest.raises(NotImplementedError, match=r"a sparse view \(view 1\) is not supported: no fp64 sparse shuffle exists"):
        spurious.check_biclusters([data[0], sp.csc_matrix(data[1])], F, 3, precision="fp64", shuffle_sparse=True)
    with pytest.raises(ValueError, match="grouped and group do not apply"):
        spurious.check_biclusters(data, F, 3, precision="fp64", grouped=True)
    assert len(calls) == 3


# ---- res_nmtf_inner / apply_resnmtf ----------------------------------------------------------------------------------
def _checker(log, score):
    def check(data, output_f, num_repeats, **kw):
        log.append((data, output_f, num_repeats, kw))
        n_v = len(output_f)
        return {"score": np.array(score, dtype=np.float64), "avg_threshold": np.full(n_v, 0.2), "max_threshold": np.full(n_v, 0.3)}
    return check


def test_inner_routes_check_removal_and_score_in_r_order(monkeypatch):
    monkeypatch.setattr(api, "Engine", _never)
    seen, log, scored = {}, [], []
    a = _inner_args(2)

    def sil(v, rc, cc, distance):
        scored.append((v, np.array(rc), np.array(cc)))
        return 0.5 * np.asarray(rc), 0.5 * np.asarray(cc)
    kw = dict(row_names=None, col_names=None, device_id=1, max_iters=10, seed=4, engine_opts=None, host_init=False,
              return_init=False, score_bisil=True, spurious_on_device=True, output="numpy", init_lm=None, return_state=False,
              post_on_device=False, fp64_bisil=True, runner=_echo(seen), sil=sil, fp64_spurious=True, num_repeats=3)
    res = api._res_nmtf_inner_fp64(*a[:11], True, "euclidean", False, checker=_checker(log, [[0.1, 0.9], [0.0, 0.9]]), **kw)
    data, output_f, num_repeats, ckw = log[0]
    assert len(log) == 1 and all(x is y for x, y in zip(data, seen["problem"]["data"]))      # the views as the run received them
    assert all(x is y for x, y in zip(output_f, res["output_f"])) and num_repeats == 3
    assert ckw == dict(seed=4, device_id=1, max_iters=10, precision="fp64")
    plain = api._res_nmtf_inner_fp64(*a[:11], False, "euclidean", False, **{**kw, "score_bisil": False})
    assert "spurious" not in plain
    want = spurious.apply_removal(plain, {"score": np.array([[0.1, 0.9], [0.0, 0.9]]), "avg_threshold": np.full(2, 0.2),
                                          "max_threshold": np.full(2, 0.3)})
    assert want["spurious"]["removed"].any() and not want["spurious"]["removed"].all()
    for key in ("score", "avg_threshold", "max_threshold", "removed"):
        assert np.array_equal(res["spurious"][key], want["spurious"][key])
    for v in range(2):
        assert np.array_equal(res["row_clusters"][v], want["row_clusters"][v])
        assert np.array_equal(res["col_clusters"][v], want["col_clusters"][v])
        assert np.array_equal(scored[v][1], want["row_clusters"][v])                         # the score saw the cleaned clusters
    assert res["bisil"] is not None and list(res).index("spurious") > list(res).index("col_clusters")
    # no_clusts: nothing is checked
    log.clear()
    api._res_nmtf_inner_fp64(*a[:11], True, "euclidean", True, checker=_checker(log, None), **kw)
    assert log == []


def test_flag_is_a_no_op_under_f32(monkeypatch):
    from test_fp64_host import _CallLog
    monkeypatch.setattr(api, "Engine", _CallLog)
    monkeypatch.setattr(engine, "fp64_run", _never)
    monkeypatch.setattr(engine, "fp64_shuffle", _never)
    monkeypatch.setattr(spurious, "shuffled_fits_fp64", _never)
    args = _inner_args(2)
    plain = api.res_nmtf_inner(*args, spurious=False)
    want = list(_CallLog.calls)
    flagged = api.res_nmtf_inner(*args, spurious=False, fp64_spurious=True)
    assert _CallLog.calls == want and list(plain) == list(flagged)
    with pytest.raises(NotImplementedError, match="pass k_val"):
        api.apply_resnmtf(_raw_data(), spurious=False, precision="f32", fp64_spurious=True)


def test_without_the_flag_every_refusal_stands_word_for_word(monkeypatch):
    monkeypatch.setattr(api, "Engine", _never)
    monkeypatch.setattr(engine, "fp64_run", _never)
    monkeypatch.setattr(engine, "fp64_shuffle", _never)
    with pytest.raises(NotImplementedError) as e:
        api.res_nmtf_inner(*_inner_args(), spurious=True, spurious_on_device=True, precision="fp64")
    assert str(e.value) == ('precision="fp64": spurious_on_device needs a live engine handle, which the fp64 path does not keep '
                            '(it runs through resnmtf_fp64_run); use precision="f32" for it')
    for more in (dict(), dict(fp64_spurious=True)):                       # the flag does not replace spurious_on_device
        with pytest.raises(NotImplementedError) as e:
            api.res_nmtf_inner(*_inner_args(), spurious=True, precision="fp64", **more)
        assert str(e.value) == ("spurious-bicluster removal (R/obtain_bicl.r:31-133) is outside the accelerated path; "
                                "pass spurious=False or do it on the R side (INTEGRATION.md).")
    data = _raw_data()
    for more in (dict(), dict(spurious_on_device=True)):
        with pytest.raises(NotImplementedError) as e:
            api.apply_resnmtf(data, k_val=3, stability=False, precision="fp64", **more)
        assert str(e.value) == ('apply_resnmtf(precision="fp64"): spurious=True is not supported: spurious-bicluster removal runs '
                                'on the f32 engine; pass spurious=False')
        with pytest.raises(NotImplementedError) as e:
            api.apply_resnmtf(data, stability=False, precision="fp64", k_sweep=True, sweep_runner=_never, **more)
        assert "spurious=True is not supported" in str(e.value)
    with pytest.raises(TypeError):                                        # keyword-only
        api.res_nmtf_inner(*_inner_args(), 5, False, "euclidean", False, True)


def test_new_refusals_and_their_texts(monkeypatch):
    monkeypatch.setattr(api, "Engine", _never)
    monkeypatch.setattr(engine, "fp64_run", _never)
    monkeypatch.setattr(engine, "fp64_shuffle", _never)
    args = list(_inner_args(2))
    mixed = [[args[0][0], sp.csc_matrix(args[0][1])]] + args[1:]
    with pytest.raises(NotImplementedError) as e:
        api.res_nmtf_inner(*mixed, precision="fp64", fp64_sparse=True, **FLAGS)
    assert str(e.value) == ('precision="fp64": spurious-bicluster removal in double precision (fp64_spurious) shuffles dense views '
                            'only; a sparse view (view 1) is not supported: no fp64 sparse shuffle exists')
    with pytest.raises(NotImplementedError, match="sparse views"):        # without fp64_sparse: the earlier refusal, as before
        api.res_nmtf_inner(*mixed, precision="fp64", **FLAGS)
    with pytest.raises(ValueError, match="num_repeats must be an integer >= 2"):
        api.res_nmtf_inner(*args[:11], 1, precision="fp64", **FLAGS)
    data = _raw_data()
    with pytest.raises(NotImplementedError, match=r'precision="fp64"\): stability=True is not supported: the stability repeats'):
        api.apply_resnmtf(data, k_val=3, precision="fp64", **FLAGS)
    with pytest.raises(NotImplementedError) as e:
        api.apply_resnmtf([sp.csc_matrix(data[0]), data[1]], k_val=3, stability=False, precision="fp64", fp64_sparse=True, **FLAGS)
    assert str(e.value) == ('apply_resnmtf(precision="fp64"): a sparse view with fp64_spurious is not supported: no fp64 sparse '
                            'shuffle exists; pass spurious=False')
    with pytest.raises(NotImplementedError, match="outside the accelerated path; pass spurious=False"):
        api.apply_resnmtf(data, k_val=3, stability=False, precision="fp64", spurious=True, fp64_spurious=True)


def test_apply_resnmtf_passes_the_flags_for_a_k_val_and_for_every_k_of_the_sweep(monkeypatch):
    calls = []
    scores = {3: 0.2, 4: 0.6, 5: 0.7, 6: 0.4}

    def inner(data, row_idx, col_idx, f, s, g, k_vec, phi, xi, psi, n_iters, num_repeats, spurious, distance, no_clusts, **kw):
        calls.append((list(k_vec), kw, spurious, num_repeats))
        return {"bisil": scores[k_vec[0]], "k": k_vec[0]}
    monkeypatch.setattr(api, "res_nmtf_inner", inner)
    data = _raw_data()
    out = api.apply_resnmtf(data, k_val=3, stability=False, num_repeats=4, seed=11, precision="fp64", **FLAGS)
    k_vec, kw, spur, num_repeats = calls.pop()
    assert out["k"] == 3 and spur is True and num_repeats == 4 and kw["seed"] == 11
    assert kw["spurious_on_device"] is True and kw["fp64_spurious"] is True and kw["precision"] == "fp64"
    out = api.apply_resnmtf(data, stability=False, k_min=3, k_max=5, seed=100, precision="fp64", k_sweep=True, return_sweep=True,
                            num_repeats=4, **FLAGS)
    assert [c[0] for c in calls] == [[3, 3], [4, 4], [5, 5], [6, 6]]                     # the extension k included
    for k_vec, kw, spur, num_repeats in calls:
        assert spur is True and num_repeats == 4 and kw["seed"] == 100 + k_vec[0]
        assert kw["spurious_on_device"] is True and kw["fp64_spurious"] is True
        assert kw["score_bisil"] is True and kw["fp64_bisil"] is True
    assert out["k"] == 5 and out["k_sweep"] == {"k": [3, 4, 5, 6], "bisil": [0.2, 0.6, 0.7, 0.4]}
    # without the flag the calls carry neither keyword
    calls.clear()
    api.apply_resnmtf(data, stability=False, spurious=False, k_min=3, k_max=4, precision="fp64", k_sweep=True)
    assert all("fp64_spurious" not in kw and "spurious_on_device" not in kw and spur is False for _, kw, spur, _ in calls)
