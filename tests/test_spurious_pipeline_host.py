"""CPU tests of the opt-in ``spurious_on_device=True`` (spurious-bicluster removal inside res_nmtf_inner, stability_check
and apply_resnmtf): the refusals without it, the plumbing through the stand-in hooks, and the new library symbols."""
import ctypes as C
import warnings

import numpy as np
import pytest
import scipy.sparse

import resnmtf_amd
from resnmtf_amd import api, batched, spurious
from stability_ref import fake_results, fake_runner

_X = [np.abs(np.random.default_rng(0).standard_normal((12, 9)))]


def test_refusals_without_the_opt_in_are_unchanged():
    with pytest.raises(NotImplementedError, match="spurious"):
        resnmtf_amd.res_nmtf_inner(_X, None, None, k_vec=[3], spurious=True)
    with pytest.raises(NotImplementedError, match="spurious"):
        resnmtf_amd.apply_resnmtf(_X, k_val=3, stability=False)
    with pytest.raises(NotImplementedError, match="stability"):
        resnmtf_amd.apply_resnmtf(_X, k_val=3)
    with pytest.raises(NotImplementedError, match="spurious"):
        resnmtf_amd.apply_resnmtf(_X, k_sweep=True, stability=False)
    res = {"row_clusters": [np.ones((12, 3))], "col_clusters": [np.ones((9, 3))]}
    with pytest.raises(NotImplementedError, match="spurious"):
        api.stability_check(_X, res, 3, None, None, None, None, True, 5, False, "euclidean")


def test_num_repeats_below_two_refused_as_check_biclusters_refuses_it():
    results, data = fake_results()
    for bad in (1, 0, 2.5, True):
        with pytest.raises(ValueError, match="num_repeats must be an integer >= 2"):
            resnmtf_amd.res_nmtf_inner(_X, None, None, k_vec=[3], spurious=True, num_repeats=bad, spurious_on_device=True)
        with pytest.raises(ValueError, match="num_repeats must be an integer >= 2"):
            api.stability_check(data, results, 4, None, None, None, 20, True, bad, False, "euclidean",
                                repeat_runner=fake_runner(2, 4), spurious_on_device=True)
    with pytest.raises(ValueError, match="num_repeats must be an integer >= 2"):
        resnmtf_amd.apply_resnmtf(_X, k_sweep=True, num_repeats=1, stability=False, spurious_on_device=True,
                                  sweep_runner=lambda k: {"bisil": 0.0})


def test_sparse_views_keep_the_shuffle_refusal():
    with pytest.raises(NotImplementedError, match="device shuffles of sparse views are not supported"):
        resnmtf_amd.res_nmtf_inner([scipy.sparse.csc_matrix(_X[0])], None, None, k_vec=[3], spurious=True,
                                   spurious_on_device=True)


def _stand_in_check(data, res, R=3, seed=0):
    """check_biclusters through its stand-in hooks (no device): shuffled F's drawn from ``seed``, a JSD stand-in."""
    rng = np.random.default_rng(seed)
    shuffled = [[rng.random(f.shape) for f in res["output_f"]] for _ in range(R)]
    return spurious.check_biclusters(data, res["output_f"], R, shuffled_f=shuffled,
                                     jsd=lambda cols, pairs: np.abs(cols[:, pairs[:, 0]] - cols[:, pairs[:, 1]]).mean(0))


def test_removal_runs_before_the_bisilhouette():
    results, data = fake_results(seed=5)
    check = _stand_in_check(data, results)
    check["score"][0, 1] = 0.0                                          # flagged whatever the thresholds
    seen = []

    def score_fn(rc, cc):
        seen.append(([r.copy() for r in rc], [c.copy() for c in cc]))
        return 0.25

    out = api._remove_then_score(results, check, score_fn)
    want = spurious.apply_removal(results, check)
    assert out["bisil"] == 0.25 and len(seen) == 1
    for v in range(2):
        assert np.array_equal(seen[0][0][v], want["row_clusters"][v])    # bisil saw the cleaned clusters
        assert np.array_equal(seen[0][1][v], want["col_clusters"][v])
    rel = np.argmax(results["output_s"][0], axis=0)
    assert out["spurious"]["removed"][0][rel == 1].all()
    assert not np.array_equal(out["row_clusters"][0], results["row_clusters"][0])
    assert results["row_clusters"][0][:, rel == 1].any()                   # the input is not modified
    plain = api._remove_then_score(results, None, None)                   # no check: nothing removed, bisil None
    assert plain["bisil"] is None and "spurious" not in plain


def test_remove_spurious_is_the_shared_removal():
    results, data = fake_results(seed=6)
    rng = np.random.default_rng(1)
    shuffled = [[rng.random(f.shape) for f in results["output_f"]] for _ in range(3)]
    jsd = lambda cols, pairs: np.abs(cols[:, pairs[:, 0]] - cols[:, pairs[:, 1]]).mean(0)   # noqa: E731
    a = spurious.remove_spurious(data, results, 3, shuffled_f=shuffled, jsd=jsd)
    check = spurious.check_biclusters(data, results["output_f"], 3, shuffled_f=shuffled, jsd=jsd)
    b = spurious.apply_removal(results, check)
    for key in ("row_clusters", "col_clusters"):
        for x, y in zip(a[key], b[key]):
            assert x.tobytes() == y.tobytes()
    assert np.array_equal(spurious.removal_flags(check)[0][np.argmax(results["output_s"][0], axis=0)],
                          a["spurious"]["removed"][0])


def test_thresholds_are_check_biclusters_host_part():
    null = np.random.default_rng(2).random(90)
    avg, mx = spurious.thresholds(null)
    assert avg == float(np.mean(null)) and mx == spurious.density_mode(null)


def test_stability_with_spurious_runs_the_repeats_and_keeps_remove_unstable(monkeypatch):
    results, data = fake_results()
    seen = {}
    real = batched.stability_relevance_on_device

    def spy(*args, **kwargs):
        seen["spurious_repeats"] = kwargs.get("spurious_repeats")
        return real(*args, **kwargs)

    monkeypatch.setattr(batched, "stability_relevance_on_device", spy)
    out = api.stability_check(data, results, 4, None, None, None, 20, True, 4, False, "euclidean", stab_thres=0.5,
                              repeat_runner=fake_runner(2, 4), spurious_on_device=True)
    assert seen["spurious_repeats"] == 4
    plain = api.stability_check(data, results, 4, None, None, None, 20, False, 4, False, "euclidean", stab_thres=0.5,
                                repeat_runner=fake_runner(2, 4))
    assert seen["spurious_repeats"] == 0
    for key in ("row_clusters", "col_clusters"):                          # remove_unstable as without the removal
        for a, b in zip(out[key], plain[key]):
            assert np.array_equal(a, b)
    kept = api.stability_check(data, results, 4, None, None, None, 20, True, 4, False, "euclidean",
                               remove_unstable=False, repeat_runner=fake_runner(2, 4), spurious_on_device=True)
    assert kept["res"] is results and kept["relevance"].shape == (2, 4)


def test_no_biclusters_left_after_the_removal_warns_and_returns():
    x = [np.abs(np.random.default_rng(3).standard_normal((20, 12)))]

    def run(k):                                                           # every cluster removed
        return {"bisil": 1.0 / k, "k": k, "row_clusters": [np.zeros((20, k))], "col_clusters": [np.zeros((12, k))]}

    with pytest.warns(UserWarning, match="No biclusters detected!"):
        res = resnmtf_amd.apply_resnmtf(x, k_min=3, k_max=4, k_sweep=True, sweep_runner=run, spurious_on_device=True,
                                        n_stability=2)
    assert res["k"] == 3 and not res["row_clusters"][0].any()


def test_new_symbols_are_exported_and_null_handles_refused():
    from resnmtf_amd import _lib
    lib = _lib.load()
    for name in ("resnmtf_spurious_scores", "resnmtf_relevance_masked"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert lib.resnmtf_spurious_scores(None, 0, None, 2, None, None) == 1
        flags = (C.c_ubyte * 4)()
        assert lib.resnmtf_relevance_masked(None, 0, None, 0, None, None, flags, None) == 1
