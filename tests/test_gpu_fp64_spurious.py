"""Spurious-bicluster removal in double precision: res_nmtf_inner / apply_resnmtf with
precision="fp64", spurious=True, spurious_on_device=True, fp64_spurious=True against their compositions -- the fp64 run
followed by remove_spurious(precision="fp64"), and check_biclusters on the driver's own F's followed by apply_removal --,
the tensor route, what shuffle r is made of (its draw, its start), the check against the restatement (jsd_ref) within the
bars of tests/test_gpu_spurious.py (the scoring kernels are the same), the reference's tests and the refusals.

The problem is the planted two-view 180 x 180 one of tests/test_gpu_spurious.py, k = 3, R = 3; every fit, shuffled or
not, is guarded by max_iters = MAX_ITERS (the same guard on both sides of every comparison)."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import jsd_ref as J
import shuffle_ref as S
from resnmtf_amd import api, engine, problem, spurious
from resnmtf_amd.engine import Engine
from test_gpu_spurious import AVG_BAR, MODE_BAR, SCORE_BAR, planted

gpu = pytest.mark.gpu

R, K, MAX_ITERS, SEED = 3, 3, 300, 7
FLAGS = dict(spurious=True, spurious_on_device=True, fp64_spurious=True)
RESULT_KEYS = ("output_f", "output_s", "output_g", "row_clusters", "col_clusters", "lambda", "mu")
CHECK_KEYS = ("score", "avg_threshold", "max_threshold", "removed")


@functools.lru_cache(maxsize=None)
def prepared():
    x1, rc, cc = planted(1)
    x2, _, _ = planted(2)
    return api.prepare([x1, x2], None, None, None, None, None, normalise=True, symmetrise=True), rc, cc


def inner(data=None, **kw):
    p, _, _ = prepared()
    return api.res_nmtf_inner(p.data if data is None else data, p.row_shared, p.col_shared, k_vec=[K, K], phi=p.phi, xi=p.xi,
                              psi=p.psi, num_repeats=R, row_names=p.row_names, col_names=p.col_names, precision="fp64",
                              max_iters=MAX_ITERS, seed=SEED, **kw)


@functools.lru_cache(maxsize=None)
def plain():
    return inner(spurious=False)


@functools.lru_cache(maxsize=None)
def flagged():
    return inner(**FLAGS)


@functools.lru_cache(maxsize=None)
def driver():
    """The driver's F's for the planted data, with every repeat's draws (brought to the host) and attempt counts."""
    p, _, _ = prepared()
    seen = []
    fs = problem.shuffled_fits_fp64(p.data, K, R, SEED, max_iters=MAX_ITERS,
                                    keep=lambda r, tensors, attempts: seen.append(([t.cpu().numpy() for t in tensors], attempts)))
    return fs, seen


def same_result(a, b, keys=RESULT_KEYS):
    for key in keys:
        for v in range(2):
            x, y = (np.asarray(t.cpu().numpy() if hasattr(t, "cpu") else t) for t in (a[key][v], b[key][v]))
            assert np.array_equal(x, y), (key, v)
    for key in CHECK_KEYS:
        assert np.asarray(a["spurious"][key]).tobytes() == np.asarray(b["spurious"][key]).tobytes(), key


@gpu
def test_inner_equals_the_run_followed_by_remove_spurious():
    p, _, _ = prepared()
    res = flagged()
    assert set(res["spurious"]) == set(CHECK_KEYS) and res["spurious"]["score"].shape == (2, K)
    post = api.remove_spurious(p.data, plain(), R, seed=SEED, precision="fp64", max_iters=MAX_ITERS)
    same_result(res, post)
    assert np.array_equal(res["All_Error"], plain()["All_Error"])
    # ... and check_biclusters on the driver's own F's followed by apply_removal
    fs, _ = driver()
    check = api.check_biclusters(p.data, plain()["output_f"], R, shuffled_f=fs)
    same_result(res, spurious.apply_removal(plain(), check))


@gpu
def test_tensors_in_and_out_give_the_same_bits():
    import torch
    p, _, _ = prepared()
    dev = torch.device("cuda", 0)
    data = [torch.as_tensor(p.data[0], device=dev), torch.as_tensor(p.data[1], device=dev).t().contiguous().t()]
    there = inner(data, fp64_device=True, output="torch", **FLAGS)
    assert isinstance(there["row_clusters"][0], torch.Tensor) and there["row_clusters"][0].device == dev
    same_result(there, flagged())


@gpu
def test_shuffle_r_is_the_fp64_draw_and_starts_where_the_f32_shuffle_engine_would():
    p, _, _ = prepared()
    fs, seen = driver()
    assert len(fs) == R and len(seen) == R
    for r, (draws, attempts) in enumerate(seen):
        shuffle_seed = SEED * 7919 + r + 1
        tensors = []
        for v, x in enumerate(p.data):
            need = next(a + 1 for a in range(64) if _no_empty_line(S.shuffle_dense(x, S.draw_seed(shuffle_seed, a, v))))
            assert attempts[v] == need
            t, _, er, ec = engine.fp64_shuffle(x, S.draw_seed(shuffle_seed, need - 1, v), normalise=True)
            assert not er.any() and not ec.any() and np.array_equal(t.cpu().numpy(), draws[v])
            tensors.append(t)
        if r != 1:
            continue
        fit = api.res_nmtf_inner(tensors, None, None, None, None, None, [K, K], None, None, None, 1, spurious=False,
                                 seed=SEED + 1000 + r, max_iters=MAX_ITERS, precision="fp64", fp64_device=True, output="torch",
                                 return_init=True)
        with Engine([180, 180], [180, 180], [K, K]) as e:
            for v in range(2):
                e.set_view_device(v, tensors[v])
                e.init_svd(v, seed=SEED + 1000 + r + v)
            e.set_restrictions(None, None, None)
            for v in range(2):
                for got, want in zip(fit["init"][v], e.get_factors(v)):
                    assert np.array_equal(got.cpu().numpy().reshape(np.shape(want)), want), (r, v)
        again = api.res_nmtf_inner(tensors, None, None, None, None, None, [K, K], None, None, None, None, spurious=False,
                                   seed=SEED + 1000 + r, max_iters=MAX_ITERS, precision="fp64", fp64_device=True, output="torch")
        for v in range(2):
            assert np.array_equal(again["output_f"][v].cpu().numpy(), fs[r][v])


def _no_empty_line(d):
    return not ((d.sum(axis=0) == 0).any() or (d.sum(axis=1) == 0).any())


@gpu
def test_check_agrees_with_the_restatement():
    fs, _ = driver()
    got = flagged()["spurious"]
    want = J.check_biclusters(plain()["output_f"], fs)
    for key in ("score", "avg_threshold", "max_threshold"):
        print(f"MEASURED {key}: worst |device - restatement| = {float(np.max(np.abs(got[key] - want[key]))):.3e}")
    np.testing.assert_allclose(got["score"], want["score"], rtol=0, atol=SCORE_BAR)
    np.testing.assert_allclose(got["avg_threshold"], want["avg_threshold"], rtol=0, atol=AVG_BAR)
    np.testing.assert_allclose(got["max_threshold"], want["max_threshold"], rtol=0, atol=MODE_BAR)


@gpu
def test_reference_test_without_stability_with_spurious_removal():
    """test-resnmtf.R:63-72 ("resnmtf runs without stability with spurious removal") under precision="fp64", with the
    assertions of its f32 twin in tests/test_gpu_spurious.py."""
    x1, rc, cc = planted(1)
    x2, _, _ = planted(2)
    out = api.apply_resnmtf([x1, x2], k_val=3, stability=False, seed=SEED, precision="fp64", max_iters=MAX_ITERS, **FLAGS)
    assert len(out["output_f"]) == 2
    assert out["output_f"][0].shape == (180, 3)
    for v in (1, 0):
        assert sorted(out["row_clusters"][v].sum(0)) == sorted(rc.sum(0))
        assert sorted(out["col_clusters"][v].sum(0)) == sorted(cc.sum(0))
    assert not out["spurious"]["removed"].any()


@gpu
def test_fp64_k_sweep_with_spurious_removal_picks_the_planted_k():
    """test-resnmtf.R:123-135 ("resnmtf runs with k not specified") in fp64 with spurious=True: the k section 26's test
    picks, every k with its own check at seed + k, the pick bitwise res_nmtf_inner(fp64_spurious=True, seed=seed + k)."""
    from test_gpu_bisil import planted as planted_blocks
    x1, rc, cc = planted_blocks(1)
    x2, _, _ = planted_blocks(2)
    data = [x1, x2]
    common = dict(precision="fp64", num_repeats=2, max_iters=MAX_ITERS, spurious=True, spurious_on_device=True, fp64_spurious=True)
    res = api.apply_resnmtf(data, k_max=5, stability=False, k_sweep=True, return_sweep=True, seed=3, **common)
    sweep = res["k_sweep"]
    assert sweep["k"][:3] == [3, 4, 5] and sweep["k"][int(np.argmax(sweep["bisil"]))] == 3
    assert res["output_f"][0].shape == (180, 3) and res["bisil"] == max(sweep["bisil"])
    assert res["spurious"]["score"].shape == (2, 3) and not res["spurious"]["removed"].any()
    for v in range(2):
        assert sorted(res["row_clusters"][v].sum(0)) == sorted(rc.sum(0))
        assert sorted(res["col_clusters"][v].sum(0)) == sorted(cc.sum(0))
    p = api.prepare(data, None, None, None, None, None, normalise=True, symmetrise=True)
    one = api.res_nmtf_inner(p.data, p.row_shared, p.col_shared, k_vec=[3, 3], phi=p.phi, xi=p.xi, psi=p.psi,
                             row_names=p.row_names, col_names=p.col_names, seed=3 + 3, score_bisil=True, fp64_bisil=True, **common)
    assert one["bisil"] == res["bisil"]
    same_result(one, res)
    assert np.array_equal(one["All_Error"], res["All_Error"])


@gpu
def test_refusals_with_the_flag():
    p, _, _ = prepared()
    mixed = [p.data[0], sp.csc_matrix(p.data[1])]
    with pytest.raises(NotImplementedError, match=r"a sparse view \(view 1\) is not supported: no fp64 sparse shuffle exists"):
        inner(mixed, fp64_sparse=True, **FLAGS)
    x1, _, _ = planted(1)
    with pytest.raises(NotImplementedError, match=r'precision="fp64"\): stability=True is not supported'):
        api.apply_resnmtf([x1], k_val=3, precision="fp64", **FLAGS)
    with pytest.raises(NotImplementedError, match=r"a sparse view with fp64_spurious is not supported: no fp64 sparse shuffle exists"):
        api.apply_resnmtf([sp.csc_matrix(x1)], k_val=3, stability=False, precision="fp64", fp64_sparse=True, **FLAGS)
