"""CPU tests of stability selection's host side (R/stability_analysis.r:302-338): the closed count form of
relevance_results against a literal pair-set restatement, api.stability_check's reduction and output paths with a
stand-in repeat runner (world 1 and a gloo world of 2), and the argument refusals of apply_resnmtf."""
import os
import pickle
import socket
import subprocess
import sys
import warnings

import numpy as np
import pytest

from helpers import ROOT
from resnmtf_amd import api
from stability_ref import fake_relevance, fake_results, fake_runner, relevance_counts, relevance_sets


def _rand_binary(rng, n, k, p):
    return (rng.random((n, k)) < p).astype(np.float64)


@pytest.mark.parametrize("seed", range(12))
def test_count_form_equals_pair_sets(seed):
    """Random small binary clusterings, with empty columns mixed in: the count form is bitwise the pair-set form."""
    rng = np.random.default_rng(seed)
    n, m, k = int(rng.integers(3, 14)), int(rng.integers(3, 12)), int(rng.integers(1, 6))
    mats = [_rand_binary(rng, n, k, 0.4), _rand_binary(rng, m, k, 0.5), _rand_binary(rng, n, k, 0.3),
            _rand_binary(rng, m, k, 0.6)]
    for a in mats:                          # some clusters empty on one side
        if k > 1:
            a[:, rng.integers(0, k)] = 0.0
    a, b = relevance_counts(*mats), relevance_sets(*mats)
    assert a.shape == (k,) and np.array_equal(a, b)
    assert ((a >= 0) & (a <= 1)).all()


def test_edge_cases_broadcast_zero_and_one():
    rng = np.random.default_rng(7)
    n, m, k = 9, 7, 3
    rc, cc, tr, tc = (_rand_binary(rng, n, k, 0.5), _rand_binary(rng, m, k, 0.5), _rand_binary(rng, n, k, 0.5),
                      _rand_binary(rng, m, k, 0.5))
    rc[0] = tr[0] = 1.0
    z = np.zeros((n, k))
    for args, want in (((z, cc, tr, tc), 0.0), ((rc, cc, z, tc), 0.0), ((z, cc, z, tc), 1.0)):
        for f in (relevance_counts, relevance_sets):
            out = f(*args)
            assert np.array_equal(out, np.full(k, want))
    # the edge cases look at the ROW clusters only: empty column clusters with rows present go through Jaccard
    out = relevance_counts(rc, np.zeros((m, k)), tr, tc)
    assert np.array_equal(out, relevance_sets(rc, np.zeros((m, k)), tr, tc)) and np.array_equal(out, np.zeros(k))


def test_identical_and_disjoint_clusterings():
    n, m = 14, 10                           # rows 12 and 13 belong to no cluster
    rc = np.zeros((n, 3)); cc = np.zeros((m, 3))
    for i in range(3):
        rc[4 * i:4 * i + 4, i] = 1; cc[3 * i:3 * i + 3, i] = 1
    assert np.array_equal(relevance_counts(rc, cc, rc, cc), np.ones(3))
    assert np.array_equal(relevance_sets(rc, cc, rc, cc), np.ones(3))
    perm = [2, 0, 1]                        # a permutation of the clusters changes nothing (max over i)
    assert np.array_equal(relevance_counts(rc[:, perm], cc[:, perm], rc, cc), np.ones(3))
    other_r = np.zeros((n, 3)); other_r[12:, :] = 1
    dis = relevance_counts(rc, cc, other_r, cc)
    assert np.array_equal(dis, np.zeros(3))
    assert np.array_equal(dis, relevance_sets(rc, cc, other_r, cc))
    # partial overlap: one exact value
    tr = rc.copy(); tr[0, 0] = 0                 # |TR_0| = 3: J = 3 * 3 / (4 * 3 + 3 * 3 - 9) = 9 / 12
    got = relevance_counts(rc, cc, tr, cc)
    assert got[0] == 9 / 12 and got[0] == relevance_sets(rc, cc, tr, cc)[0]


def _check(results, data, **kw):
    args = dict(n_stability=5, stab_thres=0.5, remove_unstable=True, repeat_runner=fake_runner(2, 4))
    args.update(kw)
    return api.stability_check(data, results, 4, None, None, None, 20, False, 5, False, "euclidean", **args)


def _sequential_mean(n_stability, n_views=2, k=4):
    total = np.zeros((n_views, k))
    for r in range(n_stability):
        total = total + fake_relevance(r, n_views, k)
    return total / n_stability


def test_reduction_is_the_sum_in_repeat_order_over_n_stability():
    results, data = fake_results()
    out = _check(results, data, n_stability=7, remove_unstable=False)
    want = _sequential_mean(7)
    assert set(out) == {"res", "relevance"} and out["res"] is results
    assert np.array_equal(out["relevance"], want)
    rev = np.zeros((2, 4))
    for r in reversed(range(7)):
        rev = rev + fake_relevance(r)
    assert not np.array_equal(rev / 7, want), "the stand-in values do not tell the summation order apart"


def test_unstable_columns_zeroed_on_a_copy():
    results, data = fake_results()
    before = {key: [a.copy() for a in results[key]] for key in ("row_clusters", "col_clusters", "output_f")}
    rel = _sequential_mean(5)
    thr = float(np.median(rel))
    out = _check(results, data, stab_thres=thr)
    assert out is not results and out["output_f"] is results["output_f"]          # F / S / G untouched
    for key in ("row_clusters", "col_clusters", "output_f"):                       # caller's dict not mutated
        assert all(np.array_equal(a, b) for a, b in zip(results[key], before[key]))
    for i in range(2):
        drop = rel[i] < thr
        assert drop.any() and (~drop).any()
        for key in ("row_clusters", "col_clusters"):
            assert np.array_equal(out[key][i][:, drop], np.zeros_like(out[key][i][:, drop]))
            assert np.array_equal(out[key][i][:, ~drop], results[key][i][:, ~drop])
    assert np.array_equal(_check(results, data, stab_thres=0.0)["row_clusters"][0], results["row_clusters"][0])


def test_results_returned_unchanged():
    results, data = fake_results()
    with pytest.warns(UserWarning, match="sparsity"):
        assert _check(results, data, repeat_runner=fake_runner(2, 4, fail_at=3)) is results
    empty = dict(results, row_clusters=[np.zeros_like(a) for a in results["row_clusters"]])
    with pytest.warns(UserWarning, match="No biclusters detected"):
        assert _check(empty, data) is empty
    no_clusts = {key: results[key] for key in ("output_f", "output_s", "output_g")}
    with pytest.warns(UserWarning, match="No biclusters detected"):
        assert _check(no_clusts, data) is no_clusts
    with pytest.warns(UserWarning, match="No biclusters detected"):      # spurious is not looked at then (R order)
        assert api.stability_check(data, no_clusts, 4, None, None, None, 20, True, 5, True, "euclidean") is no_clusts


def test_repeats_hook_exposes_the_repeats():
    results, data = fake_results()
    out = _check(results, data, return_repeats=True)
    reps = out["stability"]["repeats"]
    assert [r["tag"] for r in reps] == [f"stability={r}" for r in range(5)]
    assert np.array_equal(out["stability"]["relevance"], _sequential_mean(5))


def test_world_2_is_bitwise_world_1(tmp_path):
    results, data = fake_results()
    one_rel = _check(results, data, n_stability=7, remove_unstable=False)["relevance"]
    one = _check(results, data, n_stability=7)
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]
    out = str(tmp_path / "stability.pkl")
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "stability_worker.py"), "--rank", str(r),
                               "--world", "2", "--port", str(port), "--out", out], stdout=subprocess.PIPE,
                              stderr=subprocess.STDOUT, env=dict(os.environ, OMP_NUM_THREADS="2")) for r in range(2)]
    logs = [p.communicate(timeout=300)[0].decode(errors="replace") for p in procs]
    assert all(p.returncode == 0 for p in procs), "\n".join(logs)
    two = pickle.load(open(out, "rb"))
    assert np.array_equal(two["relevance"], one_rel) and two["relevance"].tobytes() == one_rel.tobytes()
    for key in ("row_clusters", "col_clusters"):
        assert all(np.array_equal(a, b) for a, b in zip(two[key], one[key]))


def test_argument_refusals():
    import resnmtf_amd
    x = [np.abs(np.random.default_rng(0).standard_normal((12, 9)))]
    for bad in (0.0, -0.1, 1.5):
        with pytest.raises(ValueError, match="sample_rate"):
            resnmtf_amd.apply_resnmtf(x, k_val=3, spurious=False, sample_rate=bad)
    for bad in (-0.01, 1.01):
        with pytest.raises(ValueError, match="stab_thres"):
            resnmtf_amd.apply_resnmtf(x, k_val=3, spurious=False, stab_thres=bad)
    with pytest.raises(ValueError, match="sample_rate"):
        resnmtf_amd.apply_resnmtf(x, k_val=3, spurious=False, sample_rate="0.5")
    with pytest.raises(NotImplementedError, match="stability"):
        resnmtf_amd.apply_resnmtf(x, k_val=3, spurious=True)
    results, data = fake_results()
    with pytest.raises(NotImplementedError, match="stability"):
        api.stability_check(data, results, 4, None, None, None, 20, True, 5, False, "euclidean",
                            repeat_runner=fake_runner(2, 4))
    with pytest.raises(ValueError, match="stab_thres"):
        _check(results, data, stab_thres=2.0)
    with pytest.raises(ValueError, match="sample_rate"):
        _check(results, data, sample_rate=0.0)


def test_null_handle_refused_by_the_abi():
    """The new entry points refuse a NULL handle without touching a device (no GPU needed)."""
    from resnmtf_amd import _lib
    lib = _lib.load()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert lib.resnmtf_set_reference_clusters(None, 0, 3, None, None) == 1
        assert lib.resnmtf_relevance(None, 0, None, 0, None, None, None) == 1
