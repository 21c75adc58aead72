"""GPU tests of spurious-bicluster scoring: resnmtf_jsd_pairs against the fp64 NumPy restatement (tests/jsd_ref.py),
its determinism and host refusals, check_biclusters / remove_spurious on real shuffled factorisations, and the
reference's "resnmtf runs without stability with spurious removal" test (test-resnmtf.R:63-72) as a post-step."""
import ctypes as C

import numpy as np
import pytest

import jsd_ref as J
import resnmtf_amd
from resnmtf_amd import _lib, api, batched, naming, spurious
from resnmtf_amd.engine import jsd_pairs

pytestmark = pytest.mark.gpu

_WORST = {}
# Worst |device - restatement| measured on one MI355X times a margin of at most 8 [measured, case]; the sums run in another
# order than NumPy's, so the bars cannot be derived (tests/test_gpu_jsd_stages.py has the stages and a wider pool).
PAIRS_BAR = 1.9e-14        # the five-column pool, every ordered pair        [2.4e-15, n = 100 000; 1.1e-15 at 10 000, <= 7.8e-16 below]
GRID_BAR = 8.8e-16         # the same pool at n = 513                         [1.1e-16]
SCORE_BAR = 8.8e-16        # check_biclusters' score on the planted problem   [1.1e-16]
AVG_BAR = 2.7e-17          # ... its avg_threshold, a mean of 54 null scores  [3.5e-18]
# max_threshold is x[which.max(y)] of stats::density(null scores): while the arg max stays on its grid point, the
# coordinate follows the scores' minimum, maximum and bandwidth, and moves 1.3 x the perturbation of the scores (measured
# with the restatement: 54 scores moved by up to 1.4e-15 move the mode by up to 1.7e-15, by 1.7e-16 2.2e-16).  Null
# scores within SCORE_BAR therefore put it within 1.3 x SCORE_BAR; an arg max that jumped to a neighbouring point would
# be a grid step away (1e-4) and fail any bar.  Measured on the device: 6.9e-18.
MODE_BAR = 1.3 * SCORE_BAR


def _pool(n, seed):
    rng = np.random.default_rng(seed)
    f = rng.random(n) ** 6
    return np.stack([rng.random(n), f / f.sum(), np.full(n, 0.37), np.zeros(n), rng.random(n) ** 2 * 3.0], axis=1)


@pytest.mark.parametrize("n", [2, 3, 511, 512, 513, 10_000, 100_000])
def test_jsd_pairs_matches_restatement(n):
    cols = _pool(n, n)
    C_ = cols.shape[1]
    pairs = np.array([(a, b) for a in range(C_) for b in range(C_)], dtype=np.int32)
    got = jsd_pairs(cols, pairs)
    want = np.array([J.jsd_calc(cols[:, a], cols[:, b]) for a, b in pairs])
    diff = float(np.max(np.abs(got - want)))
    _WORST[n] = diff
    print(f"n={n}: worst |device - restatement| = {diff:.3e}")
    assert diff <= PAIRS_BAR
    for (a, b), v in zip(pairs, got):
        if a == b:
            assert v == 0.0
    assert np.all(got >= -1e-15) and np.all(got <= 1.0)


def test_jsd_pairs_is_bitwise_reproducible():
    rng = np.random.default_rng(4)
    n = 10_000
    f = rng.random((n, 12)) ** 6
    cols = f / f.sum(axis=0)
    pairs = np.array([(a, b) for a in range(12) for b in range(12)], dtype=np.int32)
    a = jsd_pairs(cols, pairs)
    b = jsd_pairs(cols, pairs)
    assert a.tobytes() == b.tobytes()
    perm = rng.permutation(len(pairs))
    c = jsd_pairs(cols, pairs[perm])
    assert c.tobytes() == a[perm].tobytes()
    parts = np.concatenate([jsd_pairs(cols, pairs[s:s + 37]) for s in range(0, len(pairs), 37)])
    assert parts.tobytes() == a.tobytes()
    sub = jsd_pairs(cols[:, [3, 7]], np.array([[0, 1], [1, 0]], dtype=np.int32))   # a pair's value needs its columns only
    assert sub.tobytes() == a[[3 * 12 + 7, 7 * 12 + 3]].tobytes()


def test_jsd_pairs_second_grid():
    """enqueue_jsd launches the pairs in grids of at most 2^20 workgroups and offsets ``pairs`` and ``out`` for the next:
    2^20 + 37 pairs (the 25 distinct ones of five columns, shuffled) reach the second grid, and every output is bitwise
    the value a 25-pair call gives for its pair."""
    n = 513
    cols = _pool(n, n)
    C_ = cols.shape[1]
    pairs = np.array([(a, b) for a in range(C_) for b in range(C_)], dtype=np.int32)
    base = jsd_pairs(cols, pairs)
    want = np.array([J.jsd_calc(cols[:, a], cols[:, b]) for a, b in pairs])
    diff = float(np.max(np.abs(base - want)))
    print(f"second grid, n={n}: worst |device - restatement| = {diff:.3e}")
    assert diff <= GRID_BAR
    total = (1 << 20) + 37
    pick = np.random.default_rng(513).permutation(np.arange(total) % len(pairs))
    assert len(set(pick[1 << 20:])) > 1 and len(set(pick[:1 << 20])) == len(pairs)
    got = jsd_pairs(cols, pairs[pick])
    assert got.shape == (total,)
    assert got.tobytes() == base[pick].tobytes()


def test_jsd_pairs_host_refusals():
    lib = _lib.load()
    dp = C.POINTER(C.c_double); ip = C.POINTER(C.c_int)
    cols = np.asfortranarray(np.random.default_rng(0).random((8, 3)))
    pairs = np.array([0, 1, 2, 2], dtype=np.int32)
    out = np.full(2, -7.0)

    def call(n=8, nc=3, c=cols, np_=2, p=pairs, o=out):
        return lib.resnmtf_jsd_pairs(0, n, nc, None if c is None else c.ctypes.data_as(dp), np_,
                                     None if p is None else p.ctypes.data_as(ip), None if o is None else o.ctypes.data_as(dp))

    assert call(n=1) == 1
    assert call(nc=0) == 1
    assert call(np_=-1) == 1
    assert call(c=None) == 1 and call(p=None) == 1 and call(o=None) == 1
    bad = cols.copy(order="F"); bad[5, 2] = np.nan
    assert call(c=bad) == 1 and b"non-finite" in lib.resnmtf_last_error(None)
    bad[5, 2] = np.inf
    assert call(c=bad) == 1
    assert call(p=np.array([0, 3, 0, 0], dtype=np.int32)) == 1 and b"out of range" in lib.resnmtf_last_error(None)
    assert call(p=np.array([-1, 0, 0, 0], dtype=np.int32)) == 1
    assert call(np_=0) == 0
    assert np.all(out == -7.0)                                  # nothing was written: no launch
    assert call() == 0 and out[1] == 0.0
    with pytest.raises(_lib.ResnmtfError):
        jsd_pairs(np.ones((1, 2)), [[0, 1]])


def planted(seed):
    """test-resnmtf.R:38-52: three 60 x 60 blocks of height 10 + 0.1 |N(0, 1)|."""
    rng = np.random.default_rng(seed)
    rc = np.kron(np.eye(3), np.ones((60, 1))); cc = np.kron(np.eye(3), np.ones((60, 1)))
    x = rc @ np.diag([10.0, 10.0, 10.0]) @ cc.T + 0.1 * np.abs(rng.normal(size=(180, 180)))
    return x, rc, cc


def _planted_run(seed=7):
    x1, rc, cc = planted(1)
    x2, _, _ = planted(2)
    res = resnmtf_amd.apply_resnmtf([x1, x2], k_val=3, spurious=False, stability=False, seed=seed)
    return naming.check_data([x1, x2]), res, rc, cc


def test_check_biclusters_matches_restatement_on_device_shuffles():
    data, res, _, _ = _planted_run()
    R = 4
    dev = batched.DeviceData(data, pre_processed=True)
    try:
        shuffled = [rep["output_f"] for rep in batched.shuffles_on_device(dev, 3, R, seed=5)]
    finally:
        dev.close()
    got = api.check_biclusters(data, res["output_f"], R, shuffled_f=shuffled)
    want = J.check_biclusters(res["output_f"], shuffled)
    for key in ("score", "avg_threshold", "max_threshold"):
        print(f"{key}: worst |device - restatement| = {float(np.max(np.abs(got[key] - want[key]))):.3e}")
    np.testing.assert_allclose(got["score"], want["score"], rtol=0, atol=SCORE_BAR)
    np.testing.assert_allclose(got["avg_threshold"], want["avg_threshold"], rtol=0, atol=AVG_BAR)
    np.testing.assert_allclose(got["max_threshold"], want["max_threshold"], rtol=0, atol=MODE_BAR)
    out = api.remove_spurious(data, res, R, shuffled_f=shuffled)
    _, _, masks = J.removal(res["row_clusters"], res["col_clusters"], res["output_s"], want)
    for i in range(2):
        rel = np.argmax(res["output_s"][i], axis=0)
        clear = np.abs(want["score"][i] - want["max_threshold"][i])[rel] > 1e-8
        assert np.array_equal(out["spurious"]["removed"][i][clear], masks[i][clear])


def test_reference_test_without_stability_with_spurious_removal():
    """test-resnmtf.R:63-72 as apply_resnmtf(spurious=False, stability=False) + remove_spurious; then also followed by
    stability_check (as apply_resnmtf with stability would run after the removal)."""
    data, res, rc, cc = _planted_run()
    out = api.remove_spurious(data, res, 5, seed=3)
    assert len(out["output_f"]) == 2
    assert out["output_f"][0].shape == (180, 3)
    for v in (1, 0):
        assert sorted(out["row_clusters"][v].sum(0)) == sorted(rc.sum(0))
        assert sorted(out["col_clusters"][v].sum(0)) == sorted(cc.sum(0))
    assert not out["spurious"]["removed"].any()
    n_v = 2
    z = np.zeros((n_v, n_v))
    st = api.stability_check(data, out, [3, 3], z, z, z, None, False, 5, False, "euclidean", seed=11)
    for v in (1, 0):
        assert sorted(st["row_clusters"][v].sum(0)) == sorted(rc.sum(0))
        assert sorted(st["col_clusters"][v].sum(0)) == sorted(cc.sum(0))


def test_same_seed_same_bits_end_to_end():
    data, res, _, _ = _planted_run()
    a = api.remove_spurious(data, res, 3, seed=21)
    b = api.remove_spurious(data, res, 3, seed=21)
    for key in ("score", "avg_threshold", "max_threshold", "removed"):
        assert np.asarray(a["spurious"][key]).tobytes() == np.asarray(b["spurious"][key]).tobytes()
    for v in range(2):
        assert a["row_clusters"][v].tobytes() == b["row_clusters"][v].tobytes()
