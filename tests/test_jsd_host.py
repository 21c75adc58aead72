"""CPU tests of spurious-bicluster scoring (R/obtain_bicl.r:55-188, R/utils.r:95-106): the NumPy restatement's pieces
against independent forms, the package's density mode, resnmtf_amd.spurious' pair order, relations mapping and removal
rule with stand-in scores, and the refusals -- the new ones and the pinned ones, which stay as they were."""
import numpy as np
import pytest
import scipy.sparse
import scipy.stats

import jsd_ref as J
import resnmtf_amd
from resnmtf_amd import spurious


def _flike(rng, n, k):
    f = rng.random((n, k)) ** 6
    return f / f.sum(axis=0)


@pytest.mark.parametrize("n", [2, 3, 7, 100, 1001])
def test_quantiles_and_sd(n):
    rng = np.random.default_rng(n)
    for x in (rng.random(n), rng.random(n) ** 6, np.round(rng.random(n) * 3)):
        for p in (0.25, 0.75, 0.5, 0.0, 1.0):
            assert J.quantile7(x, p) == pytest.approx(float(np.quantile(x, p, method="linear")), rel=1e-15, abs=1e-300)
        assert J.sd(x) == pytest.approx(float(np.std(x, ddof=1)), rel=1e-13)


@pytest.mark.parametrize("seed", range(4))
def test_fft_form_equals_direct_toeplitz_sum(seed):
    rng = np.random.default_rng(seed)
    x = rng.random(500 + 300 * seed) ** (1 + 2 * seed)
    for frm, to in ((None, None), (0.0, float(x.max()))):
        a = J.density(x, frm, to)[1]
        b = J.density(x, frm, to, direct=True)[1]
        assert np.max(np.abs(a - b)) <= 1e-15 * max(1.0, float(np.max(np.abs(b))))


def test_bw_nrd0_fallbacks():
    n = 10
    assert J.bw_nrd0(np.full(n, 2.5)) == 0.9 * 2.5 * n ** -0.2                 # sd = IQR = 0: abs(x[1])
    assert J.bw_nrd0(np.zeros(n)) == 0.9 * 1.0 * n ** -0.2                     # ... and then 1
    x = np.zeros(n); x[-1] = 1.0                                               # IQR = 0, sd > 0: sd
    assert J.bw_nrd0(x) == pytest.approx(0.9 * np.std(x, ddof=1) * n ** -0.2, rel=1e-15)
    x = np.array([0.0, 0.0, 4.0])                                              # the fallback reads the first entry as given
    assert J.bw_nrd0(np.array([3.0, 3.0, 3.0])) == 0.9 * 3.0 * 3 ** -0.2
    assert J.bw_nrd0(x) > 0
    for x in (np.full(n, 2.5), np.zeros(n), np.arange(n, dtype=float)):
        assert spurious.bw_nrd0(x) == pytest.approx(J.bw_nrd0(x), rel=1e-14)
    with pytest.raises(ValueError):
        J.bw_nrd0(np.ones(1))


def test_jsd_identity_symmetry_range():
    rng = np.random.default_rng(3)
    cols = [rng.random(300), _flike(rng, 300, 1)[:, 0], np.full(300, 0.5), np.zeros(300), rng.random(300) ** 3]
    for a in cols:
        assert J.jsd_calc(a, a) == 0.0
        for b in cols:
            v = J.jsd_calc(a, b)
            assert v == pytest.approx(J.jsd_calc(b, a), abs=1e-15)
            assert -1e-15 <= v <= 1.0


def test_density_matches_gaussian_kde():
    rng = np.random.default_rng(11)
    x = rng.standard_normal(100_000)
    bw = J.bw_nrd0(x)
    gx, gy = J.density(x)
    kde = scipy.stats.gaussian_kde(x, bw_method=bw / np.std(x, ddof=1))
    assert np.max(np.abs(gy - kde(gx))) < 1e-2


@pytest.mark.parametrize("seed", range(6))
def test_package_density_mode_equals_restatement(seed):
    rng = np.random.default_rng(seed)
    scores = rng.beta(2, 5 + seed, size=60 + 40 * seed) * 0.3
    if seed == 5:
        scores = np.concatenate([scores, np.full(20, 0.01)])
    x1, y1 = J.density(scores)
    x2, y2 = spurious.density(scores)
    np.testing.assert_allclose(x1, x2, rtol=1e-14, atol=1e-16)
    assert np.max(np.abs(y1 - y2)) <= 1e-12 * np.max(y1)
    assert spurious.density_mode(scores) == pytest.approx(J.density_mode(scores), rel=1e-14, abs=1e-16)


def _fake(rng, shapes, K, R):
    data = [rng.random(s) for s in shapes]
    out_f = [_flike(rng, s[0], K) for s in shapes]
    shuffled = [[_flike(rng, s[0], K) for s in shapes] for _ in range(R)]
    return data, out_f, shuffled


def test_pair_order_is_r_order():
    K, R = 3, 4
    null, score = spurious.pool_pairs(K, R)
    assert len(null) == K * K * R * (R - 1) // 2 and len(score) == K * R * K
    want = [(K + j * K + k, K + l * K + m) for j, k, l, m in J.null_pairs(K, R)]
    assert [tuple(p) for p in null] == want
    assert [tuple(p) for p in score] == [(k, K + y) for k in range(K) for y in range(R * K)]


def test_check_biclusters_with_stand_ins_equals_restatement():
    rng = np.random.default_rng(5)
    K, R = 2, 3
    data, out_f, shuffled = _fake(rng, [(60, 20), (60, 15)], K, R)
    got = spurious.check_biclusters(data, out_f, R, shuffled_f=shuffled,
                                    jsd=lambda cols, pairs: np.array([J.jsd_calc(cols[:, a], cols[:, b]) for a, b in pairs]))
    want = J.check_biclusters(out_f, shuffled)
    np.testing.assert_allclose(got["score"], want["score"], rtol=0, atol=1e-15)
    np.testing.assert_allclose(got["avg_threshold"], want["avg_threshold"], rtol=0, atol=1e-15)
    np.testing.assert_allclose(got["max_threshold"], want["max_threshold"], rtol=1e-14, atol=0)


def _results(rng, n, m, K, s):
    rc = (rng.random((n, K)) < 0.5).astype(float)
    cc = (rng.random((m, K)) < 0.5).astype(float)
    return {"output_f": [_flike(rng, n, K)], "output_s": [s], "output_g": [_flike(rng, m, K)],
            "row_clusters": [rc], "col_clusters": [cc]}


def test_remove_spurious_relations_and_zero_rule():
    """Crafted scores: null scores spread over 0.30-0.32, so the threshold lies in between; F column scores are read off
    a table by the F column index.  Column 0 scores above the threshold, column 1 below, column 2 exactly 0; S maps
    cluster j to F column relations[j] = (2, 0, 1)."""
    rng = np.random.default_rng(9)
    K, R, n, m = 3, 2, 40, 12
    data = [rng.random((n, m))]
    s = np.array([[0.0, 5.0, 0.0], [0.0, 0.0, 5.0], [5.0, 0.0, 0.0]])    # which.max per column: (2, 0, 1)
    res = _results(rng, n, m, K, s)
    shuffled = [[_flike(rng, n, K)] for _ in range(R)]
    table = {0: 0.9, 1: 0.01, 2: 0.0}
    seen = []

    def fake_jsd(cols, pairs):
        seen.append(np.array(pairs))
        null_n = K * K * R * (R - 1) // 2
        vals = [0.3 + 0.01 * (t % 3) for t in range(null_n)]
        vals += [table[int(a)] for a, _ in pairs[null_n:]]
        return np.array(vals)

    before = {k: [np.array(v) for v in res[k]] for k in ("row_clusters", "col_clusters", "output_f")}
    out = resnmtf_amd.remove_spurious(data, res, R, shuffled_f=shuffled, jsd=fake_jsd)
    for k, v in before.items():                                                     # the input is not modified
        for a, b in zip(v, res[k]):
            np.testing.assert_array_equal(a, b)
    null_p, score_p = spurious.pool_pairs(K, R)
    np.testing.assert_array_equal(seen[0], np.concatenate([null_p, score_p]))
    sp = out["spurious"]
    thr = sp["max_threshold"][0]
    assert 0.01 < thr < 0.9
    np.testing.assert_array_equal(sp["score"][0], [0.9, 0.01, 0.0])
    indices = np.array([False, True, True])
    relations = np.array([2, 0, 1])
    np.testing.assert_array_equal(sp["removed"][0], indices[relations])            # (True, False, True)
    for key in ("row_clusters", "col_clusters"):
        want = res[key][0].copy()
        want[:, indices[relations]] = 0.0
        np.testing.assert_array_equal(out[key][0], want)
    assert out["output_f"] is res["output_f"]
    rr, cc, masks = J.removal(res["row_clusters"], res["col_clusters"], res["output_s"], sp)
    np.testing.assert_array_equal(out["row_clusters"][0], rr[0])
    np.testing.assert_array_equal(masks, sp["removed"])


def test_refusals():
    rng = np.random.default_rng(2)
    data, out_f, shuffled = _fake(rng, [(30, 10)], 2, 3)
    stand_in = lambda cols, pairs: np.full(len(pairs), 0.1)   # noqa: E731
    for bad in (1, 0, 2.5, True):
        with pytest.raises(ValueError, match="num_repeats"):
            spurious.check_biclusters(data, out_f, bad, shuffled_f=shuffled, jsd=stand_in)
    with pytest.raises(NotImplementedError, match="sparse"):
        spurious.check_biclusters([scipy.sparse.csc_matrix(data[0])], out_f, 3, shuffled_f=shuffled, jsd=stand_in)
    bad_f = [out_f[0].copy()]
    bad_f[0][3, 1] = np.nan
    with pytest.raises(ValueError, match="non-finite"):
        spurious.check_biclusters(data, bad_f, 3, shuffled_f=shuffled, jsd=stand_in)
    bad_sh = [[f.copy() for f in fs] for fs in shuffled]
    bad_sh[1][0][0, 0] = np.inf
    with pytest.raises(ValueError, match="non-finite"):
        spurious.check_biclusters(data, out_f, 3, shuffled_f=bad_sh, jsd=stand_in)
    one = [[f[:, :1]] for f in [out_f[0], out_f[0]]]
    with pytest.raises(ValueError, match="single null score"):
        spurious.check_biclusters(data, [out_f[0][:, :1]], 2, shuffled_f=one, jsd=stand_in)
    with pytest.raises(ValueError, match="not finite"):
        spurious.check_biclusters(data, out_f, 3, shuffled_f=shuffled, jsd=lambda c, p: np.full(len(p), np.nan))
    with pytest.raises(ValueError, match="no_clusts"):
        resnmtf_amd.remove_spurious(data, {"output_f": out_f, "output_s": [np.eye(2)], "output_g": [np.ones((10, 2))]}, 3,
                                    shuffled_f=shuffled, jsd=stand_in)


def test_pinned_refusals_still_fire():
    x = [np.abs(np.random.default_rng(0).standard_normal((12, 9)))]
    with pytest.raises(NotImplementedError, match="spurious"):
        resnmtf_amd.res_nmtf_inner(x, None, None, k_vec=[3], spurious=True)
    with pytest.raises(NotImplementedError, match="spurious"):
        resnmtf_amd.apply_resnmtf(x, k_val=3, stability=False)
    with pytest.raises(NotImplementedError, match="stability"):
        resnmtf_amd.apply_resnmtf(x, k_val=3)
    from resnmtf_amd import api
    res = {"row_clusters": [np.ones((12, 3))], "col_clusters": [np.ones((9, 3))]}
    with pytest.raises(NotImplementedError, match="spurious"):
        api.stability_check(x, res, 3, None, None, None, None, True, 5, False, "euclidean")
