"""CPU conditions of the JSD stage pool (tests/jsd_cases.py): from the NumPy restatement alone, every column still reaches
the branch of csrc/resnmtf_jsd.hip.inc it is in the pool for, so an edit of the pool cannot silently lose coverage; and
the stage references (jsd_ref.column_stats / pair_stages, jsd_cases.Reference) are jsd_calc's own numbers, bit for bit."""
import numpy as np
import pytest

import jsd_cases as K
import jsd_ref as J

IX = {name: i for i, name in enumerate(K.NAMES)}


def _jsd_calc_as_written(x1, x2):
    """jsd_calc (R/utils.r:95-106) in one piece, as jsd_ref had it before pair_stages was split off."""
    max_val = max(float(np.max(x1)), float(np.max(x2)))
    d1x, d1y = J.density(x1, 0.0, max_val)
    d2x, d2y = J.density(x2, 0.0, max_val)
    d1y[d1x > np.max(x1)] = 0.0
    d2y[d2x > np.max(x2)] = 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        return J.jsd(d1y, d2y)


def test_pool_shape_and_sizes():
    assert K.pool(17, 1).shape == (17, len(K.NAMES)) and len(K.NAMES) == 14
    assert np.array_equal(K.pool(17, 1), K.pool(17, 1))
    assert any((n - 1) % 4 == 0 for n in K.SIZES) and any((n - 1) % 4 != 0 for n in K.SIZES)
    for n in (K.TILE, K.TILE + 1, 2 * K.TILE, 2 * K.TILE + 1, 3 * K.TILE + 1, 4 * K.TILE + 1, 1024, 1025):
        assert n in K.SIZES
    c = K.pool(1000, 3)
    assert np.all(np.isfinite(c))
    assert np.all(np.diff(c[:, IX["ascending"]]) >= 0) and np.all(np.diff(c[:, IX["descending"]]) <= 0)
    nz = c[:, IX["neg_zero"]]
    assert np.sum(np.signbit(nz) & (nz == 0)) == 500
    assert np.all(c[:, IX["all_negative"]] < 0)
    assert len(np.unique(c[:, IX["few_levels"]])) == 7
    assert np.sum(c[:, IX["iqr0"]] == 0.25) >= 800 and np.sum(c[:, IX["mostly_zero"]] == 0.0) >= 850
    assert np.sum(c[:, IX["outlier"]] == 1.0) == 1 and np.sort(c[:, IX["outlier"]])[-2] < 1e-3


@pytest.mark.parametrize("n", K.SIZES)
def test_bandwidth_branches(n):
    c = K.pool(n, n)
    for name in ("const", "zeros"):                             # sd exactly 0: abs(x[1]), then 1
        assert J.sd(c[:, IX[name]]) == 0.0
    if n >= 513:
        for name in ("iqr0", "mostly_zero"):                    # IQR exactly 0, sd > 0: lo = sd
            iqr, sd = K.iqr_and_sd(c[:, IX[name]])
            assert iqr == 0.0 and sd > 0.0
            assert J.bw_nrd0(c[:, IX[name]]) == 0.9 * sd * n ** -0.2
        iqr, sd = K.iqr_and_sd(c[:, IX["flike"]])              # the main branch, both ways: the IQR term is the minimum
        assert 0.0 < iqr / 1.34 < sd
        iqr, sd = K.iqr_and_sd(c[:, IX["uniform"]])            # ... and sd is
        assert 0.0 < sd < iqr / 1.34


@pytest.mark.parametrize("n", [n for n in K.SIZES if n >= 2049] + [K.LARGE_N])
def test_signed_reaches_key_minus_one_the_low_clamp_and_bin_zero(n):
    c = K.pool(n, n)
    s = c[:, IX["signed"]]
    keys = J.bin_keys(s, max(float(s.max()), float(c[:, IX["uniform"]].max())))
    assert np.sum(keys == -1) >= 1 and np.sum(keys < -1) >= 1 and np.sum(keys == 0) >= 1
    assert keys.max() <= 510


@pytest.mark.parametrize("n", [10_000, K.LARGE_N])
def test_outlier_reaches_key_510(n):
    c = K.pool(n, n)
    o = c[:, IX["outlier"]]
    keys = J.bin_keys(o, float(o.max()))
    assert keys.max() == 510 and np.sum(keys == 510) == 1        # (511 is out of any input's reach: x <= M < up)


def test_few_levels_runs_cover_whole_chunks():
    for n, cols in ((8193, K.reference(8193).cols[:, IX["few_levels"]]), (K.LARGE_N, K.pool(K.LARGE_N, K.LARGE_N)[:, IX["few_levels"]])):
        keys = np.sort(J.bin_keys(cols, float(cols.max())))
        runs = K.whole_chunk_runs(keys)
        assert len(runs) == 7 and max(runs.values()) >= 3
        L = -(-n // K.N_BINS)
        starts = np.flatnonzero(np.diff(keys)) + 1                # where a key's run begins: both on and inside chunk edges
        assert np.any(starts % L != 0)
    keys = np.repeat(np.arange(4), [1024, 2048, 1000, 1048])       # n = 5120, L = 10: runs on chunk edges and inside
    assert K.whole_chunk_runs(keys) == {0: 102, 1: 204, 2: 99, 3: 104}


@pytest.mark.parametrize("n", K.SIZES)
def test_nan_pairs_are_those_of_all_negative(n):
    """A pair of all_negative with any other column is NaN: that column's maximum puts every output coordinate beyond
    max(all_negative), the whole density is zeroed and 0 / 0 follows.  No other pair is NaN.  Its self-pair has a
    negative M: only the last coordinate (M itself) survives the zeroing, so the restatement gives NaN when approx puts
    M outside the binning grid or the density there is 0, and exactly 0 otherwise; the device must give the same."""
    r = K.reference(n)
    an = IX["all_negative"]
    nan = np.isnan(r.val)
    for (a, b), v, is_nan in zip(r.pairs, r.val, nan):
        if (a == an) != (b == an):
            assert is_nan
        elif a == an:
            assert is_nan or v == 0.0
        else:
            assert not is_nan and -1e-15 <= v <= 1.0
            if a == b:
                assert v == 0.0
    assert 26 <= int(nan.sum()) <= 27
    assert np.all(np.isfinite(r.dens[~nan]))


def test_large_case_is_finite_and_in_range():
    r = K.large_reference()
    assert r.cols.shape == (K.LARGE_N, 5) and len(r.pairs) == 25
    assert np.all(r.val >= -1e-15) and np.all(r.val <= 1.0)
    assert -(-K.LARGE_N // K.TILE) == 49 and -(-K.LARGE_N // K.N_BINS) == 196


def test_stage_references_are_jsd_calc_bitwise():
    n = 513
    r = K.reference(n)
    for c in range(len(K.NAMES)):
        s, bw, mx = J.column_stats(r.cols[:, c])
        assert s.tobytes() == (np.sort(r.cols[:, c]) + 0.0).tobytes() and not np.any(np.signbit(s) & (s == 0))
        assert bw == J.bw_nrd0(r.cols[:, c]) and mx == r.cols[:, c].max()
        assert r.sorted[:, c].tobytes() == s.tobytes() and r.bw[c] == bw and r.mx[c] == mx
    for p, (a, b) in enumerate(r.pairs):
        x1, x2 = r.cols[:, a], r.cols[:, b]
        d1, d2, v = J.pair_stages(x1, x2)
        want = _jsd_calc_as_written(x1, x2)
        got = J.jsd_calc(x1, x2)
        for val in (v, got, r.val[p]):
            assert np.array([val]).tobytes() == np.array([want]).tobytes() or (np.isnan(val) and np.isnan(want))
        assert r.dens[p, 0].tobytes() == d1.tobytes() and r.dens[p, 1].tobytes() == d2.tobytes()
        with np.errstate(divide="ignore", invalid="ignore"):
            again = J.jsd(d1, d2)
        assert np.array([again]).tobytes() == np.array([want]).tobytes() or (np.isnan(again) and np.isnan(want))
