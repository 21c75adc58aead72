"""The host references of the view routes and of finalise (tests/data_ref.py) without a GPU: each reference is the
oracle's own arithmetic, and each statistic separates the bugs it exists to catch -- by MUTANT_MARGIN times its bar, or
by a failed equality where the check is exact."""
import numpy as np
import pytest

import data_ref as D
from oracle import resnmtf_oracle as O
from sweep_ref import half_image
from test_gpu_sweep_elementwise import MUTANT_MARGIN

GUARD = 3.0e-5              # kHalfGuard of resnmtf_hip.hip: the x_half = 3 guard on the 16-bit image's relative error


# ---------------------------------------------------------------------------------------------------------------------
# upload image
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", D.SHAPE_CASES[:12], ids=D.shape_id)
def test_image_mutants_fail_the_equality(case):
    n, m, _ = case
    for x in (D.distinct(n, m), D.positive(n, m, 1) + 1e-3):
        img = D.upload_image(x)
        assert img.dtype == np.float64 and np.array_equal(img.astype(np.float32).astype(np.float64), img)
        for name, bad in D.image_mutants(img).items():
            assert not np.array_equal(bad, img), f"{name} is invisible at {n} x {m}"
    assert not np.array_equal(D.upload_image(D.positive(n, m, 1)), D.positive(n, m, 1))      # (the rounding is real)


# ---------------------------------------------------------------------------------------------------------------------
# raw upload
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", D.SHAPE_CASES[:12], ids=D.shape_id)
def test_raw_reference_is_the_oracle_and_separates_its_mutants(case):
    n, m, _ = case
    x = D.mixed_raw(n, m, 100 + n)
    ref32, ref64, neg = D.raw_reference(x)
    want = O.matrix_normalisation(O.make_non_neg(x))
    assert neg and D.nan_stat(ref64, want)[0] <= n * 2.0 ** -52 and D.nan_stat(ref64, want)[1:] == (0, 0)
    assert D.nan_stat(ref32, ref64)[0] <= 2.0 ** -24                    # (the image is the fp64 quotient rounded once)
    assert np.all(ref32.min(axis=0)[(x < 0).any(axis=0)] == 0.0)        # the minimum of a shifted column is exactly 0
    kinds = D.column_kinds(x)
    assert kinds["negative"] >= 1 and kinds["last row only"] >= 1
    if m >= 4:
        assert kinds["non-negative"] >= 1
    if n > 256:
        assert kinds["beyond row 256 only"] >= 1

    def stat(**mutant):
        worst, nz, nan = D.nan_stat(D.raw_reference(x, **mutant)[0], ref32)
        return np.inf if nz or nan else worst
    assert stat() == 0.0
    assert stat(shift=False) >= MUTANT_MARGIN * D.RAW_BAR
    assert stat(sum_before_shift=True) >= MUTANT_MARGIN * D.RAW_BAR
    if n > 256:
        assert stat(sum_rows=256) >= MUTANT_MARGIN * D.RAW_BAR
    # a shift taken from the first 256 rows only: the column that is negative beyond them keeps its negative entry
    if n > 256:
        y = x.copy(); y[256:] = np.maximum(y[256:], 0.0)
        short = (x + (O.make_non_neg(y) - y)[:1]) / D.fsum_cols(O.make_non_neg(x))[None, :]
        assert D.nan_stat(short.astype(np.float32), ref32)[0] >= MUTANT_MARGIN * D.RAW_BAR


def test_raw_reference_constant_negative_column():
    x = D.mixed_raw(65, 129, 3, constant_negative=7)
    ref32, _, neg = D.raw_reference(x)
    assert neg and np.isnan(ref32[:, 7]).all() and np.isnan(ref32).sum() == 65
    got = ref32.copy(); got[:, 7] = 0.0
    assert D.nan_stat(got, ref32)[2] == 65                               # a zero column instead of NaN is a mismatch
    got = ref32.copy(); got[3, 8] = np.nan
    assert D.nan_stat(got, ref32)[0] == np.inf


def test_one_ulp_is_inside_the_raw_bar_and_two_are_not():
    ref = np.array([1.0, 1.0 + 2.0 ** -23, 2.0 - 2.0 ** -23, 3e-5], dtype=np.float32)
    up = np.nextafter(ref, np.float32(4.0))
    assert D.nan_stat(up, ref)[0] <= D.RAW_BAR and D.nan_stat(np.nextafter(ref, np.float32(0.0)), ref)[0] <= D.RAW_BAR
    assert D.nan_stat(np.nextafter(up, np.float32(4.0)), ref)[0] > D.RAW_BAR


# ---------------------------------------------------------------------------------------------------------------------
# shuffle
# ---------------------------------------------------------------------------------------------------------------------
def test_chi_square_condition():
    """50 uniform permutations of the 500 x 260 entries stay below the bar in both destination orders.  What does not
    mix in the device's own index (destination column-major, source row-major: the identity, a rotation, a swap of
    neighbours, a seed-dependent rotation) exceeds it in the device's order -- and would pass in the matrix's, where it
    looks like a transposition; what does not mix as a matrix (the identity, a rotation, a shuffle within rows) exceeds
    it in the matrix's order."""
    n, m = 500, 260
    count = n * m
    src = D.distinct(n, m)
    rng = np.random.default_rng(0)
    worst = 0.0
    for _ in range(50):
        worst = max(worst, *D.mixing_stats(D.device_draw(src, rng.permutation(count))).values())
    assert worst < D.CHI2_BAR
    assert 133.0 < D.CHI2_BAR < 133.5 and D.CHI2_DOF == 49
    i = np.arange(count)
    device_side = {"identity": i, "rotation": (i + 12345) % count, "neighbours swapped": i ^ 1,
                   "seed-dependent rotation": (i + 2 ** 63 % count + 1) % count}
    for name, pi in device_side.items():
        st = D.mixing_stats(D.device_draw(src, pi))
        assert st["F"] > MUTANT_MARGIN * D.CHI2_BAR, name
        assert st["C"] < D.CHI2_BAR, name                       # (the matrix's order alone would let it through)
        assert np.array_equal(D.recover_permutation(D.device_draw(src, pi)), pi)
    matrix_side = {"identity": src, "rotation": np.roll(src.ravel(), 12345).reshape(n, m),
                   "shuffle within rows": np.stack([r[rng.permutation(m)] for r in src])}
    for name, drawn in matrix_side.items():
        assert D.mixing_stats(drawn)["C"] > MUTANT_MARGIN * D.CHI2_BAR, name
    with pytest.raises(AssertionError):                                   # an entry drawn twice is no permutation
        bad = src.copy(); bad[0, 0] = bad[1, 1]
        D.recover_permutation(bad)


# ---------------------------------------------------------------------------------------------------------------------
# finalise
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", D.FINALISE_IDS)
def test_finalise_cases_are_what_they_claim(cid):
    """The constructed inputs do what their names say under the ORACLE, the threshold band holds exactly the entries a
    case puts there (none for the random inputs, at the seeds the GPU test uses), and every cluster mutant shows."""
    c = D.finalise_case(cid)
    n, m, k = c["n"], c["m"], c["k"]
    f, s, g, rc, cc = D.finalise_reference(c["F"], c["S"], c["G"])
    rel = D.relations_of(c["F"], c["S"], c["G"])
    for j, i in c["relations"].items():
        assert rel[j] == i
    assert int(D.threshold_band(f, n).sum()) == c["band"] and int(D.threshold_band(g, m).sum()) == 0
    assert 0 < rc.sum() < rc.size and 0 < cc.sum() < cc.size
    kind = c["kind"]
    if kind == "perm_diag":
        assert sorted(rel) == list(range(k)) and not np.any(rel == np.arange(k))
    if kind == "tie":
        (j, a), = c["relations"].items()
        assert np.count_nonzero(s[:, j] == s[:, j].max()) == 2 and a == np.flatnonzero(s[:, j] == s[:, j].max())[0]
        assert not np.array_equal(D.finalise_reference(c["F"], c["S"], c["G"], last_max=True)[3], rc)
    if kind == "zero_s_column":
        assert np.all(s[:, 5] == 0.0)
    if kind == "same_arg_max":
        assert np.array_equal(rc[:, 1], rc[:, 7]) and rc[:, 1].any()
    if kind == "equal_f_column":
        assert np.all(f[:, 6] == 1.0 / 64) and not rc[:, 10].any()
        assert D.finalise_reference(c["F"], c["S"], c["G"], ge=True)[3][:, 10].all()           # >= for >
    if kind == "equal_f_column_one_ulp":
        want = np.zeros(64); want[D.ULP_ROW] = 1.0
        assert np.array_equal(rc[:, 10], want) and np.count_nonzero(f[:, 6] == 1.0 / 64) == 63
    if kind == "zero_f_column":
        assert np.isnan(f[:, 4]).all() and np.isnan(f).sum() == n and np.all(s[:, 4] == 0.0) and not rc[:, 11].any()
    if kind in ("random", "perm_diag"):
        assert not np.array_equal(rel, np.arange(k))
        # relations applied to the column clusters instead of the row clusters
        mut = D.finalise_reference(c["F"], c["S"], c["G"], relations_on="cols")
        assert not np.array_equal(mut[3], rc) and not np.array_equal(mut[4], cc)
    # the bars: one ulp of fp64 is inside them, a wrong column sum (one term missing) is MUTANT_MARGIN outside
    F2 = c["F"].copy(); F2[n - 1, :] = 0.0
    f2 = D.finalise_reference(F2, c["S"], c["G"])[0]
    assert D.nan_stat(f2[:n - 1], f[:n - 1])[0] >= MUTANT_MARGIN * D.factor_bar(n)
    assert D.nan_stat(np.nextafter(f, 2.0), f)[0] <= D.factor_bar(n)
    assert D.factor_bar(n) == (2 * n + 2) * 2.0 ** -53 and D.s_bar(n, m) == (2 * n + 2 * m + 4) * 2.0 ** -53


def test_finalise_reference_is_the_oracle():
    c = D.finalise_case("random_257x300_k17")
    f, s, g, rc, cc = D.finalise_reference(c["F"], c["S"], c["G"])
    of, og, os_ = O.normalisation_check([c["F"]], [c["G"]], [c["S"]])
    orc, occ = O.binary_clusters(of, og, os_)
    for a, b in ((f, of[0]), (s, os_[0]), (g, og[0]), (rc, orc[0]), (cc, occ[0])):
        assert np.array_equal(a, b)
    np.testing.assert_allclose(f.sum(axis=0), 1.0, rtol=1e-13)


# ---------------------------------------------------------------------------------------------------------------------
# the x_half = 3 guard of the reused-handle cases (tests/test_gpu_view_routes.py)
# ---------------------------------------------------------------------------------------------------------------------
def test_guard_data_lies_on_both_sides():
    from test_gpu_view_routes import GUARD_SHAPE, guard_data
    ok, bad = guard_data()
    assert ok.shape == bad.shape == GUARD_SHAPE
    assert half_image(ok, True)[1] < GUARD / 2 and half_image(bad, True)[1] > 2 * GUARD
