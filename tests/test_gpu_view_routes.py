"""Every route a view takes onto the device, checked ENTRY BY ENTRY (host references: tests/data_ref.py).

The sweep tests take the image they read back as their truth, so nothing they assert can see a wrong image.  Here the
images themselves are pinned: the upload (both the X and the Xt image, bitwise), the raw upload against fp64 (one f32
ulp), the shuffle (a bijection for every count and seed, well mixed, independent of the destination), the sub-sample,
the empty-line masks, the 2-byte images and the first sweep after every route, and handles that are loaded twice.

Every bar is exact equality, ``data_ref.RAW_BAR`` (derived there) or ``ERR_BAR`` of the sweep test.  Measured on the
MI355X (the tests print each figure as ``MEASURED ...``):

* RAW_BAR = 2^-23 = 1.19e-7: worst 0 -- every raw upload and every normalised shuffle came out bitwise the
  reference's f32 image (the n 2^-52 freedom of the column sum moved no f32 rounding), largest case 1000 x 333.
* ERR_BAR = 5e-7 (absolute): worst 9.5e-9, normalised shuffle at 257 x 300, k = 32.
* CHI2_BAR = 133.3: worst 59.9 (destination in the device's order, seed 1) and 69.8 (in the matrix's, seed 2^64 - 1)
  over the four seeds, 500 x 260.
"""
import numpy as np
import pytest
import scipy.sparse as sp

import data_ref as D
from resnmtf_amd import synth
from resnmtf_amd.engine import Engine
from sweep_ref import half_image, step_reference
from test_gpu_sweep_elementwise import ERR_BAR, outliers, sparse_one

pytestmark = pytest.mark.gpu

SEEDS = [0, 1, 2 ** 63, 2 ** 64 - 1]
FACTOR_STATE = ("F", "S", "G", "lambda", "mu")


def eng(n, m, k=1, **opts):
    return Engine([n], [m], [k], **opts)


def measured(what, value):
    print(f"MEASURED {what}: {value:.3e}")


def x_image(e, n, m):
    """The X image (``X32``) of a dense view, read through the gather that streams it: an identity sub-sample into a
    second engine (whose own read-back is its Xt image, written by the direct half of the upload)."""
    with eng(n, m) as other:
        other.subsample_view_from(0, e, 0, np.arange(n), np.arange(m))
        return other.get_view(0)


def assert_raw(got, x, what):
    ref32, _, _ = D.raw_reference(x)
    worst, nz, nan = D.nan_stat(got, ref32)
    measured(what, worst)
    assert nan == 0, f"{what}: {nan} entries NaN on one side only"
    assert nz == 0, f"{what}: {nz} entries non-zero where the reference is exactly zero"
    assert worst <= D.RAW_BAR, f"{what}: max |got / ref - 1| = {worst:.3e} (bar {D.RAW_BAR:.3e})"


# ---------------------------------------------------------------------------------------------------------------------
# a. upload: both images, bitwise
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", D.SHAPE_CASES, ids=D.shape_id)
def test_upload_writes_both_images_bitwise(case):
    n, m, flat = case
    for x in (D.positive(n, m, n + m), D.distinct(n, m)):
        want = D.upload_image(x)
        with eng(n, m, no_pitch_pad=flat) as e:
            e.set_view(0, x)
            assert np.array_equal(e.get_view(0), want), "the Xt image (direct store)"
            assert np.array_equal(x_image(e, n, m), want), "the X image (store through the LDS transpose)"


# ---------------------------------------------------------------------------------------------------------------------
# b. raw upload against fp64
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", D.SHAPE_CASES, ids=D.shape_id)
def test_raw_upload_matches_fp64(case):
    n, m, flat = case
    x = D.mixed_raw(n, m, 100 + n)
    with eng(n, m, no_pitch_pad=flat) as e:
        assert e.set_view_raw(0, x) is D.raw_reference(x)[2] is True
        got = e.get_view(0)
        assert_raw(got, x, f"raw upload {D.shape_id(case)}")
        assert np.array_equal(x_image(e, n, m), got), "the X and Xt images of a raw upload differ"
        assert e.set_view_raw(0, np.abs(x)) is D.raw_reference(np.abs(x))[2] is False
        assert_raw(e.get_view(0), np.abs(x), f"raw upload, non-negative {D.shape_id(case)}")
        # a constant negative column shifts to all zero: 0 / 0 = NaN there, every other column untouched
        xc = D.mixed_raw(n, m, 100 + n, constant_negative=m - 1)
        assert e.set_view_raw(0, xc) is True
        got = e.get_view(0)
        assert np.isnan(got[:, m - 1]).all()
        assert_raw(got, xc, f"raw upload, constant column {D.shape_id(case)}")


# ---------------------------------------------------------------------------------------------------------------------
# c. shuffle
# ---------------------------------------------------------------------------------------------------------------------
SHUFFLE_SHAPES = [(3, 2), (64, 32), (64, 64), (17, 241), (500, 260)]      # 6, 2 4^5, 4^6, 4^6 + 1, 130000 entries


@pytest.mark.parametrize("n,m", SHUFFLE_SHAPES, ids=[f"{n}x{m}" for n, m in SHUFFLE_SHAPES])
def test_shuffle_is_a_seeded_bijection(n, m):
    src = D.distinct(n, m)
    draws = []
    with eng(n, m) as base, eng(n, m) as e:
        base.set_view(0, src)
        for seed in SEEDS:
            e.shuffle_view_from(0, base, 0, seed=seed, normalise=False)
            d = e.get_view(0)
            assert np.array_equal(np.sort(d.ravel()), np.sort(src.ravel())), f"seed {seed}: not a bijection"
            e.set_view(0, np.zeros((n, m)))                      # (the second draw below does not read a stale image)
            e.shuffle_view_from(0, base, 0, seed=seed, normalise=False)
            assert np.array_equal(e.get_view(0), d), f"seed {seed}: the draw is not reproducible"
            draws.append(d)
    if n * m >= 2048:
        for i in range(len(SEEDS)):
            assert not np.array_equal(draws[i], src)
            for j in range(i):
                assert not np.array_equal(draws[i], draws[j]), f"seeds {SEEDS[j]} and {SEEDS[i]} give one draw"


@pytest.mark.parametrize("n,m", [(64, 64), (500, 260)])
def test_shuffle_is_independent_of_the_destination(n, m):
    src = D.distinct(n, m)
    k = 2
    with eng(n, m) as base, eng(n, m, k) as plain, eng(n, m, k, x_half=2) as half, eng(n, m, k, no_pitch_pad=True) as flat:
        base.set_view(0, src)
        for e in (plain, half, flat):
            e.shuffle_view_from(0, base, 0, seed=5, normalise=False)
        want = plain.get_view(0)
        assert half.view_plan(0)["image"] == "u16" and not flat.view_plan(0)["pitch_pad"]
        assert np.array_equal(half.get_view(0), want) and np.array_equal(flat.get_view(0), want)


@pytest.mark.parametrize("negative", [False, True], ids=["non_negative", "negative_entries"])
@pytest.mark.parametrize("n,m", [(17, 241), (500, 260)])
def test_normalised_shuffle_is_the_reference_of_its_draw(n, m, negative):
    """normalise = 1 is the raw route applied to the normalise = 0 draw of the same seed; with negative entries in the
    source (uploaded with set_view, f32 images) the shift is non-zero in nearly every column."""
    x = D.upload_image(D.mixed_raw(n, m, 7) if negative else np.abs(D.mixed_raw(n, m, 7)))
    with eng(n, m) as base, eng(n, m) as e:
        base.set_view(0, x)
        for seed in SEEDS[:2] if negative else SEEDS[2:]:
            e.shuffle_view_from(0, base, 0, seed=seed, normalise=False)
            draw = e.get_view(0)
            assert bool((draw < 0).any()) is negative
            e.shuffle_view_from(0, base, 0, seed=seed, normalise=True)
            got = e.get_view(0)
            assert_raw(got, draw, f"normalised shuffle {n}x{m} seed {seed}" + (" negative" if negative else ""))
            assert np.array_equal(x_image(e, n, m), got)


def test_shuffle_mixes():
    """The 8 x 8 table of source octile by destination octile of the recovered permutation is that of a uniform draw:
    chi-square below its 1 - 1e-9 quantile, with the destination indexed as the device does (column-major: the table of
    the kernel's own pi) AND as the matrix reads (row-major).  The identity, a rotation, a seed-dependent rotation and a
    swap of neighbours in the device's index, and the identity, a rotation and a shuffle within rows of the matrix, are
    far above it in one order or the other: tests/test_data_ref_host.py."""
    n, m = 500, 260
    with eng(n, m) as base, eng(n, m) as e:
        base.set_view(0, D.distinct(n, m))
        for seed in SEEDS:
            e.shuffle_view_from(0, base, 0, seed=seed, normalise=False)
            drawn = e.get_view(0)
            for order, stat in D.mixing_stats(drawn).items():
                measured(f"chi-square of the octile table, destination order {order}, seed {seed}", stat)
                assert stat < D.CHI2_BAR, f"seed {seed}, order {order}: chi-square {stat:.1f} (bar {D.CHI2_BAR:.1f})"
                perm = D.recover_permutation(drawn, order)
                assert np.mean(perm == np.arange(perm.size)) < 1e-3
                assert np.mean(np.abs(perm - np.arange(perm.size)) <= 1) < 1e-3      # (no entry next to where it was)


# ---------------------------------------------------------------------------------------------------------------------
# d. sub-sample
# ---------------------------------------------------------------------------------------------------------------------
def _subsample_cases():
    n, m = 65, 129
    rng = np.random.default_rng(3)
    yield "unsorted", rng.permutation(n)[:40], rng.permutation(m)[:33], False, False
    yield "last_row_last_column", np.array([n - 1]), np.array([m - 1]), False, False
    yield "one_row", np.array([n - 1]), np.arange(m), False, False            # (resnmtf_create accepts 1 x m and n x 1 at k = 1)
    yield "one_column", np.arange(n), np.array([m - 1]), False, False
    yield "repeated", rng.integers(0, n, 70), rng.integers(0, m, 140), False, False
    yield "flat_source", rng.permutation(n)[:64], rng.permutation(m)[:64], True, False
    yield "flat_destination", rng.permutation(n)[:64], rng.permutation(m)[:64], False, True


@pytest.mark.parametrize("name,rows,cols,flat_src,flat_dst", list(_subsample_cases()), ids=[c[0] for c in _subsample_cases()])
def test_subsample_gathers_exactly(name, rows, cols, flat_src, flat_dst):
    n, m = 65, 129
    with eng(n, m, no_pitch_pad=flat_src) as base, eng(len(rows), len(cols), no_pitch_pad=flat_dst) as e:
        base.set_view(0, D.distinct(n, m))
        assert base.view_plan(0)["pitch_pad"] == (not flat_src) and e.view_plan(0)["pitch_pad"] == (not flat_dst)
        e.subsample_view_from(0, base, 0, rows, cols)
        want = base.get_view(0)[np.ix_(rows, cols)]
        assert np.array_equal(e.get_view(0), want)
        assert np.array_equal(x_image(e, len(rows), len(cols)), want)


# ---------------------------------------------------------------------------------------------------------------------
# e. empty lines
# ---------------------------------------------------------------------------------------------------------------------
def empty_lines_raw(e):
    """(row mask, column mask, row count, column count) as resnmtf_view_empty_lines returns them."""
    rm, cm, nr, nc = e.empty_lines(0, counts=True)
    return rm.astype(np.uint8), cm.astype(np.uint8), nr, nc


def assert_empty_lines(e, what):
    got = e.get_view(0)
    rm, cm, nr, nc = empty_lines_raw(e)
    want_r, want_c = got.sum(axis=1) == 0, got.sum(axis=0) == 0
    assert np.array_equal(rm, want_r.astype(np.uint8)) and np.array_equal(cm, want_c.astype(np.uint8)), what
    assert (nr, nc) == (int(want_r.sum()), int(want_c.sum())), what
    return nr, nc


@pytest.mark.parametrize("n,m", [(63, 65), (257, 300), (300, 257)])
def test_empty_lines_after_shuffles_and_subsamples(n, m):
    rng = np.random.default_rng(n)
    x = D.positive(n, m, 5) * (rng.random((n, m)) < 0.03)              # 97 % zero
    x[:, 3] = 0.0; x[n - 1, :] = 0.0                                    # (an empty column and the last row empty in the source)
    seen = np.zeros(2, dtype=int)
    with eng(n, m) as base, eng(n, m) as e:
        base.set_view(0, x)
        for seed in SEEDS:
            e.shuffle_view_from(0, base, 0, seed=seed, normalise=False)
            seen += assert_empty_lines(e, f"shuffle, seed {seed}")
        e.subsample_view_from(0, base, 0, rng.permutation(n), rng.permutation(m))
        assert assert_empty_lines(e, "permuting sub-sample") == (int((x.sum(1) == 0).sum()), int((x.sum(0) == 0).sum()))
        e.set_view(0, x)                                                # a host upload clears them, empty lines or not
        rm, cm, nr, nc = empty_lines_raw(e)
        assert not rm.any() and not cm.any() and (nr, nc) == (0, 0)
    # narrow sub-samples: many empty lines, and the last line among them
    for rows, cols in ((rng.permutation(n)[:40], np.arange(m)), (np.arange(n), rng.permutation(m)[:40]),
                       (np.r_[rng.permutation(n - 1)[:30], n - 1], np.r_[rng.permutation(m)[:30], 3])):
        with eng(n, m) as base, eng(len(rows), len(cols)) as e:
            base.set_view(0, x)
            e.subsample_view_from(0, base, 0, rows, cols)
            nr, nc = assert_empty_lines(e, "narrow sub-sample")
            assert 0 < nr + nc < len(rows) + len(cols)
            seen += (nr, nc)
    assert seen.min() > 0


# ---------------------------------------------------------------------------------------------------------------------
# f. the norm and the first sweep after every route
# ---------------------------------------------------------------------------------------------------------------------
ROUTE_SHAPE = (257, 300)
SOURCE_SHAPE = (300, 340)                  # of the sub-samples
SWEEP_FORMS = [(8, 0, "f32"), (8, 1, "fp16"), (8, 2, "u16"), (32, 0, "f32")]


def route_source(route):
    """f32-exact data (so that a copied ||X||^2 is the one a fresh upload of the read-back computes)."""
    n, m = SOURCE_SHAPE if route == "subsample" else ROUTE_SHAPE
    return D.upload_image(synth.planted_view(n, m, 4, 11))


def take_route(e, base, route):
    n, m = ROUTE_SHAPE
    if route == "copy":
        e.copy_view_from(0, base, 0)
    elif route == "shuffle":
        e.shuffle_view_from(0, base, 0, seed=3, normalise=False)
    else:
        rng = np.random.default_rng(8)
        e.subsample_view_from(0, base, 0, rng.permutation(SOURCE_SHAPE[0])[:n], rng.permutation(SOURCE_SHAPE[1])[:m])


def one_sweep(e):
    err = e.run(1)
    return (err,) + tuple(e.get_factors(0))


def assert_same_sweep(got, want, what):
    assert np.array_equal(got[0], want[0]), f"{what}: error {got[0]!r} against {want[0]!r}"
    for name, a, b in zip(FACTOR_STATE, got[1:], want[1:]):
        assert np.array_equal(a, b), f"{what}: {name} differs in {np.count_nonzero(a != b)} entries"


@pytest.mark.parametrize("route", ["copy", "shuffle", "subsample"])
@pytest.mark.parametrize("k,x_half,image", SWEEP_FORMS, ids=[f"k{k}_half{h}" for k, h, _ in SWEEP_FORMS])
def test_first_sweep_after_a_route_is_a_fresh_upload_bitwise(route, k, x_half, image):
    n, m = ROUTE_SHAPE
    f0, s0, g0 = synth.random_init(n, m, k, 21)
    src = route_source(route)
    with eng(*src.shape) as base, eng(n, m, k, x_half=x_half) as e, eng(n, m, k, x_half=x_half) as fresh:
        base.set_view(0, src)
        take_route(e, base, route)
        back = e.get_view(0)
        e.set_factors(0, f0, s0, g0)
        got = one_sweep(e)
        fresh.set_view(0, back)
        fresh.set_factors(0, f0, s0, g0)
        want = one_sweep(fresh)
        assert e.view_plan(0)["image"] == fresh.view_plan(0)["image"] == image
        assert e.view_plan(0)["nt"] == (2 if k == 32 else 1)
        assert_same_sweep(got, want, f"{route}, k {k}, x_half {x_half}")
        assert np.isfinite(got[0]).all() and got[0][0] > 0


@pytest.mark.parametrize("route", ["raw", "normalised_shuffle"])
@pytest.mark.parametrize("k", [8, 32])
def test_first_sweep_error_after_a_normalising_route(route, k):
    """The device squares the fp64 quotient before rounding it: ||X||^2 is that of the fp64 pre-processed matrix, and
    the sweep's error is the reference's on it (sweep_ref.step_reference with data=), under the sweep test's ERR_BAR."""
    n, m = ROUTE_SHAPE
    f0, s0, g0 = synth.random_init(n, m, k, 22)
    x = D.upload_image(D.mixed_raw(n, m, 9))
    names = ([[f"row_{i}" for i in range(n)]], [[f"col_{j}" for j in range(m)]])
    z = np.zeros((1, 1))
    with eng(n, m) as base, eng(n, m, k) as e:
        if route == "raw":
            staged = x
            assert e.set_view_raw(0, x) is True
        else:
            base.set_view(0, x)
            e.shuffle_view_from(0, base, 0, seed=4, normalise=False)
            staged = e.get_view(0)
            e.shuffle_view_from(0, base, 0, seed=4, normalise=True)
        image = e.get_view(0)
        e.set_factors(0, f0, s0, g0)
        before = e.get_factors(0)
        err = e.run(1)
        after = e.get_factors(0)
    data = D.preprocess64(staged)
    ref = step_reference([image], [before], [after], z, z, z, names[0], names[1], data=[data])
    d_err = abs(float(err[-1]) - float(ref["err"][0]))
    measured(f"first sweep's error after {route}, k {k}", d_err)
    assert d_err < ERR_BAR, f"error {err[-1]!r} against {ref['err'][0]!r}"


# ---------------------------------------------------------------------------------------------------------------------
# g. the 2-byte images after a route
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["copy", "shuffle", "subsample"])
@pytest.mark.parametrize("x_half", [1, 2, 3])
def test_half_image_error_after_a_route(route, x_half):
    n, m = ROUTE_SHAPE
    src = route_source(route)
    with eng(*src.shape) as base, eng(n, m, 8, x_half=x_half) as e:
        base.set_view(0, src)
        take_route(e, base, route)
        kind, rel = e.view_image_info(0)
        want = half_image(e.get_view(0), x_half >= 2)[1]
        assert kind == (1 if x_half == 1 else 2)
        assert rel == pytest.approx(want, rel=1e-12, abs=0), f"2-byte image error after {route}"
        assert rel > 0


# ---------------------------------------------------------------------------------------------------------------------
# h. handles that are loaded twice
# ---------------------------------------------------------------------------------------------------------------------
GUARD_SHAPE = (257, 300)
GUARD_K = 8


def guard_data():
    """(data whose 16-bit image passes the x_half = 3 guard, data whose image fails it), f32-exact; the host test
    checks both against the guard through sweep_ref.half_image."""
    n, m = GUARD_SHAPE
    return D.upload_image(synth.planted_view(n, m, 4, 31)), D.upload_image(outliers(n, m, GUARD_K, 61).data[0])


@pytest.mark.parametrize("again", [False, True], ids=["factors_kept", "set_factors_again"])
@pytest.mark.parametrize("order", ["pass_then_fail", "fail_then_pass"])
def test_reused_guarded_handle_is_a_fresh_handle_bitwise(order, again):
    """x_half = 3: a second load into one handle that flips the guard re-writes the f32 factor operand copies in the
    other image's layout (build_half_images); the sweep after it is bitwise that of a fresh handle."""
    n, m = GUARD_SHAPE
    ok, bad = guard_data()
    first, second = (ok, bad) if order == "pass_then_fail" else (bad, ok)
    images = ("u16", "f32") if order == "pass_then_fail" else ("f32", "u16")
    f0, s0, g0 = synth.random_init(n, m, GUARD_K, 23)
    with eng(n, m) as base, eng(n, m, GUARD_K, x_half=3) as e, eng(n, m, GUARD_K, x_half=3) as fresh:
        base.set_view(0, second)
        e.set_view(0, first)
        e.set_factors(0, f0, s0, g0)
        e.run(3)
        assert e.view_plan(0)["image"] == images[0]
        e.copy_view_from(0, base, 0)                                 # (as the batched driver re-fills a handle)
        assert e.view_plan(0)["image"] == images[1], "the guard did not flip"
        if again:
            e.set_factors(0, f0, s0, g0)
        state = e.get_factors(0)
        got = one_sweep(e)
        fresh.set_view(0, second)
        fresh.set_factors(0, *state)
        want = one_sweep(fresh)
        assert e.view_plan(0)["image"] == fresh.view_plan(0)["image"] == images[1]
        assert_same_sweep(got, want, f"{order}, {'set_factors again' if again else 'factors kept'}")


def test_reused_sparse_handle_is_a_fresh_handle_bitwise():
    """A second upload into a sparse handle with another nnz and another skew: the work-block lists are re-planned and
    re-allocated (view_plan's sparse_blocks differ); the sweep after it is bitwise that of a fresh handle."""
    n, m, k = 600, 400, 8
    a = sp.csc_matrix(sparse_one(n, m, k, 0.05, 70).data[0])
    b = sp.csc_matrix(sparse_one(n, m, k, 0.01, 71, skew=True).data[0])
    cap = max(a.nnz, b.nnz)
    assert a.nnz != b.nnz
    f0, s0, g0 = synth.random_init(n, m, k, 24)
    with eng(n, m, k, nnz=[cap]) as e, eng(n, m, k, nnz=[cap]) as fresh:
        e.set_view_sparse(0, a, pre_processed=True)
        e.set_factors(0, f0, s0, g0)
        e.run(3)
        blocks_a = e.view_plan(0)["sparse_blocks"]
        e.set_view_sparse(0, b, pre_processed=True)
        state = e.get_factors(0)
        got = one_sweep(e)
        blocks_b = e.view_plan(0)["sparse_blocks"]
        assert blocks_a[0] != blocks_b[0] and blocks_a[1] != blocks_b[1], (blocks_a, blocks_b)
        fresh.set_view_sparse(0, b, pre_processed=True)
        fresh.set_factors(0, *state)
        want = one_sweep(fresh)
        assert fresh.view_plan(0)["sparse_blocks"] == blocks_b
        assert_same_sweep(got, want, "second sparse upload")
