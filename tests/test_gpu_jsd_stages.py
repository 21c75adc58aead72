"""GPU tests of the JSD scoring kernels stage by stage (csrc/resnmtf_jsd.hip.inc through resnmtf_jsd_stages): the sort,
the per-column statistics, both sides' densities and the value, each against the fp64 NumPy restatement
(tests/jsd_ref.py) on the pool of tests/jsd_cases.py, at every tile, merge and chunk edge.  One jsd_stages call per size;
the cost of this file is the restatement on the CPU.  tests/test_jsd_cases_host.py shows that the pool reaches the
branches it is here for."""
import functools
import json
import os
from fractions import Fraction

import numpy as np
import pytest

import jsd_cases as K
import jsd_ref as J
from resnmtf_amd.engine import jsd_pairs, jsd_stages

pytestmark = pytest.mark.gpu

IX = {name: i for i, name in enumerate(K.NAMES)}
CASES = list(K.SIZES) + ["large"]

# Worst deviation from the restatement measured on one MI355X, times MARGIN [measured, case].  The sort and the zeros of
# the density are exact and have no bar.  The sums run in another order than NumPy's (fixed 256- / 512-lane trees, chunked
# bin sums, the direct Toeplitz sum against the FFT form), so these cannot be derived.  The density's deviation grows with
# n -- BinDist adds n weights one after the other in the restatement, the device by chunks -- so it has a bar per size.
MARGIN = 8.0
BW_WORST = 1.95e-15        # |bw - ref| / ref per column                       [few_levels, n = 100 000]
VAL_WORST = 1.89e-14       # |out - ref| per finite pair                       [neg_zero,outlier, n = 4097]
DENS_WORST = {             # max |dens - ref| / max(ref) per pair and side
    2: 3.07e-15,           # uniform,signed side 0
    3: 7.77e-16,           # flike,descending side 1
    511: 2.14e-15,         # descending,outlier side 0
    512: 6.39e-15,         # uniform,iqr0 side 1
    513: 1.20e-14,         # zeros,descending side 0
    1023: 2.76e-14,        # const,zeros side 1
    1024: 2.71e-14,        # const,few_levels side 0
    1025: 2.06e-14,        # const,zeros side 1
    2047: 5.52e-14,        # zeros,ascending side 0
    2048: 4.69e-14,        # zeros,few_levels side 0
    2049: 3.86e-14,        # zeros,iqr0 side 0
    4096: 8.04e-14,        # const,few_levels side 0
    4097: 9.39e-14,        # const,mostly_zero side 0
    6145: 1.28e-13,        # const,zeros side 1
    8193: 1.59e-13,        # const,few_levels side 0
    "large": 2.66e-13,     # flike,few_levels side 1
}
FFT_NOISE = 2.3e-15         # relative to the density's maximum: 1024-point transforms, eps log2(1024); 5.6e-17 on this pool
MEASURED = {}


def _names(case):
    return K.LARGE_NAMES if case == "large" else K.NAMES


def _ref(case):
    return K.large_reference() if case == "large" else K.reference(case)


@functools.lru_cache(maxsize=None)
def _got(case):
    r = _ref(case)
    return jsd_stages(r.cols, r.pairs)


@functools.lru_cache(maxsize=None)
def _direct_side(case, c, max_val):
    """One side's zeroed density from the restatement's direct Toeplitz sum (the form the kernel computes; it equals the
    FFT form to 1e-15 of the maximum, tests/test_jsd_host.py): a sum of non-negative products, so exactly 0 where the FFT
    form's inverse transform leaves noise of either sign."""
    x = _ref(case).cols[:, c]
    dx, dy = J.density(x, 0.0, max_val, direct=True)
    dy[dx > np.max(x)] = 0.0
    return dy


def _record(case, key, value, where):
    MEASURED.setdefault(str(case), {})[key] = [value, where]
    print(f"{case}: worst {key} = {value:.3e} ({where})")
    path = os.environ.get("RESNMTF_JSD_STAGES_OUT")
    if path:
        with open(path, "w") as f:
            json.dump(MEASURED, f, indent=1, sort_keys=True)


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


def _sums_exact(x):
    """True when every sum, quotient and square of the restatement's sd(x) is exact in fp64: the order of the sums and a
    fused multiply-add then change nothing, and the device's bandwidth must equal the restatement's bit for bit."""
    def exact(fr):
        return Fraction(float(fr)) == fr
    xs = [Fraction(float(v)) for v in x]
    n = len(xs)
    steps = [sum(xs[:i + 1]) for i in range(n)] + [sum(xs[i:]) for i in range(n)]
    m0 = sum(xs) / n
    steps += [m0] + [v - m0 for v in xs]
    m = m0 + sum(v - m0 for v in xs) / n
    d = [v - m for v in xs]
    steps += [m] + d + [v * v for v in d] + [sum(v * v for v in d[:i + 1]) for i in range(n)] + [sum(v * v for v in d) / (n - 1)]
    return all(exact(s) for s in steps)


def bw_deviation(case):
    """(worst relative deviation of the bandwidth, its column); the exact cases are asserted on the way."""
    r, g = _ref(case), _got(case)
    n = r.cols.shape[0]
    worst, where = 0.0, "-"
    for c, name in enumerate(_names(case)):
        bw = float(g["stats"][c, 0])
        if name == "const":
            assert bw == 0.9 * 0.37 * n ** -0.2, name
        elif name == "zeros":
            assert bw == 0.9 * 1.0 * n ** -0.2, name
        if n <= 3 and _sums_exact(r.cols[:, c]):
            assert bw == r.bw[c], f"{name}: exact sums, {bw!r} != {r.bw[c]!r}"
        dev = abs(bw - r.bw[c]) / r.bw[c]
        if dev > worst:
            worst, where = dev, name
    return worst, where


def dens_deviation(case):
    """(worst max |dens - ref| / max(ref) over the non-NaN pairs and both sides, its pair and side)."""
    r, g = _ref(case), _got(case)
    names = _names(case)
    worst, where = 0.0, "-"
    for p, (a, b) in enumerate(r.pairs):
        if np.isnan(r.val[p]):
            continue
        for s in range(2):
            dev = float(np.max(np.abs(g["dens"][p, s] - r.dens[p, s])) / np.max(r.dens[p, s]))
            if not dev <= worst:
                worst, where = dev, f"{names[a]},{names[b]} side {s}"
    return worst, where


def val_deviation(case):
    r, g = _ref(case), _got(case)
    names = _names(case)
    fin = ~np.isnan(r.val)
    d = np.abs(g["out"][fin] - r.val[fin])
    i = int(np.argmax(np.where(np.isnan(d), np.inf, d)))
    a, b = r.pairs[fin][i]
    return float(d[i]), f"{names[a]},{names[b]}"


@pytest.mark.parametrize("case", CASES)
def test_sort_is_exact(case):
    """Exact by definition: the sorted buffer is np.sort of the column with -0 as +0, bit for bit (hence a permutation
    of it), and the statistics' maximum is its last entry."""
    r, g = _ref(case), _got(case)
    for c, name in enumerate(_names(case)):
        s = g["sorted"][:, c]
        assert not np.any(np.signbit(s) & (s == 0)), f"{name}: a negative zero survived"
        assert _bits(s) == _bits(np.sort(r.cols[:, c]) + 0.0), f"{name}: first difference at {int(np.argmax(s != r.sorted[:, c]))}"
        assert _bits(g["stats"][c, 1]) == _bits(s[-1]) and g["stats"][c, 1] == r.mx[c], name


@pytest.mark.parametrize("case", CASES)
def test_bandwidth(case):
    r, g = _ref(case), _got(case)
    n = r.cols.shape[0]
    worst, where = bw_deviation(case)
    _record(case, "bw", worst, where)
    assert worst <= MARGIN * BW_WORST
    if "iqr0" in _names(case) and n >= 513:                      # IQR = 0, sd > 0: the sd branch, not the IQR's or abs(x[1])
        for name in ("iqr0", "mostly_zero"):
            c = IX[name]
            want = 0.9 * J.sd(r.cols[:, c]) * n ** -0.2
            assert want > 0 and abs(g["stats"][c, 0] - want) <= MARGIN * BW_WORST * want, name
            assert abs(g["stats"][c, 0] - 0.9 * abs(r.cols[0, c]) * n ** -0.2) > 1e-3 * want, name


@pytest.mark.parametrize("case", CASES)
def test_density(case):
    r, g = _ref(case), _got(case)
    names = _names(case)
    for p, (a, b) in enumerate(r.pairs):
        M = max(r.mx[a], r.mx[b])
        xout = J.seq_len_out(0.0, M, K.N_BINS)
        for s, c in enumerate((a, b)):
            d = g["dens"][p, s]
            beyond = xout > r.mx[c]
            assert not np.any(d[beyond] != 0.0) and not np.any(np.signbit(d[beyond])), f"{names[a]},{names[b]} side {s}: not zeroed"
            if not np.isnan(r.val[p]):
                assert np.all(np.isfinite(d))
                lost = (d == 0.0) & (r.dens[p, s] != 0.0)
                if np.any(lost):                                 # (the FFT form leaves rounding noise where every term underflows)
                    direct = _direct_side(case, int(c), float(M))
                    assert np.all(direct[lost] == 0.0) and np.all(r.dens[p, s][lost] <= FFT_NOISE * np.max(r.dens[p, s])), \
                        f"{names[a]},{names[b]} side {s}: a zero where the reference has mass"
                assert np.all(d >= 0.0)
            assert np.array_equal(np.isnan(d), np.isnan(r.dens[p, s])), f"{names[a]},{names[b]} side {s}: NaN positions"
    worst, where = dens_deviation(case)
    _record(case, "dens", worst, where)
    assert worst <= MARGIN * DENS_WORST[case]


@pytest.mark.parametrize("case", CASES)
def test_value(case):
    r, g = _ref(case), _got(case)
    names = _names(case)
    assert np.array_equal(np.isnan(g["out"]), np.isnan(r.val))
    worst, where = val_deviation(case)
    _record(case, "val", worst, where)
    assert worst <= MARGIN * VAL_WORST
    assert _bits(jsd_pairs(r.cols, r.pairs)) == _bits(g["out"])     # the density store changed nothing
    for (a, b), v, want in zip(r.pairs, g["out"], r.val):
        if a == b:                                               # (all_negative's self-pair: NaN exactly where R's is)
            assert (np.isnan(v) and np.isnan(want)) or (v == 0.0 and want == 0.0), names[a]
            assert names[a] == "all_negative" or v == 0.0
    fin = g["out"][~np.isnan(g["out"])]
    assert np.all(fin >= -1e-15) and np.all(fin <= 1.0)


@pytest.mark.parametrize("case", CASES)
def test_stages_depend_on_their_columns_only(case):
    """A column's sort and statistics are bitwise the same in the pool and alone; a pair's densities and value are
    bitwise the same under another pair order, and with the stages not asked for."""
    r, g = _ref(case), _got(case)
    for c in range(r.cols.shape[1]):
        alone = jsd_stages(r.cols[:, [c]], np.zeros((0, 2), dtype=np.int32), dens=False)
        assert _bits(alone["sorted"][:, 0]) == _bits(g["sorted"][:, c])
        assert _bits(alone["stats"][0]) == _bits(g["stats"][c])
    perm = np.random.default_rng(7).permutation(len(r.pairs))
    other = jsd_stages(r.cols, r.pairs[perm], sorted=False, stats=False)
    assert other["sorted"] is None and other["stats"] is None
    assert _bits(other["dens"]) == _bits(g["dens"][perm])
    assert _bits(other["out"]) == _bits(g["out"][perm])


def test_stages_host_refusals():
    cols = np.random.default_rng(0).random((8, 3))
    from resnmtf_amd import _lib
    with pytest.raises(_lib.ResnmtfError):
        jsd_stages(np.ones((1, 2)), [[0, 1]])
    with pytest.raises(_lib.ResnmtfError, match="out of range"):
        jsd_stages(cols, [[0, 3]])
    bad = cols.copy(); bad[5, 2] = np.nan
    with pytest.raises(_lib.ResnmtfError, match="non-finite"):
        jsd_stages(bad, [[0, 1]])
    got = jsd_stages(cols, np.zeros((0, 2), dtype=np.int32), sorted=False, stats=False, dens=False)
    assert got["out"].shape == (0,)
