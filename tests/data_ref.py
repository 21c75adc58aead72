"""Host references of what a view becomes on its way onto the device, and of ``resnmtf_finalise`` (test infrastructure
in the manner of tests/sweep_ref.py; imports the oracle).

* the upload image: ``float32`` of the fp64 matrix, nothing else (``upload_image``);
* the raw upload: ``float32((x + shift) / colsum)`` with ``oracle.make_non_neg`` / ``matrix_normalisation`` and the
  column sums taken by ``math.fsum`` (``preprocess64`` / ``raw_reference``), under ``RAW_BAR``;
* the shuffle: the permutation recovered from distinct values and its 8 x 8 octile table against ``CHI2_BAR``;
* finalise: ``oracle.normalisation_check`` + ``binary_clusters`` (``finalise_reference``), its derived bars and the
  constructed inputs the GPU test feeds (``finalise_case``), so that the host test checks the very same seeds.

Each reference takes switches that turn it into the MUTANT of one bug the GPU tests exist to catch; the host test
(tests/test_data_ref_host.py) shows that every statistic separates its mutants.
"""
from __future__ import annotations

import math

import numpy as np
from scipy import stats

from oracle import resnmtf_oracle as O
from sweep_ref import rel_stat

# The device's column sum is a tree sum in fp64 of at most n non-negative terms: within n 2^-52 (relative) of the exact
# sum, so the fp64 quotient is within n 2^-52 of the reference's and its f32 rounding at most one f32 ulp away.
# Worst measured on the MI355X: 0 -- every raw upload and every normalised shuffle of tests/test_gpu_view_routes.py came
# out bitwise the reference's f32 image (largest case 1000 x 333): the freedom of the sum moved no f32 rounding.
RAW_BAR = 2.0 ** -23

# The twelve shapes at the edges of the 32 x 32 upload tile, the 64-column image tile and the 256-thread blocks; the
# last two again without the pitch padding.
SHAPES = [(5, 4), (3, 70), (200, 2), (31, 33), (32, 32), (33, 31), (63, 65), (64, 64), (65, 129), (129, 64), (257, 300),
          (1000, 333)]
SHAPE_CASES = [(n, m, False) for n, m in SHAPES] + [(64, 64, True), (65, 129, True)]


def shape_id(case):
    n, m, flat = case
    return f"{n}x{m}" + ("_no_pitch_pad" if flat else "")


# ---------------------------------------------------------------------------------------------------------------------
# the upload image
# ---------------------------------------------------------------------------------------------------------------------
def upload_image(x) -> np.ndarray:
    """What ``get_view`` must return after ``set_view(x)``: every entry rounded to f32 (as fp64)."""
    return np.asarray(x, dtype=np.float64).astype(np.float32).astype(np.float64)


def distinct(n: int, m: int) -> np.ndarray:
    """``x.flat[i] = i + 1``: distinct f32-exact values (counts below 2^24), so equality proves where an entry went."""
    assert n * m < 2 ** 24
    return np.arange(1, n * m + 1, dtype=np.float64).reshape(n, m)


def positive(n: int, m: int, seed: int) -> np.ndarray:
    """Non-negative fp64 data that is NOT f32-exact (the rounding of the upload is part of what is checked)."""
    return np.random.default_rng(seed).uniform(0.0, 1.0, size=(n, m)) ** 3


def image_mutants(img: np.ndarray) -> dict:
    """Images of the upload bugs: one 32 x 32 tile stored transposed, the last row / column not written."""
    n, m = img.shape
    out = {}
    t = img.copy()
    h = min(n, m, 32)                                            # the first tile (its square part)
    t[:h, :h] = img[:h, :h].T
    out["one tile transposed"] = t
    t = img.copy(); t[n - 1, :] = 0.0
    out["last row dropped"] = t
    t = img.copy(); t[:, m - 1] = 0.0
    out["last column dropped"] = t
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the raw upload: make_non_neg + matrix_normalisation
# ---------------------------------------------------------------------------------------------------------------------
def fsum_cols(x: np.ndarray) -> np.ndarray:
    return np.array([math.fsum(x[:, c]) for c in range(x.shape[1])])


def preprocess64(x, shift=True, sum_before_shift=False, sum_rows=None) -> np.ndarray:
    """``matrix_normalisation(make_non_neg(x))`` in fp64 with exactly rounded column sums.  The switches are the mutants:
    ``shift=False`` leaves the shift out, ``sum_before_shift`` divides by the sums of the unshifted columns,
    ``sum_rows=256`` sums the first 256 rows only.  A column that shifts to all zero divides 0 / 0 = NaN, as R does."""
    x = np.asarray(x, dtype=np.float64)
    y = O.make_non_neg(x) if shift else x
    base = x if sum_before_shift else y
    cs = fsum_cols(base if sum_rows is None else base[:sum_rows])
    with np.errstate(divide="ignore", invalid="ignore"):
        return y / cs[None, :]


def raw_reference(x, **mutant):
    """``(image, fp64 matrix, was_negative)`` of a raw upload."""
    p = preprocess64(x, **mutant)
    with np.errstate(invalid="ignore"):
        return p.astype(np.float32).astype(np.float64), p, bool((np.asarray(x) < 0).any())


def nan_stat(got, ref):
    """``rel_stat`` over the entries where the reference is a number, plus the count of entries where exactly one of
    the two is NaN: ``(worst, non-zero where the reference is zero, NaN mismatches)``."""
    got = np.asarray(got, dtype=np.float64); ref = np.asarray(ref, dtype=np.float64)
    nan = np.isnan(ref)
    worst, nz = rel_stat(got[~nan], ref[~nan])
    return worst, nz, int(np.count_nonzero(np.isnan(got) != nan))


def mixed_raw(n: int, m: int, seed: int, constant_negative=None) -> np.ndarray:
    """Raw data whose columns cycle through: negative in the last row only; negative in one row beyond the first 256
    only (n <= 256: in the first row only); non-negative; negative throughout.  ``constant_negative``: that column is a
    constant below zero (it shifts to all zero, so its normalisation is NaN)."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(0.05, 4.0, size=(n, m)) * rng.uniform(0.5, 50.0, size=(1, m))
    for c in range(m):
        kind = c % 4
        if kind == 0:
            x[n - 1, c] = -rng.uniform(0.5, 3.0)
        elif kind == 1:
            x[256 + (c % (n - 256)) if n > 256 else 0, c] = -rng.uniform(0.5, 3.0)
        elif kind == 3:
            x[:, c] -= rng.uniform(1.0, 5.0)
    if constant_negative is not None:
        x[:, constant_negative] = -1.5
    return x


def column_kinds(x: np.ndarray) -> dict:
    """How many columns of ``x`` are of each kind ``mixed_raw`` plants (the tests assert that the mix is there)."""
    n = x.shape[0]
    neg = x < 0
    return {"non-negative": int((~neg.any(axis=0)).sum()),
            "negative": int(neg.any(axis=0).sum()),
            "last row only": int((neg[n - 1] & (neg.sum(axis=0) == 1)).sum()),
            "beyond row 256 only": int((neg[256:].any(axis=0) & ~neg[:256].any(axis=0)).sum())}


# ---------------------------------------------------------------------------------------------------------------------
# the shuffle
# ---------------------------------------------------------------------------------------------------------------------
CHI2_DOF = 49
# A uniform permutation exceeds it once in 10^9 draws.  133.3; worst measured on the MI355X 59.9 (destination in the
# device's order, seed 1) and 69.8 (in the matrix's, seed 2^64 - 1), over the four seeds at 500 x 260.
CHI2_BAR = float(stats.chi2.ppf(1.0 - 1e-9, CHI2_DOF))


def recover_permutation(drawn: np.ndarray, order: str = "F") -> np.ndarray:
    """For a draw from ``distinct(n, m)``: ``perm[i]`` = the source position (row-major, as the gather addresses the
    source) of the entry now at destination position i.  ``order="F"``: i counts down the columns, which is the
    device's own index (``staging[i] = X[pi(i)]`` fills a column-major matrix), so ``perm`` IS the kernel's ``pi``;
    ``order="C"``: i counts along the rows, as a reader of the matrix sees it.  Asserts that the draw is a bijection."""
    src = np.rint(np.asarray(drawn).ravel(order=order)).astype(np.int64) - 1
    assert np.array_equal(np.sort(src), np.arange(src.size)), "not a permutation of the source's entries"
    return src


def octile_chi2(perm: np.ndarray) -> float:
    """Chi-square statistic of the 8 x 8 table of source-index octile by destination-index octile."""
    count = perm.size
    dst = np.arange(count)
    table = np.zeros((8, 8))
    np.add.at(table, ((perm * 8) // count, (dst * 8) // count), 1.0)
    exp = np.outer(table.sum(axis=1), table.sum(axis=0)) / count
    return float(np.sum((table - exp) ** 2 / exp))


def mixing_stats(drawn: np.ndarray) -> dict:
    """The octile chi-square of a draw in BOTH destination orders, each to be below ``CHI2_BAR``.  The device's order
    sees a ``pi`` that does not mix in the kernel's own index (the identity, a rotation, a swap of neighbours: in the
    other order those look like a transposition and fill the table evenly); the matrix order sees a draw that leaves
    entries in their rows.  A uniform permutation is uniform in either."""
    return {order: octile_chi2(recover_permutation(drawn, order)) for order in ("F", "C")}


def device_draw(src: np.ndarray, pi: np.ndarray) -> np.ndarray:
    """The matrix the device's shuffle produces from the permutation ``pi`` of its own index: destination entry i
    (column-major) is source entry ``pi[i]`` (row-major)."""
    return src.ravel()[pi].reshape(src.shape, order="F")


# ---------------------------------------------------------------------------------------------------------------------
# finalise
# ---------------------------------------------------------------------------------------------------------------------
def factor_bar(length: int) -> float:
    """F / G outputs: two sums of at most ``length`` non-negative terms in any order (the device's and the oracle's
    column sum, each within length 2^-53 of the exact one) and one division.  Worst measured on the MI355X: 4.4e-16
    against 5.7e-14 (F) and 6.7e-14 (G), random_257x300_k17 of tests/test_gpu_finalise.py."""
    return (2 * length + 2) * 2.0 ** -53


def s_bar(n: int, m: int) -> float:
    """S output: the two column sums on either side, two products on either side.  Worst measured on the MI355X: 7.8e-16
    against 4.0e-13, perm_diag_k64 of tests/test_gpu_finalise.py."""
    return (2 * n + 2 * m + 4) * 2.0 ** -53


def finalise_reference(F, S, G, ge=False, last_max=False, relations_on="rows"):
    """``(F, S, G, row clusters, column clusters)`` of ``normalisation_check`` + ``binary_clusters``.  Without a switch
    the clusters are the oracle's own (asserted); the switches are the mutants: ``ge`` thresholds with >=, ``last_max``
    takes the last maximum of an S column, ``relations_on="cols"`` re-orders the column clusters instead of the row
    clusters."""
    out_f, out_g, out_s = O.normalisation_check([np.asarray(F, float)], [np.asarray(G, float)], [np.asarray(S, float)])
    f, g, s = out_f[0], out_g[0], out_s[0]
    with np.errstate(invalid="ignore"):
        rc = ((f >= 1.0 / f.shape[0]) if ge else (f > 1.0 / f.shape[0])).astype(np.float64)
        cc = ((g >= 1.0 / g.shape[0]) if ge else (g > 1.0 / g.shape[0])).astype(np.float64)
    k = s.shape[0]
    rel = (k - 1 - np.argmax(s[::-1], axis=0)) if last_max else np.argmax(s, axis=0)
    if relations_on == "rows":
        rc = rc[:, rel]
    else:
        cc = cc[:, rel]
    if not (ge or last_max) and relations_on == "rows":
        orc, occ = O.binary_clusters(out_f, out_g, out_s)
        assert np.array_equal(rc, orc[0]) and np.array_equal(cc, occ[0])
    return f, s, g, rc, cc


def relations_of(F, S, G) -> np.ndarray:
    return np.argmax(O.normalisation_check([F], [G], [S])[2][0], axis=0)


def threshold_band(out: np.ndarray, length: int) -> np.ndarray:
    """The entries of a normalised factor within the F / G bar of the threshold 1 / length, where a device sum in
    another order may land on the other side (one more ulp allowed for the product formed here)."""
    with np.errstate(invalid="ignore"):
        return np.abs(out * length - 1.0) <= factor_bar(length) + 2.0 ** -52


FINALISE_SHAPES = [(5, 4, 2), (64, 128, 16), (257, 300, 17), (1100, 700, 64), (1000, 333, 8)]
# (id, (n, m, k), kind): random inputs at every shape, then the constructed cases
FINALISE_CASES = [(f"random_{n}x{m}_k{k}", (n, m, k), "random") for n, m, k in FINALISE_SHAPES] + [
    ("perm_diag_k17", (257, 300, 17), "perm_diag"),
    ("perm_diag_k64", (1100, 700, 64), "perm_diag"),
    ("tie_k2", (5, 4, 2), "tie"),
    ("tie_k16", (64, 128, 16), "tie"),
    ("zero_s_column", (64, 128, 16), "zero_s_column"),
    ("same_arg_max", (64, 128, 16), "same_arg_max"),
    ("equal_f_column", (64, 128, 16), "equal_f_column"),
    ("equal_f_column_one_ulp", (64, 128, 16), "equal_f_column_one_ulp"),
    ("zero_f_column", (257, 300, 17), "zero_f_column"),
]
FINALISE_IDS = [c[0] for c in FINALISE_CASES]
EQUAL_VALUE = 0.75          # 64 of them sum to 48 exactly in any order (every partial sum is exact), 0.75 / 48 = 1 / 64
ULP_ROW = 37


def finalise_case(cid: str) -> dict:
    """The inputs of a finalise case and what is known about its answer: ``F, S, G``; ``relations`` where the case fixes
    them ({column: row}); ``band``: how many entries of F the case puts inside the threshold band on purpose."""
    _, (n, m, k), kind = FINALISE_CASES[FINALISE_IDS.index(cid)]
    rng = np.random.default_rng(4000 + FINALISE_IDS.index(cid))
    F = rng.uniform(0.1, 1.0, size=(n, k)) * rng.uniform(0.5, 20.0, size=(1, k))      # un-normalised, as the loop leaves them
    G = rng.uniform(0.1, 1.0, size=(m, k)) * rng.uniform(0.5, 20.0, size=(1, k))
    F[rng.random((n, k)) < 0.3] *= 0.01                                                 # entries on both sides of 1 / n
    G[rng.random((m, k)) < 0.3] *= 0.01
    S = rng.uniform(0.01, 1.0, size=(k, k))
    case = {"n": n, "m": m, "k": k, "kind": kind, "relations": {}, "band": 0}
    if kind == "perm_diag":                       # a permuted dominant diagonal: relations is that permutation
        perm = rng.permutation(k)
        while np.any(perm == np.arange(k)):
            perm = rng.permutation(k)
        S *= 0.05
        S[perm, np.arange(k)] += 1.0
        case["relations"] = {j: int(perm[j]) for j in range(k)}
    elif kind == "tie":                           # two equal maxima in one column: the first wins
        j, a, b = k - 1, 0, k - 1
        if k >= 16:
            j, a, b = 3, 2, 9
        S[a, j] = S[b, j] = 2.0
        case["relations"] = {j: a}
    elif kind == "zero_s_column":
        S[:, 5] = 0.0
        case["relations"] = {5: 0}
    elif kind == "same_arg_max":                  # two columns with one arg-max: the row-cluster column is duplicated
        S[4, 1] = S[4, 7] = 3.0
        case["relations"] = {1: 4, 7: 4}
    elif kind in ("equal_f_column", "equal_f_column_one_ulp"):
        assert n == 64
        F[:, 6] = EQUAL_VALUE
        if kind.endswith("one_ulp"):
            F[ULP_ROW, 6] = np.nextafter(EQUAL_VALUE, 1.0)
        S[6, 10] = 3.0                            # row-cluster column 10 is F column 6's
        case["relations"] = {10: 6}
        case["band"] = n
    elif kind == "zero_f_column":
        F[:, 4] = 0.0
        S[4, 11] = 3.0                            # row-cluster column 11 is the dead column's; S column 4 scales to 0
        case["relations"] = {11: 4, 4: 0}
    case.update(F=np.asfortranarray(F), S=np.asfortranarray(S), G=np.asfortranarray(G))
    return case
