"""The host reference of the SVD initialisation (tests/init_ref.py) without a GPU: its fp64 algorithm finds the singular
triplets, its finish is the oracle's init_mats_inner, and every statistic of tests/test_gpu_init_svd.py separates the
mutants it exists to catch from its bar by MUTANT_MARGIN.  The mutants are emulated in init_ref.sketch_svd's replaceable
products: what a wrong row block, a dropped slab or a wrong interleave in the kernels would hand to the host."""
import numpy as np
import pytest

import init_ref as R
import test_gpu_init_svd as G
from oracle import resnmtf_oracle as O

MARGIN = G.MUTANT_MARGIN
N, M, K = 333, 200, 8               # odd sizes: a ragged last 16-row step, a last Gram block of 13 rows
L = R.sketch_width(K)
RPS = 128                           # rows of one split of the Xt.Q pass in the emulation: three slabs, the last of 77 rows


@pytest.fixture(scope="module")
def clean():
    x = G.dense_data(N, M, K, 5).astype(np.float32).astype(np.float64)
    U, V, d = R.sketch_svd(x, L, G.N_POWER, np.random.default_rng(0))
    return x, U, V, d, np.linalg.svd(x, compute_uv=False)


def stats(x, U, V, d, sigma, cols=K):
    return {"orth": R.orth_stat(U, cols), "product": R.product_stat(x, U, V, d, L, cols)[0],
            "residual": R.residual_stat(x, U, V, d, cols), "sv": R.sv_stat(d, sigma, cols)}


def bars(x, sigma):
    """The bars the GPU test would apply to this view (class L16)."""
    refs = [R.sketch_svd(x, L, G.N_POWER, np.random.default_rng(s)) for s in G.REF_SEEDS]
    f32 = G.BARS[f"L{L}"]
    return {"orth": G.orth_bar(N, L), "product": f32,
            "residual": max(f32, 4.0 * max(R.residual_stat(x, u, v, d, K) for u, v, d in refs)),
            "sv": max(f32, 4.0 * max(R.sv_stat(d, sigma, K) for u, v, d in refs))}


def test_clean_run_is_inside_every_bar(clean):
    x, U, V, d, sigma = clean
    got, bar = stats(x, U, V, d, sigma), bars(x, sigma)
    for key in got:
        assert got[key] <= bar[key], (key, got[key], bar[key])
    assert got["orth"] < 1e-14 and got["product"] < 1e-14


def _drop_rows(first):
    def xtq(x, q):
        return x[:first].T @ q[:first]
    return xtq


def _short_gram(Y):
    rpb = R.gram_rows_per_block(Y.shape[0])
    last = (-(-Y.shape[0] // rpb) - 1) * rpb
    return Y[:last].T @ Y[:last]


PERM = np.arange(L).reshape(-1, 2)[:, ::-1].ravel()       # neighbouring columns swapped: an interleave at the wrong nt

MUTANTS = [
    # (name, sketch_svd arguments, the statistics meant to catch it)
    ("Xt.Q without the last row of X", dict(xtq=_drop_rows(N - 1)), ("product",)),      # (one row of 333: below the convergence bars)
    ("Xt.Q without the last 16-row step", dict(xtq=_drop_rows(16 * ((N - 1) // 16))), ("product", "residual", "sv")),
    ("Xt.Q without the last split's slab", dict(xtq=_drop_rows(RPS * ((N - 1) // RPS))), ("product", "residual", "sv")),
    ("a Gram that skips its last row block", dict(gram=_short_gram), ("orth",)),
    ("ts_apply with M transposed", dict(apply=lambda Y, Mx: Y @ Mx.T), ("orth",)),
    ("fperm at the wrong nt for the f32 operand copy", dict(q_perm=PERM), ("product",)),
]


@pytest.mark.parametrize("name,kw,meant", MUTANTS, ids=[mu[0] for mu in MUTANTS])
def test_mutant_exceeds_the_bar_of_its_statistic(clean, name, kw, meant):
    x, _, _, _, sigma = clean
    U, V, d = R.sketch_svd(x, L, G.N_POWER, np.random.default_rng(0), **kw)
    got, bar = stats(x, U, V, d, sigma), bars(x, sigma)
    for key in meant:
        assert got[key] >= MARGIN * bar[key], f"{name}: {key} = {got[key]:.3e} against the bar {bar[key]:.3e}"


def test_swapped_columns_of_u_fail_the_last_product(clean):
    x, U, V, d, sigma = clean
    U = U.copy(); U[:, [2, 3]] = U[:, [3, 2]]
    got, bar = stats(x, U, V, d, sigma), bars(x, sigma)
    assert got["orth"] <= bar["orth"]                     # (still orthonormal: only the product sees it)
    assert got["product"] >= MARGIN * bar["product"] and got["residual"] >= MARGIN * bar["residual"]


def test_thin_gram_mutant_fails_the_thin_checks():
    """The thin route: a Gram without its ragged last row block (4100 rows: blocks of 32, the last of 4) moves the singular
    values and the long side's orthonormality far beyond their bars."""
    n, m, k = 4100, 12, 12
    x = G.dense_data(n, m, k, 7)
    sigma = np.linalg.svd(x, compute_uv=False)
    U, V, d = R.thin_svd(x)
    assert R.sv_stat(d, sigma, k) < 1e-13 and R.orth_stat(U, k) < 1e-11 and R.product_stat(x, U, V, d, m, k)[0] < 1e-13
    lam, W = np.linalg.eigh(_short_gram(x))
    order = np.argsort(-lam)
    d2 = np.sqrt(lam[order]); W = W[:, order]
    U2 = x @ (W / d2[None, :])
    bar = G.BARS["thin"]
    assert R.product_stat(x, U2, W, d2, m, k)[0] >= MARGIN * bar
    strong = int(np.count_nonzero(d2 > 1e-3 * d2[0]))
    assert R.orth_stat(U2, strong) >= MARGIN * G.orth_bar(n, m) * (d2[0] / d2[strong - 1]) ** 2


@pytest.mark.parametrize("shape,k", [((70, 50), 4), ((40, 90), 7)])
def test_finish_is_the_oracle_init(shape, k):
    x = G.dense_data(*shape, k, 3)
    u, d, vt = np.linalg.svd(x, full_matrices=False)
    ref = O.init_mats_inner([x], [k], np.random.default_rng(0), sigma=0.0)
    for got, want in zip(R.finish(u, vt.T, d, k), ref):
        assert np.array_equal(got, want[0])


def test_finish_replaces_zero_vectors():
    U = np.zeros((9, 2)); U[:, 0] = 1.0 / 3.0
    V = np.zeros((4, 2)); V[:, 0] = 0.5
    f, s, g, lam, mu = R.finish(U, V, np.array([2.0, 0.0]), 2)
    assert np.allclose(f[:, 1], 1.0 / 9.0) and np.allclose(g[:, 1], 0.25) and s[1, 1] == 0.0
    assert np.allclose(lam, 1.0) and np.allclose(mu, 1.0)


def test_sketch_svd_finds_the_leading_triplets(clean):
    x, U, V, d, sigma = clean
    assert R.sv_stat(d, sigma, K) < 1e-5 and R.residual_stat(x, U, V, d, K) < 1e-3
    # exactly rank-deficient data: the rank cut zeroes the dependent columns, the leading triplets are exact
    for xl, rank in ((G.three_blocks(), 3), (G.ten_rows(400, 300, 1), 10)):
        Ul, Vl, dl = R.sketch_svd(xl, 16, G.N_POWER, np.random.default_rng(1))
        sl = np.linalg.svd(xl, compute_uv=False)
        assert np.isfinite(Ul).all() and np.isfinite(Vl).all()
        assert R.sv_stat(dl, sl, rank) < 1e-13 and R.orth_stat(Ul, rank) < 1e-13 and dl[rank:].max() <= 1e-7 * dl[0]


def test_cholesky_cut_leaves_dependent_columns_out():
    rng = np.random.default_rng(2)
    Y = rng.standard_normal((50, 6))
    Y[:, 3] = Y[:, 0] - 2.0 * Y[:, 1]                     # exactly dependent, up to rounding
    Y[:, 5] = 0.0
    C = Y.T @ Y
    Rm = R.cholesky_cut(C, R.RANK_CUT * np.trace(C))
    assert [bool(v) for v in np.diag(Rm) != 0] == [True, True, True, False, True, False]
    Q = Y @ R.invert_cut(Rm)
    keep = [0, 1, 2, 4]
    assert np.abs(Q[:, keep].T @ Q[:, keep] - np.eye(4)).max() < 1e-13 and not Q[:, [3, 5]].any()


def test_half_normal_z_tells_sd_from_variance():
    rng = np.random.default_rng(4)
    sig = 0.05
    z = R.half_normal_z(np.abs(rng.normal(0.0, np.sqrt(sig), 4096)), sig)
    assert abs(z[0]) < 5 and abs(z[1]) < 5
    z = R.half_normal_z(np.abs(rng.normal(0.0, sig, 4096)), sig)          # sd = sigma: the bug
    assert abs(z[0]) > 5 and abs(z[1]) > 5


def test_route_and_width():
    assert [R.sketch_width(k) for k in (1, 8, 9, 24, 25, 40, 41, 56, 57, 64)] == [16, 16, 32, 32, 48, 48, 64, 64, 64, 64]
    assert R.takes_sketch(64, 200, 48) and not R.takes_sketch(63, 200, 48)
    assert R.gram_rows_per_block(4100) == 32 and R.gram_rows_per_block(129) == 16
