"""Sparse data views on the device (resnmtf_create_sparse / resnmtf_set_view_csc) against the fp64
oracle on the DENSIFIED matrix, from the same initial factors -- the dense path's bars: F / G within 2e-5 relative
Frobenius, All_Error within 2e-5 at every sweep, cluster matrices identical except entries on the 1/n threshold."""
import numpy as np
import pytest
import scipy.sparse as sp

import resnmtf_amd
import loop_ref
from helpers import load_golden, golden_problem, rel_fro, run_hip, run_oracle
from resnmtf_amd import synth
from resnmtf_amd.engine import Engine
from resnmtf_amd._lib import ResnmtfError
from test_gpu_parity import check_against

pytestmark = pytest.mark.gpu


def sparsify(x, density, seed, keep=None):
    """x with a random `density` of its entries kept (plus `keep`, a mask, and one entry per column), columns
    re-normalised: a pre-processed view, dense fp64 (for the oracle)."""
    rng = np.random.default_rng(seed)
    mask = rng.random(x.shape) < density
    if keep is not None:
        mask |= keep
    mask[rng.integers(0, x.shape[0], x.shape[1]), np.arange(x.shape[1])] = True
    y = np.where(mask, x, 0.0)
    return y / y.sum(axis=0)[None, :]


def sparse_problem(prob, fmt="csr"):
    """The same problem with every view handed over as a scipy.sparse matrix."""
    conv = sp.csr_matrix if fmt == "csr" else sp.coo_matrix
    return synth.Problem([conv(x) for x in prob.data], prob.init_f, prob.init_s, prob.init_g, prob.phi, prob.xi, prob.psi,
                         prob.k, prob.name, row_names=prob.row_names, col_names=prob.col_names)


def single(x, k, seed, name):
    n, m = x.shape
    f, s, g = synth.random_init(n, m, k, seed)
    z = np.zeros((1, 1))
    return synth.Problem([x], [f], [s], [g], z, z, z, k, name, row_names=[[f"row_{i}" for i in range(n)]],
                         col_names=[[f"col_{j}" for j in range(m)]])


def one_view(n, m, k, density, seed):
    return single(sparsify(synth.planted_view(n, m, max(k // 2, 2), seed), density, seed + 1), k, seed + 2, "sparse")


def check_parity(prob, n_iters):
    ref = run_oracle(prob, n_iters=n_iters)
    res = run_hip(sparse_problem(prob), n_iters=n_iters)
    check_against(res, ref["output_f"], ref["output_s"], ref["output_g"], ref["row_clusters"], ref["col_clusters"],
                  ref["All_Error"])
    return res


@pytest.mark.parametrize("k", [3, 16, 17, 32, 40, 64])
def test_one_view_matches_oracle_across_k(k):
    check_parity(one_view(400, 300, k, 0.05, 10 + k), 40)


@pytest.mark.parametrize("k", [48, 64])
def test_wide_k_many_lines_matches_oracle(k):
    """KP = 48 / 64 (one workgroup per CU: the k x k job's LDS) with more Xt.F waves than the device holds at once."""
    check_parity(one_view(600, 5000, k, 0.02, 30 + k), 30)


@pytest.mark.parametrize("density", [0.001, 0.05, 0.5])
def test_one_view_matches_oracle_across_densities(density):
    check_parity(one_view(3000, 700, 8, density, 40), 40)


def test_skewed_view_matches_oracle():
    """A dense row (60 %), a dense column (60 %) and empty rows among rows at 0.2 %: the work split by nnz."""
    n, m, k = 2500, 900, 6
    rng = np.random.default_rng(3)
    x = synth.planted_view(n, m, 3, 4)
    keep = np.zeros((n, m), dtype=bool)
    keep[7, rng.random(m) < 0.6] = True
    keep[rng.random(n) < 0.6, 11] = True
    y = sparsify(x, 0.002, 5, keep)
    empty = rng.choice(np.setdiff1d(np.arange(n), [7]), 40, replace=False)
    y[empty, :] = 0.0
    y = np.where(y.sum(axis=0)[None, :] > 0, y, x)          # (no column left empty)
    y /= y.sum(axis=0)[None, :]
    check_parity(single(y, k, 6, "skewed"), 40)


@pytest.mark.parametrize("name,mixed", [("g2_two_views_phi_partial", False), ("g3_three_views_phi_psi_xi", True)])
def test_coupled_views_match_oracle(name, mixed):
    """The g2 / g3 golden problems (phi / psi / xi, partially shared names), sparsified; g3 mixes a dense view in."""
    prob = golden_problem(load_golden(name))
    prob.data = [sparsify(x, 0.3, 70 + v) for v, x in enumerate(prob.data)]
    ref = run_oracle(prob, n_iters=60)
    sprob = sparse_problem(prob, fmt="coo")
    if mixed:
        sprob.data[1] = prob.data[1]
    res = run_hip(sprob, n_iters=60)
    check_against(res, ref["output_f"], ref["output_s"], ref["output_g"], ref["row_clusters"], ref["col_clusters"],
                  ref["All_Error"])


def test_convergence_mode_matches_oracle():
    prob = one_view(800, 500, 5, 0.05, 90)
    ref = run_oracle(prob, n_iters=None, max_iters=3000)
    res = run_hip(sparse_problem(prob), n_iters=None, max_iters=3000)
    n_ref, n_hip = len(ref["All_Error"]), len(res["All_Error"])
    assert abs(n_ref - n_hip) <= 2, (n_ref, n_hip)
    assert n_hip == loop_ref.stop_sweep(res["All_Error"], 1e-6)      # exact on the device's own trace
    m = min(n_ref, n_hip)
    np.testing.assert_allclose(res["All_Error"][:m], ref["All_Error"][:m], atol=2e-5)


def test_run_to_run_and_graph_replay_are_bitwise_equal():
    prob = sparse_problem(one_view(2500, 900, 16, 0.02, 50))
    a = run_hip(prob, n_iters=37, use_graph=True)
    b = run_hip(prob, n_iters=37, use_graph=True)
    c = run_hip(prob, n_iters=37, use_graph=False)
    for r in (b, c):
        assert np.array_equal(a["All_Error"], r["All_Error"])
        for key in ("output_f", "output_s", "output_g"):
            assert np.array_equal(a[key][0], r[key][0])


@pytest.mark.parametrize("n,m,k", [(600, 400, 8), (500, 12, 4)])      # sketch route and thin (exact) route
def test_init_svd_singular_values_match_dense_view(n, m, k):
    x = sparsify(synth.planted_view(n, m, 4, 8), 0.1, 9)
    with Engine([n], [m], [k]) as dense, Engine([n], [m], [k], nnz=[int((x != 0).sum())]) as sparse_eng:
        dense.set_view(0, x)
        sparse_eng.set_view_sparse(0, sp.csc_matrix(x), pre_processed=True)
        d_dense = dense.init_svd(0, seed=3)
        d_sparse = sparse_eng.init_svd(0, seed=3)
    assert np.all(np.abs(d_sparse - d_dense) <= 2e-5 * np.abs(d_dense).max())


def test_device_preprocessing_equals_check_data():
    """pre_processed=False: matrix_normalisation on the device = naming.check_data on the dense matrix (the error trace
    and factors of the run agree with a host-normalised upload)."""
    prob = one_view(700, 300, 5, 0.05, 11)
    raw = sp.csc_matrix(prob.data[0] * np.random.default_rng(1).uniform(0.5, 3.0, size=(1, 300)))
    out = []
    for pre in (False, True):
        with Engine([700], [300], [5], nnz=[raw.nnz]) as e:
            e.set_view_sparse(0, raw if not pre else resnmtf_amd.naming.check_data([raw])[0], pre_processed=pre)
            e.set_factors(0, prob.init_f[0], prob.init_s[0], prob.init_g[0])
            out.append((e.run(20), e.get_factors(0)[0]))
    np.testing.assert_allclose(out[0][0], out[1][0], rtol=1e-6, atol=1e-9)
    assert rel_fro(out[0][1], out[1][1]) < 1e-6


def planted(seed):
    """test-resnmtf.R:38-52 (three 60 x 60 blocks of height 10 + 0.1 |N(0, 1)|), the noise kept at 5 %."""
    rng = np.random.default_rng(seed)
    rc = np.kron(np.eye(3), np.ones((60, 1)))
    x = rc @ np.diag([10.0, 10.0, 10.0]) @ rc.T + 0.1 * np.abs(rng.normal(size=(180, 180))) * (rng.random((180, 180)) < 0.05)
    return sp.csr_matrix(x), rc


def test_apply_resnmtf_with_stability_recovers_planted_clusters():
    x1, rc = planted(1)
    x2, _ = planted(2)
    res = resnmtf_amd.apply_resnmtf([x1, x2], k_val=3, spurious=False, seed=7)
    for v in (0, 1):
        assert sorted(res["row_clusters"][v].sum(0)) == sorted(rc.sum(0))
        assert sorted(res["col_clusters"][v].sum(0)) == sorted(rc.sum(0))


def test_view_entries_refuse_sparse_views():
    x = sp.random(200, 100, density=0.1, random_state=1, format="csc") + sp.eye(200, 100, format="csc")
    with Engine([200, 200], [100, 100], [3, 3], nnz=[x.nnz, None]) as e, Engine([200], [100], [3], nnz=[x.nnz]) as other:
        assert e.view_storage(0) == (True, 0, x.nnz) and e.view_storage(1) == (False, 0, -1)
        e.set_view_sparse(0, x, pre_processed=False)
        assert e.view_storage(0) == (True, x.nnz, x.nnz)
        assert e.view_image_info(0)[0] == 0
        e.set_view(1, x.toarray() / x.toarray().sum(0))
        other.set_view_sparse(0, x)
        for call, what in ((lambda: e.get_view(0), "get_view"), (lambda: other.copy_view_from(0, e, 0), "copy"),
                           (lambda: e.copy_view_from(1, other, 0), "copy"), (lambda: e.shuffle_view_from(1, other, 0), "shuffle"),
                           (lambda: other.subsample_view_from(0, e, 1, np.arange(200), np.arange(100)), "sub-sample")):
            with pytest.raises(ResnmtfError) as info:
                call()
            assert info.value.code == 1, what
        with pytest.raises(ResnmtfError, match="dense"):
            e.set_view_sparse(1, x)
        with pytest.raises(ResnmtfError, match="sparse"):
            e.set_view(0, x.toarray())
        with pytest.raises(ResnmtfError, match="capacity"):
            other.set_view_sparse(0, x + sp.eye(200, 100, k=1, format="csc"))
        with pytest.raises(ResnmtfError, match="negative"):
            other.set_view_sparse(0, -x)
