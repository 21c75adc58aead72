"""GPU tests of spurious-bicluster removal inside the pipeline (the opt-in ``spurious_on_device=True``):
resnmtf_spurious_scores bitwise against resnmtf_jsd_pairs on the pool of finalise's F's, resnmtf_relevance_masked bitwise
against the restatement on the cleaned clusters, res_nmtf_inner / stability_check / the k sweep bitwise against host
compositions of existing pieces, and the reference's "resnmtf runs with stability and spurious removal"
(test-resnmtf.R:74-83)."""
import numpy as np
import pytest

import resnmtf_amd
from resnmtf_amd import api, batched, bisil, naming, spurious
from resnmtf_amd._lib import ResnmtfError
from resnmtf_amd.engine import Engine, jsd_pairs
from stability_ref import relevance_counts

pytestmark = pytest.mark.gpu


def _factors(rng, n, m, k, power=4.0):
    f = rng.random((n, k)) ** power + 1e-4
    g = rng.random((m, k)) ** power + 1e-4
    s = rng.random((k, k)) + np.eye(k)
    return f, s, g


def _engine_with_factors(rng, n, m, k):
    eng = Engine([n], [m], [k])
    eng.set_factors(0, *_factors(rng, n, m, k))
    return eng


@pytest.mark.parametrize("K,R,n", [(3, 2, 700), (3, 5, 1000), (16, 2, 513), (16, 5, 700), (64, 2, 1030), (64, 5, 600)])
def test_spurious_scores_equal_jsd_pairs_bitwise(K, R, n):
    rng = np.random.default_rng(100 * K + R)
    m = max(K + 16, 40)
    engs = [_engine_with_factors(rng, n, m, K) for _ in range(R + 1)]
    try:
        score, null = engs[0].spurious_scores(0, engs[1:])
        pool = np.concatenate([e.finalise(0)[0] for e in engs], axis=1)
        null_p, score_p = spurious.pool_pairs(K, R)
        vals = jsd_pairs(pool, np.concatenate([null_p, score_p]))
        assert null.tobytes() == vals[:len(null_p)].tobytes()
        want = vals[len(null_p):].reshape(K, R * K).mean(axis=1)
        assert score.tobytes() == want.tobytes(), (score, want)
        again = engs[0].spurious_scores(0, engs[1:])
        assert again[0].tobytes() == score.tobytes() and again[1].tobytes() == null.tobytes()
    finally:
        for e in engs:
            e.close()


def test_spurious_scores_refusals():
    rng = np.random.default_rng(5)
    a, b, c = (_engine_with_factors(rng, 300, 40, 4) for _ in range(3))
    other_n = _engine_with_factors(rng, 301, 40, 4)
    other_k = _engine_with_factors(rng, 300, 40, 5)
    bare = Engine([300], [40], [4])
    try:
        with pytest.raises(ResnmtfError, match="R must be") as ei:
            a.spurious_scores(0, [b])
        assert ei.value.code == 1
        with pytest.raises(ResnmtfError, match="n or k"):
            a.spurious_scores(0, [b, other_n])
        with pytest.raises(ResnmtfError, match="n or k"):
            a.spurious_scores(0, [b, other_k])
        with pytest.raises(ResnmtfError, match="no factors") as ei:
            a.spurious_scores(0, [b, bare])
        assert ei.value.code == 5
        with pytest.raises(ResnmtfError, match="no factors"):
            bare.spurious_scores(0, [b, c])
        with pytest.raises(ResnmtfError, match="view index"):
            a.spurious_scores(1, [b, c])
        f, s, g = _factors(rng, 300, 40, 4)
        f[7, 2] = np.nan
        c.set_factors(0, f, s, g)
        with pytest.raises(ResnmtfError, match="non-finite"):
            a.spurious_scores(0, [b, c])
    finally:
        for e in (a, b, c, other_n, other_k, bare):
            e.close()


@pytest.mark.parametrize("k,n,m,N,M", [(3, 150, 90, 170, 100), (16, 700, 300, 800, 333), (64, 1000, 200, 1111, 222)])
def test_masked_relevance_bitwise_equals_restatement(k, n, m, N, M):
    rng = np.random.default_rng(10 * k + n)
    rc_ref = (rng.random((N, k)) < 0.35).astype(np.float64)
    cc_ref = (rng.random((M, k)) < 0.35).astype(np.float64)
    ref = Engine([N], [M], [2])
    ref.set_reference_clusters(0, rc_ref, cc_ref)
    eng = Engine([n], [m], [k])
    try:
        masks = [rng.random(k) < 0.4, np.zeros(k, dtype=bool), np.ones(k, dtype=bool)]
        for trial, flags in enumerate(masks):
            eng.set_factors(0, *_factors(rng, n, m, k, power=3.0))
            rows = rng.choice(N, n, replace=False); cols = rng.choice(M, m, replace=False)
            got = eng.relevance_masked(0, ref, 0, rows, cols, flags)
            _, s_out, _, rc, cc = eng.finalise(0)
            drop = flags[np.argmax(s_out, axis=0)]
            rc[:, drop] = 0.0; cc[:, drop] = 0.0
            want = relevance_counts(rc, cc, rc_ref[rows], cc_ref[cols])
            assert got.tobytes() == want.tobytes(), (trial, got, want)
            if trial == 1:                                 # no flag: resnmtf_relevance itself
                assert got.tobytes() == eng.relevance(0, ref, 0, rows, cols).tobytes()
            if trial == 2:                                 # every cluster emptied, the reference's are not: 0
                assert np.array_equal(got, np.zeros(k))
    finally:
        eng.close(); ref.close()


def planted(seed, noise=0.1):
    """test-resnmtf.R:38-52: three 60 x 60 blocks of height 10 + 0.1 |N(0, 1)|."""
    rng = np.random.default_rng(seed)
    rc = np.kron(np.eye(3), np.ones((60, 1))); cc = np.kron(np.eye(3), np.ones((60, 1)))
    x = rc @ np.diag([10.0, 10.0, 10.0]) @ cc.T + noise * np.abs(rng.normal(size=(180, 180)))
    return x, rc, cc


def _inner_args(data):
    rn, cn = naming.give_names(data, None, None, None, None)
    return naming.check_data(data), naming.shared_names(rn), naming.shared_names(cn), rn, cn


@pytest.mark.parametrize("k,R,noise", [(3, 5, False), (5, 3, False), (4, 5, True)])
def test_res_nmtf_inner_equals_remove_spurious_bitwise(k, R, noise):
    rng = np.random.default_rng(k)
    data = ([rng.random((150, 120)) ** 3, rng.random((150, 90)) ** 3] if noise     # (no structure: removals)
            else [planted(1, 1.5)[0], planted(2, 1.5)[0]])
    pre, ri, ci, rn, cn = _inner_args(data)
    kw = dict(k_vec=[k, k], row_names=rn, col_names=cn, seed=11, num_repeats=R)
    got = api.res_nmtf_inner(pre, ri, ci, spurious=True, spurious_on_device=True, score_bisil=True, **kw)
    plain = api.res_nmtf_inner(pre, ri, ci, spurious=False, **kw)
    want = spurious.remove_spurious(pre, plain, R, seed=11)
    for key in ("output_f", "output_s", "output_g", "lambda", "mu"):
        for a, b in zip(got[key], want[key]):
            assert a.tobytes() == b.tobytes(), key
    assert got["Error"] == want["Error"] and got["All_Error"].tobytes() == want["All_Error"].tobytes()
    for key in ("row_clusters", "col_clusters"):
        for a, b in zip(got[key], want[key]):
            assert a.tobytes() == b.tobytes(), key
    for key in ("score", "avg_threshold", "max_threshold", "removed"):
        assert np.asarray(got["spurious"][key]).tobytes() == np.asarray(want["spurious"][key]).tobytes(), key
    print(f"k={k}, R={R}: removed {got['spurious']['removed'].sum(axis=1).tolist()}")
    eng = batched.DeviceData(pre, pre_processed=True)
    try:
        assert got["bisil"] == bisil.score(want["row_clusters"], want["col_clusters"], "euclidean", engine=eng.base)
    finally:
        eng.close()


def test_stability_with_spurious_equals_host_composition_bitwise():
    data = [planted(3, 1.0)[0], planted(4, 1.0)[0]]
    pre, ri, ci, rn, cn = _inner_args(data)
    k, R, n_stab, rate, seed = 3, 3, 3, 0.8, 9
    res = api.res_nmtf_inner(pre, ri, ci, k_vec=[k, k], row_names=rn, col_names=cn, seed=4, num_repeats=R,
                             spurious=True, spurious_on_device=True)
    zero = np.zeros((2, 2))
    out = api.stability_check(pre, res, k, zero, zero, zero, None, True, R, False, "euclidean", rate, n_stab,
                              remove_unstable=False, row_names=rn, col_names=cn, seed=seed, spurious_on_device=True)
    dev = batched.DeviceData(pre, zero, zero, zero, rn, cn, pre_processed=True)
    try:
        draws = batched.stability_draws(dev.data_shapes, n_stab, rate, seed)
        total = None
        for r in range(n_stab):
            rep = dev.factorise(k, None, seed + 2000 + r, samples=draws[r], return_data=True)
            cleaned = spurious.remove_spurious(rep["data"], rep, R, seed=seed + 2000 + r)
            rows, cols = rep["extras"]["row_samples"], rep["extras"]["col_samples"]
            one = np.stack([relevance_counts(cleaned["row_clusters"][v], cleaned["col_clusters"][v],
                                             res["row_clusters"][v][rows[v]], res["col_clusters"][v][cols[v]])
                            for v in range(2)])
            total = one if total is None else total + one
    finally:
        dev.close()
    assert out["relevance"].tobytes() == (total / n_stab).tobytes()


def test_k_sweep_with_spurious_picks_the_res_nmtf_inner_result():
    data = [planted(1)[0], planted(2)[0]]
    res = resnmtf_amd.apply_resnmtf(data, k_max=5, stability=False, k_sweep=True, return_sweep=True, seed=3,
                                    num_repeats=3, spurious_on_device=True)
    k = res["k_sweep"]["k"][int(np.argmax(res["k_sweep"]["bisil"]))]
    pre, ri, ci, rn, cn = _inner_args(data)
    one = api.res_nmtf_inner(pre, ri, ci, k_vec=[k, k], spurious=True, spurious_on_device=True, row_names=rn,
                             col_names=cn, seed=3 + k, score_bisil=True, num_repeats=3)
    assert one["bisil"] == res["bisil"]
    for key in ("output_f", "output_s", "row_clusters", "col_clusters"):
        for a, b in zip(one[key], res[key]):
            assert a.tobytes() == b.tobytes(), key
    for key in ("score", "max_threshold", "removed"):
        assert np.asarray(one["spurious"][key]).tobytes() == np.asarray(res["spurious"][key]).tobytes(), key


def _recovered(res, rc, cc):
    for v in range(2):
        assert sorted(res["row_clusters"][v].sum(0)) == sorted(rc.sum(0))
        assert sorted(res["col_clusters"][v].sum(0)) == sorted(cc.sum(0))


def test_reference_test_stability_with_spurious_removal():
    """test-resnmtf.R:74-83 ("resnmtf runs with stability and spurious removal"), k_val = 3, defaults otherwise; the
    same seed gives the same bits (two calls)."""
    x1, rc, cc = planted(1)
    x2, _, _ = planted(2)
    res = resnmtf_amd.apply_resnmtf([x1, x2], k_val=3, seed=7, spurious_on_device=True)
    assert len(res["output_f"]) == 2 and res["output_f"][0].shape == (180, 3)
    assert "spurious" in res
    _recovered(res, rc, cc)
    again = resnmtf_amd.apply_resnmtf([x1, x2], k_val=3, seed=7, spurious_on_device=True)
    for key in ("output_f", "output_s", "output_g", "row_clusters", "col_clusters"):
        for a, b in zip(res[key], again[key]):
            assert a.tobytes() == b.tobytes(), key
    assert np.asarray(res["spurious"]["score"]).tobytes() == np.asarray(again["spurious"]["score"]).tobytes()


def test_reference_default_pipeline_with_the_k_sweep():
    """The reference's default call (k sweep 3..8, spurious = TRUE, stability = TRUE) on the same problem."""
    x1, rc, cc = planted(1)
    x2, _, _ = planted(2)
    res = resnmtf_amd.apply_resnmtf([x1, x2], k_sweep=True, seed=7, spurious_on_device=True, return_sweep=True)
    assert res["k_sweep"]["k"][:6] == [3, 4, 5, 6, 7, 8]
    assert res["output_f"][0].shape == (180, 3)
    _recovered(res, rc, cc)
