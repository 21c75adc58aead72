"""Stability selection in double precision: stability_check(precision="fp64") and
apply_resnmtf(precision="fp64", fp64_stability=True) against their parts -- every repeat's relevance bit for bit
stability_ref.relevance_counts of the clusters it kept, the mean bit for bit total / n_stability, a repeat rebuilt by hand
(engine.fp64_subsample at the trimmed draws, res_nmtf_inner, engine.fp64_relevance), the draws and the starts of the f32
route on data fp32 holds, the removal inside a repeat against remove_spurious on its sub-sample, and the reference's tests.

Every fit is guarded by ``max_iters`` = MAX_ITERS where the test leaves the stopping to convergence (the same guard on both
sides of every comparison)."""
import functools

import numpy as np
import pytest

from resnmtf_amd import api, batched, engine, naming
from stability_ref import relevance_counts
from test_gpu_stability import _two_view_problem, planted

pytestmark = pytest.mark.gpu

MAX_ITERS = 300
N_STAB, RATE, ITERS, SEED = 3, 0.8, 40, 9


def host(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)


@functools.lru_cache(maxsize=None)
def two_views():
    """The two-view problem of the f32 twin, pre-processed, with its fp64 fit."""
    data, rn, cn, phi, k = _two_view_problem()
    res = api.apply_resnmtf(data, k_val=k, phi=phi, spurious=False, stability=False, n_iters=ITERS, row_names=rn, col_names=cn,
                            seed=4, precision="fp64")
    pre = naming.check_data(data)
    phi_m = naming.init_rest_mats(phi, 2)
    return pre, res, rn, cn, phi_m, np.zeros((2, 2)), k


def check(pre=None, res=None, **more):
    p, r, rn, cn, phi_m, zero, k = two_views()
    kw = dict(row_names=rn, col_names=cn, seed=SEED, n_stability=N_STAB, sample_rate=RATE, precision="fp64")
    kw.update(more)
    return api.stability_check(p if pre is None else pre, r if res is None else res, k, phi_m, zero, zero, ITERS, False, 5, False,
                               "euclidean", **kw)


@functools.lru_cache(maxsize=None)
def checked():
    return check(remove_unstable=False, return_repeats=True)


def test_every_repeat_is_relevance_counts_of_its_clusters_and_the_mean_is_the_total_over_n():
    pre, res, _, _, _, _, k = two_views()
    out = checked()
    rel = out["relevance"]
    assert out["res"] is res and rel.shape == (2, k)
    reps = out["stability"]["repeats"]
    assert len(reps) == N_STAB
    draws = batched.stability_draws([d.shape for d in pre], N_STAB, RATE, SEED)
    total = np.zeros((2, k))
    for r, rep in enumerate(reps):
        assert list(rep) == ["stability_performed", "relevance", "Error", "All_Error", "tag", "extras", "row_clusters", "col_clusters"]
        rows, cols = rep["extras"]["row_samples"], rep["extras"]["col_samples"]
        assert np.array_equal(cols[0], cols[1]) and len(rows[0]) != len(rows[1])
        for v in range(2):                                       # positive data: nothing is trimmed, the draws are the f32 route's
            assert np.array_equal(rows[v], draws[r][0][v]) and np.array_equal(cols[v], draws[r][1][v])
        one = np.stack([relevance_counts(rep["row_clusters"][v], rep["col_clusters"][v], res["row_clusters"][v][rows[v]],
                                         res["col_clusters"][v][cols[v]]) for v in range(2)])
        assert one.tobytes() == np.asarray(rep["relevance"]).tobytes()
        assert len(rep["All_Error"]) == ITERS and rep["tag"] == f"stability={r}"
        total = total + one
    assert (total / N_STAB).tobytes() == rel.tobytes()
    assert rel.max() > 0.5                                       # the tall blocks are found again
    again = check(remove_unstable=False)
    assert again["relevance"].tobytes() == rel.tobytes()        # same seed, same bits


def test_threshold_zeroes_the_unstable_columns():
    _, res, _, _, _, _, _ = two_views()
    rel = checked()["relevance"]
    vals = np.unique(rel)
    thr = float((vals[0] + vals[1]) / 2) if len(vals) > 1 else float(vals[0]) + 1e-9
    kept = check(stab_thres=thr)
    for v in range(2):
        drop = rel[v] < thr
        for key in ("row_clusters", "col_clusters"):
            assert np.array_equal(kept[key][v][:, drop], np.zeros_like(kept[key][v][:, drop]))
            assert np.array_equal(kept[key][v][:, ~drop], res[key][v][:, ~drop])
        assert kept["output_f"][v] is res["output_f"][v]
    assert any((rel[v] < thr).any() for v in range(2))


def test_tensors_in_and_torch_out_give_the_same_bits():
    import torch
    pre, res, _, _, _, _, _ = two_views()
    dev = torch.device("cuda", 0)
    data = [torch.as_tensor(pre[0], device=dev), torch.as_tensor(pre[1], device=dev).t().contiguous().t()]
    res_t = dict(res, row_clusters=[torch.as_tensor(a, device=dev) for a in res["row_clusters"]],
                 col_clusters=[torch.as_tensor(a, device=dev) for a in res["col_clusters"]])
    rel = checked()["relevance"]
    there = check(pre=data, res=res_t, remove_unstable=False, output="torch")
    assert there["relevance"].tobytes() == rel.tobytes()
    thr = float(np.sort(np.unique(rel))[:2].mean())
    cut_t, cut = check(pre=data, res=res_t, stab_thres=thr, output="torch"), check(stab_thres=thr)
    for key in ("row_clusters", "col_clusters"):
        for v in range(2):
            assert isinstance(cut_t[key][v], torch.Tensor) and cut_t[key][v].device == dev
            assert np.array_equal(host(cut_t[key][v]), cut[key][v])


def test_a_repeat_rebuilt_by_hand_is_equal_bit_for_bit():
    pre, res, rn, cn, phi_m, zero, k = two_views()
    r = 1
    rep = checked()["stability"]["repeats"][r]
    rows, cols = rep["extras"]["row_samples"], rep["extras"]["col_samples"]
    subs = []
    for v in range(2):
        t, er, ec = engine.fp64_subsample(pre[v], rows[v], cols[v])
        assert not er.any() and not ec.any()
        assert np.array_equal(host(t), pre[v][np.ix_(rows[v], cols[v])])
        subs.append(t)
    fit = api.res_nmtf_inner(subs, None, None, None, None, None, [k, k], phi_m, zero, zero, ITERS, spurious=False,
                             row_names=[[rn[v][t] for t in rows[v]] for v in range(2)],
                             col_names=[[cn[v][t] for t in cols[v]] for v in range(2)], seed=SEED + 2000 + r,
                             precision="fp64", fp64_device=True, output="torch")
    assert np.array_equal(fit["All_Error"], rep["All_Error"])
    for v in range(2):
        assert np.array_equal(host(fit["row_clusters"][v]), rep["row_clusters"][v])
        assert np.array_equal(host(fit["col_clusters"][v]), rep["col_clusters"][v])
        got = engine.fp64_relevance(fit["row_clusters"][v], fit["col_clusters"][v], res["row_clusters"][v], res["col_clusters"][v],
                                    rows[v], cols[v])
        assert got.tobytes() == np.asarray(rep["relevance"][v]).tobytes()


def test_on_data_fp32_holds_the_trimmed_draws_and_every_start_are_the_f32_routes():
    pre, _, rn, cn, phi_m, zero, k = two_views()
    data = [d.astype(np.float32).astype(np.float64) for d in pre]
    # rows that hold a single entry: empty in every sub-sample that does not draw its column, so the trimming runs
    for i in range(0, 40, 4):
        data[0][i, :] = 0.0; data[0][i, (7 * i) % 100] = 0.25
        data[1][i + 1, :] = 0.0; data[1][i + 1, (11 * i) % 100] = 0.125
    n_stab = 3
    draws = batched.stability_draws([d.shape for d in data], n_stab, RATE, SEED)
    dev = batched.DeviceData(data, phi_m, zero, zero, rn, cn, pre_processed=True)
    trimmed_any = False
    try:
        for r in range(n_stab):
            f32 = dev.factorise(k, ITERS, SEED + 2000 + r, samples=draws[r], return_init=True)
            rep = batched.stability_repeat_fp64(data, {"row_clusters": [np.ones((160, k)), np.ones((120, k))],
                                                       "col_clusters": [np.ones((100, k))] * 2},
                                                k, ITERS, SEED + 2000 + r, draws[r], phi_m, zero, zero, rn, cn, return_init=True)
            for v in range(2):
                assert np.array_equal(rep["extras"]["row_samples"][v], f32["extras"]["row_samples"][v])
                assert np.array_equal(rep["extras"]["col_samples"][v], f32["extras"]["col_samples"][v])
                trimmed_any |= len(rep["extras"]["row_samples"][v]) < len(draws[r][0][v])
                for a, b in zip(rep["init"][v], f32["init"][v]):
                    assert host(a).tobytes() == np.asarray(b, dtype=np.float64).tobytes()
    finally:
        dev.close()
    assert trimmed_any


def test_reference_test_stability_without_spurious_removal():
    """test-resnmtf.R:85-97 ("resnmtf runs with stability and no spurious removal") under precision="fp64", with the
    assertions of its f32 twin in tests/test_gpu_stability.py."""
    x1, rc, cc = planted(1)
    x2, _, _ = planted(2)
    res = api.apply_resnmtf([x1, x2], k_val=3, spurious=False, seed=7, precision="fp64", fp64_stability=True, max_iters=MAX_ITERS)
    assert len(res["output_f"]) == 2                                                   # :90
    assert res["output_f"][0].shape[0] == 180 and res["output_f"][0].shape[1] == 3       # :91-92
    for v in (1, 0):                                                                     # :93-96
        assert sorted(res["row_clusters"][v].sum(0)) == sorted(rc.sum(0))
        assert sorted(res["col_clusters"][v].sum(0)) == sorted(cc.sum(0))


def test_one_repeat_with_removal_equals_remove_spurious_on_its_sub_sample():
    x1, _, _ = planted(1)
    x2, _, _ = planted(2)
    p = api.prepare([x1, x2], None, None, None, None, None, normalise=True, symmetrise=True)
    k, R, r, seed = 3, 2, 0, 7
    ref = {"row_clusters": [np.kron(np.eye(3), np.ones((60, 1)))] * 2, "col_clusters": [np.kron(np.eye(3), np.ones((60, 1)))] * 2}
    draws = batched.stability_draws([d.shape for d in p.data], 1, 0.9, seed)
    rep = batched.stability_repeat_fp64(p.data, ref, k, None, seed + 2000 + r, draws[r], p.phi, p.xi, p.psi, p.row_names, p.col_names,
                                        max_iters=MAX_ITERS, keep_clusters=True, spurious_repeats=R)
    rows, cols = rep["extras"]["row_samples"], rep["extras"]["col_samples"]
    subs = [p.data[v][np.ix_(rows[v], cols[v])] for v in range(2)]
    rn = [[p.row_names[v][t] for t in rows[v]] for v in range(2)]
    cn = [[p.col_names[v][t] for t in cols[v]] for v in range(2)]
    plain = api.res_nmtf_inner(subs, None, None, None, None, None, [k, k], p.phi, p.xi, p.psi, None, spurious=False, row_names=rn,
                               col_names=cn, seed=seed + 2000 + r, max_iters=MAX_ITERS, precision="fp64")
    post = api.remove_spurious(subs, plain, R, seed=seed + 2000 + r, precision="fp64", max_iters=MAX_ITERS)
    for v in range(2):
        assert np.array_equal(rep["row_clusters"][v], post["row_clusters"][v])
        assert np.array_equal(rep["col_clusters"][v], post["col_clusters"][v])
        want = relevance_counts(post["row_clusters"][v], post["col_clusters"][v], ref["row_clusters"][v][rows[v]],
                                ref["col_clusters"][v][cols[v]])
        assert want.tobytes() == np.asarray(rep["relevance"][v]).tobytes()
    assert np.array_equal(rep["All_Error"], plain["All_Error"])


def test_fp64_default_pipeline_picks_the_planted_k():
    """test-resnmtf.R:123-135 ("resnmtf runs with k not specified") in fp64 with spurious=True and stability=True: the
    reference's default pipeline; the k section 27's test picks, and the planted blocks survive the stability filter."""
    from test_gpu_bisil import planted as planted_blocks
    x1, rc, cc = planted_blocks(1)
    x2, _, _ = planted_blocks(2)
    res = api.apply_resnmtf([x1, x2], k_max=5, k_sweep=True, return_sweep=True, seed=3, precision="fp64", num_repeats=2,
                            n_stability=2, max_iters=MAX_ITERS, spurious=True, spurious_on_device=True, fp64_spurious=True,
                            fp64_stability=True)
    sweep = res["k_sweep"]
    assert sweep["k"][:3] == [3, 4, 5] and sweep["k"][int(np.argmax(sweep["bisil"]))] == 3
    assert res["output_f"][0].shape == (180, 3)
    for v in range(2):
        assert sorted(res["row_clusters"][v].sum(0)) == sorted(rc.sum(0))
        assert sorted(res["col_clusters"][v].sum(0)) == sorted(cc.sum(0))
