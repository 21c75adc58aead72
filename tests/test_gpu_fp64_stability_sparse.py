"""Stability selection in double precision on SPARSE views: stability_check(precision="fp64",
fp64_subsample_sparse=True) and apply_resnmtf(precision="fp64", fp64_stability=True, fp64_subsample_sparse=True) against
their parts -- the trimmed lists against trim_samples with a NumPy probe and against the f32 route, every repeat's relevance
bit for bit stability_ref.relevance_counts of the clusters it kept, the mean bit for bit total / n_stability, a repeat
rebuilt by hand, device tensors in, a sparse + dense pair, the removal inside a repeat against remove_spurious on its
sub-sample, the dense fp64 route on the densified views, the whole pipeline, and the refusals that remain.

The problem is the planted two-view 180 x 180 one of tests/subsample_ref.planted_sparse(1) and (2), column-normalised, k = 3,
n_stability = 3, sample_rate = 0.8, seed 9; every fit is guarded by max_iters = MAX_ITERS (the same guard on both sides of
every comparison).  So that the trimming runs: in view s, for i in 0, 4, ..., 36, row i + (s - 1) is zeroed and its entry in
column (7 i + 11 s) mod 180 set to 0.25 -- such a row is empty in every sub-sample that does not draw that column.  With
these views trim_samples drops one or two rows in each of the three repeats and reaches its fixed point in the second
round: the lists go from (144, 144) to 142-143 rows (checked below on the CPU).

Against the dense fp64 route on the densified views the trimmed lists are identical (the masks are bit-equal); the fits
differ by the sum orders of the sparse and the dense fp64 runs, so no tolerance is fixed in advance: the decisions
`relevance < 0.6` must be equal, and the test prints the largest |relevance difference| and the dense route's smallest
margin |relevance - 0.6| before it asserts.  Measured on the MI355X: largest difference 0.0, smallest margin 0.339
(DESIGN.md section 31)."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import resnmtf_amd
from resnmtf_amd import api, batched, engine, naming, sparse
from stability_ref import relevance_counts
from subsample_ref import f32, planted_sparse, subsample_csc

gpu = pytest.mark.gpu

K, N_STAB, RATE, SEED, MAX_ITERS, FIT_SEED = 3, 3, 0.8, 9, 300, 4
ZERO = np.zeros((2, 2))


def host(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)


@functools.lru_cache(maxsize=None)
def dense_views():
    """The two pre-processed views as dense arrays, with the single-entry rows that make the trimming run."""
    out = []
    for s in (1, 2):
        x = planted_sparse(s)[0].toarray()
        x = x / x.sum(axis=0)
        for i in range(0, 40, 4):
            x[i + (s - 1), :] = 0.0
            x[i + (s - 1), (7 * i + 11 * s) % 180] = 0.25
        out.append(x)
    return out


@functools.lru_cache(maxsize=None)
def prepared():
    pre = [sparse.canonical_csc(sp.csc_matrix(x)) for x in dense_views()]
    rn, cn = naming.give_names(pre, None, None, None, None)
    return pre, naming.shared_names(rn), naming.shared_names(cn), rn, cn


@functools.lru_cache(maxsize=None)
def fitted():
    """The fp64 fit of the whole views: the reference clusters of every check below."""
    pre, ri, ci, rn, cn = prepared()
    return api.res_nmtf_inner(pre, ri, ci, k_vec=[K, K], row_names=rn, col_names=cn, spurious=False, precision="fp64",
                              fp64_sparse=True, max_iters=MAX_ITERS, seed=FIT_SEED)


def check(data=None, res=None, **more):
    pre, _, _, rn, cn = prepared()
    kw = dict(row_names=rn, col_names=cn, seed=SEED, n_stability=N_STAB, sample_rate=RATE, precision="fp64", max_iters=MAX_ITERS,
              fp64_subsample_sparse=True)
    kw.update(more)
    return api.stability_check(pre if data is None else data, fitted() if res is None else res, K, ZERO, ZERO, ZERO, None, False, 5,
                               False, "euclidean", **kw)


@functools.lru_cache(maxsize=None)
def checked():
    return check(remove_unstable=False, return_repeats=True)


def numpy_trim(views, r):
    shapes = [v.shape for v in views]
    draws = batched.stability_draws(shapes, N_STAB, RATE, SEED)
    rounds = [0]

    def probe(i, rows, cols):
        rounds[0] += 1
        sub = views[i][np.ix_(rows, cols)]
        return ~(sub > 0).any(axis=1), ~(sub > 0).any(axis=0)
    rows, cols = batched.trim_samples(shapes, draws[r], probe)
    return draws[r], rows, cols, rounds[0]


def test_the_trimming_runs_and_ends_on_these_views():
    for r in range(N_STAB):
        drawn, rows, cols, probes = numpy_trim(dense_views(), r)
        assert [len(x) for x in drawn[0]] == [144, 144] and probes == 4              # two rounds of two views
        assert all(142 <= len(x) <= 143 for x in rows) and [len(x) for x in cols] == [144, 144]


@gpu
def test_trimmed_lists_relevance_and_mean():
    pre = prepared()[0]
    res = fitted()
    out = checked()
    rel = out["relevance"]
    assert out["res"] is res and rel.shape == (2, K)
    reps = out["stability"]["repeats"]
    assert len(reps) == N_STAB
    total = np.zeros((2, K))
    for r, rep in enumerate(reps):
        assert list(rep) == ["stability_performed", "relevance", "Error", "All_Error", "tag", "extras", "row_clusters", "col_clusters"]
        rows, cols = rep["extras"]["row_samples"], rep["extras"]["col_samples"]
        _, want_r, want_c, _ = numpy_trim(dense_views(), r)
        for v in range(2):                                           # the trimmed lists are those of the NumPy probe
            assert np.array_equal(rows[v], want_r[v]) and np.array_equal(cols[v], want_c[v])
            assert len(rows[v]) < 144
        one = np.stack([relevance_counts(rep["row_clusters"][v], rep["col_clusters"][v], res["row_clusters"][v][rows[v]],
                                         res["col_clusters"][v][cols[v]]) for v in range(2)])
        assert one.tobytes() == np.asarray(rep["relevance"]).tobytes()
        assert rep["tag"] == f"stability={r}" and len(rep["All_Error"]) <= MAX_ITERS
        total = total + one
    assert (total / N_STAB).tobytes() == rel.tobytes()
    assert rel.max() > 0.5                                           # the planted blocks are found again
    again = check(remove_unstable=False)
    assert again["relevance"].tobytes() == rel.tobytes()            # same seed, same bits
    assert sparse.is_sparse(pre[0])


@gpu
def test_on_data_fp32_holds_the_trimmed_lists_are_the_f32_routes():
    pre, _, _, rn, cn = prepared()
    data = []
    for d in pre:
        c = d.copy(); c.data = f32(c.data)
        data.append(c)
    draws = batched.stability_draws([d.shape for d in data], N_STAB, RATE, SEED)
    ref = {"row_clusters": [np.ones((180, K))] * 2, "col_clusters": [np.ones((180, K))] * 2}
    dev = batched.DeviceData(data, ZERO, ZERO, ZERO, rn, cn, pre_processed=True)
    try:
        for r in range(N_STAB):
            want = dev.factorise(K, 2, SEED + 2000 + r, samples=draws[r], sparse_on_device=True)
            rep = batched.stability_repeat_fp64(data, ref, K, 2, SEED + 2000 + r, draws[r], ZERO, ZERO, ZERO, rn, cn)
            _, np_r, np_c, _ = numpy_trim(dense_views(), r)
            for v in range(2):
                assert np.array_equal(rep["extras"]["row_samples"][v], want["extras"]["row_samples"][v])
                assert np.array_equal(rep["extras"]["col_samples"][v], want["extras"]["col_samples"][v])
                assert np.array_equal(rep["extras"]["row_samples"][v], np_r[v]) and len(np_r[v]) < 144
    finally:
        dev.close()


@gpu
def test_a_repeat_rebuilt_by_hand_is_equal_bit_for_bit():
    pre, _, _, rn, cn = prepared()
    res = fitted()
    r = 1
    rep = checked()["stability"]["repeats"][r]
    rows, cols = rep["extras"]["row_samples"], rep["extras"]["col_samples"]
    subs = []
    for v in range(2):
        t, er, ec = engine.fp64_subsample_sparse(pre[v], rows[v], cols[v])
        assert not er.any() and not ec.any()                       # the fixed point
        subs.append(t)
    fit = api.res_nmtf_inner(subs, None, None, None, None, None, [K, K], ZERO, ZERO, ZERO, None, spurious=False,
                             row_names=[[rn[v][t] for t in rows[v]] for v in range(2)],
                             col_names=[[cn[v][t] for t in cols[v]] for v in range(2)], seed=SEED + 2000 + r, max_iters=MAX_ITERS,
                             precision="fp64", fp64_device=True, fp64_sparse_device=True, output="torch")
    assert np.array_equal(fit["All_Error"], rep["All_Error"])
    for v in range(2):
        assert np.array_equal(host(fit["row_clusters"][v]), rep["row_clusters"][v])
        assert np.array_equal(host(fit["col_clusters"][v]), rep["col_clusters"][v])
        got = engine.fp64_relevance(fit["row_clusters"][v], fit["col_clusters"][v], res["row_clusters"][v], res["col_clusters"][v],
                                    rows[v], cols[v])
        assert got.tobytes() == np.asarray(rep["relevance"][v]).tobytes()


@gpu
def test_device_tensors_in_and_a_sparse_and_dense_pair():
    import torch
    pre = prepared()[0]
    res = fitted()
    dev = torch.device("cuda", 0)
    rel = checked()["relevance"]
    there = [torch.sparse_csc_tensor(torch.as_tensor(c.indptr, dtype=torch.int64, device=dev), torch.as_tensor(c.indices, dtype=torch.int64, device=dev),
                                     torch.as_tensor(c.data, device=dev), c.shape) for c in pre]
    res_t = dict(res, row_clusters=[torch.as_tensor(a, device=dev) for a in res["row_clusters"]],
                 col_clusters=[torch.as_tensor(a, device=dev) for a in res["col_clusters"]])
    on_device = check(data=there, res=res_t, remove_unstable=False, output="torch")
    assert on_device["relevance"].tobytes() == rel.tobytes()        # the bits of the scipy.sparse route
    cut_t, cut = check(data=there, res=res_t, stab_thres=0.6, output="torch"), check(stab_thres=0.6)
    for key in ("row_clusters", "col_clusters"):
        for v in range(2):
            assert isinstance(cut_t[key][v], torch.Tensor) and cut_t[key][v].device == dev
            assert np.array_equal(host(cut_t[key][v]), cut[key][v])
    # a sparse and a dense view: runs, and the trimmed lists are still those of the NumPy probe
    mixed = check(data=[pre[0], dense_views()[1]], remove_unstable=False, return_repeats=True)
    assert mixed["relevance"].shape == (2, K) and np.isfinite(mixed["relevance"]).all()
    for r, rep in enumerate(mixed["stability"]["repeats"]):
        _, want_r, want_c, _ = numpy_trim(dense_views(), r)
        assert all(np.array_equal(a, b) for a, b in zip(rep["extras"]["row_samples"], want_r))
        assert all(np.array_equal(a, b) for a, b in zip(rep["extras"]["col_samples"], want_c))


@gpu
def test_one_repeat_with_removal_equals_remove_spurious_on_its_sub_sample():
    pre, _, _, rn, cn = prepared()
    ref = fitted()
    R, r = 3, 0
    draws = batched.stability_draws([d.shape for d in pre], N_STAB, RATE, SEED)
    seed = SEED + 2000 + r
    rep = batched.stability_repeat_fp64(pre, ref, K, None, seed, draws[r], ZERO, ZERO, ZERO, rn, cn, max_iters=MAX_ITERS,
                                        keep_clusters=True, spurious_repeats=R)
    rows, cols = rep["extras"]["row_samples"], rep["extras"]["col_samples"]
    subs = [subsample_csc(pre[v], rows[v], cols[v]) for v in range(2)]
    names = dict(row_names=[[rn[v][t] for t in rows[v]] for v in range(2)], col_names=[[cn[v][t] for t in cols[v]] for v in range(2)])
    plain = api.res_nmtf_inner(subs, None, None, None, None, None, [K, K], ZERO, ZERO, ZERO, None, spurious=False, seed=seed,
                               max_iters=MAX_ITERS, precision="fp64", fp64_sparse=True, **names)
    post = api.remove_spurious(subs, plain, R, seed=seed, precision="fp64", max_iters=MAX_ITERS, fp64_shuffle_sparse=True)
    for v in range(2):
        assert np.array_equal(rep["row_clusters"][v], post["row_clusters"][v])
        assert np.array_equal(rep["col_clusters"][v], post["col_clusters"][v])
        want = relevance_counts(post["row_clusters"][v], post["col_clusters"][v], ref["row_clusters"][v][rows[v]],
                                ref["col_clusters"][v][cols[v]])
        assert want.tobytes() == np.asarray(rep["relevance"][v]).tobytes()
    assert np.array_equal(rep["All_Error"], plain["All_Error"])


@gpu
def test_decisions_are_those_of_the_dense_fp64_route_on_the_densified_views():
    got = checked()
    dense = check(data=dense_views(), remove_unstable=False, return_repeats=True, fp64_subsample_sparse=False)
    for a, b in zip(got["stability"]["repeats"], dense["stability"]["repeats"]):
        for key in ("row_samples", "col_samples"):                   # the masks are bit-equal, so the lists are identical
            assert all(np.array_equal(x, y) for x, y in zip(a["extras"][key], b["extras"][key]))
    diff = float(np.abs(got["relevance"] - dense["relevance"]).max())
    margin = float(np.abs(dense["relevance"] - 0.6).min())
    print(f"MEASURED largest |relevance difference| sparse - dense: {diff:.3e}; the dense route's smallest margin "
          f"|relevance - 0.6|: {margin:.3e}")
    assert np.array_equal(got["relevance"] < 0.6, dense["relevance"] < 0.6)


@gpu
def test_the_default_pipeline_on_sparse_views():
    """The sparsified planted views of tests/test_gpu_fp64_spurious_sparse.py, k sweep 2 ... 4: the sweep picks the planted
    k = 3, and the stability step is stability_check(precision="fp64", fp64_subsample_sparse=True) on the prepared data."""
    from test_gpu_bisil_sparse import planted
    data = []
    for seed in (1, 2):
        x = planted(seed)
        data.append(sp.csc_matrix(np.where(x > 0.2, x, 0.0)))
    common = dict(precision="fp64", num_repeats=2, max_iters=MAX_ITERS, n_iters=40, fp64_sparse=True, fp64_bisil_sparse=True,
                  spurious=True, spurious_on_device=True, fp64_spurious=True, fp64_shuffle_sparse=True, k_min=2, k_max=4, k_sweep=True,
                  seed=3)
    full = resnmtf_amd.apply_resnmtf(data, n_stability=2, return_sweep=True, fp64_stability=True, fp64_subsample_sparse=True, **common)
    sweep = full["k_sweep"]
    print("MEASURED fp64 default pipeline on sparse views:", sweep)
    assert sweep["k"][:3] == [2, 3, 4] and sweep["k"][int(np.argmax(sweep["bisil"]))] == 3
    assert [f.shape[1] for f in full["output_f"]] == [3, 3]
    before = resnmtf_amd.apply_resnmtf(data, stability=False, **common)
    p = api.prepare(api._views(data), None, None, None, None, None, normalise=True, symmetrise=True)
    want = api.stability_check(p.data, before, [3, 3], p.phi, p.xi, p.psi, 40, True, 2, False, "euclidean", 0.9, 2, 0.4, True,
                               row_names=p.row_names, col_names=p.col_names, seed=3, max_iters=MAX_ITERS, spurious_on_device=True,
                               precision="fp64", fp64_subsample_sparse=True, fp64_shuffle_sparse=True)
    for key in ("row_clusters", "col_clusters", "output_f", "output_s", "output_g"):
        for v in range(2):
            assert np.asarray(full[key][v]).tobytes() == np.asarray(want[key][v]).tobytes(), (key, v)
    assert any(np.asarray(c).any() for c in full["row_clusters"])


@gpu
def test_refusals_that_remain():
    import torch
    pre = prepared()[0]
    res = fitted()
    with pytest.raises(NotImplementedError, match=r"a sparse view \(view 0\) is not supported: resnmtf_fp64_subsample gathers dense views"):
        check(fp64_subsample_sparse=False)
    with pytest.raises(NotImplementedError, match=r"spurious=True on a sparse view \(view 0\) is not supported without fp64_shuffle_sparse=True"):
        api.stability_check(pre, res, K, ZERO, ZERO, ZERO, None, True, 3, False, "euclidean", precision="fp64", spurious_on_device=True,
                            fp64_subsample_sparse=True)
    for flag in ("sparse_on_device", "shuffle_sparse"):
        with pytest.raises(NotImplementedError, match=flag + " is not supported: the fp64 repeats run one after the other on dense views"):
            check(**{flag: True})
    with pytest.raises(NotImplementedError, match="a sparse view with fp64_stability is not supported: resnmtf_fp64_subsample gathers dense views"):
        resnmtf_amd.apply_resnmtf([pre[0]], k_val=3, spurious=False, precision="fp64", fp64_sparse=True, fp64_stability=True)
    t = torch.as_tensor(pre[0].toarray(), device=torch.device("cuda", 0)).to_sparse_csc()
    with pytest.raises(NotImplementedError, match="a view in device memory is not supported"):
        resnmtf_amd.apply_resnmtf([t], k_val=3, spurious=False, precision="fp64", fp64_sparse_device=True, fp64_stability=True,
                                  fp64_subsample_sparse=True)
