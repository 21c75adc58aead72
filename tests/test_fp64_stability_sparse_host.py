"""Host side of fp64 stability selection on sparse views (no GPU): the routing of
stability_check(precision="fp64", fp64_subsample_sparse=True) and apply_resnmtf(fp64_stability=True,
fp64_subsample_sparse=True) through stand-ins (``repeat_runner``, ``runner``, stand-in probes, fits and scorings), the extra
fit flags present only when a sub-sample is sparse, the flag as a no-op under f32 and without fp64_stability, every earlier
refusal word for word without the flag, the new refusals, and the exported symbol, struct and header lines."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import helpers
from resnmtf_amd import _lib, api, batched, build, engine
from stability_ref import fake_relevance, fake_results, fake_runner
from test_fp64_bisil_host import _never, _raw_data

CHECK_ARGS = (None, None, None, 5, False, 5, False, "euclidean")          # phi, xi, psi, n_iters, spurious, num_repeats, no_clusts, distance


def test_symbol_struct_and_header_lines():
    assert _lib.SIGNATURES["resnmtf_fp64_subsample_sparse"] == (C.c_int, [C.c_int, C.POINTER(_lib.Fp64SubsampleSparseJob)])
    assert [f[0] for f in _lib.Fp64SubsampleSparseJob._fields_] == [
        "struct_size", "n", "m", "n_sub", "m_sub", "rows", "cols", "x", "x_dev", "stream", "out_col_ptr", "out_row_idx", "out_values",
        "out_capacity", "nnz_sub", "n_empty_rows", "n_empty_cols", "row_mask", "col_mask"]
    # 5 ints (+ 4 of padding), 2 pointers, the host view (3 pointers), the device view (3 ints + 4 of padding, 3 pointers, a
    # long long), the stream, 3 pointers, a long long, 5 pointers
    assert C.sizeof(_lib.Fp64SubsampleSparseJob) == 24 + 16 + 24 + 48 + 8 + 24 + 8 + 40
    assert C.sizeof(_lib.Fp64SubsampleSparseJob) == (C.sizeof(_lib.Fp64ShuffleSparseJob) - 8) + 8 + 16 + 16
    lib = C.CDLL(build.build(verbose=False))                              # the built library exports the new entry
    assert hasattr(lib, "resnmtf_fp64_subsample_sparse")
    header = open(helpers.ROOT + "/include/resnmtf_hip.h").read()
    assert "int resnmtf_fp64_subsample_sparse(int device_id, const resnmtf_fp64_subsample_sparse_job* job);" in header
    comment = header.split("typedef struct resnmtf_fp64_subsample_sparse_job")[0][-6000:]
    assert "R/stability_analysis.r:124" in comment and "COUNT MODE" in comment and "DESIGN.md section 31" in comment
    body = header.split("typedef struct resnmtf_fp64_subsample_sparse_job {")[1].split("}")[0]
    for line in ("long long out_capacity;", "long long* nnz_sub;", "resnmtf_fp64_sparse_view x;", "resnmtf_fp64_sparse_device_view x_dev;"):
        assert line in body
    assert "#define RESNMTF_ABI_VERSION 2 " in header                    # the ABI version does not move


def test_engine_entries_refuse_before_the_library(monkeypatch):
    monkeypatch.setattr(_lib, "load", lambda: None)
    with pytest.raises(ValueError, match="fp64_subsample_sparse gathers sparse views .*: fp64_subsample takes a dense one"):
        engine.fp64_subsample_sparse(np.ones((4, 3)), [0], [0])
    x = sp.csc_matrix(np.eye(4))
    with pytest.raises(ValueError, match="fp64_subsample_sparse: rows must be a non-empty 1-D index list"):
        engine.fp64_subsample_sparse(x, [], [0])
    with pytest.raises(ValueError, match="fp64_subsample_sparse: cols must hold integers"):
        engine.fp64_subsample_sparse(x, [0], [0.5])
    with pytest.raises(ValueError, match="fp64_sparse_device_view takes sparse views"):
        engine.fp64_sparse_device_view(np.eye(3))


# ---- the repeats: which probe, which upload, which fit flags ----------------------------------------------------------
def _stand_ins(monkeypatch, n_v=2, k=4):
    log = {"dense": [], "sparse": [], "uploads": [], "sparse_uploads": [], "fits": [], "scored": []}

    def dense_probe(x, rows, cols, device_id=0):
        log["dense"].append(x)
        return ("dense sub", len(rows), len(cols)), np.zeros(len(rows), dtype=bool), np.zeros(len(cols), dtype=bool)

    def sparse_probe(x, rows, cols, device_id=0):
        log["sparse"].append(x)
        return ("sparse sub", len(rows), len(cols)), np.zeros(len(rows), dtype=bool), np.zeros(len(cols), dtype=bool)

    def inner(views, row_idx, col_idx, f, s, g, k_vec, phi, xi, psi, n_iters, num_repeats, spurious, **kw):
        log["fits"].append((views, num_repeats, spurious, kw))
        return {"row_clusters": [("rc", v, kw["seed"]) for v in range(n_v)], "col_clusters": [("cc", v, kw["seed"]) for v in range(n_v)],
                "Error": 0.25, "All_Error": np.array([0.5, 0.25])}

    def relevance(row_c, col_c, true_r, true_c, rows, cols, device_id=0):
        log["scored"].append((row_c, col_c))
        return fake_relevance(row_c[2], n_v, k)[row_c[1]]
    monkeypatch.setattr(engine, "fp64_subsample", dense_probe)
    monkeypatch.setattr(engine, "fp64_subsample_sparse", sparse_probe)
    monkeypatch.setattr(engine, "fp64_device_view", lambda x, device_id=0: log["uploads"].append(x) or x)
    monkeypatch.setattr(engine, "fp64_sparse_device_view", lambda x, device_id=0: log["sparse_uploads"].append(x) or x)
    monkeypatch.setattr(engine, "fp64_relevance", relevance)
    monkeypatch.setattr(api, "res_nmtf_inner", inner)
    return log


def _names(data):
    return [[f"r{t}" for t in range(d.shape[0])] for d in data], [[f"v{v}c{t}" for t in range(d.shape[1])] for v, d in enumerate(data)]


def test_a_sparse_view_takes_the_sparse_probe_and_the_fit_gets_the_flags_only_then(monkeypatch):
    res, data = fake_results()
    log = _stand_ins(monkeypatch)
    mixed = [sp.csc_matrix(data[0]), data[1]]
    rn, cn = _names(mixed)
    z = np.zeros((2, 2))
    out = batched.stability_relevance_fp64(mixed, res, 4, 3, 0.9, 11, 7, z, z, z, rn, cn, max_iters=500)
    assert out["stability_performed"] and len(log["fits"]) == 3
    # every view is brought to the device once, the sparse one as a sparse view; per repeat one probe per view
    assert log["sparse_uploads"] == [mixed[0]] and len(log["uploads"]) == 1 and log["uploads"][0] is mixed[1]
    assert len(log["sparse"]) == 3 and all(x is mixed[0] for x in log["sparse"])
    assert len(log["dense"]) == 3 and all(x is mixed[1] for x in log["dense"])
    draws = batched.stability_draws([d.shape for d in mixed], 3, 0.9, 7)
    total = np.zeros((2, 4))
    for r, (views, num_repeats, spurious, kw) in enumerate(log["fits"]):
        # the tensor of a view's last probe IS its sub-sample: nothing is gathered twice
        assert views == [("sparse sub", len(draws[r][0][0]), len(draws[r][1][0])), ("dense sub", len(draws[r][0][1]), len(draws[r][1][1]))]
        assert kw["fp64_sparse_device"] is True and kw["fp64_device"] is True and kw["output"] == "torch" and kw["precision"] == "fp64"
        assert kw["seed"] == 7 + 2000 + r and kw["max_iters"] == 500 and spurious is False
        assert "fp64_shuffle_sparse" not in kw and "fp64_spurious" not in kw and "spurious_on_device" not in kw
        total = total + np.stack([fake_relevance(7 + 2000 + r)[v] for v in range(2)])
    assert out["relevance"].tobytes() == (total / 3).tobytes()       # the scoring and the reduction are unchanged
    assert len(log["scored"]) == 6
    # with removal inside the repeats: the sparse shuffle's flag beside the removal's
    log["fits"].clear()
    batched.stability_relevance_fp64(mixed, res, 4, 1, 0.9, 11, 7, z, z, z, rn, cn, spurious_repeats=4)
    views, num_repeats, spurious, kw = log["fits"][0]
    assert num_repeats == 4 and spurious is True
    assert kw["spurious_on_device"] is True and kw["fp64_spurious"] is True and kw["fp64_sparse_device"] is True and kw["fp64_shuffle_sparse"] is True
    # without a sparse view the calls are exactly the calls they were
    for key in log:
        log[key].clear()
    rn, cn = _names(data)
    batched.stability_relevance_fp64(data, res, 4, 2, 0.9, 11, 7, z, z, z, rn, cn, spurious_repeats=4)
    assert log["sparse"] == [] and log["sparse_uploads"] == [] and len(log["uploads"]) == 2 and len(log["dense"]) == 4
    for views, num_repeats, spurious, kw in log["fits"]:
        assert "fp64_sparse_device" not in kw and "fp64_shuffle_sparse" not in kw and kw["fp64_spurious"] is True
        assert sorted(kw) == sorted(["row_names", "col_names", "device_id", "max_iters", "seed", "spurious_on_device", "fp64_spurious",
                                     "precision", "fp64_device", "output"])


def test_a_sparse_sub_sample_with_empty_lines_is_trimmed_through_the_same_loop(monkeypatch):
    res, data = fake_results()
    log = _stand_ins(monkeypatch)
    x = sp.csc_matrix(data[0])
    probes = []

    def sparse_probe(view, rows, cols, device_id=0):
        probes.append((np.array(rows), np.array(cols)))
        er = np.asarray(rows) == 5                                    # source row 5 is empty whenever it is drawn
        return ("sparse sub", len(rows), len(cols)), er, np.zeros(len(cols), dtype=bool)
    monkeypatch.setattr(engine, "fp64_subsample_sparse", sparse_probe)
    rn, cn = _names([x])
    z = np.zeros((1, 1))
    rows, cols = np.arange(30)[::-1].copy(), np.arange(20)
    rep = batched.stability_repeat_fp64([x], res, 4, 11, 7, ([rows], [cols]), z, z, z, rn, cn)
    assert len(probes) == 2 and 5 in probes[0][0] and 5 not in probes[1][0]
    assert np.array_equal(rep["extras"]["row_samples"][0], rows[rows != 5])
    assert log["fits"][0][0] == [("sparse sub", 29, 20)]              # the last probe's tensor, at the trimmed lists
    assert log["fits"][0][3]["row_names"] == [[rn[0][t] for t in rows[rows != 5]]]


def test_stability_check_admits_sparse_views_with_the_flag_and_calls_as_before(monkeypatch):
    seen = {}

    def stand_in(data, results, k, n_stability, sample_rate, n_iters, seed, phi, xi, psi, row_names, col_names, max_iters, device_id,
                 keep_clusters=False, spurious_repeats=0, runner=None):          # (the signature as it was: nothing new is passed)
        seen.update(locals())
        return {"stability_performed": True, "relevance": np.full((2, 4), 0.7), "repeats": []}
    monkeypatch.setattr(batched, "stability_relevance_fp64", stand_in)
    monkeypatch.setattr(batched, "DeviceData", _never)
    res, data = fake_results()
    mixed = [data[0], sp.csr_matrix(data[1])]
    z = np.zeros((2, 2))
    api.stability_check(mixed, res, [4, 4], z, z, z, 9, True, 3, False, "euclidean", 0.8, 2, seed=5, max_iters=77, spurious_on_device=True,
                        precision="fp64", fp64_subsample_sparse=True, fp64_shuffle_sparse=True)
    assert (seen["k"], seen["n_stability"], seen["spurious_repeats"], seen["max_iters"]) == (4, 2, 3, 77)
    assert seen["data"][0] is not None and sp.issparse(seen["data"][1]) and [len(r) for r in seen["row_names"]] == [30, 25]
    # through repeat_runner: the reduction is the one every route shares
    monkeypatch.undo()
    monkeypatch.setattr(batched, "DeviceData", _never)
    monkeypatch.setattr(engine, "fp64_subsample_sparse", _never)
    out = api.stability_check(mixed, res, 4, *CHECK_ARGS, 0.9, 5, 0.6, False, repeat_runner=fake_runner(), seed=3, precision="fp64",
                              fp64_subsample_sparse=True)
    total = np.zeros((2, 4))
    for r in range(5):
        total = total + fake_relevance(r)
    assert out["relevance"].tobytes() == (total / 5).tobytes()


# ---- refusals -------------------------------------------------------------------------------------------------------
def test_new_refusals_and_the_ones_that_stay(monkeypatch):
    monkeypatch.setattr(batched, "DeviceData", _never)
    monkeypatch.setattr(batched, "stability_relevance_fp64", _never)
    res, data = fake_results()
    mixed = [data[0], sp.csc_matrix(data[1])]
    with pytest.raises(TypeError):                                        # keyword-only
        api.stability_check(data, res, 4, *CHECK_ARGS, 0.9, 5, 0.6, True, "fp64", True)
    with pytest.raises(NotImplementedError) as e:                         # without the flag: word for word
        api.stability_check(mixed, res, 4, *CHECK_ARGS, precision="fp64")
    assert str(e.value) == ('stability_check(precision="fp64"): a sparse view (view 1) is not supported: resnmtf_fp64_subsample '
                            'gathers dense views')
    with pytest.raises(NotImplementedError) as e:                         # the shuffle's flag alone does not admit it
        api.stability_check(mixed, res, 4, *CHECK_ARGS, precision="fp64", fp64_shuffle_sparse=True)
    assert "a sparse view (view 1) is not supported: resnmtf_fp64_subsample gathers dense views" in str(e.value)
    with pytest.raises(NotImplementedError) as e:                         # new: removal on a sparse view needs the second flag
        api.stability_check(mixed, res, 4, None, None, None, 5, True, 5, False, "euclidean", precision="fp64", spurious_on_device=True,
                            fp64_subsample_sparse=True)
    assert str(e.value) == ('stability_check(precision="fp64"): spurious=True on a sparse view (view 1) is not supported without '
                            'fp64_shuffle_sparse=True: the removal inside a repeat shuffles the sparse sub-sample '
                            '(resnmtf_fp64_shuffle_sparse)')
    for flag, kw in (("group", dict(group=object())), ("sparse_on_device", dict(sparse_on_device=True)),
                     ("shuffle_sparse", dict(shuffle_sparse=True))):     # these stay refused, with the flag too
        with pytest.raises(NotImplementedError) as e:
            api.stability_check(mixed, res, 4, *CHECK_ARGS, precision="fp64", fp64_subsample_sparse=True, **kw)
        assert str(e.value) == (f'stability_check(precision="fp64"): {flag} is not supported: the fp64 repeats run one after the '
                                'other on dense views')
    with pytest.raises(NotImplementedError, match="outside the accelerated path; pass spurious=False"):
        api.stability_check(mixed, res, 4, None, None, None, 5, True, 5, False, "euclidean", precision="fp64", fp64_subsample_sparse=True,
                            fp64_shuffle_sparse=True)
    # under f32 the two flags are not read: the f32 refusal of removal on sparse views stands
    with pytest.raises(NotImplementedError, match="device shuffles of sparse views are not supported"):
        api.stability_check(mixed, res, 4, None, None, None, 5, True, 5, False, "euclidean", spurious_on_device=True,
                            fp64_subsample_sparse=True, fp64_shuffle_sparse=True)


def test_the_flag_is_a_no_op_under_f32_and_without_fp64_stability(monkeypatch):
    calls = []

    def inner(*args, **kw):
        calls.append(("inner", sorted(kw)))
        return fake_results()[0]

    def check(*args, **kw):
        calls.append(("check", sorted(kw)))
        return "checked"
    monkeypatch.setattr(api, "res_nmtf_inner", inner)
    monkeypatch.setattr(api, "stability_check", check)
    data = _raw_data()
    plain = api.apply_resnmtf(data, k_val=3, spurious=False, seed=1)
    want = list(calls)
    calls.clear()
    flagged = api.apply_resnmtf(data, k_val=3, spurious=False, seed=1, fp64_subsample_sparse=True)
    assert plain == flagged == "checked" and calls == want and "fp64_subsample_sparse" not in dict(calls)["check"]
    # precision="fp64" with stability=False: no check at all, and the fit is the call it was
    calls.clear()
    api.apply_resnmtf(data, k_val=3, spurious=False, stability=False, precision="fp64")
    want = list(calls)
    calls.clear()
    api.apply_resnmtf(data, k_val=3, spurious=False, stability=False, precision="fp64", fp64_subsample_sparse=True)
    assert calls == want and [c[0] for c in calls] == ["inner"]
    # the flag does not replace fp64_stability
    with pytest.raises(NotImplementedError, match="stability=True is not supported: the stability repeats run on the f32 engine"):
        api.apply_resnmtf([sp.csc_matrix(data[0]), data[1]], k_val=3, spurious=False, precision="fp64", fp64_sparse=True,
                          fp64_subsample_sparse=True)
    with pytest.raises(TypeError):                                        # keyword-only
        api.apply_resnmtf(data, None, None, None, 3, None, None, None, 5, 3, 8, "euclidean", False, 5, False, 0.9, 5, True, 0.4,
                          True, True, True)


def test_without_the_flag_every_refusal_of_apply_stands_word_for_word(monkeypatch):
    monkeypatch.setattr(api, "Engine", _never)
    monkeypatch.setattr(engine, "fp64_run", _never)
    monkeypatch.setattr(engine, "fp64_subsample_sparse", _never)
    data = _raw_data()
    sparse_data = [sp.csc_matrix(data[0]), data[1]]
    with pytest.raises(NotImplementedError) as e:
        api.apply_resnmtf(sparse_data, k_val=3, spurious=False, precision="fp64", fp64_sparse=True, fp64_stability=True)
    assert str(e.value) == ('apply_resnmtf(precision="fp64"): a sparse view with fp64_stability is not supported: '
                            'resnmtf_fp64_subsample gathers dense views; pass stability=False')
    with pytest.raises(NotImplementedError) as e:                         # the shuffle's flag does not lift it
        api.apply_resnmtf(sparse_data, k_val=3, spurious=False, precision="fp64", fp64_sparse=True, fp64_stability=True,
                          fp64_shuffle_sparse=True)
    assert "a sparse view with fp64_stability is not supported" in str(e.value)
    with pytest.raises(NotImplementedError) as e:                         # with it, removal on a sparse view still needs its own flag
        api.apply_resnmtf(sparse_data, k_val=3, precision="fp64", fp64_sparse=True, fp64_stability=True, fp64_subsample_sparse=True,
                          spurious_on_device=True, fp64_spurious=True)
    assert str(e.value) == ('apply_resnmtf(precision="fp64"): a sparse view with fp64_spurious is not supported: no fp64 sparse '
                            'shuffle exists; pass spurious=False')


def test_apply_passes_the_flags_on_only_when_set_after_the_fit_and_after_the_pick(monkeypatch):
    calls, checks = [], []
    scores = {3: 0.2, 4: 0.6, 5: 0.7, 6: 0.4}

    def inner(data, row_idx, col_idx, f, s, g, k_vec, *rest, **kw):
        calls.append((list(k_vec), kw))
        return {"bisil": scores[k_vec[0]], "k": k_vec[0]}

    def check(data, results, k, phi, xi, psi, n_iters, spurious, num_repeats, no_clusts, distance, *rest, **kw):
        checks.append((data, list(k), spurious, rest, kw))
        return dict(results, checked=True)
    monkeypatch.setattr(api, "res_nmtf_inner", inner)
    monkeypatch.setattr(api, "stability_check", check)
    dense = _raw_data()
    data = [sp.csc_matrix(dense[0]), dense[1]]
    sparse_flags = dict(precision="fp64", fp64_sparse=True, fp64_stability=True, fp64_subsample_sparse=True)
    out = api.apply_resnmtf(data, k_val=3, spurious=False, seed=11, **sparse_flags)
    assert out["checked"] and [c[0] for c in calls] == [[3, 3]]
    views, k, spurious, rest, kw = checks.pop()
    assert kw["fp64_subsample_sparse"] is True and "fp64_shuffle_sparse" not in kw and kw["precision"] == "fp64" and k == [3, 3]
    assert sp.issparse(views[0]) and abs(np.asarray(views[0].sum(0)) - 1).max() < 1e-12            # the prepared data, still sparse
    calls.clear()
    out = api.apply_resnmtf(data, k_min=3, k_max=5, seed=100, k_sweep=True, num_repeats=4, spurious=True, spurious_on_device=True,
                            fp64_spurious=True, fp64_shuffle_sparse=True, fp64_bisil_sparse=True, remove_unstable=False, **sparse_flags)
    assert [c[0] for c in calls] == [[3, 3], [4, 4], [5, 5], [6, 6]] and out["k"] == 5 and out["checked"]
    assert all(c[1]["fp64_shuffle_sparse"] is True and "fp64_subsample_sparse" not in c[1] for c in calls)
    views, k, spurious, rest, kw = checks.pop()
    assert k == [5, 5] and spurious is True and rest == (0.9, 5, 0.4, False)
    assert kw["fp64_subsample_sparse"] is True and kw["fp64_shuffle_sparse"] is True and kw["spurious_on_device"] is True
    # dense data without the flag: the check's keywords are exactly those of before
    api.apply_resnmtf(dense, k_val=3, spurious=False, seed=11, precision="fp64", fp64_stability=True)
    views, k, spurious, rest, kw = checks.pop()
    assert sorted(kw) == sorted(["row_names", "col_names", "device_id", "seed", "max_iters", "spurious_on_device", "output", "precision"])
