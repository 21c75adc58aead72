"""Host side of the fp64 bisilhouette of sparse views (api.res_nmtf_inner / api.apply_resnmtf(fp64_bisil_sparse=True),
engine.fp64_bisil_sparse; no GPU): with the flag a sparse view is scored through a stand-in for
``engine.fp64_bisil_sparse`` and a dense one through ``engine.fp64_bisil``, on the views as the run received them; the flag
does nothing under f32 and without ``fp64_bisil``; without it every earlier refusal keeps its text; with it the refusals
that remain carry theirs; ``apply_resnmtf`` passes it through for a ``k_val`` and for every k of the sweep; the library
exports the symbol and agrees with the binding on the struct's size."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

from resnmtf_amd import _lib, api, bisil, build, device_views, engine
from test_fp64_bisil_host import _echo, _inner_args, _never, _raw_data, _sil_log

FLAGS = dict(spurious=False, precision="fp64", fp64_sparse=True, score_bisil=True, fp64_bisil=True)


def _mixed(n_views=2, sparse_at=1):
    """The arguments of res_nmtf_inner with view ``sparse_at`` given as a scipy.sparse matrix."""
    args = list(_inner_args(n_views))
    data = [sp.csc_matrix(x) if v == sparse_at else x for v, x in enumerate(args[0])]
    return [data] + args[1:]


def test_symbol_struct_and_size():
    assert "resnmtf_fp64_bisil_sparse" in _lib.SIGNATURES
    names = [f[0] for f in _lib.Fp64BisilSparseJob._fields_]
    assert names == ["struct_size", "n", "m", "k", "metric", "x", "x_dev", "stream", "row_clusters", "col_clusters",
                     "row_sil", "col_sil"]
    # five ints (padded to 24), the host CSC (three pointers), the device view (three ints padded to 16, three pointers,
    # one int64), the stream and four pointers
    assert C.sizeof(_lib.Fp64BisilSparseJob) == 24 + 24 + 48 + 8 + 32
    lib = C.CDLL(build.build(verbose=False))
    assert hasattr(lib, "resnmtf_fp64_bisil_sparse")
    # the library's own sizeof: a job of the binding's size passes the size check and meets the next refusal (k = 0)
    lib.resnmtf_last_error.restype = C.c_char_p
    job = _lib.Fp64BisilSparseJob()
    job.struct_size = C.sizeof(job)
    assert lib.resnmtf_fp64_bisil_sparse(0, C.byref(job)) == 1
    assert lib.resnmtf_last_error(None) == b"k must be in [1, 64]"
    job.struct_size += 8
    assert lib.resnmtf_fp64_bisil_sparse(0, C.byref(job)) == 1
    assert lib.resnmtf_last_error(None) == b"resnmtf_fp64_bisil_sparse_job struct_size mismatch"
    assert lib.resnmtf_fp64_bisil_sparse(0, None) == 1
    header = open(build.ROOT + "/include/resnmtf_hip.h").read()
    assert "int resnmtf_fp64_bisil_sparse(int device_id, const resnmtf_fp64_bisil_sparse_job* job);" in header
    assert "#define RESNMTF_ABI_VERSION 2 " in header                    # the ABI version does not move


def test_library_refusals_need_no_device():
    """What resnmtf_fp64_bisil_sparse refuses of a host view comes before any device work, with the texts of
    resnmtf_fp64_bisil and resnmtf_fp64_run_sparse; the outputs keep their sentinel."""
    lib = _lib.load()
    n, m, k = 6, 4, 2
    rc, cc = np.asfortranarray(np.ones((n, k))), np.asfortranarray(np.ones((m, k)))
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))              # noqa: E731

    def call(ptr=(0, 2, 3, 5, 6), idx=(0, 3, 1, 0, 5, 2), vals=(1, 2, 3, 4, 5, 6), metric=0, dev=False, no_x=False, **over):
        keep = [np.array(ptr, dtype=np.int64), np.array(idx, dtype=np.int32), np.array(vals, dtype=np.float64)]
        rs, cs = np.full((n, k), -7.0, order="F"), np.full((m, k), -7.0, order="F")
        job = _lib.Fp64BisilSparseJob()
        job.struct_size = C.sizeof(job)
        job.n, job.m, job.k, job.metric = over.get("n", n), m, over.get("k", k), metric
        if not no_x:
            job.x.col_ptr = keep[0].ctypes.data_as(C.POINTER(C.c_longlong))
            job.x.row_idx = keep[1].ctypes.data_as(C.POINTER(C.c_int))
            job.x.values = None if over.get("null_values") else dp(keep[2])
        if dev:
            job.x_dev.nnz = 1
        job.row_clusters, job.col_clusters = dp(over.get("rc", rc)), dp(cc)
        job.row_sil, job.col_sil = (None if over.get("null_out") else dp(rs)), dp(cs)
        code = lib.resnmtf_fp64_bisil_sparse(0, C.byref(job))
        assert np.all(rs == -7.0) and np.all(cs == -7.0)
        return code, (lib.resnmtf_last_error(None) or b"").decode()

    half = rc.copy(); half[1, 1] = 0.5
    cases = [(dict(k=0), "k must be in [1, 64]"), (dict(k=65), "k must be in [1, 64]"),
             (dict(n=0), "view dimensions must be positive"),
             (dict(metric=3), "metric must be 0 (euclidean), 1 (manhattan) or 2 (cosine)"),
             (dict(dev=True), "X is given in two places (job->x and job->x_dev)"),
             (dict(no_x=True), "X is given in no place (job->x or job->x_dev)"),
             (dict(null_out=True), "row_clusters / col_clusters / row_sil / col_sil are NULL"),
             (dict(null_values=True), "view 0: values is NULL"),
             (dict(ptr=(1, 2, 3, 5, 6)), "view 0: col_ptr[0] must be 0 (0-based CSC)"),
             (dict(ptr=(0, 3, 2, 5, 6)), "view 0: col_ptr is not monotone (column 1)"),
             (dict(idx=(0, 6, 1, 0, 5, 2)), "view 0: row index out of range in column 0"),
             (dict(idx=(3, 0, 1, 0, 5, 2)), "view 0: row indices must be strictly increasing within a column (column 0)"),
             (dict(vals=(1, 2, np.inf, 4, 5, 6)), "view 0: non-finite entry in column 1"),
             (dict(vals=(1, 2, 3, -4, 5, 6)), "view 0: negative entry in column 2"),
             (dict(rc=half), "row_clusters entries must be 0 or 1")]
    for over, text in cases:
        assert call(**over) == (1, text), over


def test_engine_function_refuses_before_the_library(monkeypatch):
    monkeypatch.setattr(_lib, "load", _never)
    x, rc, cc = sp.csc_matrix(np.eye(6, 4)), np.ones((6, 2)), np.ones((4, 2))
    with pytest.raises(ValueError, match="distance must be one of"):
        engine.fp64_bisil_sparse(x, rc, cc, "chebyshev")
    monkeypatch.undo()
    with pytest.raises(ValueError, match="fp64_bisil takes a dense one"):
        engine.fp64_bisil_sparse(np.eye(6, 4), rc, cc)
    with pytest.raises(ValueError, match="negative entry"):
        engine.fp64_bisil_sparse(sp.csc_matrix(-np.eye(6, 4)), rc, cc)
    with pytest.raises(ValueError, match="row clusters must be 6 x k"):
        engine.fp64_bisil_sparse(x, np.ones((5, 2)), cc)
    with pytest.raises(NotImplementedError, match="a sparse view is not supported"):     # the dense function, as before
        engine.fp64_bisil(x, rc, cc)


def test_job_of_a_host_view_holds_its_canonical_csc():
    x = sp.coo_matrix(([2.0, 0.0, 1.0, 3.0], ([4, 1, 0, 4], [2, 1, 2, 2])), shape=(6, 4))      # a duplicate and a zero
    c = engine._sparse.canonical_csc(x)
    keep = []
    job = engine._fp64_bisil_sparse_job(c, 6, 4, 0, keep)
    assert (job.n, job.m) == (6, 4) and job.x_dev.nnz == 0 and job.x_dev.layout == 0
    assert not job.x_dev.ptr_or_rows and not job.x_dev.values and not job.stream
    assert [job.x.col_ptr[i] for i in range(5)] == [0, 0, 0, 2, 2]
    assert [job.x.row_idx[i] for i in range(2)] == [0, 4] and [job.x.values[i] for i in range(2)] == [1.0, 5.0]
    empty = engine._fp64_bisil_sparse_job(sp.csc_matrix((3, 2)), 3, 2, 0, keep)            # never a NULL pointer
    assert bool(empty.x.row_idx) and bool(empty.x.values) and [empty.x.col_ptr[i] for i in range(3)] == [0, 0, 0]


def test_views_are_routed_by_their_kind(monkeypatch):
    monkeypatch.setattr(api, "Engine", _never)
    seen, dense_calls, sparse_calls = {}, [], []
    monkeypatch.setattr(engine, "fp64_run", _echo(seen))
    monkeypatch.setattr(engine, "fp64_bisil", _sil_log(dense_calls))
    monkeypatch.setattr(engine, "fp64_bisil_sparse", _sil_log(sparse_calls))
    args = _mixed(3, sparse_at=1)
    res = api.res_nmtf_inner(*args, distance="cosine", device_id=2, fp64_bisil_sparse=True, **FLAGS)
    assert len(dense_calls) == 2 and len(sparse_calls) == 1
    assert dense_calls[0][0] is seen["problem"]["data"][0] and dense_calls[1][0] is seen["problem"]["data"][2]
    x = sparse_calls[0][0]
    assert x is seen["problem"]["data"][1] and sp.issparse(x)            # the view the run received, still sparse
    np.testing.assert_array_equal(x.toarray(), args[0][1].toarray())
    for calls, views in ((dense_calls, (0, 2)), (sparse_calls, (1,))):
        for (_, rc, cc, distance, device_id), v in zip(calls, views):
            np.testing.assert_array_equal(rc, res["row_clusters"][v])
            np.testing.assert_array_equal(cc, res["col_clusters"][v])
            assert distance == "cosine" and device_id == 2
    # the stand-ins scale by their own call count: views 0 and 2 by 0.25 and 0.5, view 1 by 0.25
    scale = [0.25, 0.25, 0.5]
    want = bisil.overall([bisil.view_score(res["row_clusters"][v], res["col_clusters"][v], scale[v] * res["row_clusters"][v],
                                           2.0 * scale[v] * res["col_clusters"][v]) for v in range(3)])
    assert res["bisil"] == want and want != 0.0


def test_sil_hook_sees_every_view():
    seen, calls = {}, []
    a = _mixed(2, sparse_at=0)

    def sil(v, rc, cc, distance):
        calls.append((v, distance))
        return 0.5 * np.asarray(rc), 0.5 * np.asarray(cc)
    res = api._res_nmtf_inner_fp64(*a[:11], False, "manhattan", False, row_names=None, col_names=None, device_id=0, max_iters=10,
                                   seed=None, engine_opts=None, host_init=False, return_init=False, score_bisil=True,
                                   spurious_on_device=False, output="numpy", init_lm=None, return_state=False,
                                   post_on_device=False, fp64_sparse=True, fp64_bisil=True, fp64_bisil_sparse=True,
                                   runner=_echo(seen), sil=sil)
    assert calls == [(0, "manhattan"), (1, "manhattan")]
    assert res["bisil"] == bisil.score(res["row_clusters"], res["col_clusters"], "manhattan", sil=sil)


def test_flag_is_a_no_op_under_f32_and_without_fp64_bisil(monkeypatch):
    from test_fp64_host import _CallLog
    monkeypatch.setattr(api, "Engine", _CallLog)
    monkeypatch.setattr(engine, "fp64_run", _never)
    monkeypatch.setattr(engine, "fp64_bisil", _never)
    monkeypatch.setattr(engine, "fp64_bisil_sparse", _never)
    args = _inner_args(2)
    plain = api.res_nmtf_inner(*args, spurious=False)
    want = list(_CallLog.calls)
    flagged = api.res_nmtf_inner(*args, spurious=False, fp64_bisil_sparse=True)
    assert _CallLog.calls == want and list(plain) == list(flagged) and flagged["bisil"] is None
    with pytest.raises(NotImplementedError, match="the bisilhouette score of sparse views is not supported"):   # f32: its own opt-in
        api.res_nmtf_inner(*_mixed(), spurious=False, score_bisil=True, fp64_bisil_sparse=True)
    # fp64 without fp64_bisil: score_bisil is refused as before, with the flag or without it
    monkeypatch.setattr(api, "Engine", _never)
    texts = []
    for more in ({}, {"fp64_bisil_sparse": True}):
        with pytest.raises(NotImplementedError) as e:
            api.res_nmtf_inner(*_mixed(), spurious=False, precision="fp64", fp64_sparse=True, score_bisil=True, **more)
        texts.append(str(e.value))
    assert texts[0] == texts[1] == ('precision="fp64": score_bisil needs a live engine handle, which the fp64 path does not keep '
                                    '(it runs through resnmtf_fp64_run); use precision="f32" for it')
    # fp64 without score_bisil: nothing is scored, the flag changes nothing
    monkeypatch.setattr(engine, "fp64_run", _echo({}))
    res = api.res_nmtf_inner(*_mixed(), spurious=False, precision="fp64", fp64_sparse=True, fp64_bisil=True, fp64_bisil_sparse=True)
    assert res["bisil"] is None


def test_without_the_flag_every_refusal_keeps_its_text(monkeypatch):
    monkeypatch.setattr(api, "Engine", _never)
    monkeypatch.setattr(engine, "fp64_run", _never)
    monkeypatch.setattr(engine, "fp64_bisil", _never)
    monkeypatch.setattr(engine, "fp64_bisil_sparse", _never)
    with pytest.raises(NotImplementedError) as e:
        api.res_nmtf_inner(*_mixed(), **FLAGS)
    assert str(e.value) == ('precision="fp64": score_bisil with fp64_bisil=True scores dense views only; sparse views (view 1) '
                            'are not supported by resnmtf_fp64_bisil')
    with pytest.raises(NotImplementedError) as e:                        # without fp64_sparse the flag admits nothing
        api.res_nmtf_inner(*_mixed(), spurious=False, precision="fp64", score_bisil=True, fp64_bisil=True, fp64_bisil_sparse=True)
    assert str(e.value) == ('precision="fp64": sparse views (view 1) needs a live engine handle, which the fp64 path does not '
                            'keep (it runs through resnmtf_fp64_run); use precision="f32" for it')
    data = _raw_data()
    with pytest.raises(NotImplementedError) as e:
        api.apply_resnmtf([sp.csc_matrix(data[0]), data[1]], stability=False, spurious=False, precision="fp64", k_sweep=True,
                          fp64_sparse=True, sweep_runner=_never)
    assert str(e.value) == ('apply_resnmtf(precision="fp64"): a sparse view in the k sweep is not supported: resnmtf_fp64_bisil '
                            'scores dense views only; pass k_val (with fp64_sparse=True)')


def test_refusals_that_remain_with_the_flag(monkeypatch):
    monkeypatch.setattr(api, "Engine", _never)
    monkeypatch.setattr(engine, "fp64_run", _never)
    monkeypatch.setattr(engine, "fp64_bisil_sparse", _never)
    data = _raw_data()
    mixed = [sp.csc_matrix(data[0]), data[1]]
    on = dict(precision="fp64", fp64_sparse=True, fp64_bisil=True, fp64_bisil_sparse=True)
    with pytest.raises(NotImplementedError, match=r"a sparse view \(view 1\) is not supported: no fp64 sparse shuffle exists"):
        api.res_nmtf_inner(*_mixed(), spurious=True, spurious_on_device=True, fp64_spurious=True, score_bisil=True, **on)
    for sweep in (dict(k_val=3), dict(k_sweep=True, sweep_runner=_never)):
        with pytest.raises(NotImplementedError) as e:
            api.apply_resnmtf(mixed, stability=False, spurious_on_device=True, fp64_spurious=True, **sweep, **on)
        assert str(e.value) == ('apply_resnmtf(precision="fp64"): a sparse view with fp64_spurious is not supported: no fp64 sparse '
                                'shuffle exists; pass spurious=False')
        with pytest.raises(NotImplementedError) as e:
            api.apply_resnmtf(mixed, spurious=False, fp64_stability=True, **sweep, **on)
        assert str(e.value) == ('apply_resnmtf(precision="fp64"): a sparse view with fp64_stability is not supported: '
                                'resnmtf_fp64_subsample gathers dense views; pass stability=False')
    # a view in device memory (a stand-in: _views would ask a real tensor for its device)
    monkeypatch.setattr(api, "_views", lambda d, device_id=0: list(d))
    there = [device_views.RawDeviceView(data[0]), data[1]]
    for sweep in (dict(k_val=3), dict(k_sweep=True, sweep_runner=_never)):
        with pytest.raises(NotImplementedError, match=r'precision="fp64"\): a view in device memory is not supported'):
            api.apply_resnmtf(there, stability=False, spurious=False, fp64_device=True, **sweep, **on)


def test_apply_resnmtf_passes_the_flag_through_for_a_k_val(monkeypatch):
    seen = []

    def inner(*args, **kw):
        seen.append((args, kw))
        return {"bisil": 0.5}
    monkeypatch.setattr(api, "res_nmtf_inner", inner)
    data = _raw_data()
    mixed = [sp.csc_matrix(data[0]), data[1]]
    more = dict(k_val=3, stability=False, spurious=False, precision="fp64", score_bisil=True, fp64_bisil=True, fp64_sparse=True)
    assert api.apply_resnmtf(mixed, fp64_bisil_sparse=True, **more) == {"bisil": 0.5}
    assert api.apply_resnmtf(mixed, **more) == {"bisil": 0.5}
    assert seen[0][1]["fp64_bisil_sparse"] is True and seen[0][1]["fp64_bisil"] is True and seen[0][1]["fp64_sparse"] is True
    assert "fp64_bisil_sparse" not in seen[1][1]                          # without the flag: the call it was
    assert {k: v for k, v in seen[0][1].items() if k != "fp64_bisil_sparse"} == seen[1][1]
    assert sp.issparse(seen[0][0][0][0]) and seen[0][0][6] == [3, 3]      # the prepared view is still sparse


def test_apply_resnmtf_sweep_on_sparse_views_passes_the_flag_per_k(monkeypatch):
    calls = []
    scores = {3: 0.2, 4: 0.8, 5: 0.3}

    def inner(data, row_idx, col_idx, f, s, g, k_vec, phi, xi, psi, n_iters, num_repeats, spurious, distance, no_clusts, **kw):
        calls.append((list(k_vec), kw, data))
        return {"bisil": scores[k_vec[0]], "k": k_vec[0]}
    monkeypatch.setattr(api, "res_nmtf_inner", inner)
    data = _raw_data()
    mixed = [sp.csc_matrix(data[0]), data[1]]
    out = api.apply_resnmtf(mixed, stability=False, spurious=False, k_min=3, k_max=5, seed=40, precision="fp64", k_sweep=True,
                            fp64_sparse=True, fp64_bisil_sparse=True, return_sweep=True)
    assert [c[0] for c in calls] == [[3, 3], [4, 4], [5, 5]] and out["k"] == 4
    p = api.prepare(api._views(mixed), None, None, None, None, None, normalise=True, symmetrise=True)
    for k_vec, kw, seen in calls:
        assert kw["fp64_bisil_sparse"] is True and kw["fp64_sparse"] is True and kw["score_bisil"] is True and kw["fp64_bisil"] is True
        assert kw["precision"] == "fp64" and kw["seed"] == 40 + k_vec[0]
        assert sp.issparse(seen[0]) and not sp.issparse(seen[1])
        np.testing.assert_array_equal(seen[0].toarray(), p.data[0].toarray())
