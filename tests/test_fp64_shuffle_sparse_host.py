"""Host side of spurious-bicluster removal in double precision on sparse views (api.res_nmtf_inner / api.apply_resnmtf /
spurious.check_biclusters(fp64_shuffle_sparse=True), problem._draw_shuffle_fp64, engine.fp64_shuffle_sparse; DESIGN.md
section 30; no GPU): with the flag a sparse view is drawn through a stand-in for ``engine.fp64_shuffle_sparse`` and a dense
one through ``engine.fp64_shuffle``, with the driver's seeds, its redraw loop and its bound of 64; a view with fewer stored
entries than lines is refused before the first draw; the flag does nothing under f32 and without ``fp64_spurious``; without
it every earlier refusal keeps its text; with it the refusals that remain carry theirs; ``apply_resnmtf`` passes it through
for a ``k_val`` and for every k of the sweep; the library exports the symbol and agrees with the binding on the struct's
size."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import helpers
import shuffle_ref as S
from resnmtf_amd import _lib, api, build, device_views, engine, problem, spurious
from test_fp64_bisil_host import _echo, _inner_args, _never, _raw_data
from test_fp64_spurious_host import _Shuffle, _checker, _jsd

FLAGS = dict(spurious=True, spurious_on_device=True, fp64_spurious=True, precision="fp64", fp64_sparse=True)


def _mixed(n_views=2, sparse_at=1):
    """The arguments of res_nmtf_inner with view ``sparse_at`` given as a scipy.sparse matrix."""
    args = list(_inner_args(n_views))
    data = [sp.csc_matrix(x) if v == sparse_at else x for v, x in enumerate(args[0])]
    return [data] + args[1:]


class _SparseShuffle:
    """Stands in for engine.fp64_shuffle_sparse: logs every call and reports an empty column for the first ``empty`` draws
    of a view (three values back, where the dense entry gives four)."""

    def __init__(self, empty=0):
        self.calls, self.empty = [], empty

    def __call__(self, x, seed, normalise=True, device_id=0):
        self.calls.append((x, seed, normalise, device_id))
        n, m = x.shape
        ec = np.zeros(m, dtype=bool)
        ec[0] = len([c for c in self.calls if c[0] is x]) <= self.empty
        return ("sparse draw", seed), np.zeros(n, dtype=bool), ec


def test_symbol_struct_and_size():
    assert _lib.SIGNATURES["resnmtf_fp64_shuffle_sparse"] == (C.c_int, [C.c_int, C.POINTER(_lib.Fp64ShuffleSparseJob)])
    names = [f[0] for f in _lib.Fp64ShuffleSparseJob._fields_]
    assert names == ["struct_size", "n", "m", "normalise", "seed", "x", "x_dev", "stream", "out_col_ptr", "out_row_idx", "out_values",
                     "n_empty_rows", "n_empty_cols", "row_mask", "col_mask"]
    # four ints, the seed, the host CSC (three pointers), the device view (three ints padded to 16, three pointers, one
    # int64), the stream, three outputs, two counts, two masks
    assert C.sizeof(_lib.Fp64ShuffleSparseJob) == 16 + 8 + 24 + 48 + 8 + 24 + 16 + 16
    lib = C.CDLL(build.build(verbose=False))
    assert hasattr(lib, "resnmtf_fp64_shuffle_sparse")
    # the library's own sizeof: a job of the binding's size passes the size check and meets the next refusal (n = 0)
    lib.resnmtf_last_error.restype = C.c_char_p
    job = _lib.Fp64ShuffleSparseJob()
    job.struct_size = C.sizeof(job)
    assert lib.resnmtf_fp64_shuffle_sparse(0, C.byref(job)) == 1
    assert lib.resnmtf_last_error(None) == b"view dimensions must be positive"
    job.struct_size += 8
    assert lib.resnmtf_fp64_shuffle_sparse(0, C.byref(job)) == 1
    assert lib.resnmtf_last_error(None) == b"resnmtf_fp64_shuffle_sparse_job struct_size mismatch"
    assert lib.resnmtf_fp64_shuffle_sparse(0, None) == 1 and lib.resnmtf_last_error(None) == b"job is NULL"
    header = open(helpers.ROOT + "/include/resnmtf_hip.h").read()
    assert "int resnmtf_fp64_shuffle_sparse(int device_id, const resnmtf_fp64_shuffle_sparse_job* job);" in header
    assert "R/obtain_bicl.r:11-22" in header.split("typedef struct resnmtf_fp64_shuffle_sparse_job")[0][-5000:]
    assert "#define RESNMTF_ABI_VERSION 2 " in header                    # the ABI version does not move


def test_library_refusals_of_a_host_view_need_no_device():
    """What resnmtf_fp64_shuffle_sparse refuses of a host view comes before any device work, with the texts of
    resnmtf_fp64_shuffle and resnmtf_fp64_run_sparse; the counts keep their sentinel."""
    lib = _lib.load()
    n, m = 6, 4

    def call(ptr=(0, 2, 3, 5, 6), idx=(0, 3, 1, 0, 5, 2), vals=(1, 2, 3, 4, 5, 6), dev=False, no_x=False, **over):
        keep = [np.array(ptr, dtype=np.int64), np.array(idx, dtype=np.int32), np.array(vals, dtype=np.float64)]
        nr, nc = C.c_int(-7), C.c_int(-7)
        job = _lib.Fp64ShuffleSparseJob()
        job.struct_size = C.sizeof(job)
        job.n, job.m, job.seed = over.get("n", n), m, 3
        if not no_x:
            job.x.col_ptr = keep[0].ctypes.data_as(C.POINTER(C.c_longlong))
            job.x.row_idx = keep[1].ctypes.data_as(C.POINTER(C.c_int))
            job.x.values = None if over.get("null_values") else keep[2].ctypes.data_as(C.POINTER(C.c_double))
        if dev:
            job.x_dev.nnz = 1
        # (stand-in addresses: every case below is refused before an output is looked at)
        job.out_col_ptr, job.out_row_idx, job.out_values = (None if over.get("null_ptr") else 8), (None if over.get("null_idx") else 8), 8
        job.n_empty_rows, job.n_empty_cols = (None if over.get("null_count") else C.pointer(nr)), C.pointer(nc)
        code = lib.resnmtf_fp64_shuffle_sparse(0, C.byref(job))
        assert nr.value == -7 and nc.value == -7
        return code, (lib.resnmtf_last_error(None) or b"").decode()

    cases = [(dict(n=0), "view dimensions must be positive"),
             (dict(dev=True), "X is given in two places (job->x and job->x_dev)"),
             (dict(no_x=True), "X is given in no place (job->x or job->x_dev)"),
             (dict(null_ptr=True), "out_col_ptr is NULL"),
             (dict(null_count=True), "n_empty_rows / n_empty_cols are NULL"),
             (dict(null_values=True), "view 0: values is NULL"),
             (dict(ptr=(1, 2, 3, 5, 6)), "view 0: col_ptr[0] must be 0 (0-based CSC)"),
             (dict(ptr=(0, 3, 2, 5, 6)), "view 0: col_ptr is not monotone (column 1)"),
             (dict(idx=(0, 6, 1, 0, 5, 2)), "view 0: row index out of range in column 0"),
             (dict(idx=(3, 0, 1, 0, 5, 2)), "view 0: row indices must be strictly increasing within a column (column 0)"),
             (dict(vals=(1, 2, np.inf, 4, 5, 6)), "view 0: non-finite entry in column 1"),
             (dict(vals=(1, 2, 3, -4, 5, 6)), "view 0: negative entry in column 2"),
             (dict(null_idx=True), "out_row_idx / out_values are NULL")]
    for over, text in cases:
        assert call(**over) == (1, text), over


def test_engine_function_refuses_a_dense_view_and_the_dense_one_a_sparse_view(monkeypatch):
    monkeypatch.setattr(_lib, "load", lambda: None)
    with pytest.raises(ValueError, match="fp64_shuffle takes a dense one"):
        engine.fp64_shuffle_sparse(np.eye(6, 4), 1)
    with pytest.raises(NotImplementedError, match="fp64_shuffle draws dense views: a sparse view is not supported"):
        engine.fp64_shuffle(sp.csc_matrix(np.eye(3)), 1)                   # as before


def test_job_of_a_host_view_holds_its_canonical_csc():
    x = sp.coo_matrix(([2.0, 0.0, 1.0, 3.0], ([4, 1, 0, 4], [2, 1, 2, 2])), shape=(6, 4))      # a duplicate and a zero
    keep = []
    job = _lib.Fp64ShuffleSparseJob()
    engine._fill_fp64_sparse_source(job, engine._sparse.canonical_csc(x), 0, keep, "x")
    assert job.x_dev.nnz == 0 and job.x_dev.layout == 0 and not job.x_dev.ptr_or_rows and not job.stream
    assert [job.x.col_ptr[i] for i in range(5)] == [0, 0, 0, 2, 2]
    assert [job.x.row_idx[i] for i in range(2)] == [0, 4] and [job.x.values[i] for i in range(2)] == [1.0, 5.0]


# ---- the driver: routing, seeds, redraws, the bound, the early refusal ------------------------------------------------
def test_driver_routes_views_by_their_kind_with_the_seeds_of_the_f32_shuffles():
    rng = np.random.default_rng(0)
    data = [sp.csc_matrix(rng.random((6, 4)) + 0.1), rng.random((6, 5)), sp.csc_matrix(rng.random((6, 3)) + 0.1)]
    dense, sparse_, fits, kept = _Shuffle(), _SparseShuffle(), [], []

    def fit(tensors, k, seed, max_iters, device_id):
        fits.append((tensors, k, seed, max_iters, device_id))
        return [np.full((6, k), float(seed) + v) for v in range(3)]
    out = problem.shuffled_fits_fp64(data, 2, 3, seed=11, max_iters=77, device_id=2, shuffle=dense, shuffle_sparse=sparse_, fit=fit,
                                     keep=lambda r, tensors, attempts: kept.append((r, attempts)))
    assert len(out) == 3 and all(len(fs) == 3 for fs in out)
    assert len(dense.calls) == 3 and len(sparse_.calls) == 6
    for r in range(3):
        shuffle_seed = 11 * 7919 + r + 1
        for at, v in enumerate((0, 2)):
            x, seed, normalise, device_id = sparse_.calls[2 * r + at]
            assert x is data[v] and seed == S.draw_seed(shuffle_seed, 0, v) and normalise is True and device_id == 2
        x, seed, normalise, device_id = dense.calls[r]
        assert x is data[1] and seed == S.draw_seed(shuffle_seed, 0, 1) and normalise is True and device_id == 2
        tensors, k, seed, max_iters, device_id = fits[r]
        assert tensors == [("sparse draw", S.draw_seed(shuffle_seed, 0, 0)), ("draw", S.draw_seed(shuffle_seed, 0, 1)),
                           ("sparse draw", S.draw_seed(shuffle_seed, 0, 2))]
        assert (k, seed, max_iters, device_id) == (2, 11 + 1000 + r, 77, 2)
    assert kept == [(r, [1, 1, 1]) for r in range(3)]


def test_redraw_loop_of_a_sparse_view_counts_attempts_and_is_bounded_at_64():
    x = sp.csc_matrix(np.ones((5, 4)))
    sh = _SparseShuffle(3)
    t, attempts = problem._draw_shuffle_fp64(x, 1, 500, device_id=0, shuffle=_never, shuffle_sparse=sh)
    assert attempts == 4 and t == ("sparse draw", S.draw_seed(500, 3, 1))
    assert [c[1] for c in sh.calls] == [S.draw_seed(500, a, 1) for a in range(4)]
    sh = _SparseShuffle(64)
    with pytest.raises(RuntimeError, match="shuffle_view: every draw left an all-zero row or column"):
        problem._draw_shuffle_fp64(x, 0, 9, shuffle_sparse=sh)
    assert len(sh.calls) == 64
    assert problem._draw_shuffle_fp64(x, 0, 9, shuffle_sparse=_SparseShuffle(63))[1] == 64


def test_view_with_fewer_stored_entries_than_lines_is_refused_before_the_first_draw():
    x = sp.csc_matrix((np.ones(5), (np.arange(5), np.arange(5) % 4)), shape=(6, 4))
    with pytest.raises(ValueError) as e:
        problem._draw_shuffle_fp64(x, 2, 9, shuffle=_never, shuffle_sparse=_never)
    assert str(e.value) == ("shuffle_view: view 2 stores 5 entries, fewer than max(n, m) = 6: every shuffle of it has an all-zero "
                            "row or column, and the reference's shuffle_view (R/obtain_bicl.r:14-18) would not terminate on this view")
    full = sp.csc_matrix((np.ones(6), (np.arange(6), np.arange(6) % 4)), shape=(6, 4))          # max(n, m) entries: drawn
    assert problem._draw_shuffle_fp64(full, 2, 9, shuffle_sparse=_SparseShuffle())[1] == 1


def test_default_fit_takes_sparse_draws_as_sparse_device_views(monkeypatch):
    import torch
    seen = []

    def inner(data, row_idx, col_idx, f, s, g, k_vec, phi, xi, psi, n_iters, **kw):
        seen.append((data, kw))
        return {"output_f": [np.ones((6, 2)), np.ones((6, 2))]}
    monkeypatch.setattr(api, "res_nmtf_inner", inner)
    draw = torch.sparse_csc_tensor(torch.tensor([0, 1, 2]), torch.tensor([0, 1]), torch.tensor([1.0, 2.0], dtype=torch.float64), size=(6, 2))

    def sparse_shuffle(x, seed, normalise=True, device_id=0):
        return draw, np.zeros(6, dtype=bool), np.zeros(2, dtype=bool)
    data = [sp.csc_matrix(np.ones((6, 2))), np.ones((6, 5))]
    problem.shuffled_fits_fp64(data, 2, 2, seed=5, max_iters=40, device_id=1, shuffle=_Shuffle(), shuffle_sparse=sparse_shuffle)
    for r, (tensors, kw) in enumerate(seen):
        assert tensors[0] is draw and tensors[1][0] == "draw"
        assert kw == dict(spurious=False, seed=5 + 1000 + r, max_iters=40, device_id=1, precision="fp64", fp64_device=True,
                          output="torch", fp64_sparse_device=True)
    # without a sparse draw: the call it was
    seen.clear()
    problem.shuffled_fits_fp64([np.ones((6, 4)), np.ones((6, 5))], 2, 1, seed=5, max_iters=40, device_id=1, shuffle=_Shuffle())
    assert "fp64_sparse_device" not in seen[0][1]


# ---- check_biclusters / remove_spurious --------------------------------------------------------------------------------
def test_check_biclusters_hands_sparse_views_to_the_driver_as_canonical_csc(monkeypatch):
    rng = np.random.default_rng(0)
    dup = sp.coo_matrix((np.r_[rng.random(40) + 0.1, 0.5], (np.r_[np.arange(40) % 8, 0], np.r_[np.arange(40) // 8, 0])), shape=(8, 5))
    data = [dup, rng.random((8, 6))]
    F = [rng.random((8, 2)), rng.random((8, 2))]
    shuffled = [[rng.random((8, 2)), rng.random((8, 2))] for _ in range(3)]
    calls = []

    def fits(views, k, num_repeats, seed, max_iters, device_id):
        calls.append((views, k, num_repeats, seed, max_iters, device_id))
        return shuffled
    monkeypatch.setattr(spurious, "shuffled_fits_fp64", fits)
    monkeypatch.setattr(spurious, "shuffled_engines", _never)
    got = spurious.check_biclusters(data, F, 3, seed=9, device_id=1, max_iters=50, jsd=_jsd, precision="fp64", fp64_shuffle_sparse=True)
    views, k, num_repeats, seed, max_iters, device_id = calls[0]
    assert sp.issparse(views[0]) and views[0].format == "csc" and views[0].has_canonical_format and views[0].nnz == 40
    np.testing.assert_array_equal(views[0].toarray(), dup.toarray())
    assert np.array_equal(views[1], data[1]) and (k, num_repeats, seed, max_iters, device_id) == (2, 3, 9, 50, 1)
    want = spurious.check_biclusters([dup.toarray(), data[1]], F, 3, shuffled_f=shuffled, jsd=_jsd)
    for key in ("score", "avg_threshold", "max_threshold"):
        assert np.array_equal(got[key], want[key])
    # remove_spurious hands the keyword on
    res = {"output_f": F, "output_s": [np.eye(2), np.eye(2)], "row_clusters": [np.ones((8, 2)), np.ones((8, 2))],
           "col_clusters": [np.ones((5, 2)), np.ones((6, 2))]}
    out = spurious.remove_spurious(data, res, 3, seed=9, jsd=_jsd, precision="fp64", fp64_shuffle_sparse=True)
    assert len(calls) == 2 and np.array_equal(out["spurious"]["score"], got["score"])
    # without the flag, and with the f32 route's own flag instead: refused as before
    for more in ({}, {"shuffle_sparse": True}):
        with pytest.raises(NotImplementedError, match=r"a sparse view \(view 0\) is not supported: no fp64 sparse shuffle exists"):
            spurious.check_biclusters(data, F, 3, precision="fp64", **more)
    with pytest.raises(ValueError, match="grouped and group do not apply"):
        spurious.check_biclusters(data, F, 3, precision="fp64", grouped=True, fp64_shuffle_sparse=True)
    # under f32 the flag is not read
    with pytest.raises(NotImplementedError, match="device shuffles of sparse views are not supported"):
        spurious.check_biclusters(data, F, 3, fp64_shuffle_sparse=True)
    assert len(calls) == 2


# ---- res_nmtf_inner / apply_resnmtf ------------------------------------------------------------------------------------
def _inner_kw(seen, **more):
    return dict(row_names=None, col_names=None, device_id=1, max_iters=10, seed=4, engine_opts=None, host_init=False, return_init=False,
                score_bisil=False, spurious_on_device=True, output="numpy", init_lm=None, return_state=False, post_on_device=False,
                fp64_sparse=True, runner=_echo(seen), fp64_spurious=True, num_repeats=3, **more)


def test_inner_hands_the_flag_and_the_views_as_the_run_received_them_to_the_checker(monkeypatch):
    monkeypatch.setattr(api, "Engine", _never)
    seen, log = {}, []
    a = _mixed(2, sparse_at=0)
    res = api._res_nmtf_inner_fp64(*a[:11], True, "euclidean", False, checker=_checker(log, [[0.1, 0.9], [0.0, 0.9]]),
                                   **_inner_kw(seen, fp64_shuffle_sparse=True))
    data, output_f, num_repeats, ckw = log[0]
    assert len(log) == 1 and all(x is y for x, y in zip(data, seen["problem"]["data"])) and sp.issparse(data[0])
    assert ckw == dict(seed=4, device_id=1, max_iters=10, precision="fp64", fp64_shuffle_sparse=True) and num_repeats == 3
    assert res["spurious"]["removed"].any()
    # dense views with the flag: the checker still gets it (it is a no-op there), and without it the call it was
    log.clear()
    d = _inner_args(2)
    api._res_nmtf_inner_fp64(*d[:11], True, "euclidean", False, checker=_checker(log, [[0.1, 0.9], [0.0, 0.9]]), **_inner_kw({}))
    assert log[0][3] == dict(seed=4, device_id=1, max_iters=10, precision="fp64")


def test_flag_is_a_no_op_under_f32_and_without_fp64_spurious(monkeypatch):
    from test_fp64_host import _CallLog
    monkeypatch.setattr(api, "Engine", _CallLog)
    monkeypatch.setattr(engine, "fp64_run", _never)
    monkeypatch.setattr(engine, "fp64_shuffle", _never)
    monkeypatch.setattr(engine, "fp64_shuffle_sparse", _never)
    args = _inner_args(2)
    plain = api.res_nmtf_inner(*args, spurious=False)
    want = list(_CallLog.calls)
    flagged = api.res_nmtf_inner(*args, spurious=False, fp64_shuffle_sparse=True)
    assert _CallLog.calls == want and list(plain) == list(flagged)
    # fp64 without fp64_spurious: spurious=True is refused as before, with the flag or without it
    monkeypatch.setattr(api, "Engine", _never)
    texts = []
    for more in ({}, {"fp64_shuffle_sparse": True}):
        with pytest.raises(NotImplementedError) as e:
            api.res_nmtf_inner(*_mixed(), spurious=True, spurious_on_device=True, precision="fp64", fp64_sparse=True, **more)
        texts.append(str(e.value))
    assert texts[0] == texts[1] == ('precision="fp64": spurious_on_device needs a live engine handle, which the fp64 path does not '
                                    'keep (it runs through resnmtf_fp64_run); use precision="f32" for it')
    texts = []
    for more in ({}, {"fp64_shuffle_sparse": True}):
        with pytest.raises(NotImplementedError) as e:
            api.apply_resnmtf([sp.csc_matrix(_raw_data()[0])], k_val=3, stability=False, precision="fp64", fp64_sparse=True, **more)
        texts.append(str(e.value))
    assert texts[0] == texts[1] == ('apply_resnmtf(precision="fp64"): spurious=True is not supported: spurious-bicluster removal '
                                    'runs on the f32 engine; pass spurious=False')
    # fp64 without spurious: nothing is checked, the flag changes nothing
    monkeypatch.setattr(engine, "fp64_run", _echo({}))
    res = api.res_nmtf_inner(*_mixed(), spurious=False, precision="fp64", fp64_sparse=True, fp64_spurious=True, fp64_shuffle_sparse=True)
    assert "spurious" not in res


def test_without_the_flag_every_refusal_keeps_its_text(monkeypatch):
    monkeypatch.setattr(api, "Engine", _never)
    monkeypatch.setattr(engine, "fp64_run", _never)
    monkeypatch.setattr(engine, "fp64_shuffle_sparse", _never)
    with pytest.raises(NotImplementedError) as e:
        api.res_nmtf_inner(*_mixed(), **FLAGS)
    assert str(e.value) == ('precision="fp64": spurious-bicluster removal in double precision (fp64_spurious) shuffles dense views '
                            'only; a sparse view (view 1) is not supported: no fp64 sparse shuffle exists')
    with pytest.raises(NotImplementedError) as e:                        # without fp64_sparse the flag admits nothing
        api.res_nmtf_inner(*_mixed(), **{**FLAGS, "fp64_sparse": False}, fp64_shuffle_sparse=True)
    assert str(e.value) == ('precision="fp64": sparse views (view 1) needs a live engine handle, which the fp64 path does not '
                            'keep (it runs through resnmtf_fp64_run); use precision="f32" for it')
    data = _raw_data()
    mixed = [sp.csc_matrix(data[0]), data[1]]
    for sweep in (dict(k_val=3), dict(k_sweep=True, sweep_runner=_never, fp64_bisil_sparse=True)):
        with pytest.raises(NotImplementedError) as e:
            api.apply_resnmtf(mixed, stability=False, **sweep, **FLAGS)
        assert str(e.value) == ('apply_resnmtf(precision="fp64"): a sparse view with fp64_spurious is not supported: no fp64 sparse '
                                'shuffle exists; pass spurious=False')


def test_refusals_that_remain_with_the_flag(monkeypatch):
    monkeypatch.setattr(api, "Engine", _never)
    monkeypatch.setattr(engine, "fp64_run", _never)
    monkeypatch.setattr(engine, "fp64_shuffle_sparse", _never)
    data = _raw_data()
    mixed = [sp.csc_matrix(data[0]), data[1]]
    on = dict(FLAGS, fp64_shuffle_sparse=True, fp64_bisil_sparse=True)
    for sweep in (dict(k_val=3), dict(k_sweep=True, sweep_runner=_never)):
        with pytest.raises(NotImplementedError) as e:
            api.apply_resnmtf(mixed, fp64_stability=True, **sweep, **on)
        assert str(e.value) == ('apply_resnmtf(precision="fp64"): a sparse view with fp64_stability is not supported: '
                                'resnmtf_fp64_subsample gathers dense views; pass stability=False')
        with pytest.raises(NotImplementedError, match=r'precision="fp64"\): stability=True is not supported'):
            api.apply_resnmtf(mixed, **sweep, **on)
    with pytest.raises(NotImplementedError, match="score_bisil with fp64_bisil=True scores dense views only"):   # its own opt-in
        api.res_nmtf_inner(*_mixed(), score_bisil=True, fp64_bisil=True, fp64_shuffle_sparse=True, **FLAGS)
    with pytest.raises(ValueError, match="num_repeats must be an integer >= 2"):
        api.res_nmtf_inner(*_mixed(), num_repeats=1, fp64_shuffle_sparse=True, **FLAGS)
    # a view in device memory (a stand-in: _views would ask a real tensor for its device)
    monkeypatch.setattr(api, "_views", lambda d, device_id=0: list(d))
    there = [device_views.RawDeviceView(data[0]), data[1]]
    for sweep in (dict(k_val=3), dict(k_sweep=True, sweep_runner=_never)):
        with pytest.raises(NotImplementedError, match=r'precision="fp64"\): a view in device memory is not supported'):
            api.apply_resnmtf(there, stability=False, fp64_device=True, **sweep, **on)


def test_apply_resnmtf_passes_the_flag_through_for_a_k_val_and_per_k(monkeypatch):
    calls = []
    scores = {3: 0.2, 4: 0.8, 5: 0.3}

    def inner(data, row_idx, col_idx, f, s, g, k_vec, phi, xi, psi, n_iters, num_repeats, spurious, distance, no_clusts, **kw):
        calls.append((list(k_vec), kw, data, spurious, num_repeats))
        return {"bisil": scores[k_vec[0]], "k": k_vec[0]}
    monkeypatch.setattr(api, "res_nmtf_inner", inner)
    data = _raw_data()
    mixed = [sp.csc_matrix(data[0]), data[1]]
    on = dict(stability=False, spurious_on_device=True, fp64_spurious=True, precision="fp64", fp64_sparse=True, num_repeats=3)
    assert api.apply_resnmtf(mixed, k_val=3, fp64_shuffle_sparse=True, **on)["k"] == 3
    assert api.apply_resnmtf([data[0], data[1]], k_val=3, **on)["k"] == 3
    assert calls[0][1]["fp64_shuffle_sparse"] is True and calls[0][1]["fp64_spurious"] is True and calls[0][3] is True
    assert "fp64_shuffle_sparse" not in calls[1][1]                       # without the flag: the call it was
    assert {k: v for k, v in calls[0][1].items() if k != "fp64_shuffle_sparse"} == calls[1][1]
    assert sp.issparse(calls[0][2][0]) and calls[0][4] == 3
    # spurious=False: the flag is not passed on (it is read only where the removal runs)
    calls.clear()
    api.apply_resnmtf(mixed, k_val=3, spurious=False, fp64_shuffle_sparse=True, **on)
    assert "fp64_shuffle_sparse" not in calls[0][1] and "fp64_spurious" not in calls[0][1]
    # the sweep: every k with its own check at seed + k
    calls.clear()
    out = api.apply_resnmtf(mixed, k_min=3, k_max=5, seed=40, k_sweep=True, fp64_bisil_sparse=True, fp64_shuffle_sparse=True,
                            return_sweep=True, **on)
    assert [c[0] for c in calls] == [[3, 3], [4, 4], [5, 5]] and out["k"] == 4
    for k_vec, kw, seen, remove, _ in calls:
        assert kw["fp64_shuffle_sparse"] is True and kw["fp64_bisil_sparse"] is True and kw["fp64_spurious"] is True and remove is True
        assert kw["spurious_on_device"] is True and kw["precision"] == "fp64" and kw["seed"] == 40 + k_vec[0]
        assert sp.issparse(seen[0]) and not sp.issparse(seen[1])
