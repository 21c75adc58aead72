"""Device copies and sub-samples of sparse views (resnmtf_subsample_count_sparse, resnmtf_subsample_view_sparse,
resnmtf_copy_view_sparse; DESIGN.md section 10 "Device copies and sub-samples"): the view after a device sub-sample is
bit for bit the view resnmtf_set_view_csc(pre_processed = 1) makes of the same sub-sample built on the host
(subsample_ref.subsample_csc) from the source's stored fp32 values; it is the dense path's sub-sample of the densified
view; a copy is bit for bit the upload of the source's read-back at the destination's k; refusals; and the opt-in
``sparse_on_device`` through the stability repeats, the k sweep and apply_resnmtf."""
import numpy as np
import pytest
import scipy.sparse as sp

import resnmtf_amd
from resnmtf_amd import api, batched, naming, synth
from resnmtf_amd._lib import ResnmtfError
from resnmtf_amd.engine import Engine

from subsample_ref import case, f32, host_masks, planted_sparse, random_csc, same_csc, subsample_csc, upload_csc

pytestmark = pytest.mark.gpu


def _draw(n, count, seed, keep=None, leave=None):
    """An unsorted index list without repeats, as R's sample gives it; ``keep`` / ``leave``: an index forced in / out."""
    p = np.random.default_rng(seed).permutation(n)
    if leave is not None:
        p = p[p != leave]
    p = p[:count]
    if keep is not None and keep not in p:
        p[0] = keep
    return p.astype(np.int32)


def _lists(name):
    """(source, k, sweeps, rows, cols) of every case of the bitwise test."""
    if name.startswith("300x200_dense_lines"):
        x, k, sweeps = case("300x200")
        kept = name.endswith("kept")                   # the dense row 17 and the dense column 31: both in or both out
        return (x, k, sweeps, _draw(300, 270, 21, keep=17 if kept else None, leave=None if kept else 17),
                _draw(200, 180, 22, keep=31 if kept else None, leave=None if kept else 31))
    if name == "rows_that_hold_nothing":               # nnz' = 0 from nnz > 0
        x = sp.lil_matrix((40, 30))
        x[:10, :] = f32(np.random.default_rng(8).random((10, 30)) + 0.1)
        return sp.csc_matrix(x), 2, False, (10 + _draw(30, 25, 23)).astype(np.int32), _draw(30, 27, 24)
    x, k, sweeps = case(name)
    n, m = x.shape
    if name == "300x200_1pct":
        rng = np.random.default_rng(11)
        return x, k, sweeps, rng.permutation(300)[:270].astype(np.int32), rng.permutation(200)[:180].astype(np.int32)
    if name == "70000x70000":
        return (x, k, sweeps, np.random.default_rng(12).permutation(70000)[:66500].astype(np.int32),
                np.random.default_rng(13).permutation(70000)[:66500].astype(np.int32))
    counts = {"37x23": (33, 20), "64x64": (64, 64), "130x5": (117, 5), "50x30_empty": (45, 27)}[name]
    return x, k, sweeps, _draw(n, counts[0], 31), _draw(m, counts[1], 32)


def _sparse_engine(shape, k, nnz):
    return Engine([shape[0]], [shape[1]], [k], nnz=[nnz])


def _three_sweeps(engines, n, m, k):
    f, s, g = synth.random_init(n, m, k, 9)
    out = []
    for eng in engines:
        eng.set_factors(0, f, s, g)
        errs = eng.run(3)
        out.append((errs, *eng.get_factors(0)[:3]))
    assert np.isfinite(out[0][0]).all()
    for a, b in zip(*out):
        assert a.tobytes() == b.tobytes()


def _same_plan(a, b):
    pa, pb = a.view_plan(0), b.view_plan(0)
    assert pa["sparse_blocks"] == pb["sparse_blocks"] and pa["nsplit"] == pb["nsplit"] and pa["image"] == "sparse"


CASES = ["37x23", "64x64", "130x5", "300x200_dense_lines_kept", "300x200_dense_lines_left_out", "300x200_1pct",
         "70000x70000", "50x30_empty", "rows_that_hold_nothing"]


@pytest.mark.parametrize("name", CASES)
def test_device_subsample_is_bitwise_the_host_built_subsample(name):
    x, k, sweeps, rows, cols = _lists(name)
    shape = (len(rows), len(cols))
    with _sparse_engine(x.shape, k, x.nnz) as src:
        upload_csc(src, 0, x, True)
        held = src.get_view_sparse(0)
        if name == "37x23":
            assert (held.data == 0).sum() == 1              # the explicit zero is stored on the device
        want = subsample_csc(held, rows, cols)
        if x.shape[0] <= 300:                               # the restatement against SciPy's own indexing
            assert np.array_equal(want.toarray(), held.toarray()[np.ix_(rows, cols)])
        count = src.subsample_count_sparse(0, rows, cols)
        assert count == want.nnz
        if name == "300x200_1pct":
            assert (x.nnz, count) == (600, 488)
        if name == "70000x70000":
            assert count == 1801 and shape[0] * shape[1] > 2 ** 32
        if name == "rows_that_hold_nothing":
            assert x.nnz > 0 and count == 0
        with _sparse_engine(shape, k, count) as dst, _sparse_engine(shape, k, count) as ref:
            dst.subsample_view_sparse_from(0, src, 0, rows, cols)
            got = dst.get_view_sparse(0)
            assert dst.view_storage(0) == (True, count, count)
            upload_csc(ref, 0, want, True)
            assert same_csc(got, ref.get_view_sparse(0)) and same_csc(got, want)
            er, ec = host_masks(want)
            gr, gc, nr, nc = dst.empty_lines(0, counts=True)
            assert np.array_equal(gr, er) and np.array_equal(gc, ec) and (nr, nc) == (er.sum(), ec.sum())
            if name == "300x200_1pct":
                assert (er.sum(), ec.sum()) == (44, 13)      # both masks have members
            if name in ("50x30_empty", "rows_that_hold_nothing"):
                assert er.all() and ec.all() and got.nnz == 0
            _same_plan(dst, ref)
            if sweeps:
                _three_sweeps((dst, ref), shape[0], shape[1], k)
        assert same_csc(src.get_view_sparse(0), held)       # the source is what it was


@pytest.mark.parametrize("name", ["37x23", "64x64", "300x200_dense_lines_kept", "300x200_dense_lines_left_out"])
def test_same_subsample_as_the_dense_path(name):
    x, k, _, rows, cols = _lists(name)
    n, m = x.shape
    shape = (len(rows), len(cols))
    with _sparse_engine(x.shape, k, x.nnz) as src, Engine([n], [m], [k]) as dsrc, Engine([shape[0]], [shape[1]], [k]) as ddst:
        upload_csc(src, 0, x, True)
        dsrc.set_view(0, f32(x.toarray()))
        with _sparse_engine(shape, k, src.subsample_count_sparse(0, rows, cols)) as dst:
            dst.subsample_view_sparse_from(0, src, 0, rows, cols)
            ddst.subsample_view_from(0, dsrc, 0, rows, cols)
            assert np.array_equal(dst.get_view_sparse(0).toarray(), ddst.get_view(0))
            a, b = dst.empty_lines(0, counts=True), ddst.empty_lines(0, counts=True)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


# KP groups 16 / 16 / 8 / 4.  The empty view is 50 x 30 at every k a 50 x 30 handle can have (k <= 30) and 50 x 40 at k = 33.
@pytest.mark.parametrize("name,k", [(name, k) for name in ("300x200", "50x30_empty", "50x40_empty") for k in (2, 16, 17, 33)
                                    if (name, k) != ("50x30_empty", 33) and (name != "50x40_empty" or k == 33)])
def test_copy_is_bitwise_the_upload_of_the_read_back(name, k):
    x, _, sweeps = (sp.csc_matrix((50, 40)), 2, False) if name == "50x40_empty" else case(name)
    n, m = x.shape
    with _sparse_engine(x.shape, 2, x.nnz) as src, _sparse_engine(x.shape, k, x.nnz) as dst, _sparse_engine(x.shape, k, x.nnz) as ref:
        upload_csc(src, 0, x, True)
        held = src.get_view_sparse(0)
        dst.copy_view_sparse_from(0, src, 0)
        upload_csc(ref, 0, held, True)
        assert dst.view_storage(0) == ref.view_storage(0) == (True, x.nnz, x.nnz)
        assert same_csc(dst.get_view_sparse(0), held) and same_csc(ref.get_view_sparse(0), held)
        _same_plan(dst, ref)
        if sweeps:
            _three_sweeps((dst, ref), n, m, k)


def test_determinism_and_reuse_of_a_handle():
    x, k, _, rows, cols = _lists("300x200_dense_lines_kept")
    rows2, cols2 = _draw(300, 270, 41), _draw(200, 180, 42)
    shape = (270, 180)
    with _sparse_engine(x.shape, k, x.nnz) as src:
        upload_csc(src, 0, x, True)
        cap = max(src.subsample_count_sparse(0, rows, cols), src.subsample_count_sparse(0, rows2, cols2))
        with _sparse_engine(shape, k, cap) as a, _sparse_engine(shape, k, cap) as b, _sparse_engine(shape, k, cap) as twin:
            a.subsample_view_sparse_from(0, src, 0, rows, cols)
            first = a.get_view_sparse(0)
            a.subsample_view_sparse_from(0, src, 0, rows, cols)
            assert same_csc(first, a.get_view_sparse(0))
            a.subsample_view_sparse_from(0, src, 0, rows2, cols2)            # the handle used again, other lists
            b.subsample_view_sparse_from(0, src, 0, rows2, cols2)            # a fresh one
            second = b.get_view_sparse(0)
            assert same_csc(a.get_view_sparse(0), second) and not same_csc(first, second)
            assert a.view_storage(0) == b.view_storage(0)
            _same_plan(a, b)
            _three_sweeps((a, b), shape[0], shape[1], k)
            # a shuffle drawn from a sub-sampled handle equals the shuffle of its host-built twin
            upload_csc(twin, 0, second, True)
            with _sparse_engine(shape, k, cap) as sa, _sparse_engine(shape, k, cap) as sb:
                sa.shuffle_view_sparse_from(0, b, 0, seed=77)
                sb.shuffle_view_sparse_from(0, twin, 0, seed=77)
                assert same_csc(sa.get_view_sparse(0), sb.get_view_sparse(0))
                assert sa.empty_lines(0, counts=True)[2:] == sb.empty_lines(0, counts=True)[2:]


REFUSALS = ["null_rows", "dense_dst", "dense_src", "not_owned", "dst_not_owned", "bad_source_view", "not_uploaded", "row_out_of_range", "col_out_of_range",
            "row_twice", "col_twice", "capacity", "count_dense", "count_twice", "copy_dense_dst", "copy_dense_src",
            "copy_shape", "copy_capacity", "copy_not_uploaded"]


@pytest.mark.parametrize("what", REFUSALS)
def test_refusals_leave_the_destination_as_it_was(what):
    """Host-side checks of the library (the capacity of a sub-sample after the counting pass, which writes nothing of
    the destination): the error code, a fragment of the text, and the destination still reads back what it held."""
    x = random_csc(60, 40, 0.5, 8)
    k = 3
    rows, cols = _draw(60, 50, 51), _draw(40, 30, 52)
    with _sparse_engine(x.shape, k, x.nnz) as src, Engine([60], [40], [k]) as dense, Engine([50], [30], [k]) as dense_small:
        src.set_view_sparse(0, x)
        d = x.toarray() + 1e-3
        dense.set_view(0, d / d.sum(axis=0))
        count = src.subsample_count_sparse(0, rows, cols)
        before = random_csc(50, 30, 0.2, 9)
        with _sparse_engine((50, 30), k, count) as dst, _sparse_engine(x.shape, k, x.nnz) as full, \
                _sparse_engine(x.shape, k, x.nnz) as bare:
            dst.set_view_sparse(0, before, pre_processed=True)
            full.set_view_sparse(0, random_csc(60, 40, 0.3, 10), pre_processed=True)
            held = {id(dst): dst.get_view_sparse(0), id(full): full.get_view_sparse(0)}
            check = dst
            twice_r = rows.copy(); twice_r[7] = twice_r[3]
            twice_c = cols.copy(); twice_c[5] = twice_c[0]
            far_r = rows.copy(); far_r[2] = 60
            far_c = cols.copy(); far_c[2] = -1
            if what == "null_rows":
                rc = dst._lib.resnmtf_subsample_view_sparse(dst._h, 0, src._h, 0, None, None)
                assert rc == 1 and dst._lib.resnmtf_copy_view_sparse(dst._h, 0, None, 0) == 1
                assert src._lib.resnmtf_subsample_count_sparse(src._h, 0, 50, None, 30, None, None) == 1
                call = None
            elif what == "dense_dst":
                call, code, text = (lambda: dense_small.subsample_view_sparse_from(0, src, 0, rows, cols)), 1, "destination view is dense \\(resnmtf_subsample_view"
                check = None
            elif what == "dense_src":
                call, code, text = (lambda: dst.subsample_view_sparse_from(0, dense, 0, rows, cols)), 1, "source view is dense \\(resnmtf_subsample_view"
            elif what == "not_owned":
                with Engine([60, 60], [40, 40], [k, k], owned=[True, False], nnz=[x.nnz, x.nnz]) as part:
                    part.set_view_sparse(0, x)
                    with pytest.raises(ResnmtfError, match="not owned") as info:
                        dst.subsample_view_sparse_from(0, part, 1, rows, cols)
                    assert info.value.code == 5
                    with pytest.raises(ResnmtfError, match="not owned") as info:
                        full.copy_view_sparse_from(0, part, 1)
                    assert info.value.code == 5
                call = None
            elif what == "dst_not_owned":
                with Engine([50, 50], [30, 30], [k, k], owned=[True, False], nnz=[count, count]) as part, \
                        Engine([60, 60], [40, 40], [k, k], owned=[True, False], nnz=[x.nnz, x.nnz]) as whole:
                    with pytest.raises(ResnmtfError, match="destination view is not owned") as info:
                        part.subsample_view_sparse_from(1, src, 0, rows, cols)
                    assert info.value.code == 5
                    with pytest.raises(ResnmtfError, match="destination view is not owned") as info:
                        whole.copy_view_sparse_from(1, src, 0)
                    assert info.value.code == 5
                call = None
            elif what == "bad_source_view":
                for v_src in (-1, 1):
                    with pytest.raises(ResnmtfError, match="bad source view") as info:
                        dst.subsample_view_sparse_from(0, src, v_src, rows, cols)
                    assert info.value.code == 1
                    with pytest.raises(ResnmtfError, match="bad source view") as info:
                        full.copy_view_sparse_from(0, src, v_src)
                    assert info.value.code == 1
                with pytest.raises(ResnmtfError, match="bad source view") as info:
                    src.subsample_count_sparse(1, rows, cols)
                assert info.value.code == 1
                call = None
            elif what == "not_uploaded":
                call, code, text = (lambda: dst.subsample_view_sparse_from(0, bare, 0, rows, cols)), 5, "not been uploaded"
            elif what == "row_out_of_range":
                call, code, text = (lambda: dst.subsample_view_sparse_from(0, src, 0, far_r, cols)), 1, "row index out of range"
            elif what == "col_out_of_range":
                call, code, text = (lambda: dst.subsample_view_sparse_from(0, src, 0, rows, far_c)), 1, "column index out of range"
            elif what == "row_twice":
                call, code, text = (lambda: dst.subsample_view_sparse_from(0, src, 0, twice_r, cols)), 1, f"row index {twice_r[3]} occurs twice"
            elif what == "col_twice":
                call, code, text = (lambda: dst.subsample_view_sparse_from(0, src, 0, rows, twice_c)), 1, f"column index {twice_c[0]} occurs twice"
            elif what == "capacity":                         # one entry short: the text names the needed count
                with _sparse_engine((50, 30), k, count - 1) as short:
                    short.set_view_sparse(0, before, pre_processed=True)
                    with pytest.raises(ResnmtfError, match=f"holds {count} stored entries, above the destination's nnz capacity {count - 1}") as info:
                        short.subsample_view_sparse_from(0, src, 0, rows, cols)
                    assert info.value.code == 1 and same_csc(short.get_view_sparse(0), held[id(dst)])
                call = None
            elif what == "count_dense":
                call, code, text = (lambda: dense.subsample_count_sparse(0, rows, cols)), 1, "source view is dense"
                check = None
            elif what == "count_twice":
                call, code, text = (lambda: src.subsample_count_sparse(0, twice_r, cols)), 1, "occurs twice"
                check = None
            elif what == "copy_dense_dst":
                call, code, text = (lambda: dense.copy_view_sparse_from(0, src, 0)), 1, "destination view is dense \\(resnmtf_copy_view"
                check = None
            elif what == "copy_dense_src":
                call, code, text, check = (lambda: full.copy_view_sparse_from(0, dense, 0)), 1, "source view is dense \\(resnmtf_copy_view", full
            elif what == "copy_shape":
                call, code, text = (lambda: dst.copy_view_sparse_from(0, src, 0)), 1, "differ in shape"
            elif what == "copy_capacity":
                with _sparse_engine(x.shape, k, x.nnz - 1) as short:
                    with pytest.raises(ResnmtfError, match=f"holds {x.nnz} stored entries, above the destination's nnz capacity {x.nnz - 1}") as info:
                        short.copy_view_sparse_from(0, src, 0)
                    assert info.value.code == 1 and short.view_storage(0) == (True, 0, x.nnz - 1)
                call = None
            else:
                call, code, text, check = (lambda: full.copy_view_sparse_from(0, bare, 0)), 5, "not been uploaded", full
            if call is not None:
                with pytest.raises(ResnmtfError, match=text) as info:
                    call()
                assert info.value.code == code
            for eng in (dst, full):
                assert same_csc(eng.get_view_sparse(0), held[id(eng)])
            if check is not None:                            # and it still runs
                n, m = check.n_rows[0], check.n_cols[0]
                check.set_factors(0, *synth.random_init(n, m, k, 3))
                assert np.isfinite(check.run(1)).all()


# ------------------------------------------------------------------------------------------------------ the pipeline
def _planted_pair(round_to_f32):
    data = [planted_sparse(1)[0], planted_sparse(2)[0]]
    rn, cn = naming.give_names(data, None, None, None, None)
    pre = naming.check_data(data)
    if round_to_f32:
        for d in pre:
            d.data = f32(d.data)
    return pre, rn, cn


def _same_arrays(a, b, keys):
    for key in keys:
        for u, w in zip(a[key], b[key]):
            assert np.asarray(u).tobytes() == np.asarray(w).tobytes(), key


def test_repeats_and_sweep_are_equal_on_f32_representable_data():
    pre, rn, cn = _planted_pair(True)
    zero = np.zeros((2, 2))
    dev = batched.DeviceData(pre, zero, zero, zero, rn, cn, pre_processed=True)
    try:
        res = dev.factorise(3, 50, 4)
        for v in range(2):
            dev.base.set_reference_clusters(v, res["row_clusters"][v], res["col_clusters"][v])
        draw = batched.stability_draws(dev.data_shapes, 1, 0.9, 9)[0]
        for more in ({}, {"spurious_repeats": 3, "shuffle_sparse": True}):
            off, on = (dev.stability_repeat(3, None, 2009, draw, max_iters=3000, keep_clusters=True, **more, **opt)
                       for opt in ({}, {"sparse_on_device": True}))
            assert off["stability_performed"] and on["stability_performed"]
            assert on["relevance"].tobytes() == off["relevance"].tobytes()
            assert on["All_Error"].tobytes() == off["All_Error"].tobytes() and on["Error"] == off["Error"]
            _same_arrays(on, off, ("row_clusters", "col_clusters"))
            _same_arrays(on["extras"], off["extras"], ("row_samples", "col_samples"))
        off, on = (batched.k_sweep_on_device(dev, 3, 5, 50, 7, return_lm=True, **opt) for opt in ({}, {"sparse_on_device": True}))
        assert len(on) == len(off) == 3
        for a, b in zip(on, off):
            assert list(a) == list(b) and a["All_Error"].tobytes() == b["All_Error"].tobytes()
            _same_arrays(a, b, ("output_f", "output_s", "output_g", "row_clusters", "col_clusters", "lambda", "mu"))
        # return_data reads the device copy back: the f32-rounded matrix the host route reports
        off, on = (dev.factorise(3, 5, 4, samples=draw, return_data=True, **opt) for opt in ({}, {"sparse_on_device": True}))
        _same_arrays(on, off, ("data", "output_f"))
    finally:
        dev.close()


def test_api_on_normalised_fp64_data():
    """fp64 data that are not f32-representable: a sub-sample's data_norms is summed from the f32 values the device
    holds instead of the host's fp64 ones (2^-23 relative at most); everything else is bit for bit the host route's, so
    the factors are equal and All_Error -- a ratio of order one -- stays within 1e-6 absolute."""
    x1, x2 = planted_sparse(1)[0], planted_sparse(2)[0]
    kw = dict(k_val=3, spurious=False, n_iters=200, seed=7)
    off = resnmtf_amd.apply_resnmtf([x1, x2], **kw)
    on = resnmtf_amd.apply_resnmtf([x1, x2], sparse_on_device=True, **kw)
    assert list(on) == list(off)
    _same_arrays(on, off, ("row_clusters", "col_clusters", "output_f", "output_s", "output_g"))   # the stability outcome too
    assert np.abs(on["All_Error"] - off["All_Error"]).max() <= 1e-6
    # the repeats themselves: relevance and clusters identical, All_Error within the bar
    pre, rn, cn = _planted_pair(False)
    zero = np.zeros((2, 2))
    reps = [api.stability_check(pre, off, 3, zero, zero, zero, 200, False, 5, False, "euclidean", 0.9, 5,
                                remove_unstable=False, row_names=rn, col_names=cn, seed=7, return_repeats=True, **opt)["stability"]
            for opt in ({}, {"sparse_on_device": True})]
    assert reps[1]["relevance"].tobytes() == reps[0]["relevance"].tobytes()
    worst = 0.0
    for a, b in zip(reps[1]["repeats"], reps[0]["repeats"]):
        _same_arrays(a, b, ("row_clusters", "col_clusters"))
        assert len(a["All_Error"]) == len(b["All_Error"]) == 200
        worst = max(worst, np.abs(a["All_Error"] - b["All_Error"]).max())
    print("max |All_Error difference| over the stability repeats:", worst)
    assert worst <= 1e-6
    # the factors of one repeat at a fixed number of sweeps are bitwise equal
    dev = batched.DeviceData(pre, zero, zero, zero, rn, cn, pre_processed=True)
    try:
        draw = batched.stability_draws(dev.data_shapes, 1, 0.9, 7)[0]
        a, b = (dev.factorise(3, 200, 2007, samples=draw, **opt) for opt in ({}, {"sparse_on_device": True}))
    finally:
        dev.close()
    _same_arrays(a, b, ("output_f", "output_s", "output_g", "row_clusters", "col_clusters"))
    assert np.abs(a["All_Error"] - b["All_Error"]).max() <= 1e-6


def test_k_sweep_through_the_api_is_identical():
    x1, x2 = planted_sparse(1)[0], planted_sparse(2)[0]
    kw = dict(spurious=False, k_sweep=True, bisil_sparse=True, n_iters=50, seed=7, return_sweep=True)
    off = resnmtf_amd.apply_resnmtf([x1, x2], **kw)
    on = resnmtf_amd.apply_resnmtf([x1, x2], sparse_on_device=True, **kw)
    assert list(on) == list(off) and on["k_sweep"] == off["k_sweep"]          # copies are bitwise: every score equal
    _same_arrays(on, off, ("output_f", "output_s", "output_g", "row_clusters", "col_clusters", "lambda", "mu"))
    assert on["All_Error"].tobytes() == off["All_Error"].tobytes() and on["bisil"] == off["bisil"]


def trimming_pair():
    """Two views sharing their 180 rows: the planted view and a 180 x 150 view at 1 % with one more entry per column
    (no all-zero column in the whole view).  At a 90 % row sample a column whose only entries sit in left-out rows
    comes out empty, as do rows without an entry in the sampled columns: the draws are trimmed."""
    x1 = planted_sparse(1)[0]
    rng = np.random.default_rng(3)
    thin = sp.random(180, 150, density=0.01, random_state=4, format="lil")
    thin[rng.integers(0, 180, 150), np.arange(150)] = 1.0
    return [x1, sp.csc_matrix(thin)]


def test_trimming_returns_the_same_draws():
    data = trimming_pair()
    rn, cn = naming.give_names(data, None, None, None, None)
    pre = naming.check_data(data)
    zero = np.zeros((2, 2))
    dev = batched.DeviceData(pre, zero, zero, zero, rn, cn, pre_processed=True)
    try:
        draw = batched.stability_draws(dev.data_shapes, 1, 0.9, 5)[0]
        off = dev._trim_samples(draw)
        on = dev._trim_samples(draw, sparse_on_device=True)
    finally:
        dev.close()
    assert off is not None and on is not None
    assert len(off[0][1]) < len(draw[0][1]) or len(off[1][1]) < len(draw[1][1])          # a trimming round happened
    for v in range(2):
        assert np.array_equal(on[0][v], off[0][v]) and np.array_equal(on[1][v], off[1][v])
