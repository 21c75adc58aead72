"""Device shuffles of sparse views (resnmtf_shuffle_view_sparse, DESIGN.md section 10 "Sparse shuffles"): the view after
a device shuffle is bit for bit the view resnmtf_set_view_csc makes of the same shuffle built on the host (shuffle_ref)
from the source's stored fp32 values; it is the dense path's draw of the densified view; refusals; and spurious-bicluster
removal on sparse data through res_nmtf_inner, the stability repeats and apply_resnmtf's k sweep."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import resnmtf_amd
from resnmtf_amd import api, batched, naming, sparse, spurious, synth
from resnmtf_amd._lib import ResnmtfError
from resnmtf_amd.engine import Engine, _dp, _ip
from stability_ref import relevance_counts

import shuffle_ref

pytestmark = pytest.mark.gpu


def _f32(a):
    return np.asarray(a).astype(np.float32).astype(np.float64)


def _random_csc(n, m, density, seed):
    x = sp.random(n, m, density=density, random_state=seed, format="csc")
    x.data = _f32(x.data + 0.05)
    return x


def _case(name):
    """(source CSC, k, run sweeps).  Values are fp32-representable, so a dense engine can hold the same matrix."""
    if name == "37x23":                 # 50 %, one stored entry whose fp32 value is an explicit zero on the device
        x = _random_csc(37, 23, 0.5, 1)
        x.data[5] = 1.0e-60
        return x, 3, True
    if name == "64x64":                 # fully stored: count = 4^6, no cycle walking
        return sp.csc_matrix(_f32(np.random.default_rng(2).random((64, 64)) + 0.1)), 4, True
    if name == "300x200":               # 5 % plus one dense row and one dense column: a wide block in the plan
        d = _random_csc(300, 200, 0.05, 3).toarray()
        rng = np.random.default_rng(4)
        d[17, :] = _f32(rng.random(200) + 0.1); d[:, 31] = _f32(rng.random(300) + 0.1)
        return sp.csc_matrix(d), 5, True
    if name == "300x200_1pct":          # shuffles with empty lines
        return _random_csc(300, 200, 0.01, 5), 3, False
    if name == "70000x70000":           # n m > 2^32: 64-bit keys; structure only
        rng = np.random.default_rng(6)
        pos = np.unique(rng.integers(0, 70000 * 70000, 2000, dtype=np.int64))
        return sp.csc_matrix((_f32(rng.random(len(pos)) + 0.1), (pos // 70000, pos % 70000)), shape=(70000, 70000)), 2, False
    if name == "50x30_empty":
        return sp.csc_matrix((50, 30)), 2, False
    raise KeyError(name)


def _upload_csc(eng, v, c, pre_processed):
    """resnmtf_set_view_csc with the arrays as they are (Engine.set_view_sparse would drop the explicit zeros)."""
    col_ptr = np.ascontiguousarray(c.indptr, dtype=np.int64)
    row_idx = np.ascontiguousarray(c.indices, dtype=np.int32)
    vals = np.ascontiguousarray(c.data, dtype=np.float64)
    if row_idx.size == 0:
        row_idx = np.zeros(1, dtype=np.int32); vals = np.zeros(1)
    eng._check(eng._lib.resnmtf_set_view_csc(eng._h, v, col_ptr.ctypes.data_as(C.POINTER(C.c_longlong)), _ip(row_idx), _dp(vals),
                                             1 if pre_processed else 0))


def _same_csc(a, b):
    return (np.array_equal(a.indptr, b.indptr) and np.array_equal(a.indices, b.indices)
            and a.data.tobytes() == b.data.tobytes())


def _host_masks(s):
    positive = s.data > 0
    rows = np.bincount(s.indices[positive], minlength=s.shape[0]) == 0
    cols = np.bincount(np.repeat(np.arange(s.shape[1]), np.diff(s.indptr))[positive], minlength=s.shape[1]) == 0
    return rows, cols


def _sparse_engine(x, k, nnz=None):
    n, m = x.shape
    return Engine([n], [m], [k], nnz=[x.nnz if nnz is None else nnz])


@pytest.mark.parametrize("name", ["37x23", "64x64", "300x200", "300x200_1pct", "70000x70000", "50x30_empty"])
def test_device_shuffle_is_bitwise_the_host_built_shuffle(name):
    x, k, sweeps = _case(name)
    n, m = x.shape
    seed = 1000003 * 17 + 3
    with _sparse_engine(x, k) as src, _sparse_engine(x, k) as dst, _sparse_engine(x, k) as ref:
        _upload_csc(src, 0, x, True)
        held = src.get_view_sparse(0)
        assert _same_csc(held, sp.csc_matrix((_f32(x.data), x.indices, x.indptr), shape=x.shape))
        if name == "37x23":
            assert (held.data == 0).sum() == 1              # the explicit zero is stored on the device
        want = shuffle_ref.shuffle_csc(held, seed)
        er, ec = _host_masks(want)
        for normalise in ([False] if ec.any() else [False, True]):
            dst.shuffle_view_sparse_from(0, src, 0, seed=seed, normalise=normalise)
            got = dst.get_view_sparse(0)
            assert dst.view_storage(0) == (True, x.nnz, x.nnz) and got.nnz == x.nnz
            _upload_csc(ref, 0, want, not normalise)
            assert _same_csc(got, ref.get_view_sparse(0)), (name, normalise)
            if not normalise:
                assert _same_csc(got, want)
            gr, gc, nr, nc = dst.empty_lines(0, counts=True)
            assert np.array_equal(gr, er) and np.array_equal(gc, ec) and (nr, nc) == (er.sum(), ec.sum())
            pa, pb = dst.view_plan(0), ref.view_plan(0)
            assert pa["sparse_blocks"] == pb["sparse_blocks"] and pa["nsplit"] == pb["nsplit"] and pa["image"] == "sparse"
            if sweeps:
                f, s, g = synth.random_init(n, m, k, 9)
                out = []
                for eng in (dst, ref):
                    eng.set_factors(0, f, s, g)
                    errs = eng.run(3)
                    out.append((errs, *eng.get_factors(0)[:3]))
                assert np.isfinite(out[0][0]).all()
                for a, b in zip(*out):
                    assert a.tobytes() == b.tobytes(), (name, normalise)
        if name == "300x200_1pct":
            assert er.any() and ec.any()                     # the masks were checked on a draw that has empty lines
        if name == "50x30_empty":
            assert er.all() and ec.all() and got.nnz == 0


@pytest.mark.parametrize("name", ["37x23", "64x64", "300x200", "300x200_1pct"])
def test_same_draw_as_the_dense_path(name):
    x, k, _ = _case(name)
    n, m = x.shape
    seed = 1000003 * 5 + 1
    dense_x = _f32(x.toarray())
    with _sparse_engine(x, k) as src, _sparse_engine(x, k) as dst, Engine([n], [m], [k]) as dsrc, Engine([n], [m], [k]) as ddst:
        _upload_csc(src, 0, x, True)
        dsrc.set_view(0, dense_x)
        dst.shuffle_view_sparse_from(0, src, 0, seed=seed, normalise=False)
        ddst.shuffle_view_from(0, dsrc, 0, seed=seed, normalise=False)
        assert np.array_equal(dst.get_view_sparse(0).toarray(), ddst.get_view(0))
        a, b = dst.empty_lines(0, counts=True), ddst.empty_lines(0, counts=True)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2:] == b[2:]
        if name == "300x200_1pct":
            assert a[0].any() and a[1].any()
            return
        assert not a[1].any()
        dst.shuffle_view_sparse_from(0, src, 0, seed=seed, normalise=True)
        ddst.shuffle_view_from(0, dsrc, 0, seed=seed, normalise=True)
        u, w = dst.get_view_sparse(0).toarray(), ddst.get_view(0)
        # both are the fp32 rounding of fp64 quotients whose column sums differ by summation order only (<= n 2^-53
        # relative): at most one fp32 ulp apart, 2^-23 relative to the larger; the bar is 2^-22
        assert np.array_equal(u != 0, w != 0)
        assert np.all(np.abs(u - w) <= 2.0 ** -22 * np.abs(w))


def test_determinism_and_seeds():
    x, k, _ = _case("300x200")
    with _sparse_engine(x, k) as src, _sparse_engine(x, k) as a, _sparse_engine(x, k) as b:
        _upload_csc(src, 0, x, True)
        a.shuffle_view_sparse_from(0, src, 0, seed=7)
        first = a.get_view_sparse(0)
        a.shuffle_view_sparse_from(0, src, 0, seed=7)
        b.shuffle_view_sparse_from(0, src, 0, seed=7)
        assert _same_csc(first, a.get_view_sparse(0)) and _same_csc(first, b.get_view_sparse(0))
        b.shuffle_view_sparse_from(0, src, 0, seed=8)
        other = b.get_view_sparse(0)
        assert other.nnz == first.nnz and not np.array_equal(other.indices, first.indices)
        a.shuffle_view_sparse_from(0, src, 0, seed=7, normalise=False)
        b.shuffle_view_sparse_from(0, src, 0, seed=8, normalise=False)
        ua, ub = a.get_view_sparse(0), b.get_view_sparse(0)                     # un-normalised: the same values moved
        assert np.array_equal(np.sort(ua.data), np.sort(ub.data)) and not np.array_equal(ua.indptr, ub.indptr)


def _ready(eng, x, k):
    """Data and factors on a handle, so that it can run a sweep after a refusal."""
    n, m = x.shape
    if eng.sparse[0]:
        eng.set_view_sparse(0, x, pre_processed=False)
    else:
        d = x.toarray() + 1e-3
        eng.set_view(0, d / d.sum(axis=0))
    eng.set_factors(0, *synth.random_init(n, m, k, 3))


ERROR_CASES = ["dense_dst", "dense_src", "shape", "capacity", "not_uploaded", "get_csc_dense"]


@pytest.mark.parametrize("case", ERROR_CASES)
def test_refusals_leave_the_handle_usable(case):
    """Every case is a host-side check of the library; nothing is launched for it."""
    x = _random_csc(60, 40, 0.5, 8)
    other = _random_csc(61, 40, 0.5, 9)
    k = 3
    with _sparse_engine(x, k) as src, _sparse_engine(x, k) as dst, Engine([60], [40], [k]) as dense:
        for eng in (src, dst, dense):
            _ready(eng, x, k)
        if case == "dense_dst":
            call, code, text, after = (lambda: dense.shuffle_view_sparse_from(0, src, 0, seed=1)), 1, "destination view is dense", dense
        elif case == "dense_src":
            call, code, text, after = (lambda: dst.shuffle_view_sparse_from(0, dense, 0, seed=1)), 1, "source view is dense", dst
        elif case == "get_csc_dense":
            call, code, text, after = (lambda: dense.get_view_sparse(0)), 1, "dense", dense
        elif case == "shape":
            with _sparse_engine(other, k) as odd:
                odd.set_view_sparse(0, other)
                with pytest.raises(ResnmtfError, match="differ in shape") as info:
                    dst.shuffle_view_sparse_from(0, odd, 0, seed=1)
            assert info.value.code == 1
            call = None; after = dst
        elif case == "capacity":
            with _sparse_engine(x, k, nnz=x.nnz - 1) as small:
                with pytest.raises(ResnmtfError, match="capacity") as info:
                    small.shuffle_view_sparse_from(0, src, 0, seed=1)
                assert info.value.code == 1
                small.set_view_sparse(0, _random_csc(60, 40, 0.3, 10)); small.set_factors(0, *synth.random_init(60, 40, k, 3))
                assert np.isfinite(small.run(1)).all()
            call = None; after = dst
        else:
            with _sparse_engine(x, k) as bare:
                with pytest.raises(ResnmtfError, match="not been uploaded") as info:
                    dst.shuffle_view_sparse_from(0, bare, 0, seed=1)
            assert info.value.code == 5
            call = None; after = dst
        if call is not None:
            with pytest.raises(ResnmtfError, match=text) as info:
                call()
            assert info.value.code == code
        assert np.isfinite(after.run(1)).all()


# ------------------------------------------------------------------------------------------------------ the pipeline
def planted_sparse(seed):
    """The planted problem of tests/test_gpu_sparse.py (test-resnmtf.R:38-52 with the noise kept at 5 %): three 60 x 60
    blocks of height 10 in 180 x 180, density 0.367 -- 66 stored entries per line against ln(180) = 5.2: checked on
    the CPU with shuffle_ref.attempts_needed, every draw of the seeds used here (and of the 90 % and 80 % sub-samples)
    passes the redraw rule at its first attempt."""
    rng = np.random.default_rng(seed)
    rc = np.kron(np.eye(3), np.ones((60, 1)))
    x = rc @ np.diag([10.0, 10.0, 10.0]) @ rc.T + 0.1 * np.abs(rng.normal(size=(180, 180))) * (rng.random((180, 180)) < 0.05)
    return sp.csr_matrix(x), rc


def _inner_args(data):
    rn, cn = naming.give_names(data, None, None, None, None)
    return naming.check_data(data), naming.shared_names(rn), naming.shared_names(cn), rn, cn


def _equal_results(got, want, keys):
    for key in keys:
        for a, b in zip(got[key], want[key]):
            assert a.tobytes() == b.tobytes(), key


def test_res_nmtf_inner_equals_remove_spurious_bitwise_on_sparse_views():
    data = [planted_sparse(1)[0], planted_sparse(2)[0]]
    pre, ri, ci, rn, cn = _inner_args(data)
    assert all(sparse.is_sparse(d) for d in pre)
    for v, d in enumerate(pre):
        assert shuffle_ref.attempts_needed(d, 4 * 7919 + 1, v) == 1
    k, R = 3, 3
    kw = dict(k_vec=[k, k], row_names=rn, col_names=cn, seed=4, num_repeats=R, max_iters=3000)   # (a guard, the same on both sides)
    got = api.res_nmtf_inner(pre, ri, ci, spurious=True, spurious_on_device=True, shuffle_sparse=True, **kw)
    plain = api.res_nmtf_inner(pre, ri, ci, spurious=False, **kw)
    want = spurious.remove_spurious(pre, plain, R, seed=4, max_iters=3000, shuffle_sparse=True)
    _equal_results(got, want, ("output_f", "output_s", "output_g", "lambda", "mu", "row_clusters", "col_clusters"))
    assert got["All_Error"].tobytes() == want["All_Error"].tobytes()
    for key in ("score", "avg_threshold", "max_threshold", "removed"):
        assert np.asarray(got["spurious"][key]).tobytes() == np.asarray(want["spurious"][key]).tobytes(), key
    # recorded, not asserted: the same pipeline on the densified data (DESIGN.md section 10 "Sparse shuffles")
    dense = api.res_nmtf_inner([_f32(d.toarray()) for d in pre], ri, ci, spurious=True, spurious_on_device=True, **kw)
    for key in ("score", "avg_threshold", "max_threshold", "removed"):
        print(f"sparse {key}: {np.asarray(got['spurious'][key]).tolist()}")
        print(f"dense  {key}: {np.asarray(dense['spurious'][key]).tolist()}")
    print("max |score difference|:", np.abs(got["spurious"]["score"] - dense["spurious"]["score"]).max(),
          " min margin |score - max_threshold|:",
          np.abs(got["spurious"]["score"] - got["spurious"]["max_threshold"][:, None]).min())


def test_stability_repeat_with_removal_equals_the_host_composition_on_sparse_views():
    data = [planted_sparse(3)[0], planted_sparse(4)[0]]
    pre, ri, ci, rn, cn = _inner_args(data)
    k, R, n_stab, rate, seed = 3, 2, 2, 0.8, 9
    res = api.res_nmtf_inner(pre, ri, ci, k_vec=[k, k], row_names=rn, col_names=cn, seed=4, spurious=False)
    zero = np.zeros((2, 2))
    out = api.stability_check(pre, res, k, zero, zero, zero, None, True, R, False, "euclidean", rate, n_stab,
                              remove_unstable=False, row_names=rn, col_names=cn, seed=seed, spurious_on_device=True,
                              shuffle_sparse=True)
    dev = batched.DeviceData(pre, zero, zero, zero, rn, cn, pre_processed=True)
    try:
        draws = batched.stability_draws(dev.data_shapes, n_stab, rate, seed)
        total = None
        for r in range(n_stab):
            rep = dev.factorise(k, None, seed + 2000 + r, samples=draws[r])
            rows, cols = rep["extras"]["row_samples"], rep["extras"]["col_samples"]
            sub = [sparse.subsample(dev.sp[v], rows[v], cols[v])[0] for v in range(2)]
            cleaned = spurious.remove_spurious(sub, rep, R, seed=seed + 2000 + r, shuffle_sparse=True)
            one = np.stack([relevance_counts(cleaned["row_clusters"][v], cleaned["col_clusters"][v],
                                             res["row_clusters"][v][rows[v]], res["col_clusters"][v][cols[v]])
                            for v in range(2)])
            total = one if total is None else total + one
    finally:
        dev.close()
    assert out["relevance"].tobytes() == (total / n_stab).tobytes()


def test_default_pipeline_runs_on_a_mixed_sparse_and_dense_pair():
    x1 = planted_sparse(1)[0]
    x2 = planted_sparse(2)[0].toarray()
    kw = dict(k_min=3, k_max=4, k_sweep=True, seed=7, num_repeats=2, n_stability=2, spurious_on_device=True,
              return_sweep=True)
    res = resnmtf_amd.apply_resnmtf([x1, x2], bisil_sparse=True, shuffle_sparse=True, **kw)
    dense = resnmtf_amd.apply_resnmtf([x1.toarray(), x2], **kw)
    assert list(res) == list(dense)
    assert res["output_f"][0].shape[0] == 180 and np.asarray(res["spurious"]["removed"]).shape[0] == 2
    with pytest.raises(NotImplementedError, match="device shuffles of sparse views are not supported"):
        resnmtf_amd.apply_resnmtf([x1, x2], bisil_sparse=True, **kw)
