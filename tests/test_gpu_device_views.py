"""Dense views taken from device memory and results left there (``resnmtf_set_view_device`` /
``resnmtf_finalise_device``).  The yardstick is the host route in the same process: every
comparison is on bits (``np.array_equal``, NaN positions included), no tolerance anywhere."""
import ctypes as C
import warnings

import numpy as np
import pytest

import resnmtf_amd
from resnmtf_amd import _lib, api, naming, synth
from resnmtf_amd.engine import Engine
from resnmtf_amd.problem import prepare

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DTYPES = {"fp64": torch.float64, "fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}
# ragged 32- and 64-tiles, an exact tile, and the smallest n that gives a column partial (rows r = p mod 256) a second row
SHAPES = [(70, 45), (33, 97), (64, 64), (257, 31)]


def same(a, b) -> bool:
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a, b, equal_nan=True)


def host(t) -> np.ndarray:
    return t.detach().double().cpu().numpy()


def layouts(vals):
    """The same n x m values as a row-major tensor, a column-major one, a transposed view of an m x n tensor, and a slice
    of a larger tensor with neither stride 1 and a storage offset."""
    n, m = vals.shape
    big = torch.full((n + 7, 2 * m + 9), 0.5, dtype=vals.dtype, device=vals.device)
    big[3:3 + n, 5:5 + 2 * m:2] = vals
    tr = vals.T.clone(memory_format=torch.contiguous_format)      # m x n, row-major
    out = {"row": vals.contiguous(), "col": vals.T.contiguous().T, "transposed": tr.T, "slice": big[3:3 + n, 5:5 + 2 * m:2]}
    assert out["row"].stride() == (m, 1) and out["col"].stride() == (1, n) and out["transposed"].stride() == (1, n)
    assert out["slice"].stride() == (2 * m + 9, 2) and out["slice"].storage_offset() == 3 * (2 * m + 9) + 5
    for t in out.values():
        assert torch.equal(t, vals)
    return out


def datasets(n, m, dtype, seed):
    """name -> (values in `dtype` on the device, raw, run a sweep on it)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(n, m, generator=g, dtype=torch.float64) + 0.05
    pre = x / x.sum(0, keepdim=True)                      # non-negative, column-normalised (then rounded to `dtype`)
    neg = x.clone()
    neg[:, ::3] -= 0.4                                    # negative entries in some columns
    zero = neg.clone()
    zero[:, m // 2] = 0.0                                 # one all-zero column: NaN, as sweep(..., "/") gives
    return {"pre": (pre.to(dtype).to(DEV), False, True), "raw_neg": (neg.to(dtype).to(DEV), True, True),
            "raw_zero_col": (zero.to(dtype).to(DEV), True, False), "raw_nonneg": (x.to(dtype).to(DEV), True, False)}


def one_sweep(eng, init):
    """F, S, G, lambda, mu after one sweep from `init`: they read BOTH images.  (The sweep's error, which carries
    data_norms, is compared in test_norm_and_sweeps_equal_the_host_route.)"""
    eng.set_factors(0, *init)
    eng.run(n_iters=1)
    return tuple(eng.get_factors(0))


@pytest.mark.parametrize("dname", list(DTYPES))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_images_equal_the_host_route(shape, dname):
    n, m = shape
    k = 3
    init = synth.random_init(n, m, k, 11)
    with Engine([n], [m], [k]) as eng:
        for name, (vals, raw, sweep) in datasets(n, m, DTYPES[dname], 100 * n + m).items():
            x = host(vals)
            flag_ref = eng.set_view_raw(0, x) if raw else (eng.set_view(0, x) or False)
            ref = eng.get_view(0)
            ref_sweep = one_sweep(eng, init) if sweep else None
            assert flag_ref == (name in ("raw_neg", "raw_zero_col"))
            assert np.isnan(ref).any() == (name == "raw_zero_col")
            for lname, t in layouts(vals).items():
                eng.set_view(0, np.full((n, m), 1.0 / n))          # (whatever the last upload left is gone)
                flag = eng.set_view_device(0, t, raw=raw)
                what = f"{name} / {lname}"
                assert flag == flag_ref, what
                assert same(eng.get_view(0), ref), what
                er, ec = eng.empty_lines(0)
                assert not er.any() and not ec.any(), what
                if sweep:
                    for a, b in zip(one_sweep(eng, init), ref_sweep):
                        assert np.isfinite(b).all(), what
                        assert same(a, b), what


@pytest.mark.parametrize("n, m, k, opts", [(600, 130, 5, {}), (300, 200, 20, {}), (600, 130, 5, {"x_half": 3})],
                         ids=["k5", "k20_wide", "k5_x_half3"])
def test_norm_and_sweeps_equal_the_host_route(n, m, k, opts):
    t = torch.tensor(synth.planted_view(n, m, k, 5), dtype=torch.float32, device=DEV)
    assert t.stride() == (m, 1)
    init = synth.random_init(n, m, k, 6)
    out = []
    for device_route in (True, False):
        with Engine([n], [m], [k], **opts) as eng:
            if device_route:
                eng.set_view_device(0, t)
            else:
                eng.set_view(0, host(t))
            eng.set_factors(0, *init)
            errs = eng.run(n_iters=5)
            out.append((errs, eng.view_image_info(0)) + tuple(eng.get_factors(0)))
    assert len(out[0][0]) == 5 and np.isfinite(out[0][0]).all()
    assert out[0][1] == out[1][1]
    for a, b in zip(out[0], out[1]):
        assert same(a, b)


def test_upload_is_ordered_after_the_producer_stream():
    n, m = 1500, 1100
    base = torch.rand(n, m, device=DEV, dtype=torch.float32)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=DEV)
    with Engine([n], [m], [3]) as eng:
        with torch.cuda.stream(side):
            t = base
            for _ in range(200):                       # a queue of work the upload has to wait for
                t = t * 1.0009765625 + 0.03125
            t = t / t.sum(0, keepdim=True)             # the producer, enqueued immediately before the call
            eng.set_view_device(0, t)                  # (no synchronisation by the test)
        got = eng.get_view(0)
        torch.cuda.synchronize()
        eng.set_view(0, host(t))
        assert same(got, eng.get_view(0))


def test_finalise_device_equals_finalise():
    n, m, k = 130, 75, 4
    with Engine([n], [m], [k]) as eng:
        eng.set_view(0, synth.planted_view(n, m, k, 8))
        eng.set_factors(0, *synth.random_init(n, m, k, 9))
        eng.run(n_iters=5)
        ref = eng.finalise(0)
        out = eng.finalise_device(0)
        again = eng.finalise(0)
    assert len(out) == 5
    for t, a, b, shape in zip(out, ref, again, ((n, k), (k, k), (m, k), (n, k), (m, k))):
        assert isinstance(t, torch.Tensor) and t.dtype == torch.float64 and t.device == torch.device(DEV)
        assert tuple(t.shape) == shape and t.stride() == (1, shape[0])            # column-major
        assert same(t.cpu().numpy(), a) and same(a, b)


RESULT_KEYS = ("output_f", "output_s", "output_g", "row_clusters", "col_clusters")


def assert_same_results(dev_res, ref, on_device: bool):
    for key in RESULT_KEYS:
        for t, a in zip(dev_res[key], ref[key]):
            if on_device:
                assert isinstance(t, torch.Tensor) and t.device == torch.device(DEV) and t.dtype == torch.float64
                t = t.cpu().numpy()
            assert isinstance(a, np.ndarray) and same(t, a), key
    for key in ("All_Error", "Error", "lambda", "mu"):
        if key in ref:
            assert isinstance(dev_res[key], type(ref[key]))
            assert same(np.asarray(dev_res[key], dtype=np.float64), np.asarray(ref[key], dtype=np.float64)), key


def test_res_nmtf_inner_on_device_views_returns_tensors():
    prob = synth.make_problem([(120, 60), (120, 40)], 3, phi=2.0)
    ts = [torch.tensor(d, dtype=torch.float32, device=DEV) for d in prob.data]
    rs, cs = naming.shared_names(prob.row_names), naming.shared_names(prob.col_names)
    kw = dict(k_vec=[3, 3], phi=prob.phi, xi=prob.xi, psi=prob.psi, n_iters=30, spurious=False,
              row_names=prob.row_names, col_names=prob.col_names, seed=5)
    ref = resnmtf_amd.res_nmtf_inner([host(t) for t in ts], rs, cs, **kw)
    res = resnmtf_amd.res_nmtf_inner(ts, rs, cs, output="torch", **kw)
    assert_same_results(res, ref, True)
    assert list(res) == list(ref)
    mixed = resnmtf_amd.res_nmtf_inner([ts[0], host(ts[1])], rs, cs, **kw)         # views may be mixed; NumPy out
    assert_same_results(mixed, ref, False)


def test_apply_resnmtf_on_device_views():
    """The device views are shifted and normalised on the device, the host arrays by ``check_data`` in NumPy: the column
    sums differ in their summation order, by a few ulp of fp64, and both routes round the quotient to f32 once.  The
    planted problem's 12000 entries are far too few for one of them to sit that close to an f32 rounding boundary, so
    clusters and factors are compared on bits like everything else; ``All_Error`` carries the fp64 ``data_norms`` and is
    left out."""
    prob = synth.make_problem([(120, 60), (120, 40)], 3, phi=2.0)
    ts = [torch.tensor(d, dtype=torch.float32, device=DEV) for d in prob.data]
    kw = dict(k_val=3, phi=prob.phi, n_iters=100, spurious=False, stability=True, seed=7, n_stability=3)
    ref = resnmtf_amd.apply_resnmtf([host(t) for t in ts], **kw)
    res = resnmtf_amd.apply_resnmtf(ts, output="torch", **kw)
    plain = resnmtf_amd.apply_resnmtf(ts, **kw)
    assert sum(rc.sum() for rc in ref["row_clusters"]) > 0
    for key in RESULT_KEYS:
        for t, p, a in zip(res[key], plain[key], ref[key]):
            assert isinstance(t, torch.Tensor) and t.device == torch.device(DEV)
            assert same(t.cpu().numpy(), a) and same(p, a), key
    # the relevance itself: stability_check on the pre-processed views, as exact fp64 tensors and as arrays
    p = prepare([host(t) for t in ts], prob.phi, None, None, None, None, normalise=True, symmetrise=True)
    inner = resnmtf_amd.res_nmtf_inner(p.data, p.row_shared, p.col_shared, k_vec=[3, 3], phi=p.phi, xi=p.xi, psi=p.psi,
                                       n_iters=100, spurious=False, row_names=p.row_names, col_names=p.col_names, seed=7)
    skw = dict(row_names=p.row_names, col_names=p.col_names, seed=7, n_stability=3, remove_unstable=False)
    rel_ref = api.stability_check(p.data, inner, 3, p.phi, p.xi, p.psi, 100, False, 5, False, "euclidean", **skw)
    rel_dev = api.stability_check([torch.tensor(d, dtype=torch.float64, device=DEV) for d in p.data], inner, 3, p.phi, p.xi,
                                  p.psi, 100, False, 5, False, "euclidean", **skw)
    assert rel_ref["relevance"].shape == (2, 3) and same(rel_dev["relevance"], rel_ref["relevance"])


def test_c_entry_refuses_before_any_device_work():
    n, m = 40, 30
    lib = _lib.load()
    x = np.asfortranarray(synth.planted_view(n, m, 3, 1))
    with Engine([n, n], [m, m], [3, 3], nnz=[None, 50]) as eng:
        eng.set_view(0, x)
        before = eng.get_view(0)
        t = torch.tensor(x, device=DEV)
        ptr, h = C.c_void_p(t.data_ptr()), eng._h
        calls = {"host pointer": lambda: lib.resnmtf_set_view_device(h, 0, C.c_void_p(x.ctypes.data), _lib.DTYPE_F64, 1, n, 0, None, None),
                 "NULL": lambda: lib.resnmtf_set_view_device(h, 0, None, _lib.DTYPE_F64, 1, n, 0, None, None),
                 "dtype": lambda: lib.resnmtf_set_view_device(h, 0, ptr, 7, m, 1, 0, None, None),
                 "stride": lambda: lib.resnmtf_set_view_device(h, 0, ptr, _lib.DTYPE_F64, -m, 1, 0, None, None),
                 "sparse": lambda: lib.resnmtf_set_view_device(h, 1, ptr, _lib.DTYPE_F64, m, 1, 0, None, None),
                 "host output": lambda: lib.resnmtf_finalise_device(h, 0, C.c_void_p(x.ctypes.data), None, None, None, None, None)}
        for what, call in calls.items():
            assert call() == 1, what                                              # RESNMTF_ERR_INVALID
            text = lib.resnmtf_last_error(h).decode()
            assert text, what
            if what == "host pointer":
                assert "device memory" in text
            if what == "sparse":
                assert "resnmtf_set_view_csc" in text
        assert same(eng.get_view(0), before)                                      # nothing was launched
        assert lib.resnmtf_set_view_device(h, 0, ptr, _lib.DTYPE_F64, m, 1, 0, None, None) == 0


def test_python_refusals_and_cpu_tensors():
    prob = synth.make_problem([(60, 40)], 3)
    kw = dict(k_vec=[3], n_iters=5, spurious=False, seed=1)
    x = torch.tensor(prob.data[0], dtype=torch.float32)
    with pytest.raises(ValueError, match="floating"):
        resnmtf_amd.res_nmtf_inner([torch.ones(60, 40, dtype=torch.int32, device=DEV)], None, None, **kw)
    with pytest.raises(ValueError, match="2-D"):
        resnmtf_amd.res_nmtf_inner(torch.ones(2, 60, 40, device=DEV), None, None, **kw)
    with pytest.raises(NotImplementedError, match="host_init"):
        resnmtf_amd.res_nmtf_inner(x.to(DEV), None, None, host_init=True, **kw)
    with Engine([60], [40], [3]) as eng:
        with pytest.raises(ValueError, match="lives on"):
            eng.set_view_device(0, x)
        with pytest.raises(ValueError, match="shape"):
            eng.set_view_device(0, x.to(DEV).T)
    # a CPU tensor is its NumPy array; output="torch" still returns tensors on the device; one tensor is one view
    ref = resnmtf_amd.res_nmtf_inner([host(x)], None, None, **kw)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        res = resnmtf_amd.res_nmtf_inner(x, None, None, output="torch", **kw)
    assert_same_results(res, ref, True)
