"""Factors taken from device memory and the raw state left there (``resnmtf_set_factors_device`` /
``resnmtf_get_factors_device``).  The yardstick is the host route in the same process: every
comparison is on bits (``np.array_equal``, NaN positions included), no tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

import resnmtf_amd
from resnmtf_amd import _lib, naming, synth
from resnmtf_amd._lib import ResnmtfError
from resnmtf_amd.engine import Engine

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DTYPES = {"fp64": torch.float64, "fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}
LAYOUTS = ("row", "col", "transposed", "slice")
# ragged 32-tiles of the transpose, an exact tile, several tiles; 257 rows at k = 64 are four staged chunks of the column
# sums (4096 / 64 = 64 rows each) and one row; 4097 rows at k = 1 are one more than the LARGEST chunk (4096 / 1 rows)
SHAPES = [(70, 64), (33, 97), (64, 64), (257, 70), (4097, 33)]
KS = (1, 3, 16, 17, 32, 33, 64)                # every KP form (16 / 32 / 48 / 64) and the Wk pieces above 16
RESULT_KEYS = ("output_f", "output_s", "output_g", "row_clusters", "col_clusters")


def same(a, b) -> bool:
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a, b, equal_nan=True)


def host(t) -> np.ndarray:
    return t.detach().double().cpu().numpy()


def layouts(vals):
    """The same n x m values as a row-major tensor, a column-major one, a transposed view of an m x n tensor, and a slice
    of a larger tensor with neither stride 1 and a storage offset (the construction of test_gpu_device_views.py)."""
    n, m = vals.shape
    big = torch.full((n + 7, 2 * m + 9), 0.5, dtype=vals.dtype, device=vals.device)
    big[3:3 + n, 5:5 + 2 * m:2] = vals
    tr = vals.T.clone(memory_format=torch.contiguous_format)      # m x n, row-major
    out = {"row": vals.contiguous(), "col": vals.T.contiguous().T, "transposed": tr.T, "slice": big[3:3 + n, 5:5 + 2 * m:2]}
    assert out["slice"].stride() == (2 * m + 9, 2) and out["slice"].storage_offset() == 3 * (2 * m + 9) + 5
    if m > 1:
        assert out["row"].stride() == (m, 1) and out["col"].stride() == (1, n) and out["transposed"].stride() == (1, n)
    for t in out.values():
        assert torch.equal(t, vals)
    return out


def view_data(n, m, seed):
    rng = np.random.default_rng(seed)
    x = rng.random((n, m)) + 0.05
    return x / x.sum(0, keepdims=True)


def init_tensors(n, m, k, seed, dtypes):
    """F, S, G of synth.random_init rounded to `dtypes` (one per matrix), on the device."""
    return [torch.tensor(a, dtype=torch.float64).to(dt).to(DEV) for a, dt in zip(synth.random_init(n, m, k, seed), dtypes)]


def state_and_sweep(eng, set_it):
    """(the raw state `set_it` leaves, the raw state one sweep later): the sweep reads W32 / Wk and both lm."""
    set_it()
    state = tuple(eng.get_factors(0))
    eng.run(n_iters=1)
    return state, tuple(eng.get_factors(0))


def assert_route_equals_host(eng, n, m, k, combos, seed):
    """combos: (dtype names of F, S, G; layout names of F, S, G).  The host reference is computed once per dtype triple."""
    scramble = synth.random_init(n, m, k, seed + 1)
    refs = {}
    for dnames, lnames in combos:
        ts = init_tensors(n, m, k, seed, [DTYPES[d] for d in dnames])
        if dnames not in refs:
            refs[dnames] = state_and_sweep(eng, lambda: eng.set_factors(0, *(host(t) for t in ts)))
        eng.set_factors(0, *scramble)                      # (whatever the last call left is gone)
        laid = [layouts(t)[ln] for t, ln in zip(ts, lnames)]
        got = state_and_sweep(eng, lambda: eng.set_factors_device(0, *laid))
        for stage, a_all, b_all in zip(("state", "sweep"), got, refs[dnames]):
            for name, a, b in zip(("F", "S", "G", "lambda", "mu"), a_all, b_all):
                assert same(a, b), f"{dnames} / {lnames}: {name} of the {stage}"


def single_combos(i):
    """One layout and one dtype per matrix, rotated by the case number; the three matrices differ in both."""
    d, l = list(DTYPES), list(LAYOUTS)
    return [(tuple(d[(i + j) % 4] for j in range(3)), tuple(l[(i + 2 * j + 1) % 4] for j in range(3)))]


FULL_CROSS = [((d,) * 3, (l,) * 3) for d in DTYPES for l in LAYOUTS]
# (k <= min(n, m): resnmtf_create refuses a k above either dimension, R/utils.r:444,449 -- 33 x 97 stops at k = 33)
CASES = [(shape, k) for shape in SHAPES for k in KS if k <= min(shape) and (shape[0] != 4097 or k in (1, 3, 33))]


@pytest.mark.parametrize("shape, k", CASES, ids=lambda x: f"{x[0]}x{x[1]}" if isinstance(x, tuple) else f"k{x}")
def test_state_equals_the_host_route(shape, k):
    n, m = shape
    full = shape == (70, 64) and k in (3, 33)          # the full dtype x layout cross at one k <= 16 and one above
    combos = FULL_CROSS + single_combos(0) if full else single_combos(CASES.index((shape, k)))
    with Engine([n], [m], [k]) as eng:
        eng.set_view(0, view_data(n, m, 3))
        assert_route_equals_host(eng, n, m, k, combos, seed=100 * n + k)
        if full:
            f, s, g, lam, mu = eng.get_factors(0)
            assert all(np.isfinite(a).all() for a in (f, s, g, lam, mu))


def test_state_equals_the_host_route_on_2_byte_images():
    n, m, k = 257, 70, 3
    with Engine([n], [m], [k], x_half=3) as eng:
        eng.set_view(0, synth.planted_view(n, m, k, 5))
        assert_route_equals_host(eng, n, m, k, FULL_CROSS[::5] + single_combos(1), seed=7)


def test_state_equals_the_host_route_on_a_sparse_view():
    import scipy.sparse as sp
    n, m, k = 257, 70, 17
    x = view_data(n, m, 4) * (np.random.default_rng(5).random((n, m)) < 0.3)
    x[0, :] += 1.0 / n                                     # (no empty column)
    x = sp.csc_matrix(x / x.sum(0, keepdims=True))
    with Engine([n], [m], [k], nnz=[x.nnz]) as eng:
        eng.set_view_sparse(0, x, pre_processed=True)
        assert_route_equals_host(eng, n, m, k, FULL_CROSS[::5] + single_combos(2), seed=8)


def sequential(col) -> float:
    t = 0.0
    for x in col:
        t += x
    return t


@pytest.mark.parametrize("dname", ["fp64", "fp32"])
def test_column_sums_keep_the_host_order(dname):
    """Columns of 1e16, 1.0 and -1e16 in random order: any pairwise or blocked sum differs from the sequential one
    (checked below on the CPU against NumPy's pairwise reduction).  3000 and 1500 rows at k = 3 are more than one staged
    chunk (4096 / 3 = 1365 rows) on both sides."""
    n, m, k = 3000, 1500, 3
    rng = np.random.default_rng(17)
    f, g = (np.asfortranarray(rng.choice([1e16, 1.0, -1e16], size=(rows, k), p=[0.25, 0.5, 0.25])) for rows in (n, m))
    tf, tg = (torch.tensor(a, dtype=torch.float64).to(DTYPES[dname]).to(DEV) for a in (f, g))
    ts = torch.eye(k, dtype=torch.float64, device=DEV)
    for a in (host(tf), host(tg)):
        for j in range(k):
            assert float(np.add.reduce(np.ascontiguousarray(a[:, j]))) != sequential(a[:, j])
    with Engine([n], [m], [k]) as eng:
        eng.set_factors(0, host(tf), host(ts), host(tg))
        ref = eng.get_factors(0)
        assert [sequential(host(tf)[:, j]) for j in range(k)] == list(ref[3])
        assert [sequential(host(tg)[:, j]) for j in range(k)] == list(ref[4])
        for lname in ("row", "col", "slice"):
            eng.set_factors(0, *synth.random_init(n, m, k, 1))
            eng.set_factors_device(0, layouts(tf)[lname], ts, layouts(tg)[lname])
            for a, b in zip(eng.get_factors(0), ref):
                assert same(a, b), lname
        # given lambda / mu (any dtype; a tensor or anything NumPy takes) are taken instead of the sums
        lam = torch.tensor([0.5, 3.0, 1.0e4], dtype=torch.float16, device=DEV)
        mu = [0.1, 0.7, 1.0e-3]
        eng.set_factors_device(0, tf, ts, tg, lam, mu)
        got = eng.get_factors(0)
        eng.set_factors(0, host(tf), host(ts), host(tg), host(lam), np.asarray(mu))
        for a, b in zip(got, eng.get_factors(0)):
            assert same(a, b)
        assert same(got[3], host(lam)) and same(got[4], np.asarray(mu))
        eng.set_factors_device(0, tf, ts, tg, None, torch.tensor(mu, dtype=torch.bfloat16, device=DEV))
        got = eng.get_factors(0)
        assert same(got[3], ref[3]) and same(got[4], host(torch.tensor(mu, dtype=torch.bfloat16)))


def test_mirror_view_takes_w_and_s_only():
    n, m, k = 70, 45, 5
    ts = init_tensors(n, m, k, 3, [torch.float32, torch.float64, torch.float16])
    with Engine([n, n], [m, m], [k, k], owned=[True, False]) as eng:
        eng.set_factors(1, *(host(t) for t in ts))
        ref = eng.get_factors(1, with_lm=False)
        eng.set_factors(1, *synth.random_init(n, m, k, 4))
        eng.set_factors_device(1, layouts(ts[0])["col"], ts[1], layouts(ts[2])["slice"])
        for a, b in zip(eng.get_factors(1, with_lm=False)[:3], ref[:3]):
            assert same(a, b)
        out = eng.get_factors_device(1, with_lm=False)
        assert out[3] is None and out[4] is None
        for t, b in zip(out[:3], ref[:3]):
            assert same(host(t), b)
        # lambda / mu of a view the handle does not own: refused, the view unchanged
        eng.set_factors(1, *synth.random_init(n, m, k, 4))
        before = eng.get_factors(1, with_lm=False)
        one = torch.ones(k, dtype=torch.float64, device=DEV)
        for lam, mu in ((one, None), (None, one)):
            with pytest.raises(ResnmtfError, match="owning handle") as exc:
                eng.set_factors_device(1, *ts, lam, mu)
            assert exc.value.code == 5                       # RESNMTF_ERR_STATE
        with pytest.raises(ResnmtfError, match="owning handle"):
            eng.get_factors_device(1, with_lm=True)
        for a, b in zip(eng.get_factors(1, with_lm=False)[:3], before[:3]):
            assert same(a, b)


def test_refusals_leave_the_state_as_it_was():
    """Every refusal of the C entry, made before any device work: with no factors set the view still has none (the run is
    refused), with factors set they and the next sweep are what they were."""
    n, m, k = 70, 45, 3
    lib = _lib.load()
    init = synth.random_init(n, m, k, 2)
    ts = init_tensors(n, m, k, 5, [torch.float64] * 3)
    host_f = np.ascontiguousarray(host(ts[0]))               # a host pointer

    def mat(t, **over):
        d = dict(ptr=t.data_ptr(), dtype=_lib.DTYPE_F64, row_stride=t.stride(0), col_stride=t.stride(1))
        d.update(over)
        return _lib.DeviceMatrix(d["ptr"], d["dtype"], d["row_stride"], d["col_stride"])

    good = [mat(t) for t in ts]
    lam = torch.ones(k, dtype=torch.float64, device=DEV)
    refusals = {
        "bad view": (7, good, None),
        "F NULL": (0, [None, good[1], good[2]], None),
        "G NULL": (0, [good[0], good[1], None], None),
        "S with a NULL ptr": (0, [good[0], mat(ts[1], ptr=None), good[2]], None),
        "lambda with a NULL ptr": (0, good, _lib.DeviceMatrix(None, _lib.DTYPE_F64, 1, 1)),
        "unknown dtype": (0, [good[0], good[1], mat(ts[2], dtype=9)], None),
        "unknown dtype of lambda": (0, good, _lib.DeviceMatrix(lam.data_ptr(), -1, 1, 1)),
        "negative row stride": (0, [mat(ts[0], row_stride=-k), good[1], good[2]], None),
        "negative column stride": (0, [good[0], mat(ts[1], col_stride=-1), good[2]], None),
        "host pointer": (0, [mat(ts[0], ptr=host_f.ctypes.data), good[1], good[2]], None),
        "host pointer of lambda": (0, good, _lib.DeviceMatrix(host_f.ctypes.data, _lib.DTYPE_F64, 1, 1)),
    }

    def refuse_all(eng):
        for what, (v, mats, lam_m) in refusals.items():
            args = [None if a is None else C.byref(a) for a in (*mats, lam_m, None)]
            rc = lib.resnmtf_set_factors_device(eng._h, v, *args, None)
            assert rc == 1, what                               # RESNMTF_ERR_INVALID
            assert lib.resnmtf_last_error(eng._h), what

    with Engine([n], [m], [k]) as eng, Engine([n], [m], [k]) as twin:
        for e in (eng, twin):
            e.set_view(0, view_data(n, m, 6))
        refuse_all(eng)
        with pytest.raises(ResnmtfError, match="set_factors missing"):      # has_factors is still false
            eng.run(n_iters=1)
        for e in (eng, twin):
            e.set_factors(0, *init)
        before = eng.get_factors(0)
        refuse_all(eng)
        for a, b in zip(eng.get_factors(0), before):
            assert same(a, b)
        assert same(eng.run(n_iters=1), twin.run(n_iters=1))
        for a, b in zip(eng.get_factors(0), twin.get_factors(0)):
            assert same(a, b)
        # the get direction: a host pointer is refused as resnmtf_finalise_device refuses it
        buf = np.zeros((n, k), order="F")
        assert lib.resnmtf_get_factors_device(eng._h, 0, C.c_void_p(buf.ctypes.data), None, None, None, None, None) == 1
        assert b"device memory" in lib.resnmtf_last_error(eng._h)
        assert lib.resnmtf_get_factors_device(eng._h, 3, None, None, None, None, None, None) == 1
        # python refusals
        with pytest.raises(TypeError, match="torch.Tensor"):
            eng.set_factors_device(0, init[0], ts[1], ts[2])
        with pytest.raises(ValueError, match="lives on"):
            eng.set_factors_device(0, ts[0].cpu(), ts[1], ts[2])
        with pytest.raises(ValueError, match="shape"):
            eng.set_factors_device(0, ts[0].T, ts[1], ts[2])
        with pytest.raises(ValueError, match="shape"):
            eng.set_factors_device(0, *ts, lam=torch.ones(k + 1, device=DEV))
        with pytest.raises(ValueError, match="fp64, fp32, fp16 or bf16"):
            eng.set_factors_device(0, ts[0].to(torch.int32), ts[1], ts[2])
        for a, b in zip(eng.get_factors(0), twin.get_factors(0)):
            assert same(a, b)


def test_set_is_ordered_after_the_producer_stream():
    n, m, k = 5000, 900, 8
    vals = init_tensors(n, m, k, 9, [torch.float32, torch.float64, torch.float32])
    fill = [torch.zeros_like(t) for t in vals]                # what a call that did not wait would read
    base = torch.rand(1500, 1100, device=DEV, dtype=torch.float32)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=DEV)
    with Engine([n], [m], [k]) as eng:
        with torch.cuda.stream(side):
            t = base
            for _ in range(200):                       # a queue of work the call has to wait for
                t = t * 1.0009765625 + 0.03125
            for dst, src in zip(fill, vals):           # the producers, enqueued immediately before the call
                dst.copy_(src)
            eng.set_factors_device(0, *fill)           # (no synchronisation by the test)
        got = eng.get_factors(0)
        torch.cuda.synchronize()
        eng.set_factors(0, *(host(t) for t in vals))
        for a, b in zip(got, eng.get_factors(0)):
            assert same(a, b)


def test_get_is_ordered_with_the_consumer_stream():
    n, m, k = 5000, 900, 8
    base = torch.rand(1500, 1100, device=DEV, dtype=torch.float32)
    side = torch.cuda.Stream(device=DEV)
    with Engine([n], [m], [k]) as eng:
        eng.set_view(0, view_data(n, m, 1))
        eng.set_factors(0, *synth.random_init(n, m, k, 2))
        eng.run(n_iters=2)
        ref = eng.get_factors(0)
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            t = base
            for _ in range(200):                       # work already enqueued where the outputs are allocated and used
                t = t * 1.0009765625 + 0.03125
            out = eng.get_factors_device(0)
            doubled = [x * 2.0 for x in out]           # the consumer, enqueued right after the call
        side.synchronize()
        for x, d, b in zip(out, doubled, ref):
            assert same(host(x), b) and same(host(d), b * 2.0)


def engine_resume_is_bitwise(prob, n, m, k) -> bool:
    """test_resume_is_exact's protocol on the host route: 20 sweeps against 12, then 8 on a fresh handle."""
    def fresh():
        e = Engine([n], [m], [k])
        e.set_view(0, prob.data[0]); e.set_restrictions(None, None, None)
        return e
    init = (prob.init_f[0], prob.init_s[0], prob.init_g[0])
    with fresh() as e1:
        e1.set_factors(0, *init); err_a = e1.run(20); fa = e1.get_factors(0)
    with fresh() as e2:
        e2.set_factors(0, *init); err_b1 = e2.run(12); mid = e2.get_factors(0)
    with fresh() as e3:
        e3.set_factors(0, *mid); err_b2 = e3.run(8); fb = e3.get_factors(0)
    return same(err_a, np.concatenate([err_b1, err_b2])) and all(same(x, y) for x, y in zip(fa, fb))


@pytest.mark.parametrize("n, m, k", [(500, 300, 6), (400, 320, 40)], ids=["k6", "k40"])
def test_round_trip_and_resume_through_the_public_entry(n, m, k):
    """12 + 8 sweeps, the second call started from the first call's "state" as it is, against 20 in one call.  The bar is
    the host route's: where a fresh-handle resume is bitwise with Engine (established first), the pair is bitwise the
    uninterrupted call; on either outcome the device route's pair is bitwise the host route's pair."""
    prob = synth.make_problem([(n, m)], k)
    exact = engine_resume_is_bitwise(prob, n, m, k)
    print(f"fresh-handle resume on the host route at k = {k}: {'bitwise' if exact else 'NOT bitwise'}")
    kw = dict(k_vec=[k], phi=prob.phi, xi=prob.xi, psi=prob.psi, spurious=False, return_state=True)
    init = (prob.init_f, prob.init_s, prob.init_g)

    def as_host(res, on_device):
        out = {key: [host(t) if on_device else t for t in res[key]] for key in RESULT_KEYS}
        out["state"] = [[host(t) if on_device else t for t in st] for st in res["state"]]
        return out

    pairs = {}
    for output in ("torch", "numpy"):
        dev = output == "torch"
        full = resnmtf_amd.res_nmtf_inner(prob.data, None, None, *init, n_iters=20, output=output, **kw)
        first = resnmtf_amd.res_nmtf_inner(prob.data, None, None, *init, n_iters=12, output=output, **kw)
        f, s, g, lam, mu = (list(x) for x in zip(*first["state"]))
        for t in f + s + g + lam + mu:
            assert (isinstance(t, torch.Tensor) and t.device == torch.device(DEV) and t.dtype == torch.float64) if dev \
                else isinstance(t, np.ndarray)
        if dev:
            assert f[0].stride() == (1, n) and g[0].stride() == (1, m)          # column-major, as finalise_device returns
        second = resnmtf_amd.res_nmtf_inner(prob.data, None, None, f, s, g, n_iters=8, output=output, init_lm=(lam, mu), **kw)
        errs = np.concatenate([first["All_Error"], second["All_Error"]])
        pairs[output] = (errs, as_host(second, dev))
        if exact:
            assert same(errs, full["All_Error"]), output
            want = as_host(full, dev)
            for key in RESULT_KEYS:
                assert all(same(a, b) for a, b in zip(pairs[output][1][key], want[key])), (output, key)
            assert all(same(a, b) for a, b in zip(pairs[output][1]["state"][0], want["state"][0])), output
    assert same(pairs["torch"][0], pairs["numpy"][0])
    for key in RESULT_KEYS:
        assert all(same(a, b) for a, b in zip(pairs["torch"][1][key], pairs["numpy"][1][key])), key
    assert all(same(a, b) for a, b in zip(pairs["torch"][1]["state"][0], pairs["numpy"][1]["state"][0]))
    if k == 6:
        assert exact                                    # (tests/test_gpu_parity.py::test_resume_is_exact)


def assert_same_results(res, ref, on_device, keys=("All_Error", "Error", "lambda", "mu")):
    for key in RESULT_KEYS:
        for t, a in zip(res[key], ref[key]):
            if on_device:
                assert isinstance(t, torch.Tensor) and t.device == torch.device(DEV) and t.dtype == torch.float64
                t = host(t)
            assert isinstance(a, np.ndarray) and same(t, a), key
    for key in keys:
        assert same(np.asarray(res[key], dtype=np.float64), np.asarray(ref[key], dtype=np.float64)), key


def test_public_entry_takes_device_factors():
    """Device tensors as views AND as initial factors against the all-NumPy call.  ``res_nmtf_inner`` takes its views as
    given: everything is bitwise, ``All_Error`` and ``"init"`` included.  ``apply_resnmtf`` normalises device views on the
    device and host views in NumPy (column sums in two orders, tests/test_gpu_device_views.py::
    test_apply_resnmtf_on_device_views): factors and clusters are bitwise the all-NumPy call's, and ``All_Error``, which
    carries ``data_norms``, is bitwise the call with the same device views and NumPy factors."""
    prob = synth.make_problem([(120, 60), (120, 40)], 3, phi=2.0)
    ts = [torch.tensor(d, dtype=torch.float32, device=DEV) for d in prob.data]
    rs, cs = naming.shared_names(prob.row_names), naming.shared_names(prob.col_names)
    dtypes = (torch.float64, torch.float32)
    init_host = [[host(torch.tensor(a).to(dt)) for a, dt in zip(part, dtypes)] for part in (prob.init_f, prob.init_s, prob.init_g)]
    init_dev = [[torch.tensor(a, dtype=dt, device=DEV) for a, dt in zip(part, dtypes)] for part in init_host]
    init_dev[0][1] = init_dev[0][1].T.contiguous().T           # (a column-major F beside row-major ones)
    kw = dict(k_vec=[3, 3], phi=prob.phi, xi=prob.xi, psi=prob.psi, n_iters=30, spurious=False,
              row_names=prob.row_names, col_names=prob.col_names, return_init=True)
    ref = resnmtf_amd.res_nmtf_inner([host(t) for t in ts], rs, cs, *init_host, **kw)
    res = resnmtf_amd.res_nmtf_inner(ts, rs, cs, *init_dev, output="torch", **kw)       # (a TypeError before this feature)
    assert_same_results(res, ref, True)
    assert list(res) == list(ref)
    for st, st_ref in zip(res["init"], ref["init"]):
        for t, a in zip(st, st_ref):
            assert isinstance(t, torch.Tensor) and t.device == torch.device(DEV) and same(host(t), a)
    # one view from the device, one from the host (CPU tensors: their fp64 arrays)
    mixed = resnmtf_amd.res_nmtf_inner(ts, rs, cs, *[[part[0], torch.tensor(part_h[1])] for part, part_h in zip(init_dev, init_host)], **kw)
    assert_same_results(mixed, ref, False)
    with pytest.raises(ValueError, match="view 1.*mix"):
        resnmtf_amd.res_nmtf_inner(ts, rs, cs, init_dev[0], init_dev[1], [init_dev[2][0], init_host[2][1]], **kw)

    akw = dict(k_val=3, phi=prob.phi, n_iters=30, spurious=False, stability=False)
    a_ref = resnmtf_amd.apply_resnmtf([host(t) for t in ts], *init_host, **akw)
    a_np_factors = resnmtf_amd.apply_resnmtf(ts, *init_host, output="torch", **akw)
    a_res = resnmtf_amd.apply_resnmtf(ts, *init_dev, output="torch", **akw)
    assert sum(rc.sum() for rc in a_ref["row_clusters"]) > 0
    assert_same_results(a_res, a_ref, True, keys=())
    assert_same_results(a_res, {key: [host(t) if isinstance(t, torch.Tensor) else t for t in val] if key in RESULT_KEYS else val
                                for key, val in a_np_factors.items()}, True)


@pytest.mark.parametrize("k", [3, 33])
def test_get_factors_device_equals_get_factors(k):
    n, m = 130, 75
    lib = _lib.load()
    with Engine([n], [m], [k]) as eng:
        eng.set_view(0, view_data(n, m, 8))
        eng.set_factors(0, *synth.random_init(n, m, k, 9))
        for sweeps in (0, 1, 4):                           # after 0, 1 and 5 sweeps
            if sweeps:
                eng.run(n_iters=sweeps)
            ref = eng.get_factors(0)
            out = eng.get_factors_device(0)
            assert len(out) == 5
            for t, a, shape in zip(out, ref, ((n, k), (k, k), (m, k), (k,), (k,))):
                assert t.dtype == torch.float64 and t.device == torch.device(DEV) and tuple(t.shape) == shape
                assert same(host(t), a)
            assert out[0].stride() == (1, n) and out[2].stride() == (1, m)
            # NULL outputs are skipped: S alone, the others untouched
            s_only = torch.full((k, k), -1.0, dtype=torch.float64, device=DEV)
            assert lib.resnmtf_get_factors_device(eng._h, 0, None, C.c_void_p(s_only.data_ptr()), None, None, None, None) == 0
            assert same(host(s_only.T), ref[1])            # (written column-major)
            part = eng.get_factors_device(0, with_lm=False)
            assert part[3] is None and part[4] is None and all(same(host(t), a) for t, a in zip(part[:3], ref[:3]))
            for a, b in zip(eng.get_factors(0), ref):      # (reading the state does not change it)
                assert same(a, b)
