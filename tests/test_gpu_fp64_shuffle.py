"""shuffle_view in double precision (resnmtf_fp64_shuffle): engine.fp64_shuffle against the NumPy
restatement of the draw (shuffle_ref.shuffle_dense), bit for bit the f32 route where both see the same numbers, the
normalised values against exact arithmetic, the redraw condition, what fp32 cannot see, and the guards of the C entry.

Bar of the normalised values (derived, not measured), relative and per entry, with u = 2^-53 and L = ceil(n / 256):
the device and the reference (data_ref.preprocess64) round the same numerator y = x + shift once, so it cancels.  The
device's column sum of the y's is a lane sum of at most L non-negative terms, (L - 1) u, then the 256-wide tree, 8 levels,
8 u; the reference's sum is the exactly rounded one, u.  Each side then rounds its quotient once, u + u.  To first order
the two quotients differ by at most (L - 1 + 8 + 1 + 2) u = (L + 10) u <= (L + 12) u = BAR(n), the bar the issue sets.
Worst measured on the MI355X: 4 u at 300 x 70 (bar 14 u), 3 u at 33 x 31 (13 u), 2 u at 257 x 3 (14 u) and 7 x 5 (13 u);
MEASURED_WORST below (the test prints every value before it asserts).

Every test prints ``MEASURED <what>: <value>`` before it asserts."""
import ctypes as C
import math

import numpy as np
import pytest

import data_ref as D
import shuffle_ref as S
from resnmtf_amd import _lib, engine
from resnmtf_amd.engine import Engine

gpu = pytest.mark.gpu

SHAPES = [(1, 1), (1, 7), (7, 1), (7, 5), (32, 32), (33, 31), (257, 3), (3, 257), (300, 70)]
SEEDS = [0, 1, 2 ** 64 - 1]
# worst relative |device / reference - 1| of the normalised values measured on the MI355X, in units of 2^-53, and where
MEASURED_WORST = (4.0, "300 x 70, every seed; bar there 14")     # (|got / ref - 1| itself is computed to within 2 units)


def bar(n: int) -> float:
    return (math.ceil(n / 256) + 12) * 2.0 ** -53


def measured(what, value):
    print(f"MEASURED {what}: {value:.3e}")


def shape_id(s):
    return f"{s[0]}x{s[1]}"


def fp64_data(n, m, seed):
    """Doubles that fp32 does not hold (asserted by the callers that need it)."""
    return np.random.default_rng(seed).random((n, m)) + 0.25


def host(t):
    return t.cpu().numpy()


def _torch_dev():
    import torch
    return torch, torch.device("cuda", 0)


# ---------------------------------------------------------------------------------------------------------------------
# 1. the draw, bit for bit shuffle_ref.shuffle_dense
# ---------------------------------------------------------------------------------------------------------------------
def test_the_shapes_exercise_the_cycle_walk_and_its_absence():
    assert S.half_bits(35) == 3 and 35 < 64                      # 7 x 5: the walk runs
    assert 4 ** S.half_bits(32 * 32) == 32 * 32                  # 32 x 32: no walk
    for n, m in SHAPES:
        for seed in SEEDS:
            pi = S.feistel_perm(np.arange(n * m), n * m, seed)
            assert np.array_equal(np.sort(pi), np.arange(n * m))


@gpu
@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_draw_of_a_host_array_and_of_fp64_tensors_in_every_layout(shape):
    torch, dev = _torch_dev()
    n, m = shape
    x = fp64_data(n, m, 10 * n + m)
    assert n * m == 1 or (x.astype(np.float32).astype(np.float64) != x).any()
    big = torch.as_tensor(fp64_data(2 * n, 3 * m + 1, 5), device=dev)
    sliced = big[::2, 1::3]
    assert tuple(sliced.shape) == (n, m)
    expanded = torch.as_tensor(fp64_data(n, 1, 6), device=dev).expand(n, m)
    t = torch.as_tensor(x, device=dev)
    sources = {"host": x, "row-major": t.contiguous(), "column-major": t.t().contiguous().t(), "slice": sliced, "expanded": expanded}
    assert m == 1 or n == 1 or sources["column-major"].stride() == (1, n)
    for seed in SEEDS:
        for name, src in sources.items():
            want = S.shuffle_dense(src if name == "host" else host(src), seed)
            got, neg, er, ec = engine.fp64_shuffle(src, seed, normalise=False)
            assert got.dtype == torch.float64 and tuple(got.shape) == (n, m) and (m == 1 or n == 1 or got.stride() == (1, n))
            assert np.array_equal(host(got), want), (name, seed)
            assert neg is False and er.shape == (n,) and ec.shape == (m,) and not er.any() and not ec.any()
            again = engine.fp64_shuffle(src, seed, normalise=False)[0]
            assert np.array_equal(host(again), want), (name, seed, "second call")


@gpu
@pytest.mark.parametrize("shape", [(7, 5), (257, 3), (300, 70)], ids=shape_id)
@pytest.mark.parametrize("dtype", ["float32", "float16", "bfloat16"])
def test_draw_of_narrow_dtypes_is_widened_exactly(shape, dtype):
    torch, dev = _torch_dev()
    n, m = shape
    t = torch.as_tensor(fp64_data(n, m, 3), device=dev).to(getattr(torch, dtype))
    for src in (t, t.t().contiguous().t(), t[::2, :], t[:1, :].expand(n, m)):
        want = S.shuffle_dense(host(src.double()), 1)
        got = engine.fp64_shuffle(src, 1, normalise=False)[0]
        assert np.array_equal(host(got), want)


@gpu
def test_draw_is_independent_of_the_destination_and_reproducible():
    """The caller's `out` filled with two different patterns before the call, through the C entry: the same bits."""
    torch, dev = _torch_dev()
    n, m = 33, 31
    x = np.asfortranarray(fp64_data(n, m, 8))
    outs = []
    for fill in (np.nan, -7.25):
        out = torch.full((m, n), fill, dtype=torch.float64, device=dev)
        code, _, res = _call(n=n, m=m, x=x, out=out, seed=5, normalise=1)
        assert code == 0
        outs.append(host(out).T.copy())
    assert np.array_equal(outs[0], outs[1]) and not np.isnan(outs[0]).any()
    assert np.array_equal(outs[0], host(engine.fp64_shuffle(x, 5, normalise=True)[0]))


# ---------------------------------------------------------------------------------------------------------------------
# 2. bit for bit the f32 route on fp32-valued data
# ---------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("shape", [(300, 70), (257, 3)], ids=shape_id)
def test_equals_the_f32_route_on_data_fp32_holds(shape):
    torch, dev = _torch_dev()
    n, m = shape
    x = D.upload_image(D.mixed_raw(n, m, 7))
    kinds = D.column_kinds(x)
    assert kinds["last row only"] >= 1 and kinds["beyond row 256 only"] >= 1 and kinds["non-negative"] >= (1 if m > 3 else 0)
    t32 = torch.as_tensor(x, device=dev).float()
    with Engine([n], [m], [1]) as base, Engine([n], [m], [1]) as e:
        base.set_view(0, x)
        assert np.array_equal(base.get_view(0), x)
        for seed in SEEDS:
            for src in (x, t32):
                e.shuffle_view_from(0, base, 0, seed=seed, normalise=False)
                rm, cm, nr, nc = e.empty_lines(0, counts=True)
                got, neg, er, ec = engine.fp64_shuffle(src, seed, normalise=False)
                assert np.array_equal(host(got), e.get_view(0)) and neg is False
                assert np.array_equal(er, rm) and np.array_equal(ec, cm) and (int(er.sum()), int(ec.sum())) == (nr, nc)
                e.shuffle_view_from(0, base, 0, seed=seed, normalise=True)
                rm, cm, nr, nc = e.empty_lines(0, counts=True)
                got, neg, er, ec = engine.fp64_shuffle(src, seed, normalise=True)
                assert np.array_equal(host(got.float().double()), e.get_view(0)), (seed, "normalised, rounded to fp32")
                assert neg is True
                assert np.array_equal(er, rm) and np.array_equal(ec, cm) and (int(er.sum()), int(ec.sum())) == (nr, nc)
    got, neg, _, _ = engine.fp64_shuffle(np.abs(x), 1, normalise=True)
    assert neg is False


# ---------------------------------------------------------------------------------------------------------------------
# 3. the normalised values against exact arithmetic
# ---------------------------------------------------------------------------------------------------------------------
def _worst(got, ref):
    worst, nz, nan = D.nan_stat(got, ref)
    return worst, nz, nan


@gpu
@pytest.mark.parametrize("shape", [(300, 70), (257, 3), (33, 31), (7, 5)], ids=shape_id)
def test_normalised_values_against_exactly_rounded_sums(shape):
    torch, dev = _torch_dev()
    n, m = shape
    want_draw = D.mixed_raw(n, m, 21, constant_negative=0)
    assert (want_draw.astype(np.float32).astype(np.float64) != want_draw).any()
    for seed in SEEDS:
        x = preimage(want_draw, seed)              # the source whose draw has the constant negative column: NaN there
        draw = S.shuffle_dense(x, seed)
        assert np.array_equal(draw, want_draw)
        ref = D.preprocess64(draw)
        assert np.isnan(ref[:, 0]).all() and (m == 1 or not np.isnan(ref[:, 1:]).any())
        for src in (x, torch.as_tensor(x, device=dev)):
            got, neg, _, _ = engine.fp64_shuffle(src, seed, normalise=True)
            got = host(got)
            worst, nz, nan = _worst(got, ref)
            measured(f"normalised fp64 shuffle {n}x{m} seed {seed}, in units of 2^-53", worst / 2.0 ** -53)
            assert neg is True and nan == 0 and nz == 0
            assert worst <= bar(n), f"{worst / 2.0 ** -53:.2f} u (bar {bar(n) / 2.0 ** -53:.0f} u)"
            assert np.array_equal(np.isnan(got), np.isnan(ref))
            # the mutants of the reference lie outside the bar on these data
            for mutant in (dict(shift=False), dict(sum_before_shift=True)) + ((dict(sum_rows=256),) if n > 256 else ()):
                bad = D.preprocess64(draw, **mutant)
                w, z, q = D.nan_stat(got, bad)
                assert w > bar(n) or z > 0 or q > 0, mutant


def preimage(draw, seed):
    """The source x with ``shuffle_dense(x, seed) == draw``: x.flat[pi(i)] = the draw's i-th entry in column-major order."""
    n, m = draw.shape
    pi = S.feistel_perm(np.arange(n * m), n * m, seed).astype(np.int64)
    x = np.empty(n * m)
    x[pi] = draw.ravel(order="F")
    return x.reshape(n, m)


def test_mutants_lie_outside_the_bar_on_the_reference_itself():
    """Without a GPU: the reference against its own mutants, on the draws of the test above; and ``preimage``."""
    for n, m in [(300, 70), (257, 3), (33, 31), (7, 5)]:
        draw = D.mixed_raw(n, m, 21, constant_negative=0)
        assert np.array_equal(S.shuffle_dense(preimage(draw, 1), 1), draw)
        ref = D.preprocess64(draw)
        for mutant in (dict(shift=False), dict(sum_before_shift=True)) + ((dict(sum_rows=256),) if n > 256 else ()):
            w, z, q = D.nan_stat(ref, D.preprocess64(draw, **mutant))
            assert w > bar(n) or z > 0 or q > 0, (n, m, mutant)


# ---------------------------------------------------------------------------------------------------------------------
# 4. empty lines
# ---------------------------------------------------------------------------------------------------------------------
def planted_zeros(n=33, m=31, zero_frac=0.9, seed=11):
    """Integer-valued, non-negative, mostly zero: every partial sum is exact in any order."""
    rng = np.random.default_rng(seed)
    x = rng.integers(1, 64, size=(n, m)).astype(np.float64)
    x[rng.random((n, m)) < zero_frac] = 0.0
    return x


# seed -> (empty rows, empty columns) of shuffle_ref's draw of planted_zeros(); chosen on the CPU
EMPTY_CASES = {3: (3, 0), 6: (0, 2), 5: (0, 0), 0: (1, 2)}


def test_the_empty_line_cases_are_what_the_reference_draws():
    x = planted_zeros()
    for seed, (nr, nc) in EMPTY_CASES.items():
        d = S.shuffle_dense(x, seed)
        assert (int((d.sum(axis=1) == 0).sum()), int((d.sum(axis=0) == 0).sum())) == (nr, nc)


@gpu
@pytest.mark.parametrize("seed", sorted(EMPTY_CASES))
def test_empty_lines_are_those_of_the_reference_draw(seed):
    torch, dev = _torch_dev()
    x = planted_zeros()
    d = S.shuffle_dense(x, seed)
    want_r, want_c = d.sum(axis=1) == 0, d.sum(axis=0) == 0
    for src in (x, torch.as_tensor(x, device=dev).float()):
        for normalise in (False, True):
            got, _, er, ec = engine.fp64_shuffle(src, seed, normalise=normalise)
            assert np.array_equal(er, want_r) and np.array_equal(ec, want_c)
            if not normalise:
                assert np.array_equal(host(got), d)
    # the counts as the device took them, through the C entry
    out = torch.empty((31, 33), dtype=torch.float64, device=dev)
    code, _, res = _call(n=33, m=31, x=np.asfortranarray(x), out=out, seed=seed, normalise=0)
    assert code == 0 and (res["n_empty_rows"], res["n_empty_cols"]) == EMPTY_CASES[seed]
    assert np.array_equal(res["row_mask"], want_r.astype(np.uint8)) and np.array_equal(res["col_mask"], want_c.astype(np.uint8))


# ---------------------------------------------------------------------------------------------------------------------
# 5. what fp32 cannot see
# ---------------------------------------------------------------------------------------------------------------------
@gpu
def test_a_matrix_fp32_takes_for_constant():
    n, m = 150, 90
    p = np.random.default_rng(4).integers(0, 64, size=(n, m)).astype(np.float64)
    x = 1.0 + 2.0 ** -30 * p
    assert len(np.unique(x)) == 64 and (x.astype(np.float32) == 1.0).all()
    got = host(engine.fp64_shuffle(x, 9, normalise=False)[0])
    assert np.array_equal(got, S.shuffle_dense(x, 9)) and len(np.unique(got)) == 64
    with Engine([n], [m], [1]) as base, Engine([n], [m], [1]) as e:
        base.set_view(0, x)
        e.shuffle_view_from(0, base, 0, seed=9, normalise=False)
        assert (e.get_view(0) == 1.0).all()


# ---------------------------------------------------------------------------------------------------------------------
# 6. the guards of the C entry: each refusal returns its code and leaves every output untouched
# ---------------------------------------------------------------------------------------------------------------------
SENTINEL = -7.25


def _call(n=12, m=9, x="host", x_dev=None, out="own", seed=1, normalise=1, struct_size=None, device_id=0, null=(), stream=None):
    """resnmtf_fp64_shuffle through ctypes.  ``x``: "host" (a random n x m array), "none", or an array; ``out``: "own" (a
    SENTINEL-filled device array of n m doubles), None, a tensor or a raw address.  Returns (code, text, outputs) with
    every host output pre-filled with sentinels and ``out`` (when "own") read back."""
    import torch
    lib = _lib.load()
    shape = (max(n, 1), max(m, 1))
    xh = np.asfortranarray(np.random.default_rng(0).random(shape)) if isinstance(x, str) else x
    own = None
    if isinstance(out, str):
        own = out = torch.full((shape[1], shape[0]), SENTINEL, dtype=torch.float64, device=torch.device("cuda", 0))
    neg, nr, nc = C.c_int(-5), C.c_int(-5), C.c_int(-5)
    rm, cm = np.full(shape[0], 77, dtype=np.uint8), np.full(shape[1], 77, dtype=np.uint8)
    job = _lib.Fp64ShuffleJob()
    job.struct_size = C.sizeof(job) if struct_size is None else struct_size
    job.n, job.m, job.normalise, job.seed = n, m, normalise, seed
    if not (isinstance(x, str) and x == "none"):
        job.x = xh.ctypes.data_as(C.POINTER(C.c_double))
    if x_dev is not None:
        job.x_dev = x_dev
    job.stream = stream
    job.out = None if out is None else (out if isinstance(out, int) else out.data_ptr())
    job.was_negative, job.n_empty_rows, job.n_empty_cols = C.pointer(neg), C.pointer(nr), C.pointer(nc)
    job.row_mask, job.col_mask = rm.ctypes.data_as(C.POINTER(C.c_ubyte)), cm.ctypes.data_as(C.POINTER(C.c_ubyte))
    for name in null:
        setattr(job, name, None)
    code = lib.resnmtf_fp64_shuffle(device_id, C.byref(job))
    text = (lib.resnmtf_last_error(None) or b"").decode()
    torch.cuda.synchronize()
    return code, text, {"out": None if own is None else own.cpu().numpy(), "was_negative": neg.value, "n_empty_rows": nr.value,
                        "n_empty_cols": nc.value, "row_mask": rm, "col_mask": cm}


def _refused(code, want_code, text, match, res):
    assert code == want_code and match in text, (code, text)
    assert res["out"] is None or (res["out"] == SENTINEL).all()
    assert (res["was_negative"], res["n_empty_rows"], res["n_empty_cols"]) == (-5, -5, -5)
    assert (res["row_mask"] == 77).all() and (res["col_mask"] == 77).all()


@gpu
def test_guards_of_the_c_entry():
    import torch
    dev = torch.device("cuda", 0)
    t = torch.rand((12, 9), dtype=torch.float64, device=dev)
    dm = lambda ptr, dtype=0, rs=9, cs=1: _lib.DeviceMatrix(ptr, dtype, rs, cs)      # noqa: E731
    for kw, match in ((dict(struct_size=8), "struct_size mismatch"), (dict(n=0), "view dimensions must be positive"),
                      (dict(m=-1), "view dimensions must be positive"),
                      (dict(x_dev=dm(t.data_ptr())), "X is given in two places"), (dict(x="none"), "X is given in no place"),
                      (dict(out=None), "out is NULL"), (dict(null=("n_empty_rows",)), "are NULL"),
                      (dict(x="none", x_dev=dm(t.data_ptr(), dtype=4)), "unknown dtype"),
                      (dict(x="none", x_dev=dm(t.data_ptr(), dtype=-1)), "unknown dtype"),
                      (dict(x="none", x_dev=dm(t.data_ptr(), rs=-9)), "strides must be >= 0"),
                      (dict(x="none", x_dev=dm(t.data_ptr(), cs=-1)), "strides must be >= 0"),
                      (dict(x="none", x_dev=dm(t.data_ptr(), rs=1 << 40)), "x_dev reaches beyond its allocation"),
                      (dict(device_id=99), "device_id out of range")):
        code, text, res = _call(**kw)
        _refused(code, 1, text, match, res)
    hostbuf = np.zeros((12, 9))
    code, text, res = _call(x="none", x_dev=dm(hostbuf.ctypes.data))
    _refused(code, 1, text, "x_dev is not device memory of device 0", res)
    code, text, res = _call(out=hostbuf.ctypes.data)
    _refused(code, 1, text, "out is not device memory of device 0", res)
    assert (hostbuf == 0).all()
    # out too short: the length is checked against the allocation the pointer lies in (for a tensor of torch's, the
    # caching allocator's block -- 2 MB for a small tensor), so the job asks for 2000 x 2000 doubles = 32 MB of an
    # 8-byte tensor; x is one double on the host, or one element expanded on the device: refused before either is read
    short = torch.full((1,), SENTINEL, dtype=torch.float64, device=dev)
    for route in (dict(x=np.zeros((1, 1))), dict(x="none", x_dev=dm(t.data_ptr(), rs=0, cs=0))):
        code, text, res = _call(n=2000, m=2000, out=short, **route)
        _refused(code, 1, text, "out reaches beyond its allocation", res)
        assert short.item() == SENTINEL
    # out overlapping a device source: the source itself, and its second half
    both = torch.rand((2 * 12 * 9,), dtype=torch.float64, device=dev)
    keep = both.clone()
    for off in (0, 12 * 9 - 1):
        code, text, res = _call(x="none", x_dev=dm(both.data_ptr()), out=both.data_ptr() + 8 * off)
        _refused(code, 1, text, "out overlaps x_dev", res)
    assert torch.equal(both, keep)
    assert _lib.load().resnmtf_fp64_shuffle(0, None) == 1
    # the job itself is fine: the same call without a fault runs on both routes
    code, _, res = _call()
    assert code == 0 and (res["out"] != SENTINEL).all() and res["was_negative"] == 0 and res["n_empty_rows"] == 0
    code, _, res = _call(x="none", x_dev=dm(t.data_ptr()), stream=torch.cuda.current_stream(dev).cuda_stream)
    assert code == 0 and (res["out"] != SENTINEL).all() and (res["row_mask"] == 0).all()


@gpu
def test_a_host_source_the_device_cannot_stage_is_refused_with_its_byte_count():
    """200000 x 200000 from a host pointer: the staging copy alone is 320 GB, more than the device has.  Refused on the
    byte count before x or out is read: x is one double, out one element of device memory.  Nothing is allocated."""
    import torch
    n = 200000
    out = torch.full((1,), SENTINEL, dtype=torch.float64, device=torch.device("cuda", 0))
    code, text, res = _call(n=n, m=n, x=np.zeros((1, 1)), out=out)
    assert code == 4 and "fp64_shuffle: 320000000000 bytes asked for (the fp64 staging copy of a host X)" in text, (code, text)
    assert out.item() == SENTINEL and (res["was_negative"], res["n_empty_rows"], res["n_empty_cols"]) == (-5, -5, -5)
