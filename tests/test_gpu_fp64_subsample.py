"""The sub-sample of a stability repeat in double precision (resnmtf_fp64_subsample):
engine.fp64_subsample against ``X[np.ix_(rows, cols)]`` bit for bit, from a host array and from tensors of every dtype
and layout, through both gather forms; the empty lines against a left-to-right fp64 restatement (``np.cumsum`` adds in
index order), cancellation lines included; bit for bit the f32 route where both see the same numbers; what fp32 cannot
see; and the guards of the C entry, each leaving every output untouched."""
import ctypes as C

import numpy as np
import pytest

from resnmtf_amd import _lib, engine
from resnmtf_amd.engine import Engine

gpu = pytest.mark.gpu

# (sub-sample, source)
SHAPES = [((1, 1), (1, 1)), ((6, 4), (7, 5)), ((33, 31), (33, 31)), ((29, 27), (33, 31)), ((230, 3), (257, 3)),
          ((3, 230), (3, 257)), ((270, 63), (300, 70))]
DTYPES = ["float64", "float32", "float16", "bfloat16"]


def shape_id(s):
    return f"{s[0][0]}x{s[0][1]}from{s[1][0]}x{s[1][1]}" if isinstance(s[0], tuple) else f"{s[0]}x{s[1]}"


def host(t):
    return t.cpu().numpy()


def _torch_dev():
    import torch
    return torch, torch.device("cuda", 0)


def fp64_data(n, m, seed):
    return np.random.default_rng(seed).random((n, m)) + 0.25


def draw(sub, src, seed):
    """rows / cols of a sub-sample, in the random order the reference's sample() leaves"""
    rng = np.random.default_rng(seed)
    return rng.choice(src[0], sub[0], replace=False), rng.choice(src[1], sub[1], replace=False)


def layouts(torch, dev, x, dtype):
    """the same values as tensors that are row-major, column-major, a strided slice and (the first column) expanded"""
    n, m = x.shape
    dt = getattr(torch, dtype)
    t = torch.as_tensor(x, device=dev).to(dt)
    big = torch.zeros((2 * n, 3 * m + 1), dtype=dt, device=dev)
    big[::2, 1::3] = t
    return {"row-major": t.contiguous(), "column-major": t.t().contiguous().t(), "slice": big[::2, 1::3],
            "expanded": t[:, :1].expand(n, m)}


def empty_lines_ref(sub):
    """one running fp64 sum per line, left to right"""
    return np.cumsum(sub, axis=1)[:, -1] == 0.0, np.cumsum(sub, axis=0)[-1, :] == 0.0


def check(src, want, rows, cols):
    torch, _ = _torch_dev()
    got, er, ec = engine.fp64_subsample(src, rows, cols)
    ns, ms = want.shape
    assert got.dtype == torch.float64 and tuple(got.shape) == (ns, ms) and (ns == 1 or ms == 1 or got.stride() == (1, ns))
    assert host(got).tobytes() == np.ascontiguousarray(want).tobytes()
    wr, wc = empty_lines_ref(want)
    assert er.dtype == bool and ec.dtype == bool and np.array_equal(er, wr) and np.array_equal(ec, wc)
    return got


# ---------------------------------------------------------------------------------------------------------------------
# 1. the gather, bit for bit X[np.ix_(rows, cols)] widened
# ---------------------------------------------------------------------------------------------------------------------
def test_the_form_chooser_sends_the_layouts_to_both_forms():
    plan = engine.fp64_subsample_plan
    assert plan(1, 300)["gather"] == "rows" and plan(70, 1)["gather"] == "lds"          # column-major / a host X, row-major
    assert plan(2, 600)["gather"] == "rows" and plan(2 * 211, 3)["gather"] == "lds"     # strided slices of either
    assert plan(1, 0)["gather"] == "lds" and plan(0, 0)["gather"] == "rows" and plan(1, 1)["gather"] == "rows"
    p = plan(1, 1)
    assert (p["gather_rows"], p["gather_tile"], p["row_sum_rows"], p["col_sum_rows"], p["col_sum_cols"]) == (256, 32, 64, 64, 32)
    with pytest.raises(engine.ResnmtfError):
        plan(-1, 1)


@gpu
@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_gather_from_a_host_array_and_from_tensors_of_every_dtype_and_layout(shape):
    torch, dev = _torch_dev()
    sub, src = shape
    x = fp64_data(*src, seed=10 * src[0] + src[1])
    rows, cols = draw(sub, src, 3)
    assert src == (1, 1) or (x.astype(np.float32).astype(np.float64) != x).any()
    check(x, x[np.ix_(rows, cols)], rows, cols)
    check(np.asfortranarray(x), x[np.ix_(rows, cols)], rows, cols)
    forms = set()
    for dtype in DTYPES:
        for name, t in layouts(torch, dev, x, dtype).items():
            forms.add(engine.fp64_subsample_plan(t.stride(0), t.stride(1))["gather"])
            check(t, host(t.double())[np.ix_(rows, cols)], rows, cols)
    assert forms == ({"rows", "lds"} if min(src) > 1 else forms)          # both gather forms were reached


def _edge_shapes():
    p = {"gather_rows": 256, "gather_tile": 32, "row_sum_rows": 64, "col_sum_rows": 64, "col_sum_cols": 32}    # asserted above
    edges = sorted(set(p.values()))
    out = []
    for e in edges:
        for d in (-1, 0, 1):
            out.append((e + d, 5))      # the row extent at the edge
            out.append((5, e + d))      # the column extent at the edge
    return out


@gpu
@pytest.mark.parametrize("sub", _edge_shapes(), ids=shape_id)
def test_gather_and_sums_one_below_at_and_one_above_every_tile_edge(sub):
    torch, dev = _torch_dev()
    src = (sub[0] + 3, sub[1] + 2)
    x = np.random.default_rng(sub[0] * 1000 + sub[1]).integers(0, 3, size=src).astype(np.float64)
    rows, cols = draw(sub, src, 5)
    x[rows[-1], :] = 0.0                   # the last destination row and column are empty: the far edge of the last tile
    x[:, cols[-1]] = 0.0
    want = x[np.ix_(rows, cols)]
    t = torch.as_tensor(x, device=dev)
    for s in (x, t, t.t().contiguous().t()):
        got, er, ec = engine.fp64_subsample(s, rows, cols)
        assert host(got).tobytes() == want.tobytes()
        wr, wc = empty_lines_ref(want)
        assert er[-1] and ec[-1] and np.array_equal(er, wr) and np.array_equal(ec, wc)


@gpu
def test_result_is_independent_of_the_destination_and_reproducible():
    torch, dev = _torch_dev()
    sub, src = (29, 27), (33, 31)
    x = fp64_data(*src, seed=8)
    rows, cols = draw(sub, src, 1)
    t = torch.as_tensor(x, device=dev)
    for s in (x, t, t.t().contiguous().t()):
        outs = []
        for fill in (float("nan"), -7.25, -7.25):
            out = torch.full((sub[1], sub[0]), fill, dtype=torch.float64, device=dev)
            got, er, ec = engine.fp64_subsample(s, rows, cols, out=out)
            assert got.data_ptr() == out.data_ptr() and not er.any() and not ec.any()
            outs.append(host(got).tobytes())
        assert outs[0] == outs[1] == outs[2] == x[np.ix_(rows, cols)].tobytes()


# ---------------------------------------------------------------------------------------------------------------------
# 2. the empty lines: one running sum per line, in index order
# ---------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("planted", ["none", "rows", "cols", "both"])
def test_planted_zero_rows_and_columns(planted):
    torch, dev = _torch_dev()
    sub, src = (270, 63), (300, 70)
    x = np.random.default_rng(2).integers(1, 5, size=src).astype(np.float64)
    rows, cols = draw(sub, src, 9)
    zr, zc = [rows[0], rows[64], rows[269]], [cols[0], cols[31], cols[32], cols[62]]
    if planted in ("rows", "both"):
        x[zr, :] = 0.0
    if planted in ("cols", "both"):
        x[:, zc] = 0.0
    want = x[np.ix_(rows, cols)]
    t = torch.as_tensor(x, device=dev)
    for s in (x, t, t.float(), t.t().contiguous().t()):
        got, er, ec = engine.fp64_subsample(s, rows, cols)
        assert host(got).tobytes() == want.tobytes()
        assert sorted(np.flatnonzero(er)) == ([0, 64, 269] if planted in ("rows", "both") else [])
        assert sorted(np.flatnonzero(ec)) == ([0, 31, 32, 62] if planted in ("cols", "both") else [])


@gpu
def test_cancellation_lines_across_tile_boundaries_need_the_sum_in_index_order():
    """[1e16, 1, -1e16] sums to 0 left to right (1e16 + 1 rounds to 1e16) and [1e16, -1e16, 1] to 1; a tree or any
    reordered sum gives another answer for one of the two.  The three entries straddle the column sums' 64-row tile
    (rows 63, 64, 65), the row sums' eight-column trip (columns 7, 8, 9) and the 32-column tile (columns 31, 32, 33)."""
    torch, dev = _torch_dev()
    n, m = 140, 70
    x = np.zeros((n, m))
    zero_order, one_order = [1e16, 1.0, -1e16], [1e16, -1e16, 1.0]
    x[[63, 64, 65], 2] = zero_order          # columns 2 / 3: down the rows, across the 64-row tile
    x[[63, 64, 65], 3] = one_order
    x[100, [7, 8, 9]] = zero_order           # rows 100 .. 103: along the columns
    x[101, [7, 8, 9]] = one_order
    x[102, [31, 32, 33]] = zero_order
    x[103, [31, 32, 33]] = one_order
    x[0, 40] = 1e16; x[64, 40] = 1.0; x[139, 40] = -1e16        # far apart: first tile, second tile, last row
    x[0, 41] = 1e16; x[64, 41] = -1e16; x[139, 41] = 1.0
    rows, cols = np.arange(n), np.arange(m)
    wr, wc = empty_lines_ref(x)
    assert wc[2] and not wc[3] and wr[100] and not wr[101] and wr[102] and not wr[103] and wc[40] and not wc[41]
    t = torch.as_tensor(x, device=dev)
    for s in (x, t, t.t().contiguous().t()):
        got, er, ec = engine.fp64_subsample(s, rows, cols)
        assert host(got).tobytes() == x.tobytes()
        assert np.array_equal(er, wr) and np.array_equal(ec, wc)
    # the same entries reached through a permutation of the source: the order that counts is the destination's
    pr, pc = np.random.default_rng(0).permutation(n), np.random.default_rng(1).permutation(m)
    y = np.zeros((n, m))
    y[np.ix_(pr, pc)] = x                    # y[pr[i], pc[j]] = x[i, j]
    got, er, ec = engine.fp64_subsample(y, pr, pc)
    assert host(got).tobytes() == x.tobytes() and np.array_equal(er, wr) and np.array_equal(ec, wc)


# ---------------------------------------------------------------------------------------------------------------------
# 3. bit for bit the f32 route on fp32-valued data; what fp32 cannot see
# ---------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("shape", [((270, 63), (300, 70)), ((230, 3), (257, 3))], ids=shape_id)
def test_equals_the_f32_route_on_data_fp32_holds(shape):
    torch, dev = _torch_dev()
    sub, src = shape
    rng = np.random.default_rng(7)
    x = (rng.standard_normal(src) * (rng.random(src) < 0.5)).astype(np.float32).astype(np.float64)      # mixed signs, many zeros
    rows, cols = draw(sub, src, 4)
    x[:, cols[0]] = 0.0
    x[:, cols[1]] = 0.0
    x[rows[10:13], cols[0]] = [2.0 ** 60, 1.0, -2.0 ** 60]      # fp32 holds all three; in this order the fp64 sum is 0
    x[rows[5], :] = 0.0
    with Engine([src[0]], [src[1]], [1]) as base, Engine([sub[0]], [sub[1]], [1]) as e:
        base.set_view(0, x)
        assert np.array_equal(base.get_view(0), x)
        e.subsample_view_from(0, base, 0, rows, cols)
        rm, cm, nr, nc = e.empty_lines(0, counts=True)
        want = e.get_view(0)
    assert nr >= 1 and nc >= 2 and cm[0] and cm[1]
    for s in (x, torch.as_tensor(x, device=dev).float(), torch.as_tensor(x, device=dev)):
        got, er, ec = engine.fp64_subsample(s, rows, cols)
        assert host(got).tobytes() == want.tobytes()
        assert np.array_equal(er, rm) and np.array_equal(ec, cm) and (int(er.sum()), int(ec.sum())) == (nr, nc)


@gpu
def test_a_matrix_fp32_takes_for_constant():
    n, m = 150, 90
    p = np.random.default_rng(4).integers(0, 64, size=(n, m)).astype(np.float64)
    x = 1.0 + 2.0 ** -30 * p
    assert len(np.unique(x)) == 64 and (x.astype(np.float32) == 1.0).all()
    rows, cols = draw((135, 81), (n, m), 2)
    got, er, ec = engine.fp64_subsample(x, rows, cols)
    assert np.array_equal((host(got) - 1.0) * 2.0 ** 30, p[np.ix_(rows, cols)]) and not er.any() and not ec.any()
    with Engine([n], [m], [1]) as base, Engine([135], [81], [1]) as e:
        base.set_view(0, x)
        e.subsample_view_from(0, base, 0, rows, cols)
        assert (e.get_view(0) == 1.0).all()


# ---------------------------------------------------------------------------------------------------------------------
# 4. the guards of the C entry: each refusal returns its code and leaves every output untouched
# ---------------------------------------------------------------------------------------------------------------------
SENTINEL = -7.25


def _call(n=12, m=9, n_sub=5, m_sub=4, rows="own", cols="own", x="host", x_dev=None, out="own", struct_size=None, device_id=0,
          null=(), stream=None):
    """resnmtf_fp64_subsample through ctypes.  ``x``: "host" (a random n x m array), "none", or an array; ``out``: "own" (a
    SENTINEL-filled device array), None, a tensor or a raw address; ``rows`` / ``cols``: "own" (0, 1, ...) or a list.
    Returns (code, text, outputs) with every host output pre-filled with sentinels and ``out`` (when "own") read back."""
    import torch
    lib = _lib.load()
    shape = (max(n, 1), max(m, 1))
    sub = (max(n_sub, 1), max(m_sub, 1))
    xh = np.asfortranarray(np.random.default_rng(0).random(shape)) if isinstance(x, str) else x
    own = None
    if isinstance(out, str):
        own = out = torch.full((sub[1], sub[0]), SENTINEL, dtype=torch.float64, device=torch.device("cuda", 0))
    ri = np.arange(sub[0], dtype=np.int32) if isinstance(rows, str) else np.asarray(rows, dtype=np.int32)
    ci = np.arange(sub[1], dtype=np.int32) if isinstance(cols, str) else np.asarray(cols, dtype=np.int32)
    nr, nc = C.c_int(-5), C.c_int(-5)
    rm, cm = np.full(sub[0], 77, dtype=np.uint8), np.full(sub[1], 77, dtype=np.uint8)
    job = _lib.Fp64SubsampleJob()
    job.struct_size = C.sizeof(job) if struct_size is None else struct_size
    job.n, job.m, job.n_sub, job.m_sub = n, m, n_sub, m_sub
    job.rows, job.cols = ri.ctypes.data_as(C.POINTER(C.c_int)), ci.ctypes.data_as(C.POINTER(C.c_int))
    if not (isinstance(x, str) and x == "none"):
        job.x = xh.ctypes.data_as(C.POINTER(C.c_double))
    if x_dev is not None:
        job.x_dev = x_dev
    job.stream = stream
    job.out = None if out is None else (out if isinstance(out, int) else out.data_ptr())
    job.n_empty_rows, job.n_empty_cols = C.pointer(nr), C.pointer(nc)
    job.row_mask, job.col_mask = rm.ctypes.data_as(C.POINTER(C.c_ubyte)), cm.ctypes.data_as(C.POINTER(C.c_ubyte))
    for name in null:
        setattr(job, name, None)
    code = lib.resnmtf_fp64_subsample(device_id, C.byref(job))
    text = (lib.resnmtf_last_error(None) or b"").decode()
    torch.cuda.synchronize()
    return code, text, {"out": None if own is None else own.cpu().numpy(), "n_empty_rows": nr.value, "n_empty_cols": nc.value,
                        "row_mask": rm, "col_mask": cm}


def _refused(code, want_code, text, match, res):
    assert code == want_code and match in text, (code, text)
    assert res["out"] is None or (res["out"] == SENTINEL).all()
    assert (res["n_empty_rows"], res["n_empty_cols"]) == (-5, -5)
    assert (res["row_mask"] == 77).all() and (res["col_mask"] == 77).all()


@gpu
def test_guards_of_the_c_entry():
    import torch
    dev = torch.device("cuda", 0)
    t = torch.rand((12, 9), dtype=torch.float64, device=dev)
    dm = lambda ptr, dtype=0, rs=9, cs=1: _lib.DeviceMatrix(ptr, dtype, rs, cs)      # noqa: E731
    for kw, match in ((dict(struct_size=8), "struct_size mismatch"), (dict(n=0), "view dimensions must be positive"),
                      (dict(m=-1), "view dimensions must be positive"),
                      (dict(n_sub=0), "n_sub must be in [1, n]"), (dict(n_sub=13), "n_sub must be in [1, n]"),
                      (dict(m_sub=0), "m_sub must be in [1, m]"), (dict(m_sub=10), "m_sub must be in [1, m]"),
                      (dict(null=("rows",)), "rows / cols are NULL"), (dict(null=("cols",)), "rows / cols are NULL"),
                      (dict(rows=[0, 1, 12, 3, 4]), "rows[2] = 12 is out of range [0, 12)"),
                      (dict(rows=[0, -1, 2, 3, 4]), "rows[1] = -1 is out of range [0, 12)"),
                      (dict(cols=[0, 1, 2, 9]), "cols[3] = 9 is out of range [0, 9)"),
                      (dict(rows=[3, 1, 2, 3, 4]), "rows[3] = 3 occurs twice"),
                      (dict(cols=[8, 8, 2, 0]), "cols[1] = 8 occurs twice"),
                      (dict(x_dev=dm(t.data_ptr())), "X is given in two places"), (dict(x="none"), "X is given in no place"),
                      (dict(out=None), "out is NULL"), (dict(null=("n_empty_rows",)), "are NULL"),
                      (dict(null=("n_empty_cols",)), "are NULL"),
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
    # out too short (the length is checked against the allocation the pointer lies in: 32 MB asked of an 8-byte tensor)
    short = torch.full((1,), SENTINEL, dtype=torch.float64, device=dev)
    for route in (dict(x=np.zeros((1, 1))), dict(x="none", x_dev=dm(t.data_ptr(), rs=0, cs=0))):
        code, text, res = _call(n=2000, m=2000, n_sub=2000, m_sub=2000, out=short, **route)
        _refused(code, 1, text, "out reaches beyond its allocation", res)
        assert short.item() == SENTINEL
    # out overlapping a device source: the source itself, and its last element
    both = torch.rand((2 * 12 * 9,), dtype=torch.float64, device=dev)
    keep = both.clone()
    for off in (0, 12 * 9 - 1):
        code, text, res = _call(x="none", x_dev=dm(both.data_ptr()), out=both.data_ptr() + 8 * off)
        _refused(code, 1, text, "out overlaps x_dev", res)
    assert torch.equal(both, keep)
    assert _lib.load().resnmtf_fp64_subsample(0, None) == 1
    # the job itself is fine: the same call without a fault runs on both routes
    code, _, res = _call()
    assert code == 0 and (res["out"] != SENTINEL).all() and res["n_empty_rows"] == 0 and (res["col_mask"] == 0).all()
    code, _, res = _call(x="none", x_dev=dm(t.data_ptr()), stream=torch.cuda.current_stream(dev).cuda_stream)
    assert code == 0 and np.array_equal(res["out"].T, host(t)[:5, :4]) and (res["row_mask"] == 0).all()
    # the masks may be NULL
    code, _, res = _call(null=("row_mask", "col_mask"))
    assert code == 0 and (res["row_mask"] == 77).all() and res["n_empty_cols"] == 0


@gpu
def test_a_host_source_the_device_cannot_stage_is_refused_with_its_byte_count():
    """A 200000 x 200000 source from a host pointer: the staging copy alone is 320 GB, more than the device has.  Refused
    on the byte count before x or out is read: x is one double, out one element of device memory."""
    import torch
    n = 200000
    out = torch.full((1,), SENTINEL, dtype=torch.float64, device=torch.device("cuda", 0))
    code, text, res = _call(n=n, m=n, n_sub=1, m_sub=1, x=np.zeros((1, 1)), out=out)
    assert code == 4 and "fp64_subsample: 320000000000 bytes asked for (the fp64 staging copy of a host X)" in text, (code, text)
    assert out.item() == SENTINEL and (res["n_empty_rows"], res["n_empty_cols"]) == (-5, -5)
