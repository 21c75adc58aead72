"""Thin object wrapper over the C-ABI (include/resnmtf_hip.h): one ``Engine`` = one
``resnmtf_handle`` = the device-resident state of the multiplicative-update loop on ONE GPU.

Everything numeric happens in the HIP library; this module only marshals NumPy arrays
(fp64, column-major, as R would hand them over) and raises on any error code.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import numpy as np

from . import _lib
from . import device_views as _device_views
from . import sparse as _sparse
from ._lib import ResnmtfError


def _f64_colmajor(a, shape=None) -> np.ndarray:
    arr = np.asfortranarray(np.asarray(a, dtype=np.float64))
    if shape is not None and tuple(arr.shape) != tuple(shape):
        raise ValueError(f"expected shape {tuple(shape)}, got {tuple(arr.shape)}")
    return arr


def _dp(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))


def _ip(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_int))


def device_count() -> int:
    return int(_lib.load().resnmtf_device_count())


def jsd_pairs(cols, pairs, device_id: int = 0) -> np.ndarray:
    """``jsd_calc`` (``R/utils.r:95-106``) of every column pair on the device (``resnmtf_jsd_pairs``, no handle):
    ``cols`` n x C (fp64, taken column-major), ``pairs`` P x 2 0-based column indices; returns P scores."""
    lib = _lib.load()
    cols = _f64_colmajor(cols)
    if cols.ndim != 2:
        raise ValueError("cols must be an n x C matrix")
    pairs = np.ascontiguousarray(np.asarray(pairs, dtype=np.int32).reshape(-1, 2))
    out = np.zeros(len(pairs), dtype=np.float64)
    rc = lib.resnmtf_jsd_pairs(int(device_id), int(cols.shape[0]), int(cols.shape[1]), _dp(cols), int(len(pairs)),
                               _ip(pairs), _dp(out))
    if rc != _lib.OK:
        raise ResnmtfError(rc, (lib.resnmtf_last_error(None) or b"").decode())
    return out


def jsd_stages(cols, pairs, sorted: bool = True, stats: bool = True, dens: bool = True, device_id: int = 0) -> dict:
    """``jsd_pairs`` with its stages handed back (``resnmtf_jsd_stages``; for tests of each stage): ``{"out": P scores,
    "sorted": n x C (every column ascending, as the later kernels read it), "stats": C x 2 (``bw.nrd0``, maximum),
    "dens": P x 2 x 512 (both sides' zeroed, un-normalised densities)}``; a stage not asked for is ``None``."""
    lib = _lib.load()
    cols = _f64_colmajor(cols)
    if cols.ndim != 2:
        raise ValueError("cols must be an n x C matrix")
    pairs = np.ascontiguousarray(np.asarray(pairs, dtype=np.int32).reshape(-1, 2))
    n, n_cols, n_pairs = int(cols.shape[0]), int(cols.shape[1]), int(len(pairs))
    out = np.zeros(n_pairs, dtype=np.float64)
    got = {"out": out,
           "sorted": np.zeros((n, n_cols), dtype=np.float64, order="F") if sorted else None,
           "stats": np.zeros((n_cols, 2), dtype=np.float64) if stats else None,
           "dens": np.zeros((n_pairs, 2, 512), dtype=np.float64) if dens else None}
    rc = lib.resnmtf_jsd_stages(int(device_id), n, n_cols, _dp(cols), n_pairs, _ip(pairs), _dp(out), _dp(got["sorted"]),
                                _dp(got["stats"]), _dp(got["dens"]))
    if rc != _lib.OK:
        raise ResnmtfError(rc, (lib.resnmtf_last_error(None) or b"").decode())
    return got


_DTYPE_CODES = {"torch.float64": _lib.DTYPE_F64, "torch.float32": _lib.DTYPE_F32, "torch.float16": _lib.DTYPE_F16,
                "torch.bfloat16": _lib.DTYPE_BF16}


def _dtype_code(t, what: str) -> int:
    """The ``RESNMTF_DTYPE_*`` of the tensor ``t``; any other than the four floating types is a ``ValueError``."""
    if str(t.dtype) not in _DTYPE_CODES:
        raise ValueError(f"{what} must be fp64, fp32, fp16 or bf16, got {t.dtype}")
    return _DTYPE_CODES[str(t.dtype)]


def _device_matrix(t, shape, device_id: int, what: str) -> _lib.DeviceMatrix:
    """The ``resnmtf_device_matrix`` of a ``torch`` tensor as it lies (``data_ptr``, dtype, strides in elements), after the
    checks that need no device: fp64 / fp32 / fp16 / bf16, on ``cuda:device_id``, of ``shape`` (``ValueError``)."""
    dtype = _dtype_code(t, what)
    if not _device_views.on_engine_device(t, device_id):
        raise ValueError(f"{what} lives on {t.device}, the run on cuda:{int(device_id)}")
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"{what}: expected shape {tuple(shape)}, got {tuple(t.shape)}")
    strides = [int(x) for x in t.stride()] + [1]                      # (a vector: the column stride is not read)
    return _lib.DeviceMatrix(t.data_ptr(), dtype, strides[0], strides[1])


# Where the data of one view of a problem come from: exactly one of the four places the library knows (F64Source in
# csrc/resnmtf_fp64_job.h).  ``group_run`` knows the first alone.
_HOST_DENSE, _HOST_CSC, _DEVICE_DENSE, _DEVICE_SPARSE = "job->x", "sp", "dev->x", "spd"


def _view_route(x, what: str, device_id: int, dev, spd) -> tuple:
    """(route, the view as that route takes it): a ``scipy.sparse`` matrix as its canonical CSC; with ``spd`` a sparse
    tensor on the device as a checked ``device_views.SparseDeviceView``; with ``dev`` a device tensor as it is; anything
    else as an fp64 column-major array."""
    if _sparse.is_sparse(x):
        return _HOST_CSC, _sparse.canonical_csc(x)
    if spd is not None and _device_views.is_sparse_device_view(x):
        return _DEVICE_SPARSE, _device_views.as_sparse_view(x, device_id, what)
    if dev is not None and _device_views.is_device_tensor(x):
        return _DEVICE_DENSE, x
    return _HOST_DENSE, _f64_colmajor(x)


def _fill_fp64_device_factors(dev, v: int, n: int, m: int, p, k: int, q: int, device_id: int, keep: list) -> bool:
    """The initial factors of view ``v`` of ``fp64_run``'s problem ``p`` into the ``resnmtf_fp64_device`` ``dev`` when they
    are device tensors; False when they are not, and they stay ``_fill_group_job``'s.  ``init_f[v]`` / ``init_s[v]`` /
    ``init_g[v]`` are all three device tensors or none is (``ValueError``); beside device factors ``init_lam[v]`` /
    ``init_mu[v]`` are moved to the device when they are not there."""
    parts = [p["init_f"][v], p["init_s"][v], p["init_g"][v]]
    if not _device_views.factor_route(*parts, what=f"problem {q}, view {v}"):
        return False
    for t, name, shape in zip(parts, ("f0", "s0", "g0"), ((n, k), (k, k), (m, k))):
        t = t.detach()
        keep.append(t)
        getattr(dev, name)[v] = _device_matrix(t, shape, device_id, f"problem {q}, view {v}: init_{name[0]}")
    for name, key in (("lambda0", "init_lam"), ("mu0", "init_mu")):
        vals = p.get(key)
        if vals is None or vals[v] is None:
            continue
        t = vals[v]
        if not _device_views.is_tensor(t):
            import torch            # (lazily: the factors are tensors, so it is loaded)
            t = torch.as_tensor(np.ascontiguousarray(t, dtype=np.float64), device=torch.device("cuda", int(device_id)))
        elif t.device.type == "cpu":
            t = t.to(parts[0].device)
        t = t.detach()
        keep.append(t)
        getattr(dev, name)[v] = _device_matrix(t, (k,), device_id, f"problem {q}, view {v}: {key}")
    return True


_LAYOUT_CODES = {"torch.sparse_csc": _lib.SPARSE_CSC, "torch.sparse_csr": _lib.SPARSE_CSR, "torch.sparse_coo": _lib.SPARSE_COO}


def _fill_fp64_sparse_device(spd, v: int, x, q: int, keep: list):
    """The sparse view ``x`` (a checked ``device_views.SparseDeviceView``) into entry ``v`` of the
    ``resnmtf_fp64_sparse_device`` ``spd``: the addresses of its own index and value arrays
    (``device_views.sparse_tensor_parts``), ``.contiguous()`` only on a piece that is not."""
    _fill_sparse_device_view(spd.view[v], x, f"problem {q}, view {v}: data", keep)


def _fill_sparse_device_view(c, x, what: str, keep: list):
    """One ``resnmtf_fp64_sparse_device_view`` (``c``) from the checked ``SparseDeviceView`` ``x``."""
    t = x.tensor.detach()
    dtype = _dtype_code(t, what)
    a, b, vals = (piece if piece.is_contiguous() else piece.contiguous() for piece in _device_views.sparse_tensor_parts(t))
    keep.extend([t, a, b, vals])
    c.layout, c.dtype = _LAYOUT_CODES[str(t.layout)], dtype
    c.index_type = _lib.INDEX_I64 if str(a.dtype) == "torch.int64" else _lib.INDEX_I32
    c.ptr_or_rows, c.idx_or_cols, c.values, c.nnz = a.data_ptr(), b.data_ptr(), vals.data_ptr(), int(t._nnz())


def _fp64_device_outputs(dev, j, out: dict, device_id: int, return_state: bool):
    """``output="torch"``: the five results per view (and the raw state) as fp64 tensors on ``cuda:device_id``, F, S and G
    column-major (``torch.empty((k, n)).T``, as ``Engine.get_factors_device`` wraps its own), their addresses in ``dev``."""
    import torch                    # (lazily: nothing else in this module needs it)
    where = torch.device("cuda", int(device_id))
    k = int(j.k)
    sets = [("", out)] + ([("state_", out.setdefault("state", {"f": [], "s": [], "g": [], "lambda": [], "mu": []}))] if return_state else [])
    for v in range(int(j.n_views)):
        n, m = int(j.n_rows[v]), int(j.n_cols[v])
        for prefix, store in sets:
            for key, shape in (("f", (n, k)), ("s", (k, k)), ("g", (m, k)), ("lambda", (k,)), ("mu", (k,))):
                t = (torch.empty(shape[::-1], dtype=torch.float64, device=where).T if len(shape) == 2
                     else torch.empty(shape, dtype=torch.float64, device=where))
                store[key].append(t)
                getattr(dev, (prefix + key) if prefix else key + "_out")[v] = t.data_ptr()


def _job_views(j, data, q: int, device_id: int, sp, dev, spd) -> list:
    """The views of problem ``q`` by the route each takes (``_view_route``), after the checks that need no library call;
    ``j`` (a ``resnmtf_group_job``) gets its struct size.  What ``fp64_run`` and ``fp64_init_svd`` share."""
    j.struct_size = C.sizeof(_lib.GroupJob)
    views = [_view_route(x, f"problem {q}, view {v}", device_id, dev, spd) for v, x in enumerate(data)]
    if sp is None and any(route == _HOST_CSC for route, _ in views):
        raise ValueError(f"problem {q}: a sparse view (scipy.sparse) is taken by fp64_run alone")
    if len(views) > _lib.GROUP_MAX_VIEWS:
        raise ValueError(f"problem {q}: at most {_lib.GROUP_MAX_VIEWS} views")
    if any(x.ndim != 2 for _, x in views):
        raise ValueError(f"problem {q}: every view must be a matrix")
    return views


def _fill_job_view(j, v: int, route: str, x, q: int, device_id: int, keep: list, sp, dev, spd) -> tuple:
    """View ``v`` of problem ``q`` into the one of ``j`` / ``sp`` / ``dev`` / ``spd`` its route names; returns ``(n, m)``."""
    n, m = (int(d) for d in x.shape)
    j.n_rows[v], j.n_cols[v] = n, m
    if route == _HOST_DENSE:
        keep.append(x)
        j.x[v] = _dp(x)
    elif route == _HOST_CSC:              # the CSC arrays go into sp
        csc = [np.ascontiguousarray(x.indptr, dtype=np.int64), np.ascontiguousarray(x.indices, dtype=np.int32),
               np.ascontiguousarray(x.data, dtype=np.float64)]
        sp.view[v].col_ptr = csc[0].ctypes.data_as(C.POINTER(C.c_longlong))
        sp.view[v].row_idx, sp.view[v].values = _ip(csc[1]), _dp(csc[2])
        keep.extend(csc)
    elif route == _DEVICE_DENSE:          # dev.x[v] describes the tensor as it lies
        t = x.detach()
        keep.append(t)
        dev.x[v] = _device_matrix(t, (n, m), device_id, f"problem {q}, view {v}: data")
    else:                                 # its index and value arrays go into spd
        _fill_fp64_sparse_device(spd, v, x, q, keep)
    return n, m


def _fill_group_job(j, p, q: int, max_iters: int, keep: list, sp=None, dev=None, device_id: int = 0,
                    device_out: bool = False, spd=None) -> dict:
    """Fill one ``resnmtf_group_job`` (``j``) from the problem dict ``p`` (problem ``q`` of its call; the layout
    ``group_run`` documents) and return the output arrays it points to.  ``keep`` collects every array the struct
    points into: the caller holds it until the library call has returned.  Every view takes one route (``_view_route``)
    and only a host dense view sets ``j.x[v]``.  ``sp`` (``fp64_run`` alone): the ``resnmtf_fp64_sparse`` that receives
    the canonical CSC arrays of every ``scipy.sparse`` view; without it such a view is a ``ValueError``.  ``dev``
    (``fp64_run`` alone): the ``resnmtf_fp64_device`` that receives every view and every set of initial factors that are
    ``torch`` tensors on ``cuda:device_id``; the job's own pointers to them stay NULL.  ``device_out``: the job's per-view
    output pointers stay NULL and the returned lists empty (``_fp64_device_outputs`` fills them).  ``spd`` (``fp64_run``
    alone): the ``resnmtf_fp64_sparse_device`` that receives every view that is a sparse tensor on ``cuda:device_id`` (or
    a ``SparseDeviceView`` of one), checked by ``device_views.check_sparse_tensor``."""
    views = _job_views(j, p["data"], q, device_id, sp, dev, spd)
    V, k = len(views), int(p["k"])
    for key in ("init_f", "init_s", "init_g", "init_lam", "init_mu"):
        if p.get(key) is not None and len(p[key]) != V:
            raise ValueError(f"problem {q}: {key} must hold one entry per view")
    j.n_views, j.k = V, k
    n_iters = p.get("n_iters")
    j.n_iters = 0 if n_iters is None else int(n_iters)
    cap = max(1, min(int(n_iters), int(max_iters)) if n_iters else int(max_iters))
    out = {"f": [], "s": [], "g": [], "lambda": [], "mu": [], "all_error": np.empty(cap), "iters": np.zeros(1, np.int32)}
    for v, (route, x) in enumerate(views):
        n, m = _fill_job_view(j, v, route, x, q, device_id, keep, sp, dev, spd)
        factors_there = dev is not None and _fill_fp64_device_factors(dev, v, n, m, p, k, q, device_id, keep)
        if not factors_there:
            try:                              # (the library reads n k, k k and m k doubles through these pointers)
                arrs = [_f64_colmajor(p["init_f"][v], (n, k)), _f64_colmajor(p["init_s"][v], (k, k)),
                        _f64_colmajor(p["init_g"][v], (m, k))]
            except ValueError as exc:
                raise ValueError(f"problem {q}, view {v}: initial factor: {exc}") from None
            j.f0[v], j.s0[v], j.g0[v] = (_dp(a) for a in arrs)
            keep.extend(arrs)
        for name, key in (("lambda0", "init_lam"), ("mu0", "init_mu")):
            vals = p.get(key)
            if vals is not None and vals[v] is not None and not factors_there:
                a = np.ascontiguousarray(_device_views.to_numpy(vals[v]), dtype=np.float64)
                if a.shape != (k,):
                    raise ValueError(f"problem {q}, view {v}: {key} must have k = {k} entries, got shape {a.shape}")
                keep.append(a)
                getattr(j, name)[v] = _dp(a)
        if device_out:
            continue
        for key, shape in (("f", (n, k)), ("s", (k, k)), ("g", (m, k)), ("lambda", (k,)), ("mu", (k,))):
            out[key].append(np.zeros(shape, dtype=np.float64, order="F"))
        j.f_out[v], j.s_out[v], j.g_out[v] = _dp(out["f"][v]), _dp(out["s"][v]), _dp(out["g"][v])
        j.lambda_out[v], j.mu_out[v] = _dp(out["lambda"][v]), _dp(out["mu"][v])
    for name in ("phi", "xi", "psi"):
        if p.get(name) is not None:
            a = _f64_colmajor(p[name], (V, V))
            keep.append(a)
            setattr(j, name, _dp(a))
    for key, cnt, iv_name, iw_name in (("row_pairs", j.row_count, j.row_idx_v, j.row_idx_w),
                                       ("col_pairs", j.col_count, j.col_idx_v, j.col_idx_w)):
        pairs = p.get(key)
        for v in range(V):
            for w in range(V):
                if pairs is None or v == w or pairs[v][w] is None or pairs[v][w][0] is None:
                    cnt[v][w] = -1
                    continue
                iv = np.ascontiguousarray(pairs[v][w][0], dtype=np.int32)
                iw = np.ascontiguousarray(pairs[v][w][1], dtype=np.int32)
                if iv.shape != iw.shape or iv.ndim != 1:
                    raise ValueError(f"problem {q}: index pairs ({v}, {w}) must be two vectors of one length")
                keep.extend([iv, iw])
                cnt[v][w] = len(iv)
                iv_name[v][w], iw_name[v][w] = _ip(iv), _ip(iw)
    j.all_error, j.err_capacity, j.iters_done = _dp(out["all_error"]), cap, _ip(out["iters"])
    return out


def _group_result(out: dict) -> dict:
    it = int(out["iters"][0])
    res = {"f": out["f"], "s": out["s"], "g": out["g"], "lambda": out["lambda"], "mu": out["mu"],
           "all_error": out["all_error"][:it].copy(), "iters": it}
    if "state" in out:              # (fp64_run(return_state=True)): per view (F, S, G, lambda, mu)
        st = out["state"]
        res["state"] = [tuple(st[key][v] for key in ("f", "s", "g", "lambda", "mu")) for v in range(len(st["f"]))]
    return res


def group_run(problems, tol: float = 1.0e-6, max_iters: int = 100000, device_id: int = 0) -> list:
    """Many small factorisations in one call (``resnmtf_group_run``: one workgroup per job, fp64 throughout).

    Each problem is a dict as ``res_nmtf_inner`` receives a job: ``data`` (pre-processed views), ``k``, ``init_f`` /
    ``init_s`` / ``init_g`` per view, optional ``init_lam`` / ``init_mu`` (None: colSums of the initial F / G),
    ``phi`` / ``xi`` / ``psi`` (symmetrised V x V or None), ``row_pairs`` / ``col_pairs`` (``[v][w]`` = the
    ``naming.index_pairs`` of views v and w, ``(None, None)`` for NA; None: every pair NA) and ``n_iters`` (None =
    to convergence).  Returns per problem ``{"f", "s", "g", "lambda", "mu", "all_error", "iters"}`` with F, S, G
    normalised (``normalisation_check``).  The library refuses bad input before any device work."""
    lib = _lib.load()
    problems = list(problems)
    jobs = (_lib.GroupJob * max(1, len(problems)))()
    keep = []
    outs = [_fill_group_job(jobs[q], p, q, max_iters, keep) for q, p in enumerate(problems)]
    rc = lib.resnmtf_group_run(int(device_id), len(problems), jobs, float(tol), int(max_iters))
    if rc != _lib.OK:
        raise ResnmtfError(rc, (lib.resnmtf_last_error(None) or b"").decode())
    return [_group_result(out) for out in outs]


def fp64_run(problem, tol: float = 1.0e-6, max_iters: int = 100000, device_id: int = 0, output: str = "numpy",
             return_state: bool = False) -> dict:
    """One factorisation in fp64 at any size (``resnmtf_fp64_run``: the arithmetic of ``group_run``, spread over the
    whole device).  ``problem`` is one problem dict of ``group_run`` -- without its caps: k up to
    64, no limit on n * m -- and the result is one element of its list.  Bad input is refused before any device work
    (``ResnmtfError``), a job the device cannot hold with ``RESNMTF_ERR_ALLOC`` and its byte count.

    A ``scipy.sparse`` matrix in ``problem["data"][v]`` is a SPARSE view: taken as its canonical
    CSC (``sparse.canonical_csc``, a copy), already pre-processed, stored and streamed sparse on the device
    (``resnmtf_fp64_run_sparse``); dense and sparse views mix freely.  A problem without one calls ``resnmtf_fp64_run``
    exactly as before.

    Device memory (``resnmtf_fp64_run_device``).  An entry of ``problem["data"]`` that is a ``torch``
    tensor on ``cuda:device_id`` (2-D, fp64 / fp32 / fp16 / bf16, any strides, an expanded one included) is read where it
    lies: one kernel builds both fp64 images of it, no host copy, no staging.  So are ``init_f[v]`` / ``init_s[v]`` /
    ``init_g[v]`` when all three of a view are such tensors (a mix is a ``ValueError``), and ``init_lam[v]`` / ``init_mu[v]``
    beside them (``None``: the column sums, summed on the device in the host loop's order).  The call is ordered after the
    work enqueued on torch's current stream of that device.  ``output="torch"``: F, S, G, lambda and mu come back as fp64
    tensors on the device (F, S, G column-major, as ``Engine.get_factors_device`` wraps its own) under the same keys;
    ``all_error`` and ``iters`` stay NumPy.  ``return_state=True`` (needs ``output="torch"``, else ``ValueError``) adds
    ``"state"``: per view the raw ``(F, S, G, lambda, mu)`` after the last sweep, before the normalisation -- what a later
    call resumes from.  Every result is bit for bit the host route's on ``t.double().cpu().numpy()`` of the same tensors.
    A problem with nothing on the device and the default flags makes the calls it made before.

    Sparse tensors in device memory (``resnmtf_fp64_run_sparse_device``).  An entry of
    ``problem["data"]`` that is a 2-D ``sparse_csc`` / ``sparse_csr`` / coalesced ``sparse_coo`` tensor on
    ``cuda:device_id`` (or a ``device_views.SparseDeviceView`` of one; checked by ``device_views.check_sparse_tensor``) is a
    SPARSE view read where it lies: floating values of any of the four types, int32 / int64 indices, entries in any order,
    stored positions distinct, taken as pre-processed.  It is checked and sorted on the device (its refusals surface as
    ``ResnmtfError``) and nothing of it is brought to the host.  Every result is bit for bit that of the ``scipy.sparse``
    matrix of the same stored entries -- with ONE difference: an explicitly stored zero stays stored here, while
    ``sparse.canonical_csc`` drops it on the host route (the sums then differ in their last bits, not in what they stand
    for).  Such views mix with every other kind.  A problem without one makes exactly the calls it made before."""
    _device_views.check_output(output)
    if return_state and output != "torch":
        raise ValueError("return_state=True needs output='torch' (the raw state is left on the device)")
    lib = _lib.load()
    job = _lib.GroupJob()
    keep = []
    data = problem["data"]
    tensors = [x for key in ("data", "init_f", "init_s", "init_g", "init_lam", "init_mu") for x in (problem.get(key) or ())]
    # which of the three structs the problem needs; the entry follows from which of them exist
    sp = _lib.Fp64Sparse() if any(_sparse.is_sparse(x) for x in data) else None                      # (section 22)
    spd = _lib.Fp64SparseDevice() if any(_device_views.is_sparse_device_view(x) for x in data) else None      # (section 24)
    dev = (_lib.Fp64Device() if output == "torch" or spd is not None or any(_device_views.is_device_tensor(x) for x in tensors)
           else None)                                                                                 # (section 23)
    for s in (sp, dev, spd):
        if s is not None:
            s.struct_size = C.sizeof(s)
    out = _fill_group_job(job, problem, 0, max_iters, keep, sp=sp, dev=dev, device_id=device_id, device_out=output == "torch", spd=spd)
    if dev is not None:
        import torch                # (lazily: nothing else in this module needs it)
        if output == "torch":
            _fp64_device_outputs(dev, job, out, device_id, return_state)
        dev.stream = torch.cuda.current_stream(torch.device("cuda", int(device_id))).cuda_stream
        if spd is not None:
            spd.stream = dev.stream
    head, tail = (int(device_id), C.byref(job)), (float(tol), int(max_iters))
    if spd is not None:
        rc = lib.resnmtf_fp64_run_sparse_device(*head, None if sp is None else C.byref(sp), C.byref(dev), C.byref(spd), *tail)
    elif dev is not None:
        rc = lib.resnmtf_fp64_run_device(*head, None if sp is None else C.byref(sp), C.byref(dev), *tail)
    elif sp is not None:
        rc = lib.resnmtf_fp64_run_sparse(*head, C.byref(sp), *tail)
    else:
        rc = lib.resnmtf_fp64_run(*head, *tail)
    if rc != _lib.OK:
        raise ResnmtfError(rc, (lib.resnmtf_last_error(None) or b"").decode())
    return _group_result(out)


def fp64_init_svd(views, k: int, seed=0, sigma: float = 0.05, n_power: int = 0, return_basis: bool = False,
                  output: str = "numpy", device_id: int = 0) -> list:
    """``init_mats_inner`` (``R/update_steps.r:78-125``) of every view in double precision, without an engine
    (``resnmtf_fp64_init_svd``): the algorithm of ``Engine.init_svd`` -- the same sketch width,
    rounds, ridge, rank cut and draw order, so the same seed is the same sketch -- on the fp64 values of the views, where
    the engine's starts from their f32 images.

    ``views`` are what ``fp64_run`` takes as ``problem["data"]``: fp64 arrays, ``scipy.sparse`` matrices (taken as
    pre-processed), dense and sparse ``torch`` tensors on ``cuda:device_id``; a dense view goes through the fp64 images and
    products of the run, a sparse one through its CSC + CSR copies and the fp64 SpMM.  ``k``: one k for all views.
    ``seed``: an integer (view v draws from ``seed + v``, as ``res_nmtf_inner`` seeds the engine) or one seed per view.
    Returns per view ``(F0, S0, G0, lambda0, mu0)``; with ``return_basis=True`` each tuple goes on with ``(d, U, V, d_all)``
    as ``Engine.init_svd(return_basis=True)`` returns them.  ``output="torch"``: the five come back as fp64 tensors on the
    device (F0, S0, G0 column-major) and nothing of size n or m crosses the bus; both outputs hold the same bits.  Bad
    input is refused before any device work (``ResnmtfError``)."""
    _device_views.check_output(output)
    lib = _lib.load()
    views = list(views)
    job, init, keep = _lib.GroupJob(), _lib.Fp64Init(), []
    sp = _lib.Fp64Sparse() if any(_sparse.is_sparse(x) for x in views) else None
    spd = _lib.Fp64SparseDevice() if any(_device_views.is_sparse_device_view(x) for x in views) else None
    dev = _lib.Fp64Device() if spd is not None or any(_device_views.is_device_tensor(x) for x in views) else None
    for s in (sp, dev, spd, init):
        if s is not None:
            s.struct_size = C.sizeof(s)
    routed = _job_views(job, views, 0, device_id, sp, dev, spd)
    V, k = len(routed), int(k)
    job.n_views, job.k = V, k
    seeds = [int(seed) + v for v in range(V)] if np.ndim(seed) == 0 else [int(s) for s in seed]
    if len(seeds) != V:
        raise ValueError("seed must be one integer or one seed per view")
    init.sigma, init.n_power, init.outputs_on_device = float(sigma), int(n_power), int(output == "torch")
    out, extra = [], []
    for v, (route, x) in enumerate(routed):
        n, m = _fill_job_view(job, v, route, x, 0, device_id, keep, sp, dev, spd)
        init.seed[v] = seeds[v] & 0xFFFFFFFFFFFFFFFF
        shapes = ((n, k), (k, k), (m, k), (k,), (k,))
        if output == "torch":
            import torch                # (lazily: nothing else in this module needs it)
            where = torch.device("cuda", int(device_id))
            five = [torch.empty(s[::-1], dtype=torch.float64, device=where).T if len(s) == 2
                    else torch.empty(s, dtype=torch.float64, device=where) for s in shapes]
            addr = [t.data_ptr() for t in five]
        else:
            five = [np.zeros(s, dtype=np.float64, order="F") for s in shapes]
            addr = [a.ctypes.data for a in five]
        for name, a in zip(("f0", "s0", "g0", "lambda0", "mu0"), addr):
            getattr(init, name)[v] = a
        out.append(tuple(five))
        if return_basis:
            d, u, w = np.zeros(k), np.zeros((n, k), order="F"), np.zeros((m, k), order="F")
            d_all, n_d = np.zeros(64), np.zeros(1, np.int32)
            init.singular_values[v], init.basis_u[v], init.basis_v[v], init.basis_d[v] = _dp(d), _dp(u), _dp(w), _dp(d_all)
            init.basis_n_d[v] = _ip(n_d)
            extra.append((d, u, w, d_all, n_d))
    if dev is not None:
        import torch
        dev.stream = torch.cuda.current_stream(torch.device("cuda", int(device_id))).cuda_stream
        if spd is not None:
            spd.stream = dev.stream
    rc = lib.resnmtf_fp64_init_svd(int(device_id), C.byref(job), None if sp is None else C.byref(sp),
                                   None if dev is None else C.byref(dev), None if spd is None else C.byref(spd), C.byref(init))
    if rc != _lib.OK:
        raise ResnmtfError(rc, (lib.resnmtf_last_error(None) or b"").decode())
    if return_basis:
        out = [five + (d, u, w, d_all[:int(n_d[0])].copy()) for five, (d, u, w, d_all, n_d) in zip(out, extra)]
    return out


def fp64_bisil(x, rc, cc, distance: str = "euclidean", device_id: int = 0):
    """The per-member silhouettes of one view's biclusters in double precision (``resnmtf_fp64_bisil``, no handle;
    DESIGN.md section 26): ``Engine.bisil``'s definition, metrics and result -- ``(row_sil, col_sil)``, n x k and m x k
    NumPy arrays, 0 at non-members -- on the fp64 values of ``x``, where ``Engine.bisil`` reads a handle's fp32 image.
    ``x``: a NumPy array or a CPU tensor (copied once to the device as fp64), or a 2-D floating ``torch`` tensor on
    ``cuda:device_id`` (fp64 / fp32 / fp16 / bf16, any strides, an expanded one included), read where it lies, ordered
    after the work on torch's current stream of that device (``device_views.as_view``'s checks: ``ValueError``).
    ``rc`` / ``cc``: n x k and m x k 0 / 1 matrices, NumPy arrays or tensors (brought to the host).  Two calls give equal
    bits; on data that fp32 holds exactly the result is bitwise ``Engine.bisil``'s.  Bad input is refused before any
    device work (``ResnmtfError``), a workspace the device cannot hold with ``RESNMTF_ERR_ALLOC`` and its byte count."""
    from .bisil import METRICS
    if distance not in METRICS:
        raise ValueError("distance must be one of 'euclidean', 'manhattan' or 'cosine'.")
    lib = _lib.load()
    x = _device_views.as_view(x, device_id, "fp64_bisil: x")
    if _sparse.is_sparse_view(x) or isinstance(x, _device_views.RawDeviceView):
        raise NotImplementedError("fp64_bisil scores dense views: a sparse view is not supported")
    if len(x.shape) != 2:
        raise ValueError("fp64_bisil: x must be an n x m matrix")
    n, m = int(x.shape[0]), int(x.shape[1])
    rc = np.asfortranarray(np.asarray(_device_views.to_numpy(rc), dtype=np.float64))
    if rc.ndim != 2 or rc.shape[0] != n:
        raise ValueError(f"row clusters must be {n} x k")
    cc = _f64_colmajor(_device_views.to_numpy(cc), (m, rc.shape[1]))
    k = int(rc.shape[1])
    rs = np.zeros((n, k), order="F"); cs = np.zeros((m, k), order="F")
    job = _lib.Fp64BisilJob()
    job.struct_size = C.sizeof(job)
    job.n, job.m, job.k, job.metric = n, m, k, METRICS[distance]
    if _device_views.is_tensor(x):
        import torch                # (lazily: nothing else in this module needs it)
        job.x_dev = _device_matrix(x, (n, m), device_id, "fp64_bisil: x")
        job.stream = torch.cuda.current_stream(torch.device("cuda", int(device_id))).cuda_stream
    else:
        x = _f64_colmajor(x)
        job.x = _dp(x)
    job.row_clusters, job.col_clusters, job.row_sil, job.col_sil = _dp(rc), _dp(cc), _dp(rs), _dp(cs)
    code = lib.resnmtf_fp64_bisil(int(device_id), C.byref(job))
    if code != _lib.OK:
        raise ResnmtfError(code, (lib.resnmtf_last_error(None) or b"").decode())
    return rs, cs


def _fill_fp64_sparse_source(job, x, device_id: int, keep: list, what: str):
    """The one place for X of a job struct that takes a sparse view either way (``resnmtf_fp64_bisil_sparse_job``,
    ``resnmtf_fp64_shuffle_sparse_job``, ``resnmtf_fp64_subsample_sparse_job``): a canonical ``scipy.sparse`` CSC as the host arrays ``job.x`` (``job.x_dev`` all
    zero), a checked ``SparseDeviceView`` as ``job.x_dev`` -- the addresses of the tensor's own index and value arrays,
    ``job.x`` NULL: nothing of it comes to the host -- and ``job.stream`` = torch's current stream.  ``keep`` collects what
    the struct points into."""
    if isinstance(x, _device_views.SparseDeviceView):
        import torch                # (lazily: nothing else in this module needs it)
        _fill_sparse_device_view(job.x_dev, x, what, keep)
        job.stream = torch.cuda.current_stream(torch.device("cuda", int(device_id))).cuda_stream
        return
    csc = [np.ascontiguousarray(x.indptr, dtype=np.int64), np.ascontiguousarray(x.indices, dtype=np.int32),
           np.ascontiguousarray(x.data, dtype=np.float64)]
    if csc[1].size == 0:            # (never a NULL pointer)
        csc[1], csc[2] = np.zeros(1, dtype=np.int32), np.zeros(1)
    keep.extend(csc)
    job.x.col_ptr = csc[0].ctypes.data_as(C.POINTER(C.c_longlong))
    job.x.row_idx, job.x.values = _ip(csc[1]), _dp(csc[2])


def _fp64_bisil_sparse_job(x, n: int, m: int, device_id: int, keep: list) -> _lib.Fp64BisilSparseJob:
    """The ``resnmtf_fp64_bisil_sparse_job`` of the sparse view ``x`` with its one place for X filled
    (``_fill_fp64_sparse_source``)."""
    job = _lib.Fp64BisilSparseJob()
    job.struct_size = C.sizeof(job)
    job.n, job.m = n, m
    _fill_fp64_sparse_source(job, x, device_id, keep, "fp64_bisil_sparse: x")
    return job


def fp64_bisil_sparse(x, rc, cc, distance: str = "euclidean", device_id: int = 0):
    """``fp64_bisil`` of a SPARSE view (``resnmtf_fp64_bisil_sparse``, no handle): the same
    ``(row_sil, col_sil)``, bit for bit ``fp64_bisil`` of the densified view, without the n x m fp64 matrix -- on the
    device the view is a CSC and a CSR copy (24 bytes per stored entry) and per bicluster the restricted block is
    zero-filled and scattered into.  ``x``: a ``scipy.sparse`` matrix (a CPU sparse tensor is taken as its SciPy matrix),
    made canonical with ``sparse.canonical_csc`` (a copy; duplicates summed, explicit zeros dropped) and taken as
    pre-processed -- a negative or non-finite value is refused (``ValueError``, ``sparse.validate``'s texts), an all-zero
    column is not: the score of a sub-sample or of an empty view is defined --; or a 2-D ``sparse_csc`` / ``sparse_csr`` /
    coalesced ``sparse_coo`` tensor on ``cuda:device_id`` (or its ``device_views.SparseDeviceView``), read where it lies
    on torch's current stream: checked and sorted on the device, explicit zeros kept, nothing of it brought to the host.
    A dense view is a ``ValueError`` (``fp64_bisil`` takes those).  ``rc`` / ``cc`` and the refusals as ``fp64_bisil``."""
    from .bisil import METRICS
    if distance not in METRICS:
        raise ValueError("distance must be one of 'euclidean', 'manhattan' or 'cosine'.")
    lib = _lib.load()
    x = _device_views.host_or_device(x, "fp64_bisil_sparse: x")
    if _device_views.is_sparse_device_view(x):
        x = _device_views.as_sparse_view(x, device_id, "fp64_bisil_sparse: x")
    elif _sparse.is_sparse(x):
        x = _sparse.canonical_csc(x)
        _sparse.validate_values(x, "view")
    else:
        raise ValueError("fp64_bisil_sparse scores sparse views (scipy.sparse, or a sparse torch tensor): fp64_bisil takes a dense one")
    n, m = int(x.shape[0]), int(x.shape[1])
    rc = np.asfortranarray(np.asarray(_device_views.to_numpy(rc), dtype=np.float64))
    if rc.ndim != 2 or rc.shape[0] != n:
        raise ValueError(f"row clusters must be {n} x k")
    cc = _f64_colmajor(_device_views.to_numpy(cc), (m, rc.shape[1]))
    k = int(rc.shape[1])
    rs = np.zeros((n, k), order="F"); cs = np.zeros((m, k), order="F")
    keep = []
    job = _fp64_bisil_sparse_job(x, n, m, device_id, keep)
    job.k, job.metric = k, METRICS[distance]
    job.row_clusters, job.col_clusters, job.row_sil, job.col_sil = _dp(rc), _dp(cc), _dp(rs), _dp(cs)
    code = lib.resnmtf_fp64_bisil_sparse(int(device_id), C.byref(job))
    if code != _lib.OK:
        raise ResnmtfError(code, (lib.resnmtf_last_error(None) or b"").decode())
    return rs, cs


def fp64_shuffle(x, seed: int, normalise: bool = True, device_id: int = 0):
    """``shuffle_view`` (``R/obtain_bicl.r:11-22``) of one view in double precision (``resnmtf_fp64_shuffle``, no handle;
    DESIGN.md section 27): ``Engine.shuffle_view_from``'s draw for the same ``seed`` -- ``tests/shuffle_ref.shuffle_dense``
    restates it -- made of the fp64 values of ``x``, where the engine permutes a handle's fp32 image.  Returns ``(tensor,
    was_negative, empty_rows, empty_cols)``: the draw as an fp64 column-major ``torch`` tensor on ``cuda:device_id``
    (``normalise``: shifted and column-normalised in fp64 as ``apply_resnmtf`` does to shuffled data, ``R/utils.r:416,422``),
    whether an entry was negative (False without ``normalise``), and the boolean masks of the rows / columns of the draw
    that sum to exactly zero before any shift (the redraw condition, ``:14-18``; the caller redraws with another seed).
    ``x``: a NumPy array or a CPU tensor (copied once to the device as fp64), or a 2-D floating ``torch`` tensor on
    ``cuda:device_id`` (fp64 / fp32 / fp16 / bf16, any strides, an expanded one included), read where it lies, ordered
    after the work on torch's current stream of that device (``device_views.as_view``'s checks: ``ValueError``).  Two
    calls give equal bits.  Bad input is refused before any device work (``ResnmtfError``)."""
    import torch                    # (lazily: nothing else in this module needs it)
    lib = _lib.load()
    x = _device_views.as_view(x, device_id, "fp64_shuffle: x")
    if _sparse.is_sparse_view(x) or isinstance(x, _device_views.RawDeviceView):
        raise NotImplementedError("fp64_shuffle draws dense views: a sparse view is not supported")
    if len(x.shape) != 2:
        raise ValueError("fp64_shuffle: x must be an n x m matrix")
    n, m = int(x.shape[0]), int(x.shape[1])
    if n < 1 or m < 1:
        raise ValueError("fp64_shuffle: x must have at least one row and one column")
    dev = torch.device("cuda", int(device_id))
    out = torch.empty((m, n), dtype=torch.float64, device=dev).t()          # n x m, column-major
    neg, nr, nc = C.c_int(0), C.c_int(0), C.c_int(0)
    rm = np.zeros(n, dtype=np.uint8); cm = np.zeros(m, dtype=np.uint8)
    job = _lib.Fp64ShuffleJob()
    job.struct_size = C.sizeof(job)
    job.n, job.m, job.normalise, job.seed = n, m, 1 if normalise else 0, int(seed) & 0xFFFFFFFFFFFFFFFF
    if _device_views.is_tensor(x):
        job.x_dev = _device_matrix(x, (n, m), device_id, "fp64_shuffle: x")
    else:
        x = _f64_colmajor(x)
        job.x = _dp(x)
    job.stream = torch.cuda.current_stream(dev).cuda_stream
    job.out = out.data_ptr()
    job.was_negative, job.n_empty_rows, job.n_empty_cols = C.pointer(neg), C.pointer(nr), C.pointer(nc)
    job.row_mask, job.col_mask = rm.ctypes.data_as(C.POINTER(C.c_ubyte)), cm.ctypes.data_as(C.POINTER(C.c_ubyte))
    code = lib.resnmtf_fp64_shuffle(int(device_id), C.byref(job))
    if code != _lib.OK:
        raise ResnmtfError(code, (lib.resnmtf_last_error(None) or b"").decode())
    return out, bool(neg.value), rm.astype(bool), cm.astype(bool)


def fp64_shuffle_sparse(x, seed: int, normalise: bool = True, device_id: int = 0):
    """``fp64_shuffle`` of a SPARSE view (``resnmtf_fp64_shuffle_sparse``, no handle): the same draw
    for the same ``seed``, made of the stored entries alone -- a stored entry at (r, c) lands at
    ``feistel_perm_inverse(r m + c)``, explicit zeros stay stored, no n x m array exists at any point.  Returns ``(tensor,
    empty_rows, empty_cols)``: the draw as a ``sparse_csc`` tensor on ``cuda:device_id`` with fp64 values and int64 indices
    (canonical: rows ascending within a column; what ``fp64_run`` takes as a sparse device view), and the boolean masks of
    the rows / columns that hold no stored entry > 0 (the redraw condition, ``R/obtain_bicl.r:14-18``; the caller redraws
    with another seed).  Positions, values and masks are bit for bit those of ``fp64_shuffle`` of the densified view at the
    stored positions -- with ``normalise`` too, the column sums being taken in its order --, and in an empty column a
    stored zero gives NaN as there.  ``x``: a ``scipy.sparse`` matrix (a CPU sparse tensor is taken as its SciPy matrix),
    made canonical with ``sparse.canonical_csc`` (a copy; duplicates summed, explicit zeros dropped) and taken as
    pre-processed; or a 2-D ``sparse_csc`` / ``sparse_csr`` / coalesced ``sparse_coo`` tensor on ``cuda:device_id`` (or its
    ``device_views.SparseDeviceView``), read where it lies on torch's current stream: checked and sorted on the device,
    nothing of it brought to the host.  A dense view is a ``ValueError`` (``fp64_shuffle`` takes those).  Two calls give
    equal bits.  Bad input is refused before any device work (``ResnmtfError``)."""
    import torch                    # (lazily: nothing else in this module needs it)
    lib = _lib.load()
    x = _device_views.host_or_device(x, "fp64_shuffle_sparse: x")
    if _device_views.is_sparse_device_view(x):
        x = _device_views.as_sparse_view(x, device_id, "fp64_shuffle_sparse: x")
    elif _sparse.is_sparse(x):
        x = _sparse.canonical_csc(x)
    else:
        raise ValueError("fp64_shuffle_sparse draws sparse views (scipy.sparse, or a sparse torch tensor): fp64_shuffle takes a dense one")
    n, m, nnz = int(x.shape[0]), int(x.shape[1]), int(x.nnz)
    if n < 1 or m < 1:
        raise ValueError("fp64_shuffle_sparse: x must have at least one row and one column")
    dev = torch.device("cuda", int(device_id))
    ccol = torch.empty(m + 1, dtype=torch.int64, device=dev)
    rows = torch.empty(nnz, dtype=torch.int64, device=dev)
    vals = torch.empty(nnz, dtype=torch.float64, device=dev)
    nr, nc = C.c_int(0), C.c_int(0)
    rm = np.zeros(n, dtype=np.uint8); cm = np.zeros(m, dtype=np.uint8)
    keep = []
    job = _lib.Fp64ShuffleSparseJob()
    job.struct_size = C.sizeof(job)
    job.n, job.m, job.normalise, job.seed = n, m, 1 if normalise else 0, int(seed) & 0xFFFFFFFFFFFFFFFF
    _fill_fp64_sparse_source(job, x, device_id, keep, "fp64_shuffle_sparse: x")
    job.stream = torch.cuda.current_stream(dev).cuda_stream
    job.out_col_ptr, job.out_row_idx, job.out_values = ccol.data_ptr(), rows.data_ptr() or None, vals.data_ptr() or None
    job.n_empty_rows, job.n_empty_cols = C.pointer(nr), C.pointer(nc)
    job.row_mask, job.col_mask = rm.ctypes.data_as(C.POINTER(C.c_ubyte)), cm.ctypes.data_as(C.POINTER(C.c_ubyte))
    code = lib.resnmtf_fp64_shuffle_sparse(int(device_id), C.byref(job))
    if code != _lib.OK:
        raise ResnmtfError(code, (lib.resnmtf_last_error(None) or b"").decode())
    out = torch.sparse_csc_tensor(ccol, rows, vals, size=(n, m), check_invariants=False)
    return out, rm.astype(bool), cm.astype(bool)


def _index_list(idx, what: str) -> np.ndarray:
    """An index list as contiguous int32 (the C-ABI validates its range and that no index occurs twice)."""
    arr = np.asarray(idx)
    if arr.ndim != 1 or arr.size < 1:
        raise ValueError(f"{what} must be a non-empty 1-D index list")
    if not np.issubdtype(arr.dtype, np.integer):
        raise ValueError(f"{what} must hold integers, got {arr.dtype}")
    if arr.min() < np.iinfo(np.int32).min or arr.max() > np.iinfo(np.int32).max:
        raise ValueError(f"{what} holds an index beyond 32 bits")
    return np.ascontiguousarray(arr, dtype=np.int32)


def fp64_device_view(x, device_id: int = 0):
    """The dense view ``x`` as ``fp64_subsample`` reads it many times: a tensor on ``cuda:device_id`` as it is, anything
    else (a NumPy array, a CPU tensor) copied there once as an fp64 column-major tensor -- the same values, so a sub-sample
    of the copy has the bits of a sub-sample of ``x``."""
    import torch
    if _device_views.is_tensor(x) and _device_views.on_engine_device(x, device_id):
        return x
    arr = _f64_colmajor(_device_views.to_numpy(x) if _device_views.is_tensor(x) else x)
    return torch.as_tensor(np.ascontiguousarray(arr.T)).to(torch.device("cuda", int(device_id))).t()


def fp64_subsample_plan(row_stride: int = 1, col_stride: int = 1) -> dict:
    """How ``fp64_subsample`` launches for a source with the given strides in elements (``resnmtf_fp64_subsample_plan``;
    no device work): ``{"gather": "rows" (lanes along the destination rows) or "lds" (the padded LDS tile transpose),
    "gather_rows", "gather_tile", "row_sum_rows", "col_sum_rows", "col_sum_cols"}`` -- the form and every tile edge."""
    lib = _lib.load()
    out = (C.c_int * _lib.FP64_SUBSAMPLE_PLAN_INTS)()
    rc = lib.resnmtf_fp64_subsample_plan(int(row_stride), int(col_stride), out)
    if rc != _lib.OK:
        raise ResnmtfError(rc, (lib.resnmtf_last_error(None) or b"").decode())
    v = list(out)
    return {"gather": ("rows", "lds")[v[0]], "gather_rows": v[1], "gather_tile": v[2], "row_sum_rows": v[3],
            "col_sum_rows": v[4], "col_sum_cols": v[5]}


def fp64_subsample(x, rows, cols, device_id: int = 0, out=None):
    """The sub-sample ``x[rows, cols]`` of one view in double precision (``resnmtf_fp64_subsample``, no handle; DESIGN.md
    section 28): ``stability_repeat``'s ``data[[i]][row_samples, col_samples]`` (``R/stability_analysis.r:124``) on the fp64
    values of ``x``, not re-normalised.  Returns ``(tensor, empty_rows, empty_cols)``: the sub-sample as an fp64
    column-major ``torch`` tensor on ``cuda:device_id`` and the boolean masks of its rows / columns that sum to exactly
    zero (one running fp64 sum per line, a row over ascending columns, a column over ascending rows: the flags
    ``Engine.subsample_view_from`` + ``Engine.empty_lines`` report on data fp32 holds).  ``x``: as for ``fp64_shuffle`` (a
    NumPy array or CPU tensor, copied once to the device as fp64, or a floating ``torch`` tensor on ``cuda:device_id`` of
    any strides, read where it lies after the work on torch's current stream).  ``rows`` / ``cols``: 0-based, in any
    order, each index at most once.  ``out`` (a test hook): an fp64 tensor of shape ``(len(cols), len(rows))``, contiguous,
    on the device, whose transpose receives the sub-sample instead of a fresh one.  Two calls give equal bits.  Bad input
    is refused before any device work (``ResnmtfError``)."""
    import torch                    # (lazily: nothing else in this module needs it)
    lib = _lib.load()
    x = _device_views.as_view(x, device_id, "fp64_subsample: x")
    if isinstance(x, _device_views.RawDeviceView):
        raise NotImplementedError("fp64_subsample gathers pre-processed dense views: a device tensor still to be shifted "
                                  "and column-normalised (RawDeviceView) is not supported")
    if _sparse.is_sparse_view(x) or _device_views.is_sparse_device_view(x):
        raise NotImplementedError("fp64_subsample gathers dense views: a sparse view is not supported")
    if len(x.shape) != 2:
        raise ValueError("fp64_subsample: x must be an n x m matrix")
    n, m = int(x.shape[0]), int(x.shape[1])
    if n < 1 or m < 1:
        raise ValueError("fp64_subsample: x must have at least one row and one column")
    rows, cols = _index_list(rows, "fp64_subsample: rows"), _index_list(cols, "fp64_subsample: cols")
    ns, ms = int(rows.size), int(cols.size)
    dev = torch.device("cuda", int(device_id))
    if out is None:
        out = torch.empty((ms, ns), dtype=torch.float64, device=dev)
    elif tuple(out.shape) != (ms, ns) or out.dtype != torch.float64 or not out.is_contiguous() or out.device != dev:
        raise ValueError("fp64_subsample: out must be a contiguous fp64 tensor of shape (len(cols), len(rows)) on the device")
    nr, nc = C.c_int(0), C.c_int(0)
    rm = np.zeros(ns, dtype=np.uint8); cm = np.zeros(ms, dtype=np.uint8)
    job = _lib.Fp64SubsampleJob()
    job.struct_size = C.sizeof(job)
    job.n, job.m, job.n_sub, job.m_sub = n, m, ns, ms
    job.rows, job.cols = _ip(rows), _ip(cols)
    if _device_views.is_tensor(x):
        job.x_dev = _device_matrix(x, (n, m), device_id, "fp64_subsample: x")
    else:
        x = _f64_colmajor(x)
        job.x = _dp(x)
    job.stream = torch.cuda.current_stream(dev).cuda_stream
    job.out = out.data_ptr()
    job.n_empty_rows, job.n_empty_cols = C.pointer(nr), C.pointer(nc)
    job.row_mask, job.col_mask = rm.ctypes.data_as(C.POINTER(C.c_ubyte)), cm.ctypes.data_as(C.POINTER(C.c_ubyte))
    code = lib.resnmtf_fp64_subsample(int(device_id), C.byref(job))
    if code != _lib.OK:
        raise ResnmtfError(code, (lib.resnmtf_last_error(None) or b"").decode())
    return out.t(), rm.astype(bool), cm.astype(bool)             # n_sub x m_sub, column-major


def fp64_sparse_device_view(x, device_id: int = 0):
    """The sparse view ``x`` as ``fp64_subsample_sparse`` reads it many times, the sparse twin of ``fp64_device_view``: a
    sparse tensor on ``cuda:device_id`` (or its ``SparseDeviceView``) as it is, anything else (a ``scipy.sparse`` matrix, a
    CPU sparse tensor) uploaded there once as the ``sparse_csc`` tensor of its canonical CSC (``sparse.canonical_csc``:
    fp64 values, int64 indices) -- the same stored values, so a sub-sample of the copy has the bits of a sub-sample of
    ``x``."""
    import torch
    x = _device_views.host_or_device(x, "fp64_sparse_device_view: x")
    if _device_views.is_sparse_device_view(x):
        return x
    if not _sparse.is_sparse(x):
        raise ValueError("fp64_sparse_device_view takes sparse views (scipy.sparse, or a sparse torch tensor): fp64_device_view "
                         "takes a dense one")
    c = _sparse.canonical_csc(x)
    dev = torch.device("cuda", int(device_id))
    return torch.sparse_csc_tensor(torch.as_tensor(np.ascontiguousarray(c.indptr, dtype=np.int64)).to(dev),
                                   torch.as_tensor(np.ascontiguousarray(c.indices, dtype=np.int64)).to(dev),
                                   torch.as_tensor(np.ascontiguousarray(c.data, dtype=np.float64)).to(dev),
                                   size=tuple(int(s) for s in c.shape), check_invariants=False)


def fp64_subsample_sparse(x, rows, cols, device_id: int = 0, count_only: bool = False):
    """``fp64_subsample`` of a SPARSE view (``resnmtf_fp64_subsample_sparse``, no handle): the
    sub-sample ``x[rows, cols]`` made of the stored entries alone -- a stored entry survives iff its row is in ``rows`` and
    its column in ``cols``, its value is carried as it is (widened to fp64 exactly, not re-normalised), explicit zeros stay
    stored, no n x m array exists at any point.  Returns ``(tensor, empty_rows, empty_cols)``: the sub-sample as a
    ``sparse_csc`` tensor on ``cuda:device_id`` with fp64 values and int64 indices (canonical: rows ascending within a
    column; what ``fp64_run`` takes as a sparse device view), and the boolean masks of the rows / columns that hold no
    stored entry > 0 -- the lines that sum to exactly zero, the condition under which ``stability_repeat`` trims
    (``R/stability_analysis.r:165-190``).  Structure, values and masks are bit for bit those of ``fp64_subsample`` of the
    densified view at the stored positions.  ``count_only``: nothing is sorted or written on the device; returns
    ``(nnz_sub, empty_rows, empty_cols)``.  ``x``: a ``scipy.sparse`` matrix (a CPU sparse tensor is taken as its SciPy
    matrix), made canonical with ``sparse.canonical_csc`` (a copy; duplicates summed, explicit zeros dropped) and taken as
    pre-processed; or a 2-D ``sparse_csc`` / ``sparse_csr`` / coalesced ``sparse_coo`` tensor on ``cuda:device_id`` (or its
    ``device_views.SparseDeviceView``), read where it lies on torch's current stream: checked and sorted on the device,
    nothing of it brought to the host.  ``rows`` / ``cols``: 0-based, in any order, each index at most once.  The outputs
    are allocated for ``min(nnz, len(rows) * len(cols))`` entries, one call is made and the first ``nnz_sub`` entries are
    wrapped.  A dense view is a ``ValueError`` (``fp64_subsample`` takes those).  Two calls give equal bits.  Bad input is
    refused before any device work (``ResnmtfError``)."""
    import torch                    # (lazily: nothing else in this module needs it)
    lib = _lib.load()
    x = _device_views.host_or_device(x, "fp64_subsample_sparse: x")
    if _device_views.is_sparse_device_view(x):
        x = _device_views.as_sparse_view(x, device_id, "fp64_subsample_sparse: x")
    elif _sparse.is_sparse(x):
        x = _sparse.canonical_csc(x)
    else:
        raise ValueError("fp64_subsample_sparse gathers sparse views (scipy.sparse, or a sparse torch tensor): fp64_subsample takes a dense one")
    n, m, nnz = int(x.shape[0]), int(x.shape[1]), int(x.nnz)
    if n < 1 or m < 1:
        raise ValueError("fp64_subsample_sparse: x must have at least one row and one column")
    rows, cols = _index_list(rows, "fp64_subsample_sparse: rows"), _index_list(cols, "fp64_subsample_sparse: cols")
    ns, ms = int(rows.size), int(cols.size)
    dev = torch.device("cuda", int(device_id))
    kept, nr, nc = C.c_longlong(0), C.c_int(0), C.c_int(0)
    rm = np.zeros(ns, dtype=np.uint8); cm = np.zeros(ms, dtype=np.uint8)
    keep = []
    job = _lib.Fp64SubsampleSparseJob()
    job.struct_size = C.sizeof(job)
    job.n, job.m, job.n_sub, job.m_sub = n, m, ns, ms
    job.rows, job.cols = _ip(rows), _ip(cols)
    _fill_fp64_sparse_source(job, x, device_id, keep, "fp64_subsample_sparse: x")
    job.stream = torch.cuda.current_stream(dev).cuda_stream
    if not count_only:
        cap = min(nnz, ns * ms)
        ccol = torch.empty(ms + 1, dtype=torch.int64, device=dev)
        ridx = torch.empty(cap, dtype=torch.int64, device=dev)
        vals = torch.empty(cap, dtype=torch.float64, device=dev)
        job.out_col_ptr, job.out_row_idx, job.out_values = ccol.data_ptr(), ridx.data_ptr() or None, vals.data_ptr() or None
        job.out_capacity = cap
    job.nnz_sub = C.pointer(kept)
    job.n_empty_rows, job.n_empty_cols = C.pointer(nr), C.pointer(nc)
    job.row_mask, job.col_mask = rm.ctypes.data_as(C.POINTER(C.c_ubyte)), cm.ctypes.data_as(C.POINTER(C.c_ubyte))
    code = lib.resnmtf_fp64_subsample_sparse(int(device_id), C.byref(job))
    if code != _lib.OK:
        raise ResnmtfError(code, (lib.resnmtf_last_error(None) or b"").decode())
    if count_only:
        return int(kept.value), rm.astype(bool), cm.astype(bool)
    k = int(kept.value)
    out = torch.sparse_csc_tensor(ccol, ridx[:k], vals[:k], size=(ns, ms), check_invariants=False)
    return out, rm.astype(bool), cm.astype(bool)


def fp64_relevance(row_c, col_c, true_r, true_c, rows, cols, device_id: int = 0) -> np.ndarray:
    """``relevance_results`` (``R/stability_analysis.r:45-67``) of cluster matrices in device memory
    (``resnmtf_fp64_relevance``, no handle): ``row_c`` (n_sub x k) and ``col_c`` (m_sub x k), the 0 / 1
    clusters of a sub-sample as floating ``torch`` tensors on ``cuda:device_id`` of any strides (what the fp64 run leaves
    with ``output="torch"``; anything else is copied there as fp64), scored against the reference's ``true_r`` (n x k_ref)
    and ``true_c`` (m x k_ref) gathered through ``rows`` / ``cols`` -- each a tensor on the device, read in place, or
    anything NumPy takes.  Returns the k_ref relevance values, bit for bit ``tests/stability_ref.relevance_counts`` of the
    same matrices.  An entry other than 0 / 1 and bad lists are refused (``ResnmtfError``)."""
    import torch
    lib = _lib.load()
    dev = torch.device("cuda", int(device_id))

    def on_device(a):
        return _device_views.is_tensor(a) and _device_views.on_engine_device(a, device_id) and a.dtype.is_floating_point

    keep = []

    def device_side(a, what):
        if not on_device(a):
            a = torch.as_tensor(_device_views.to_numpy(a) if _device_views.is_tensor(a) else np.asarray(a, dtype=np.float64),
                                dtype=torch.float64).to(dev)
            keep.append(a)
        if a.dim() != 2:
            raise ValueError(f"fp64_relevance: {what} must be a matrix")
        return a

    row_c, col_c = device_side(row_c, "row_c"), device_side(col_c, "col_c")
    rows, cols = _index_list(rows, "fp64_relevance: rows"), _index_list(cols, "fp64_relevance: cols")
    ns, ms, k = int(rows.size), int(cols.size), int(row_c.shape[1])
    job = _lib.Fp64RelevanceJob()
    job.struct_size = C.sizeof(job)
    job.row_c = _device_matrix(row_c, (ns, k), device_id, "fp64_relevance: row_c")
    job.col_c = _device_matrix(col_c, (ms, k), device_id, "fp64_relevance: col_c")
    refs = []
    for a, what in ((true_r, "true_r"), (true_c, "true_c")):
        if on_device(a):
            if a.dim() != 2:
                raise ValueError(f"fp64_relevance: {what} must be a matrix")
            refs.append(a)
        else:
            a = _f64_colmajor(_device_views.to_numpy(a) if _device_views.is_tensor(a) else a)
            if a.ndim != 2:
                raise ValueError(f"fp64_relevance: {what} must be a matrix")
            refs.append(a)
    n, m, k_ref = int(refs[0].shape[0]), int(refs[1].shape[0]), int(refs[0].shape[1])
    if int(refs[1].shape[1]) != k_ref:
        raise ValueError("fp64_relevance: true_r and true_c differ in their number of clusters")
    if _device_views.is_tensor(refs[0]):
        job.true_r_dev = _device_matrix(refs[0], (n, k_ref), device_id, "fp64_relevance: true_r")
    else:
        job.true_r = _dp(refs[0])
    if _device_views.is_tensor(refs[1]):
        job.true_c_dev = _device_matrix(refs[1], (m, k_ref), device_id, "fp64_relevance: true_c")
    else:
        job.true_c = _dp(refs[1])
    job.n, job.m, job.n_sub, job.m_sub, job.k, job.k_ref = n, m, ns, ms, k, k_ref
    job.rows, job.cols = _ip(rows), _ip(cols)
    job.stream = torch.cuda.current_stream(dev).cuda_stream
    out = np.zeros(max(k_ref, 1), dtype=np.float64)
    job.relevance = _dp(out)
    code = lib.resnmtf_fp64_relevance(int(device_id), C.byref(job))
    if code != _lib.OK:
        raise ResnmtfError(code, (lib.resnmtf_last_error(None) or b"").decode())
    return out[:k_ref]


def fp64_bisil_plan(n_u: int, n_mem: int, k: int, row_stride: int = 1, col_stride: int = 1) -> dict:
    """How ``fp64_bisil`` launches one side of one bicluster (``resnmtf_fp64_bisil_plan``; no device work): ``{"kq",
    "chunk_tiles", "chunks", "gather": (form of the row side, of the column side)}`` for ``n_u`` points in U, ``n_mem``
    members, ``k`` biclusters and an X with the given strides in elements; a gather form is ``"points"`` (lanes along the
    points, G written directly) or ``"lds"`` (a 32 x 32 tile through LDS, read along the features)."""
    lib = _lib.load()
    out = (C.c_int * _lib.FP64_BISIL_PLAN_INTS)()
    rc = lib.resnmtf_fp64_bisil_plan(int(n_u), int(n_mem), int(k), int(row_stride), int(col_stride), out)
    if rc != _lib.OK:
        raise ResnmtfError(rc, (lib.resnmtf_last_error(None) or b"").decode())
    v = list(out)
    forms = ("points", "lds")
    return {"kq": v[0], "chunk_tiles": v[1], "chunks": v[2], "gather": (forms[v[3]], forms[v[4]])}


def fp64_sparse_plan(x, k: int) -> dict:
    """How ``fp64_run`` streams the sparse view ``x`` (a ``scipy.sparse`` matrix, taken as its canonical CSC) at ``k``
    (``resnmtf_fp64_sparse_plan``; no device work): ``{"kp", "xg": (splits, entries per piece, longest row), "xtf":
    (splits, entries per piece, longest column), "lines_per_wave"}`` -- a function of the structure and k alone.  A
    split count above 1: the lines are cut into that many pieces, summed in piece order."""
    lib = _lib.load()
    c = _sparse.canonical_csc(x)
    ptr = np.ascontiguousarray(c.indptr, dtype=np.int64)
    idx = np.ascontiguousarray(c.indices, dtype=np.int32)
    return _sparse_plan_raw(lib, c.shape[0], c.shape[1], k, ptr, idx)


def _sparse_plan_raw(lib, n_rows: int, n_cols: int, k: int, ptr: np.ndarray, idx: np.ndarray) -> dict:
    out = (C.c_int * _lib.FP64_SPARSE_PLAN_INTS)()
    rc = lib.resnmtf_fp64_sparse_plan(int(n_rows), int(n_cols), int(k), ptr.ctypes.data_as(C.POINTER(C.c_longlong)), _ip(idx), out)
    if rc != _lib.OK:
        raise ResnmtfError(rc, (lib.resnmtf_last_error(None) or b"").decode())
    v = list(out)
    return {"kp": v[0], "xg": tuple(v[1:4]), "xtf": tuple(v[4:7]), "lines_per_wave": v[7]}


def fp64_plan(n_rows: int, n_cols: int, k: int) -> dict:
    """The launch geometry ``fp64_run`` takes for an ``n_rows`` x ``n_cols`` view at ``k`` (``resnmtf_fp64_plan``; no
    device work): ``{"kp", "xg": (row tiles, splits, indices per split), "xtf": ..., "resid": (64-row tiles, column
    splits, columns per split), "ld": (leading dimension of the fp64 image of X, of X^T)}``.  A split count above 1: partial
    products in a slab, summed in split order."""
    lib = _lib.load()
    out = (C.c_int * _lib.FP64_PLAN_INTS)()
    rc = lib.resnmtf_fp64_plan(int(n_rows), int(n_cols), int(k), out)
    if rc != _lib.OK:
        raise ResnmtfError(rc, (lib.resnmtf_last_error(None) or b"").decode())
    v = list(out)
    return {"kp": v[0], "xg": tuple(v[1:4]), "xtf": tuple(v[4:7]), "resid": tuple(v[7:10]), "ld": tuple(v[10:12])}


class Engine:
    def __init__(self, n_rows: Sequence[int], n_cols: Sequence[int], k: Sequence[int],
                 owned: Optional[Sequence[bool]] = None, device_id: int = 0, stream: int = 0,
                 use_graph: bool = True, check_every: int = 32, target_workgroups: int = 0,
                 time_kernels: bool = False, pass_waves: int = 0, pass_splits_xg: int = 0,
                 pass_splits_xtf: int = 0, pass_lds_pad_kb: int = 0, update_blocks: int = 0, no_pitch_pad: bool = False,
                 kk_mode: int = 0, bf16_split: int = 0, replicate_f: bool = False, no_f_chain: bool = False,
                 x_half: int = 0, half_unroll: int = 0, replicate_gs: bool = False, wait_mode: int = 0,
                 slice_chains: bool = False, slice_index: int = 0, slice_count: int = 0, fuse_updates: int = 0, slice_p2p: bool = False, xcd_order: bool = False,
                 nnz: Optional[Sequence[Optional[int]]] = None):
        """``nnz``: per view None (dense) or the number of stored entries a sparse view may hold
        (``resnmtf_create_sparse``; upload with ``set_view_sparse``)."""
        self._lib = _lib.load()
        self.n_views = len(n_rows)
        self.n_rows = [int(x) for x in n_rows]
        self.n_cols = [int(x) for x in n_cols]
        self.k = [int(x) for x in k]
        self.owned = [True] * self.n_views if owned is None else [bool(x) for x in owned]
        self.device_id = int(device_id)
        opts = _lib.Options()
        self._lib.resnmtf_default_options(C.byref(opts))
        opts.device_id = int(device_id)
        opts.stream = C.c_void_p(int(stream)) if stream else None
        opts.use_graph = 1 if use_graph else 0
        opts.check_every = int(check_every)
        opts.target_workgroups = int(target_workgroups)
        opts.time_kernels = 1 if time_kernels else 0
        opts.pass_waves = int(pass_waves)
        opts.pass_splits_xg = int(pass_splits_xg)
        opts.pass_splits_xtf = int(pass_splits_xtf)
        opts.pass_lds_pad_kb = int(pass_lds_pad_kb)
        opts.update_blocks = int(update_blocks)
        opts.no_pitch_pad = 1 if no_pitch_pad else 0
        opts.kk_mode = int(kk_mode)
        opts.bf16_split = int(bf16_split)
        opts.replicate_f = 1 if replicate_f else 0
        opts.no_f_chain = 1 if no_f_chain else 0
        opts.x_half = int(x_half)
        opts.half_unroll = int(half_unroll)
        opts.replicate_gs = 1 if replicate_gs else 0
        opts.wait_mode = int(wait_mode)
        opts.slice_chains = 1 if slice_chains else 0
        opts.slice_index = int(slice_index)
        opts.slice_count = int(slice_count)
        opts.fuse_updates = int(fuse_updates)
        opts.slice_p2p = int(slice_p2p)          # (True = 1: stream waits; 2: wait kernels, graph-capturable)
        opts.xcd_order = 1 if xcd_order else 0
        nr = np.asarray(self.n_rows, dtype=np.int32)
        nc = np.asarray(self.n_cols, dtype=np.int32)
        kk = np.asarray(self.k, dtype=np.int32)
        ow = np.asarray([1 if o else 0 for o in self.owned], dtype=np.int32)
        self._h = C.c_void_p()
        self.sparse = [False] * self.n_views if nnz is None else [x is not None and int(x) >= 0 for x in nnz]
        if any(self.sparse):
            if len(nnz) != self.n_views:
                raise ValueError("nnz must have one entry per view")
            cap = np.asarray([int(x) if s else -1 for x, s in zip(nnz, self.sparse)], dtype=np.int64)
            rc = self._lib.resnmtf_create_sparse(self.n_views, _ip(nr), _ip(nc), _ip(kk), _ip(ow),
                                                 cap.ctypes.data_as(C.POINTER(C.c_longlong)), C.byref(opts), C.byref(self._h))
        else:
            rc = self._lib.resnmtf_create(self.n_views, _ip(nr), _ip(nc), _ip(kk), _ip(ow), C.byref(opts),
                                          C.byref(self._h))
        if rc != _lib.OK:
            text = self._lib.resnmtf_last_error(None)
            self._h = None
            raise ResnmtfError(rc, text.decode() if text else "")

    # ------------------------------------------------------------------ plumbing
    def _check(self, rc: int):
        if rc != _lib.OK:
            text = self._lib.resnmtf_last_error(self._h)
            raise ResnmtfError(rc, text.decode() if text else "")

    def close(self):
        if getattr(self, "_h", None):
            self._lib.resnmtf_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # ------------------------------------------------------------------ inputs
    def set_view(self, v: int, x):
        x = _f64_colmajor(x, (self.n_rows[v], self.n_cols[v]))
        self._check(self._lib.resnmtf_set_view(self._h, v, _dp(x)))

    def set_view_raw(self, v: int, x_raw) -> bool:
        """Upload a raw view; the non-negativity shift and the column normalisation of
        ``check_inputs`` (``R/utils.r:416,422``) run on the device.  Returns True when an entry was
        negative (the reference warns, ``R/utils.r:23-25``)."""
        import ctypes as C
        x = _f64_colmajor(x_raw, (self.n_rows[v], self.n_cols[v]))
        neg = C.c_int(0)
        self._check(self._lib.resnmtf_set_view_raw(self._h, v, _dp(x), C.byref(neg)))
        return bool(neg.value)

    def set_view_device(self, v: int, tensor, raw: bool = False) -> bool:
        """Upload a dense view from device memory (``resnmtf_set_view_device``): ``tensor`` is a 2-D floating
        ``torch.Tensor`` (fp64 / fp32 / fp16 / bf16, any strides) on this engine's GPU; it is read in place, ordered after
        the work enqueued on torch's current stream of that device, and may be freed on return.  ``raw=False`` takes the
        values as ``set_view`` does, ``raw=True`` shifts and normalises them on the device as ``set_view_raw`` does
        (``R/utils.r:416,422``) and returns True when an entry was negative (``R/utils.r:23-25``).  The images,
        ``data_norms`` and the flag are bit for bit those of ``set_view`` / ``set_view_raw`` of
        ``tensor.double().cpu().numpy()``."""
        import torch            # (lazily: nothing else in this module needs it)
        if not isinstance(tensor, torch.Tensor):
            raise TypeError("set_view_device takes a torch.Tensor (host data: set_view / set_view_raw)")
        if tensor.ndim != 2:
            raise ValueError(f"a tensor view must be 2-D, got {tensor.ndim} dimensions")
        codes = {torch.float64: _lib.DTYPE_F64, torch.float32: _lib.DTYPE_F32, torch.float16: _lib.DTYPE_F16,
                 torch.bfloat16: _lib.DTYPE_BF16}
        if tensor.dtype not in codes:
            raise ValueError(f"a tensor view must be fp64, fp32, fp16 or bf16, got {tensor.dtype}")
        if tensor.device.type != "cuda" or tensor.device.index != self.device_id:
            raise ValueError(f"the tensor lives on {tensor.device}, the engine on cuda:{self.device_id}")
        if tuple(tensor.shape) != (self.n_rows[v], self.n_cols[v]):
            raise ValueError(f"expected shape {(self.n_rows[v], self.n_cols[v])}, got {tuple(tensor.shape)}")
        tensor = tensor.detach()
        neg = C.c_int(0)
        stream = torch.cuda.current_stream(tensor.device).cuda_stream
        self._check(self._lib.resnmtf_set_view_device(self._h, v, C.c_void_p(tensor.data_ptr()), codes[tensor.dtype],
                                                      int(tensor.stride(0)), int(tensor.stride(1)), 1 if raw else 0,
                                                      C.byref(neg), C.c_void_p(stream)))
        return bool(neg.value)

    def set_view_sparse(self, v: int, m, pre_processed: bool = False):
        """Upload a sparse view (``scipy.sparse``, any format; a canonical CSC copy is made, ``m`` is not modified) as
        0-based CSC (``resnmtf_set_view_csc``).  ``pre_processed=False``: the column normalisation of ``check_inputs``
        (``R/utils.r:86-88``) runs on the device -- negative entries and all-zero columns are refused; ``True``: the
        values are taken as given (the sub-samples of stability selection)."""
        from . import sparse
        c = sparse.canonical_csc(m)
        if tuple(c.shape) != (self.n_rows[v], self.n_cols[v]):
            raise ValueError(f"expected shape {(self.n_rows[v], self.n_cols[v])}, got {tuple(c.shape)}")
        col_ptr = np.ascontiguousarray(c.indptr, dtype=np.int64)
        row_idx = np.ascontiguousarray(c.indices, dtype=np.int32)
        vals = np.ascontiguousarray(c.data, dtype=np.float64)
        if row_idx.size == 0:               # (never a NULL pointer)
            row_idx = np.zeros(1, dtype=np.int32); vals = np.zeros(1)
        self._check(self._lib.resnmtf_set_view_csc(self._h, v, col_ptr.ctypes.data_as(C.POINTER(C.c_longlong)),
                                                   _ip(row_idx), _dp(vals), 1 if pre_processed else 0))

    def set_view_sparse_device(self, v: int, tensor, pre_processed: bool = False):
        """Upload a sparse view from device memory (``resnmtf_set_view_sparse_device``): ``tensor`` is a 2-D ``torch``
        tensor of layout ``sparse_csc``, ``sparse_csr`` or (coalesced) ``sparse_coo`` on this engine's GPU, floating values
        (fp64 / fp32 / fp16 / bf16), int32 or int64 indices, its entries in any order.  Its arrays are read in place,
        ordered after the work enqueued on torch's current stream of that device, checked on the device (a refusal raises
        ``ResnmtfError`` and leaves the view as it was) and may be freed on return.  ``pre_processed`` as for
        ``set_view_sparse``.  The view is bit for bit the one ``resnmtf_set_view_csc`` makes of the canonical CSC of the
        same values widened to fp64 (explicit zeros stay stored)."""
        import torch            # (lazily: nothing else in this module needs it)
        from . import device_views
        if not isinstance(tensor, torch.Tensor):
            raise TypeError("set_view_sparse_device takes a sparse torch.Tensor (host data: set_view_sparse)")
        device_views.check_sparse_tensor(tensor, "set_view_sparse_device")
        layouts = {torch.sparse_csc: _lib.SPARSE_CSC, torch.sparse_csr: _lib.SPARSE_CSR, torch.sparse_coo: _lib.SPARSE_COO}
        codes = {torch.float64: _lib.DTYPE_F64, torch.float32: _lib.DTYPE_F32, torch.float16: _lib.DTYPE_F16,
                 torch.bfloat16: _lib.DTYPE_BF16}
        if tensor.dtype not in codes:
            raise ValueError(f"a tensor view must be fp64, fp32, fp16 or bf16, got {tensor.dtype}")
        if tuple(tensor.shape) != (self.n_rows[v], self.n_cols[v]):
            raise ValueError(f"expected shape {(self.n_rows[v], self.n_cols[v])}, got {tuple(tensor.shape)}")
        if tensor.device.type != "cuda" or tensor.device.index != self.device_id:
            raise ValueError(f"the tensor lives on {tensor.device}, the engine on cuda:{self.device_id}")
        tensor = tensor.detach()
        # (.contiguous() only where a piece is not: the rows of a COO index matrix are, a sliced tensor's pieces may not be)
        a, b, vals = (x if x.is_contiguous() else x.contiguous() for x in device_views.sparse_tensor_parts(tensor))
        index_type = _lib.INDEX_I64 if a.dtype == torch.int64 else _lib.INDEX_I32
        stream = torch.cuda.current_stream(tensor.device).cuda_stream
        self._check(self._lib.resnmtf_set_view_sparse_device(
            self._h, v, layouts[tensor.layout], C.c_void_p(a.data_ptr()), C.c_void_p(b.data_ptr()), index_type,
            C.c_void_p(vals.data_ptr()), codes[tensor.dtype], int(tensor._nnz()), 1 if pre_processed else 0, C.c_void_p(stream)))

    def view_storage(self, v: int):
        """(is_sparse, nnz of the last upload, nnz capacity) of view ``v`` (``resnmtf_view_storage``)."""
        sp, nz, cap = C.c_int(0), C.c_longlong(0), C.c_longlong(0)
        self._check(self._lib.resnmtf_view_storage(self._h, v, C.byref(sp), C.byref(nz), C.byref(cap)))
        return bool(sp.value), int(nz.value), int(cap.value)

    def copy_view_from(self, v: int, other: "Engine", v_src: int = 0):
        """Device copy of a view another engine (same GPU, same shape) has uploaded."""
        self._check(self._lib.resnmtf_copy_view(self._h, v, other._h, v_src))

    def shuffle_view_from(self, v: int, other: "Engine", v_src: int = 0, seed: int = 0, normalise: bool = True):
        """``shuffle_view`` (``R/obtain_bicl.r:11-22``) of another engine's view, drawn on the device."""
        self._check(self._lib.resnmtf_shuffle_view(self._h, v, other._h, v_src, int(seed), 1 if normalise else 0))

    def shuffle_view_sparse_from(self, v: int, other: "Engine", v_src: int = 0, seed: int = 0, normalise: bool = True):
        """``shuffle_view`` (``R/obtain_bicl.r:11-22``) of another engine's SPARSE view into this engine's sparse view
        ``v`` (``resnmtf_shuffle_view_sparse``): the draw ``shuffle_view_from`` makes of the densified view for the same
        seed, from the stored entries alone; the shuffle stays sparse."""
        self._check(self._lib.resnmtf_shuffle_view_sparse(self._h, v, other._h, v_src, int(seed), 1 if normalise else 0))

    def _index_lists(self, rows, cols, v=None, vectors=True):
        """``rows`` / ``cols`` as contiguous int32 arrays.  ``v``: their counts must equal the shape of this engine's view
        ``v`` (``vectors``: and they must be 1-D); ``None``: they only have to be vectors."""
        rows = np.ascontiguousarray(rows, dtype=np.int32); cols = np.ascontiguousarray(cols, dtype=np.int32)
        flat = rows.ndim == 1 and cols.ndim == 1
        if v is None:
            if not flat:
                raise ValueError("rows and cols must be vectors")
        elif (vectors and not flat) or len(rows) != self.n_rows[v] or len(cols) != self.n_cols[v]:
            raise ValueError("index counts must equal the view's shape")
        return rows, cols

    def subsample_count_sparse(self, v: int, rows, cols) -> int:
        """The number of stored entries of ``X[rows, cols]`` of this engine's sparse view ``v``
        (``resnmtf_subsample_count_sparse``): the ``nnz`` an engine needs to receive that sub-sample
        (``subsample_view_sparse_from``).  Nothing is built."""
        rows, cols = self._index_lists(rows, cols)
        nnz = C.c_longlong(0)
        # (never a NULL pointer for an empty list)
        r = rows if rows.size else np.zeros(1, dtype=np.int32); c = cols if cols.size else np.zeros(1, dtype=np.int32)
        self._check(self._lib.resnmtf_subsample_count_sparse(self._h, v, int(rows.size), _ip(r), int(cols.size), _ip(c),
                                                             C.byref(nnz)))
        return int(nnz.value)

    def subsample_view_sparse_from(self, v: int, other: "Engine", v_src: int, rows, cols):
        """The sub-sample ``X[rows, cols]`` of another engine's SPARSE view (``R/stability_analysis.r:230-249``) into
        this engine's sparse view ``v`` (``resnmtf_subsample_view_sparse``), gathered on the device from the stored
        entries; the view must have the shape ``(len(rows), len(cols))`` and room for ``other.subsample_count_sparse``
        entries.  The lists come in any order, without repeats; the values are not re-normalised."""
        rows, cols = self._index_lists(rows, cols, v, vectors=False)
        self._check(self._lib.resnmtf_subsample_view_sparse(self._h, v, other._h, v_src, _ip(rows), _ip(cols)))

    def copy_view_sparse_from(self, v: int, other: "Engine", v_src: int = 0):
        """Device copy of a SPARSE view another engine (same GPU, same shape, any k) has uploaded
        (``resnmtf_copy_view_sparse``); the passes are planned for this engine's k."""
        self._check(self._lib.resnmtf_copy_view_sparse(self._h, v, other._h, v_src))

    def get_view_sparse(self, v: int):
        """The device CSC copy of sparse view ``v`` (``resnmtf_get_view_csc``; fp32 precision, explicit zeros kept) as a
        ``scipy.sparse.csc_matrix``.  A dense view is refused (``get_view``)."""
        import scipy.sparse as sp
        nnz = self.view_storage(v)[1]
        col_ptr = np.zeros(self.n_cols[v] + 1, dtype=np.int64)
        row_idx = np.zeros(max(nnz, 1), dtype=np.int32); vals = np.zeros(max(nnz, 1))
        self._check(self._lib.resnmtf_get_view_csc(self._h, v, col_ptr.ctypes.data_as(C.POINTER(C.c_longlong)), _ip(row_idx),
                                                   _dp(vals)))
        return sp.csc_matrix((vals[:nnz], row_idx[:nnz], col_ptr), shape=(self.n_rows[v], self.n_cols[v]))

    def subsample_view_from(self, v: int, other: "Engine", v_src: int, rows, cols):
        """The sub-sample ``X[rows, cols]`` of another engine's view (``R/stability_analysis.r:230-249``), gathered
        on the device; this engine's view v must have the shape ``(len(rows), len(cols))``."""
        rows, cols = self._index_lists(rows, cols, v, vectors=False)
        self._check(self._lib.resnmtf_subsample_view(self._h, v, other._h, v_src, _ip(rows), _ip(cols)))

    def empty_lines(self, v: int, counts: bool = False):
        """(row_mask, col_mask) of view ``v``'s latest device-drawn data (shuffle / sub-sample): True where a row / column
        sums to exactly zero -- the condition of the reference's redraw (``R/obtain_bicl.r:14-18``) and of its trimming
        of sub-samples (``R/stability_analysis.r:165-190``).  ``counts=True``: ``(row_mask, col_mask, n_empty_rows,
        n_empty_cols)``, the counts as the device took them."""
        nr, nc = C.c_int(0), C.c_int(0)
        rm = np.zeros(self.n_rows[v], dtype=np.uint8); cm = np.zeros(self.n_cols[v], dtype=np.uint8)
        self._check(self._lib.resnmtf_view_empty_lines(self._h, v, C.byref(nr), C.byref(nc),
                                                       rm.ctypes.data_as(C.POINTER(C.c_ubyte)), cm.ctypes.data_as(C.POINTER(C.c_ubyte))))
        if counts:
            return rm.astype(bool), cm.astype(bool), int(nr.value), int(nc.value)
        return rm.astype(bool), cm.astype(bool)

    def get_view(self, v: int) -> np.ndarray:
        """The device copy of the view's data (fp32 precision) as an fp64 matrix."""
        x = np.zeros((self.n_rows[v], self.n_cols[v]), order="F")
        self._check(self._lib.resnmtf_get_view(self._h, v, _dp(x)))
        return x

    def get_view_device(self, v: int, dtype=None, order: str = "C", out=None):
        """``get_view`` with the data left on the device (``resnmtf_get_view_device``): a ``torch`` tensor on this engine's
        GPU, ``dtype`` fp32 (default: the stored image, kept) or fp64 (widened exactly), row-major (``order="C"``) or
        column-major (``"F"``); bitwise the values ``get_view`` returns.  ``out=``: any 2-D fp32 / fp64 tensor of the
        view's shape on this GPU whose strides put no two elements on one address (a slice or transpose of a larger
        tensor included; ``device_views.check_readback_strides``) is written in place and returned; ``dtype`` and
        ``order`` are then not read.  Ordered with torch's current stream of that device.  A sparse view is refused
        (``get_view_sparse_device``)."""
        import torch            # (lazily: nothing else in this module needs it)
        from . import device_views
        n, m = self.n_rows[v], self.n_cols[v]
        dev = torch.device("cuda", self.device_id)
        codes = {torch.float64: _lib.DTYPE_F64, torch.float32: _lib.DTYPE_F32}
        if out is None:
            dtype = torch.float32 if dtype is None else dtype
            if dtype not in codes:
                raise ValueError(f"get_view_device returns fp32 or fp64 (narrowing is not a copy), got {dtype}")
            if order not in ("C", "F"):
                raise ValueError("order must be 'C' or 'F'.")
            out = torch.empty((n, m), dtype=dtype, device=dev) if order == "C" else torch.empty((m, n), dtype=dtype, device=dev).T
        else:
            if not isinstance(out, torch.Tensor):
                raise TypeError("out must be a torch.Tensor (host data: get_view)")
            if out.dtype not in codes:
                raise ValueError(f"out must be fp32 or fp64 (narrowing is not a copy), got {out.dtype}")
            if out.ndim != 2 or tuple(out.shape) != (n, m):
                raise ValueError(f"expected shape {(n, m)}, got {tuple(out.shape)}")
            if out.device.type != "cuda" or out.device.index != self.device_id:
                raise ValueError(f"out lives on {out.device}, the engine on cuda:{self.device_id}")
            device_views.check_readback_strides(out.shape, out.stride())
        stream = torch.cuda.current_stream(dev).cuda_stream
        self._check(self._lib.resnmtf_get_view_device(self._h, v, C.c_void_p(out.data_ptr()), codes[out.dtype],
                                                      int(out.stride(0)), int(out.stride(1)), C.c_void_p(stream)))
        return out

    def get_view_sparse_device(self, v: int, layout: str = "csc", index_dtype=None, dtype=None):
        """``get_view_sparse`` with the data left on the device (``resnmtf_get_view_sparse_device``): sparse view ``v`` as
        a ``torch.sparse_csc_tensor`` (``layout="csc"``: bitwise the arrays ``get_view_sparse`` returns, explicit zeros
        kept), ``sparse_csr_tensor`` (``"csr"``: columns ascending within a row) or ``sparse_coo_tensor`` (``"coo"``:
        row-major sorted, built with ``is_coalesced=True``) on this engine's GPU, indices int64 (default) or int32 (a COO
        tensor holds int64 indices whatever it is given: torch widens them), values fp32 (default) or fp64.  Ordered with torch's current stream of that device.  A dense view is refused
        (``get_view_device``)."""
        import torch            # (lazily: nothing else in this module needs it)
        layouts = {"csc": _lib.SPARSE_CSC, "csr": _lib.SPARSE_CSR, "coo": _lib.SPARSE_COO}
        if layout not in layouts:
            raise ValueError("layout must be 'csc', 'csr' or 'coo'.")
        index_dtype = torch.int64 if index_dtype is None else index_dtype
        dtype = torch.float32 if dtype is None else dtype
        if index_dtype not in (torch.int32, torch.int64):
            raise ValueError(f"index_dtype must be int32 or int64, got {index_dtype}")
        codes = {torch.float64: _lib.DTYPE_F64, torch.float32: _lib.DTYPE_F32}
        if dtype not in codes:
            raise ValueError(f"get_view_sparse_device returns fp32 or fp64 values (narrowing is not a copy), got {dtype}")
        n, m = self.n_rows[v], self.n_cols[v]
        sparse_view, nnz, _ = self.view_storage(v)
        if not sparse_view:
            nnz = 0                 # (the library refuses the dense view below, before it writes anything)
        dev = torch.device("cuda", self.device_id)
        a = torch.empty(nnz if layout == "coo" else (m if layout == "csc" else n) + 1, dtype=index_dtype, device=dev)
        b = torch.empty(nnz, dtype=index_dtype, device=dev)
        vals = torch.empty(nnz, dtype=dtype, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        # (an empty tensor has no allocation: NULL = skipped)
        ptrs = [C.c_void_p(t.data_ptr()) if t.numel() else None for t in (a, b, vals)]
        self._check(self._lib.resnmtf_get_view_sparse_device(
            self._h, v, layouts[layout], ptrs[0], ptrs[1], _lib.INDEX_I64 if index_dtype == torch.int64 else _lib.INDEX_I32,
            ptrs[2], codes[dtype], C.c_void_p(stream)))
        if layout == "csc":
            return torch.sparse_csc_tensor(a, b, vals, size=(n, m))
        if layout == "csr":
            return torch.sparse_csr_tensor(a, b, vals, size=(n, m))
        return torch.sparse_coo_tensor(torch.stack((a, b)), vals, size=(n, m), is_coalesced=True)

    def init_svd(self, v: int, seed: int = 0, sigma: float = 0.05, n_power: int = 0, return_basis: bool = False):
        """``init_mats_inner`` (``R/update_steps.r:78-125``) on the device for view ``v`` (randomized
        top-k SVD on the streaming-pass kernels); returns the k leading singular values.
        ``return_basis=True`` (``resnmtf_init_svd_basis``): ``(d, U, V, d_all)`` -- the signed vectors the factors are
        built from, n x k and m x k, and every singular value the route computed, descending; same factors."""
        d = np.zeros(self.k[v])
        if not return_basis:
            self._check(self._lib.resnmtf_init_svd(self._h, v, int(seed), float(sigma), int(n_power), _dp(d)))
            return d
        u = np.zeros((self.n_rows[v], self.k[v]), order="F"); w = np.zeros((self.n_cols[v], self.k[v]), order="F")
        d_all = np.zeros(64); n_d = C.c_int(0)
        self._check(self._lib.resnmtf_init_svd_basis(self._h, v, int(seed), float(sigma), int(n_power), _dp(d), _dp(u), _dp(w),
                                                     _dp(d_all), C.byref(n_d)))
        return d, u, w, d_all[:n_d.value].copy()

    def set_factors(self, v: int, f, s, g, lam=None, mu=None):
        k = self.k[v]
        f = _f64_colmajor(f, (self.n_rows[v], k))
        s = _f64_colmajor(s, (k, k))
        g = _f64_colmajor(g, (self.n_cols[v], k))
        lam = None if lam is None else np.ascontiguousarray(lam, dtype=np.float64)
        mu = None if mu is None else np.ascontiguousarray(mu, dtype=np.float64)
        self._check(self._lib.resnmtf_set_factors(self._h, v, _dp(f), _dp(s), _dp(g), _dp(lam), _dp(mu)))

    def set_factors_device(self, v: int, f, s, g, lam=None, mu=None):
        """``set_factors`` from device memory (``resnmtf_set_factors_device``, ``R/update_steps.r:41-56``): ``f`` (n x k),
        ``s`` (k x k) and ``g`` (m x k) are 2-D floating ``torch`` tensors (fp64 / fp32 / fp16 / bf16, one dtype each, any
        strides) on this engine's GPU, read in place, ordered after the work enqueued on torch's current stream of that
        device; they may be freed on return.  ``lam`` / ``mu``: ``None`` (the column sums of ``f`` / ``g``, summed on the
        device in ``set_factors``' order) or k values -- a 1-D tensor on that GPU, made contiguous, or anything NumPy takes,
        moved there.  The view's factor state is bit for bit what ``set_factors`` of
        ``t.double().cpu().numpy()`` leaves."""
        import torch            # (lazily: nothing else in this module needs it)
        n, m, k = self.n_rows[v], self.n_cols[v], self.k[v]
        dev = torch.device("cuda", self.device_id)
        codes = {torch.float64: _lib.DTYPE_F64, torch.float32: _lib.DTYPE_F32, torch.float16: _lib.DTYPE_F16,
                 torch.bfloat16: _lib.DTYPE_BF16}

        def check(t, name, shape):
            if not isinstance(t, torch.Tensor):
                raise TypeError(f"set_factors_device takes torch.Tensors, {name} is a {type(t).__name__} (host factors: set_factors)")
            if t.dtype not in codes:
                raise ValueError(f"{name} must be fp64, fp32, fp16 or bf16, got {t.dtype}")
            if t.device.type != "cuda" or t.device.index != self.device_id:
                raise ValueError(f"{name} lives on {t.device}, the engine on cuda:{self.device_id}")
            if tuple(t.shape) != tuple(shape):
                raise ValueError(f"{name}: expected shape {tuple(shape)}, got {tuple(t.shape)}")
            return t.detach()

        mats = [check(t, name, shape) for t, name, shape in ((f, "f", (n, k)), (s, "s", (k, k)), (g, "g", (m, k)))]
        descs = [_lib.DeviceMatrix(t.data_ptr(), codes[t.dtype], int(t.stride(0)), int(t.stride(1))) for t in mats]
        for vec, name in ((lam, "lam"), (mu, "mu")):
            if vec is None:
                descs.append(None)
                continue
            if not isinstance(vec, torch.Tensor):
                vec = torch.as_tensor(np.ascontiguousarray(vec, dtype=np.float64), device=dev)
            vec = check(vec, name, (k,)).contiguous()
            mats.append(vec)            # (kept alive until the call returns)
            descs.append(_lib.DeviceMatrix(vec.data_ptr(), codes[vec.dtype], 1, 1))
        stream = torch.cuda.current_stream(dev).cuda_stream
        self._check(self._lib.resnmtf_set_factors_device(self._h, v, *(None if d is None else C.byref(d) for d in descs),
                                                         C.c_void_p(stream)))

    def set_restrictions(self, phi=None, xi=None, psi=None):
        mats = []
        for m in (phi, xi, psi):
            mats.append(None if m is None else _f64_colmajor(m, (self.n_views, self.n_views)))
        self._check(self._lib.resnmtf_set_restrictions(self._h, _dp(mats[0]), _dp(mats[1]), _dp(mats[2])))

    def _set_shared(self, fn, v, w, idx_v, idx_w):
        if idx_v is None:           # NA
            self._check(fn(self._h, v, w, -1, None, None))
            return
        iv = np.ascontiguousarray(idx_v, dtype=np.int32)
        iw = np.ascontiguousarray(idx_w, dtype=np.int32)
        if iv.shape != iw.shape:
            raise ValueError("index arrays differ in length")
        self._check(fn(self._h, v, w, int(iv.size), _ip(iv), _ip(iw)))

    def set_shared_rows(self, v: int, w: int, idx_v, idx_w):
        self._set_shared(self._lib.resnmtf_set_shared_rows, v, w, idx_v, idx_w)

    def set_shared_cols(self, v: int, w: int, idx_v, idx_w):
        self._set_shared(self._lib.resnmtf_set_shared_cols, v, w, idx_v, idx_w)

    # ------------------------------------------------------------------ loop
    def run(self, n_iters: Optional[int] = None, tol: float = 1.0e-6, max_iters: int = 100000):
        """Fixed ``n_iters`` sweeps, or (``n_iters=None``) until |d mean err| <= tol.
        Returns the All_Error vector of the sweeps executed."""
        if n_iters is not None and n_iters <= 0:
            raise ValueError("n_iters must be positive (None = run to convergence)")
        cap = int(n_iters) if n_iters else int(max_iters)
        buf = self.__dict__.get("_err_buf")
        if buf is None or buf[0].size < cap:            # (kept across calls: a short run is a few hundred microseconds)
            arr = np.empty(max(cap, 1024), dtype=np.float64)
            buf = self._err_buf = (arr, arr.ctypes.data_as(C.POINTER(C.c_double)), C.c_int(0))
        errs, ptr, done = buf
        rc = self._lib.resnmtf_run(self._h, int(n_iters or 0), float(tol), int(max_iters), ptr, cap, C.byref(done))
        if rc != _lib.OK:
            self._check(rc)
        return errs[:done.value].copy()

    def reserve_sweeps(self, sweeps: int):
        self._check(self._lib.resnmtf_reserve_sweeps(self._h, int(sweeps)))

    def prepare(self):
        self._check(self._lib.resnmtf_prepare(self._h))

    def phase(self, v: int, phase: int, sweep: int):
        self._check(self._lib.resnmtf_phase(self._h, v, phase, sweep))

    def synchronize(self):
        self._check(self._lib.resnmtf_synchronize(self._h))

    def factor_device_ptr(self, v: int, which: int):
        ptr = C.c_void_p()
        nbytes = C.c_size_t()
        self._check(self._lib.resnmtf_factor_device_ptr(self._h, v, which, C.byref(ptr), C.byref(nbytes)))
        return int(ptr.value), int(nbytes.value)

    def view_errors(self, v: int, first: int, count: int) -> np.ndarray:
        out = np.zeros(count, dtype=np.float64)
        self._check(self._lib.resnmtf_view_errors(self._h, v, first, count, _dp(out)))
        return out

    # ------------------------------------------------------------------ outputs
    def get_factors(self, v: int, with_lm: bool = True):
        n, m, k = self.n_rows[v], self.n_cols[v], self.k[v]
        f = np.zeros((n, k), order="F"); s = np.zeros((k, k), order="F"); g = np.zeros((m, k), order="F")
        lam = np.zeros(k) if with_lm else None
        mu = np.zeros(k) if with_lm else None
        self._check(self._lib.resnmtf_get_factors(self._h, v, _dp(f), _dp(s), _dp(g), _dp(lam), _dp(mu)))
        return f, s, g, lam, mu

    def get_factors_device(self, v: int, with_lm: bool = True):
        """``get_factors`` with the raw state left on the device (``resnmtf_get_factors_device``): fp64 ``torch`` tensors
        on this engine's GPU, F, S and G column-major (``torch.empty((k, n)).T``), bitwise what ``get_factors`` returns;
        ordered with torch's current stream of that device.  ``with_lm=False``: lambda and mu are ``None``."""
        import torch            # (lazily: nothing else in this module needs it)
        n, m, k = self.n_rows[v], self.n_cols[v], self.k[v]
        dev = torch.device("cuda", self.device_id)
        f, s, g = (torch.empty((cols, rows), dtype=torch.float64, device=dev).T for rows, cols in ((n, k), (k, k), (m, k)))
        lam = torch.empty(k, dtype=torch.float64, device=dev) if with_lm else None
        mu = torch.empty(k, dtype=torch.float64, device=dev) if with_lm else None
        stream = torch.cuda.current_stream(dev).cuda_stream
        self._check(self._lib.resnmtf_get_factors_device(
            self._h, v, *(None if t is None else C.c_void_p(t.data_ptr()) for t in (f, s, g, lam, mu)), C.c_void_p(stream)))
        return f, s, g, lam, mu

    def finalise(self, v: int):
        n, m, k = self.n_rows[v], self.n_cols[v], self.k[v]
        f = np.zeros((n, k), order="F"); s = np.zeros((k, k), order="F"); g = np.zeros((m, k), order="F")
        rc = np.zeros((n, k), order="F"); cc = np.zeros((m, k), order="F")
        self._check(self._lib.resnmtf_finalise(self._h, v, _dp(f), _dp(s), _dp(g), _dp(rc), _dp(cc)))
        return f, s, g, rc, cc

    def finalise_device(self, v: int):
        """``finalise`` with the five results left on the device (``resnmtf_finalise_device``): fp64 ``torch`` tensors
        on this engine's GPU, column-major (``torch.empty((k, n)).T``), bitwise what ``finalise`` returns; ordered with
        torch's current stream of that device."""
        import torch            # (lazily: nothing else in this module needs it)
        n, m, k = self.n_rows[v], self.n_cols[v], self.k[v]
        dev = torch.device("cuda", self.device_id)
        f, s, g, rc, cc = (torch.empty((cols, rows), dtype=torch.float64, device=dev).T
                           for rows, cols in ((n, k), (k, k), (m, k), (n, k), (m, k)))
        stream = torch.cuda.current_stream(dev).cuda_stream
        self._check(self._lib.resnmtf_finalise_device(self._h, v, *(C.c_void_p(t.data_ptr()) for t in (f, s, g, rc, cc)),
                                                      C.c_void_p(stream)))
        return f, s, g, rc, cc

    def set_reference_clusters(self, v: int, rc, cc):
        """The original result's binary clusters of view ``v`` (n x k and m x k, 0 / 1; k may differ from this engine's
        k[v]), kept on the device for ``relevance`` calls of the sub-samples' engines (``stability_check``,
        ``R/stability_analysis.r:268-276``)."""
        rc = np.asfortranarray(np.asarray(rc, dtype=np.float64))
        if rc.ndim != 2 or rc.shape[0] != self.n_rows[v]:
            raise ValueError(f"row clusters must be {self.n_rows[v]} x k")
        cc = _f64_colmajor(cc, (self.n_cols[v], rc.shape[1]))
        self._check(self._lib.resnmtf_set_reference_clusters(self._h, v, int(rc.shape[1]), _dp(rc), _dp(cc)))

    def set_reference_clusters_device(self, v: int, rc, cc):
        """``set_reference_clusters`` from device memory (``resnmtf_set_reference_clusters_device``): ``rc`` (n x k) and
        ``cc`` (m x k) are 2-D floating ``torch`` tensors (fp64 / fp32 / fp16 / bf16, any strides) of 0 / 1 on this
        engine's GPU -- ``finalise_device``'s cluster matrices as they come --, read in place, ordered after the work
        enqueued on torch's current stream of that device, checked on the device (an entry other than 0 or 1 raises
        ``ResnmtfError`` and leaves the earlier reference clusters in place).  ``relevance`` / ``relevance_masked`` then
        return the bits they return after ``set_reference_clusters`` of the same values."""
        import torch            # (lazily: nothing else in this module needs it)
        codes = {torch.float64: _lib.DTYPE_F64, torch.float32: _lib.DTYPE_F32, torch.float16: _lib.DTYPE_F16,
                 torch.bfloat16: _lib.DTYPE_BF16}
        for t, name in ((rc, "rc"), (cc, "cc")):
            if not isinstance(t, torch.Tensor):
                raise TypeError(f"set_reference_clusters_device takes torch.Tensors, {name} is a {type(t).__name__} "
                                "(host matrices: set_reference_clusters)")
            if t.dtype not in codes:
                raise ValueError(f"{name} must be fp64, fp32, fp16 or bf16, got {t.dtype}")
            if t.device.type != "cuda" or t.device.index != self.device_id:
                raise ValueError(f"{name} lives on {t.device}, the engine on cuda:{self.device_id}")
        if rc.ndim != 2 or rc.shape[0] != self.n_rows[v]:
            raise ValueError(f"row clusters must be {self.n_rows[v]} x k")
        if tuple(cc.shape) != (self.n_cols[v], rc.shape[1]):
            raise ValueError(f"expected shape {(self.n_cols[v], rc.shape[1])}, got {tuple(cc.shape)}")
        rc, cc = rc.detach(), cc.detach()
        descs = [_lib.DeviceMatrix(t.data_ptr(), codes[t.dtype], int(t.stride(0)), int(t.stride(1))) for t in (rc, cc)]
        stream = torch.cuda.current_stream(torch.device("cuda", self.device_id)).cuda_stream
        self._check(self._lib.resnmtf_set_reference_clusters_device(self._h, v, int(rc.shape[1]), C.byref(descs[0]),
                                                                    C.byref(descs[1]), C.c_void_p(stream)))

    def relevance(self, v: int, ref_engine: "Engine", v_ref: int, rows, cols) -> np.ndarray:
        """``relevance_results`` (``R/stability_analysis.r:45-67``) of this engine's view ``v`` (its current factors,
        clustered as ``finalise`` would) against the clusters set on ``ref_engine``'s view ``v_ref``, gathered by
        ``rows`` / ``cols`` (0-based, one per row / column of view ``v``): k relevance values, computed on the device."""
        rows, cols = self._index_lists(rows, cols, v)
        out = np.zeros(self.k[v], dtype=np.float64)
        self._check(self._lib.resnmtf_relevance(self._h, v, ref_engine._h, v_ref, _ip(rows), _ip(cols), _dp(out)))
        return out

    def relevance_masked(self, v: int, ref_engine: "Engine", v_ref: int, rows, cols, flags) -> np.ndarray:
        """``relevance`` after a spurious-bicluster removal (``resnmtf_relevance_masked``): ``flags`` holds k[v] booleans
        indexed by F column (the removal rule of ``R/obtain_bicl.r:176-188``); the cluster columns ``j`` with
        ``flags[relations[j]]`` are zeroed on the device, through its own ``relations``, before the counting."""
        rows, cols = self._index_lists(rows, cols, v)
        fl = np.ascontiguousarray(np.asarray(flags, dtype=bool).astype(np.uint8))
        if fl.shape != (self.k[v],):
            raise ValueError(f"flags must hold k = {self.k[v]} entries")
        out = np.zeros(self.k[v], dtype=np.float64)
        self._check(self._lib.resnmtf_relevance_masked(self._h, v, ref_engine._h, v_ref, _ip(rows), _ip(cols),
                                                       fl.ctypes.data_as(C.POINTER(C.c_ubyte)), _dp(out)))
        return out

    def spurious_scores(self, v: int, shuffles: Sequence["Engine"]):
        """``check_biclusters`` / ``get_thresholds`` (``R/obtain_bicl.r:80-133``) of view ``v`` against the same view of
        the ``shuffles`` engines (R shuffled factorisations with this engine's n and k), on the device
        (``resnmtf_spurious_scores``): returns ``(score, null)`` -- the k[v] scores (means in NumPy's order) and the
        k^2 R (R - 1) / 2 null scores in ``calculate_f_shuffle_jsd``'s order.  No factor is downloaded."""
        R = len(shuffles)
        hs = (C.c_void_p * max(1, R))(*[s._h for s in shuffles])
        k = self.k[v] if 0 <= v < self.n_views else 0          # (a bad view is refused by the library)
        score = np.zeros(max(1, k), dtype=np.float64)
        null = np.zeros(max(1, k * k * R * (R - 1) // 2), dtype=np.float64)
        self._check(self._lib.resnmtf_spurious_scores(self._h, v, hs, R, _dp(score), _dp(null)))
        return score[:k], null[:k * k * R * (R - 1) // 2]

    def bisil(self, v: int, rc, cc, distance: str = "euclidean"):
        """The per-member silhouettes of view ``v``'s biclusters (``resnmtf_bisil``, the device side of
        ``bisilhouette::bisilhouette``, ``R/obtain_bicl.r:189-199``) on the view's device copy of the data: ``rc`` /
        ``cc`` are n x k and m x k 0 / 1 cluster matrices (k may differ from this engine's k[v]); returns ``(row_sil,
        col_sil)``, n x k and m x k, 0 at non-members.  ``bisil.score`` turns them into the score."""
        return self._bisil(self._lib.resnmtf_bisil, v, rc, cc, distance)

    def bisil_sparse(self, v: int, rc, cc, distance: str = "euclidean"):
        """``bisil`` for a sparse view (``resnmtf_bisil_sparse``): the same arguments and result, computed from the
        view's CSC / CSR copies -- bitwise what ``bisil`` returns on a dense view holding the same fp32 values.  A
        dense view is refused (use ``bisil``)."""
        return self._bisil(self._lib.resnmtf_bisil_sparse, v, rc, cc, distance)

    def bisil_device(self, v: int, rc, cc, distance: str = "euclidean", *, silhouettes: bool = True, out=None):
        """``bisil`` / ``bisil_sparse`` from device memory, and the view's score with them (``resnmtf_bisil_device``):
        ``rc`` (n x k) and ``cc`` (m x k) are 2-D floating ``torch`` tensors (fp64 / fp32 / fp16 / bf16, any strides) of
        0 / 1 on this engine's GPU -- ``finalise_device``'s cluster matrices as they come --, read in place, ordered after
        the work enqueued on torch's current stream of that device and checked on the device (an entry other than 0 or 1
        raises ``ResnmtfError``).  A dense view and a sparse one alike.  Returns ``(row_sil, col_sil, score)``: the
        silhouettes as fp64 column-major tensors on that GPU, bitwise what ``bisil`` / ``bisil_sparse`` return, and
        ``score == bisil.view_score(rc, cc, row_sil, col_sil)``, combined on the device.  ``silhouettes=False``: only
        the score; ``row_sil`` and ``col_sil`` are ``None``.  ``out=(row_sil, col_sil)``: two fp64 column-major tensors
        of the cluster matrices' shapes on this GPU to write into (a refusal leaves them untouched)."""
        import torch            # (lazily: nothing else in this module needs it)
        from . import device_views
        from .bisil import METRICS
        if distance not in METRICS:
            raise ValueError("distance must be one of 'euclidean', 'manhattan' or 'cosine'.")
        n, m = self.n_rows[v], self.n_cols[v]
        rc, cc, k = device_views.check_cluster_tensors(rc, cc, n, m, self.device_id, "bisil_device")
        codes = {torch.float64: _lib.DTYPE_F64, torch.float32: _lib.DTYPE_F32, torch.float16: _lib.DTYPE_F16,
                 torch.bfloat16: _lib.DTYPE_BF16}
        dev = torch.device("cuda", self.device_id)
        rs = cs = None
        if out is not None:
            if not silhouettes:
                raise ValueError("out= needs silhouettes=True")
            rs, cs = out
            for t, shape, name in ((rs, (n, k), "out[0]"), (cs, (m, k), "out[1]")):
                if not device_views.on_engine_device(t, self.device_id) or t.dtype != torch.float64:
                    raise ValueError(f"bisil_device: {name} must be an fp64 tensor on cuda:{self.device_id}")
                if tuple(t.shape) != shape or (k > 0 and (t.stride(0) != 1 or (k > 1 and t.stride(1) != shape[0]))):
                    raise ValueError(f"bisil_device: {name} must be a column-major {shape} tensor")
        elif silhouettes:
            rs, cs = (torch.empty((k, rows), dtype=torch.float64, device=dev).T for rows in (n, m))
        descs = [_lib.DeviceMatrix(t.data_ptr(), codes[t.dtype], int(t.stride(0)), int(t.stride(1))) for t in (rc, cc)]
        score = C.c_double(0.0)
        stream = torch.cuda.current_stream(dev).cuda_stream
        self._check(self._lib.resnmtf_bisil_device(
            self._h, v, k, C.byref(descs[0]), C.byref(descs[1]), METRICS[distance],
            *(None if t is None or t.numel() == 0 else C.c_void_p(t.data_ptr()) for t in (rs, cs)),
            C.byref(score), C.c_void_p(stream)))
        return rs, cs, float(score.value)

    def _bisil(self, entry, v: int, rc, cc, distance: str):
        from .bisil import METRICS
        if distance not in METRICS:
            raise ValueError("distance must be one of 'euclidean', 'manhattan' or 'cosine'.")
        rc = np.asfortranarray(np.asarray(rc, dtype=np.float64))
        if rc.ndim != 2 or rc.shape[0] != self.n_rows[v]:
            raise ValueError(f"row clusters must be {self.n_rows[v]} x k")
        cc = _f64_colmajor(cc, (self.n_cols[v], rc.shape[1]))
        k = int(rc.shape[1])
        rs = np.zeros((self.n_rows[v], k), order="F"); cs = np.zeros((self.n_cols[v], k), order="F")
        self._check(entry(self._h, v, k, _dp(rc), _dp(cc), METRICS[distance], _dp(rs), _dp(cs)))
        return rs, cs

    def view_image_info(self, v: int):
        """(kind, rel_error): kind 0 = f32 images, 1 = fp16, 2 = uniform 16-bit integers; the relative quantisation
        error of the 2-byte image of view ``v`` measured at upload (``x_half``)."""
        kind = C.c_int(0)
        rel = C.c_double(0.0)
        self._check(self._lib.resnmtf_view_image_info(self._h, v, C.byref(kind), C.byref(rel)))
        return int(kind.value), float(rel.value)

    def view_plan(self, v: int) -> dict:
        """The launch plan of view ``v``'s streaming passes (``resnmtf_view_plan``, host only): pass-wise fields are
        ``(X.G, Xt.F)`` pairs; ``image`` is "f32", "sparse", "fp16" or "u16"; the ``f_chain_*`` fields are those of
        the latest prepare (``prepared``)."""
        p = _lib.ViewPlan()
        p.struct_size = C.sizeof(_lib.ViewPlan)
        self._check(self._lib.resnmtf_view_plan(self._h, int(v), C.byref(p)))
        out = {}
        for name, typ in _lib.ViewPlan._fields_:
            if name == "struct_size":
                continue
            val = getattr(p, name)
            out[name] = tuple(int(x) for x in val) if hasattr(typ, "_length_") else int(val)
        out["image"] = ("f32", "sparse", "fp16", "u16")[out["image"]]
        for key in ("prepared", "f_chain_hoisted", "f_chain_one_slab"):
            out[key] = bool(out[key])
        return out

    def update_plan(self, v: int) -> dict:
        """The update side of view ``v``'s sweep (``resnmtf_update_plan``, host only): which ``factor_update_kernel``
        instantiation ``(kp, side, couple_bucket, emit)`` and which slab bucket its F and G updates take; side-wise
        fields are ``(F, G)`` pairs.  The coupling fields are those of the latest prepare (``prepared``), 0 before it;
        ``route`` is "kernel" (a launch of its own), "fused" (rides in the consuming pass) or "chain" (the hoisted F chain)."""
        p = _lib.UpdatePlan()
        p.struct_size = C.sizeof(_lib.UpdatePlan)
        self._check(self._lib.resnmtf_update_plan(self._h, int(v), C.byref(p)))
        out = {}
        for name, typ in _lib.UpdatePlan._fields_:
            if name == "struct_size":
                continue
            val = getattr(p, name)
            out[name] = tuple(int(x) for x in val) if hasattr(typ, "_length_") else int(val)
        out["prepared"] = bool(out["prepared"])
        out["route"] = tuple(("kernel", "fused", "chain")[r] for r in out["route"])
        return out

    def set_stop_tolerance(self, tol: float):
        """Phase API: ``tol >= 0`` = convergence mode (``R/main.r:50-81``) for the phases enqueued from now on."""
        self._check(self._lib.resnmtf_set_stop_tolerance(self._h, float(tol)))

    def loop_state(self):
        """(sweeps closed since prepare, stop flag, sweep count at which it fired) -- synchronises."""
        a, b, c = C.c_int(0), C.c_int(0), C.c_int(0)
        self._check(self._lib.resnmtf_loop_state(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return int(a.value), bool(b.value), int(c.value)

    def slice_info(self):
        a, b = C.c_int(0), C.c_int(0)
        self._check(self._lib.resnmtf_slice_info(self._h, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    def p2p_export(self) -> bytes:
        """slice_p2p: the IPC handles of this engine's receive buffers and arrival counters (opaque bytes for the peers)."""
        buf = C.create_string_buffer(1024)
        n = C.c_size_t(0)
        self._check(self._lib.resnmtf_p2p_export(self._h, buf, 1024, C.byref(n)))
        return buf.raw[:n.value]

    def p2p_import(self, rank: int, handles: bytes = b""):
        buf = C.create_string_buffer(handles, max(len(handles), 1))
        self._check(self._lib.resnmtf_p2p_import(self._h, int(rank), buf, len(handles)))

    def p2p_selftest(self, timeout_ms: int = 10000):
        """slice_p2p: probe stores, arrivals and the stream wait with host-side deadlines (every rank, after the imports and a
        barrier, before prepare); raises ResnmtfError when the node cannot run the peer-store exchange."""
        self._check(self._lib.resnmtf_p2p_selftest(self._h, int(timeout_ms)))

    def kernel_timings(self, reset: bool = False) -> dict:
        """time_kernels: {kind: (ms_total, launches)} for the kernels of a view-sharded sweep."""
        n = len(_lib.TIMED_KINDS)
        ms = (C.c_double * n)(); cnt = (C.c_longlong * n)()
        self._check(self._lib.resnmtf_kernel_timings(self._h, ms, cnt, 1 if reset else 0))
        return {name: (float(ms[i]), int(cnt[i])) for i, name in enumerate(_lib.TIMED_KINDS)}

    def pass_timings(self, reset: bool = False) -> dict:
        t = _lib.PassTiming()
        self._check(self._lib.resnmtf_pass_timings(self._h, C.byref(t), 1 if reset else 0))
        return {name: getattr(t, name) for name, _ in _lib.PassTiming._fields_}
