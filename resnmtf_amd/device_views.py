"""Dense views that are ``torch`` tensors: a 2-D floating tensor on the engine's GPU is uploaded in
place (``Engine.set_view_device``: any of fp64 / fp32 / fp16 / bf16, any strides, no host copy, no fp64 staging image) and
is never converted to NumPy; a CPU tensor is handled as its NumPy array.  ``torch`` is never imported here: an object can
only be a tensor when the caller has imported it.

``RawDeviceView`` marks a device tensor whose non-negativity shift and column normalisation (``check_data``,
``R/utils.r:416,422``) are still to be done: ``problem.prepare(normalise=True)`` wraps a device tensor in it instead of
pre-processing it on the host, and the upload then runs them on the device (``raw=True``), as ``resnmtf_set_view_raw``
does for host data.

Sparse ``torch`` tensors: a 2-D ``sparse_csc`` / ``sparse_csr`` / (coalesced) ``sparse_coo`` tensor
on the engine's GPU is a SPARSE view, uploaded from its own index and value arrays (``Engine.set_view_sparse_device``) and
never brought to the host; the host layer keeps it as a ``SparseDeviceView`` -- the tensor, its shape and its nnz, no host
copy.  A CPU sparse tensor becomes the ``scipy.sparse.csc_matrix`` of its values and takes the host route."""
from __future__ import annotations

import copy
import sys
import warnings

import numpy as np

OUTPUTS = ("numpy", "torch")


def _torch():
    return sys.modules.get("torch")


def is_tensor(x) -> bool:
    t = _torch()
    return t is not None and isinstance(x, t.Tensor)


def is_sparse_tensor(x) -> bool:
    """A ``torch`` tensor of any sparse layout (COO, CSR, CSC, BSR, BSC)."""
    return is_tensor(x) and x.layout != _torch().strided


class SparseDeviceView:
    """A sparse CUDA tensor as the host layer keeps a sparse view that lives in device memory: ``tensor``, ``shape``,
    ``nnz`` (stored entries) and ``raw`` -- True when the column normalisation of ``check_data`` (``R/utils.r:86-88``)
    is still to be done, at every upload of it (``pre_processed=False``), as for a ``RawDeviceView``."""

    def __init__(self, tensor, raw: bool = False):
        self.tensor = tensor
        self.shape = tuple(tensor.shape)
        self.nnz = int(tensor._nnz())
        self.raw = bool(raw)
        self.ndim = 2

    def as_raw(self):
        out = copy.copy(self)            # (the same tensor: nothing is read from it again)
        out.raw = True
        return out


def check_sparse_tensor(t, what: str = "view"):
    """The refusals of a sparse tensor view that need no device: a ``sparse_csc`` / ``sparse_csr`` / ``sparse_coo``
    layout, 2-D without dense or batch dimensions, floating values, int32 / int64 indices, a coalesced COO."""
    torch = _torch()
    if t.layout not in (torch.sparse_csc, torch.sparse_csr, torch.sparse_coo):
        raise ValueError(f"{what}: a sparse tensor view must be sparse_csc, sparse_csr or sparse_coo, got {t.layout} "
                         "(convert it with .to_sparse_csc())")
    if t.dense_dim() != 0:
        raise ValueError(f"{what}: a hybrid sparse tensor (dense dimensions) is not a view")
    if t.ndim != 2:
        raise ValueError(f"{what}: a sparse tensor view must be 2-D, got {t.ndim} dimensions (batched tensors are not supported)")
    if not t.dtype.is_floating_point:
        raise ValueError(f"{what}: a tensor view must have a floating dtype, got {t.dtype}")
    if t.layout == torch.sparse_coo and not t.is_coalesced():
        raise ValueError(f"{what}: the COO tensor is not coalesced: call .coalesce() first (a position stored twice is "
                         "refused, nothing is summed)")
    index = sparse_tensor_parts(t)[0]
    if index.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"{what}: the indices of a sparse tensor view must be int32 or int64, got {index.dtype}")


def sparse_tensor_parts(t):
    """(pointers or row indices, indices or column indices, values) of a checked 2-D sparse tensor, as torch holds them."""
    torch = _torch()
    if t.layout == torch.sparse_csc:
        return t.ccol_indices(), t.row_indices(), t.values()
    if t.layout == torch.sparse_csr:
        return t.crow_indices(), t.col_indices(), t.values()
    idx = t._indices()
    return idx[0], idx[1], t._values()


def sparse_tensor_to_scipy(t):
    """A CPU sparse tensor (checked) as the ``scipy.sparse.csc_matrix`` of its values widened to fp64."""
    import scipy.sparse as sp
    torch = _torch()
    a, b, vals = (x.detach() for x in sparse_tensor_parts(t))
    vals = vals.to(torch.float64).numpy()
    a, b = a.numpy(), b.numpy()
    shape = tuple(t.shape)
    if t.layout == torch.sparse_csc:
        return sp.csc_matrix((vals, b, a), shape=shape)
    if t.layout == torch.sparse_csr:
        return sp.csc_matrix(sp.csr_matrix((vals, b, a), shape=shape))
    return sp.csc_matrix(sp.coo_matrix((vals, (a, b)), shape=shape))


def is_sparse_device_view(x) -> bool:
    """A sparse view that lives in device memory: a ``SparseDeviceView`` or a sparse tensor that is not on the CPU."""
    return isinstance(x, SparseDeviceView) or (is_sparse_tensor(x) and x.device.type != "cpu")


def as_sparse_view(x, device_id: int = 0, what: str = "view") -> SparseDeviceView:
    """A sparse CUDA tensor (or ``SparseDeviceView``) as a ``SparseDeviceView``, after the checks: ``check_sparse_tensor``
    and the device (``ValueError`` otherwise)."""
    t = x.tensor if isinstance(x, SparseDeviceView) else x
    check_sparse_tensor(t, what)
    if t.device.type != "cuda" or t.device.index != int(device_id):
        raise ValueError(f"{what}: the tensor lives on {t.device}, the engine on cuda:{int(device_id)}")
    return x if isinstance(x, SparseDeviceView) else SparseDeviceView(t)


def upload_sparse(eng, v: int, x: SparseDeviceView, pre_processed: bool = True):
    """``x`` into ``eng``'s sparse view ``v`` (``Engine.set_view_sparse_device``); a ``raw`` view is normalised on the
    device whatever ``pre_processed`` says."""
    eng.set_view_sparse_device(v, x.tensor, pre_processed=pre_processed and not x.raw)


class RawDeviceView:
    """A device tensor still to be shifted and column-normalised, at its upload (module docstring)."""

    def __init__(self, tensor):
        self.tensor = tensor

    @property
    def shape(self):
        return tuple(self.tensor.shape)

    @property
    def ndim(self):
        return 2


def is_device_view(x) -> bool:
    """A view that is uploaded from device memory: a CUDA tensor (dense or sparse), a ``RawDeviceView`` or a
    ``SparseDeviceView``."""
    return isinstance(x, (RawDeviceView, SparseDeviceView)) or (is_tensor(x) and x.device.type != "cpu")


def check_tensor(t, what: str = "view"):
    """The refusals that need no device: a tensor view is 2-D and floating."""
    if t.ndim != 2:
        raise ValueError(f"{what}: a tensor view must be 2-D, got {t.ndim} dimensions")
    if not t.dtype.is_floating_point:
        raise ValueError(f"{what}: a tensor view must have a floating dtype, got {t.dtype}")


def host_or_device(x, what: str = "view"):
    """A CPU tensor as the fp64 array of its values (after the checks) -- a sparse one as the ``scipy.sparse.csc_matrix``
    of them; everything else as it is."""
    if is_sparse_tensor(x):
        check_sparse_tensor(x, what)
        return sparse_tensor_to_scipy(x) if x.device.type == "cpu" else x
    if is_tensor(x):
        check_tensor(x, what)
        if x.device.type == "cpu":
            return x.detach().to(_torch().float64).numpy()
    return x


def as_view(x, device_id: int = 0, what: str = "view"):
    """A dense view as the host layer keeps it: a CUDA tensor (or ``RawDeviceView``) as it is, after the checks -- 2-D,
    floating, on ``cuda:device_id`` (``ValueError`` otherwise) --, a CPU tensor as the fp64 array of its values, anything
    else as ``np.asarray(x, dtype=np.float64)``.  A sparse tensor is never taken for a dense view: on the GPU it becomes a
    ``SparseDeviceView`` (``as_sparse_view``), on the CPU a ``scipy.sparse.csc_matrix``; both are sparse views."""
    if isinstance(x, RawDeviceView):
        as_view(x.tensor, device_id, what)
        return x
    x = host_or_device(x, what)
    if is_sparse_device_view(x):
        return as_sparse_view(x, device_id, what)
    if type(x).__module__.startswith("scipy.sparse"):
        return x
    if not is_tensor(x):
        return np.asarray(x, dtype=np.float64)
    if x.device.type != "cuda" or x.device.index != int(device_id):
        raise ValueError(f"{what}: the tensor lives on {x.device}, the engine on cuda:{int(device_id)}")
    return x


def is_device_tensor(x) -> bool:
    """A ``torch`` tensor that does not live on the CPU."""
    return is_tensor(x) and x.device.type != "cpu"


def factor_route(f, s, g, what: str = "view", on_device=is_device_tensor) -> bool:
    """Which route the three initial factors of one view take: True = the device route
    (``Engine.set_factors_device``: all three are device tensors), False = the host route (none is).  A mix is a
    ``ValueError`` naming ``what``.  Pure: ``on_device`` decides what a device tensor is."""
    flags = [bool(on_device(x)) for x in (f, s, g)]
    if all(flags):
        return True
    if any(flags):
        where = ", ".join(f"init_{name} on the {'device' if flag else 'host'}" for name, flag in zip("fsg", flags))
        raise ValueError(f"{what}: the initial factors mix device tensors and host arrays ({where}); give all three of a "
                         "view in one place")
    return False


def factor_routes(init_f, init_s, init_g, device_id: int = 0):
    """The initial factors of every view, ready for ``Engine.set_factors`` / ``set_factors_device``: returns ``(routes,
    init_f, init_s, init_g)`` -- ``routes[v]`` as ``factor_route`` decides it, a CPU tensor replaced by the fp64 array of
    its values, a device tensor checked (2-D, floating, on ``cuda:device_id``; ``ValueError`` otherwise) and left where
    it is.  No device is touched."""
    routes, lists = [], ([], [], [])
    for v, parts in enumerate(zip(init_f, init_s, init_g)):
        parts = [host_or_device(x, f"view {v}: init_{name}") for x, name in zip(parts, "fsg")]
        routes.append(factor_route(*parts, what=f"view {v}"))
        for x, name, out in zip(parts, "fsg", lists):
            if routes[v] and (x.device.type != "cuda" or x.device.index != int(device_id)):
                raise ValueError(f"view {v}: init_{name} lives on {x.device}, the engine on cuda:{int(device_id)}")
            out.append(x)
    return (routes, *lists)


def check_init_lm(init_lm, n_views: int):
    """``init_lm`` of ``res_nmtf_inner``: ``(lambdas, mus)``, one entry per view each (``ValueError`` otherwise)."""
    try:
        ok = len(init_lm) == 2 and all(len(x) == n_views for x in init_lm)
    except TypeError:
        ok = False
    if not ok:
        raise ValueError(f"init_lm must be (lambdas, mus) with one entry per view each ({n_views} views)")
    return list(init_lm[0]), list(init_lm[1])


def upload(eng, v: int, x, raw: bool = False) -> bool:
    """``x`` (as ``as_view`` returns a dense view) into ``eng``'s view ``v``: a device view through ``set_view_device``
    (a ``RawDeviceView`` always with the pre-processing, with the reference's warning, ``R/utils.r:23-25``), a host array
    through ``set_view`` / ``set_view_raw``.  Returns True when a raw upload met a negative entry."""
    if isinstance(x, RawDeviceView):
        neg = eng.set_view_device(v, x.tensor, raw=True)
        if neg:
            warnings.warn("Matrix is not non-negative. Has been made non-negative.")       # utils.r:24
        return neg
    if is_tensor(x):
        return eng.set_view_device(v, x, raw=raw)
    if raw:
        return eng.set_view_raw(v, x)
    eng.set_view(v, x)
    return False


def on_engine_device(x, device_id: int = 0) -> bool:
    """A ``torch`` tensor that lives on ``cuda:device_id``: what the device routes read in place."""
    return is_tensor(x) and x.device.type == "cuda" and x.device.index == int(device_id)


CLUSTER_DTYPES = ("torch.float64", "torch.float32", "torch.float16", "torch.bfloat16")


def check_cluster_tensors(rc, cc, n: int, m: int, device_id: int = 0, what: str = "bisil_device"):
    """The refusals of a view's two cluster matrices in device memory that need no device (``Engine.bisil_device``):
    both ``torch`` tensors (``TypeError`` otherwise), fp64 / fp32 / fp16 / bf16, on ``cuda:device_id``, ``rc`` n x k and
    ``cc`` m x k with one k (``ValueError``).  Returns ``(rc, cc, k)``, the tensors detached."""
    for t, name in ((rc, "rc"), (cc, "cc")):
        if not is_tensor(t):
            raise TypeError(f"{what} takes torch.Tensors, {name} is a {type(t).__name__} (host matrices: bisil)")
        if str(t.dtype) not in CLUSTER_DTYPES:
            raise ValueError(f"{what}: {name} must be fp64, fp32, fp16 or bf16, got {t.dtype}")
        if not on_engine_device(t, device_id):
            raise ValueError(f"{what}: {name} lives on {t.device}, the engine on cuda:{int(device_id)}")
    if rc.ndim != 2 or rc.shape[0] != int(n):
        raise ValueError(f"{what}: row clusters must be {int(n)} x k, got {tuple(rc.shape)}")
    if cc.ndim != 2 or tuple(cc.shape) != (int(m), rc.shape[1]):
        raise ValueError(f"{what}: expected column clusters of shape {(int(m), rc.shape[1])}, got {tuple(cc.shape)}")
    return rc.detach(), cc.detach(), int(rc.shape[1])


def cluster_route(rc, cc, device_id: int = 0, what: str = "view", on_device=None) -> bool:
    """Which route one view's cluster matrices take to the bisilhouette: True = the device route
    (``Engine.bisil_device``: both are tensors on ``cuda:device_id``), False = the host route (neither is).  One of each
    is a ``ValueError`` naming ``what``.  Pure: ``on_device`` decides what a tensor on the engine's device is."""
    on_device = on_device or (lambda x: on_engine_device(x, device_id))
    flags = [bool(on_device(x)) for x in (rc, cc)]
    if all(flags):
        return True
    if any(flags):
        where = ", ".join(f"{name} on the {'device' if flag else 'host'}" for name, flag in zip(("row_clusters", "col_clusters"), flags))
        raise ValueError(f"{what}: the cluster matrices mix a device tensor and a host matrix ({where}); give both in one place")
    return False


def check_readback_strides(shape, strides, what: str = "out"):
    """The layout ``Engine.get_view_device`` may write to (``resnmtf_get_view_device``): ``shape`` =
    (n, m), ``strides`` = (row stride, column stride) in ELEMENTS.  A stride along an extent above 1 must be positive,
    and no two elements may share an address: with a <= b the two strides and e the extent along a, a (e - 1) < b --
    every slice or transpose of a contiguous tensor passes.  The stride of an extent-1 axis is never used and may be
    anything.  Pure; ``ValueError`` otherwise."""
    (n, m), (rs, cs) = (int(x) for x in shape), (int(x) for x in strides)
    if (n > 1 and rs <= 0) or (m > 1 and cs <= 0):
        raise ValueError(f"{what}: a stride along an extent above 1 must be positive, got strides ({rs}, {cs}) for shape "
                         f"({n}, {m}) (an expand()ed tensor has stride 0)")
    if n > 1 and m > 1:
        a, b, e = (rs, cs, n) if rs <= cs else (cs, rs, m)
        if a * (e - 1) >= b:
            raise ValueError(f"{what}: strides ({rs}, {cs}) make two elements of a ({n}, {m}) matrix share an address")


def to_numpy(x):
    """A NumPy copy of a small result matrix for the host steps (a tensor is downloaded; an array is returned as it is)."""
    return x.detach().cpu().numpy() if is_tensor(x) else x


def check_output(output: str):
    if output not in OUTPUTS:
        raise ValueError("output must be 'numpy' or 'torch'.")


def zero_columns_like(t, before: np.ndarray, after: np.ndarray):
    """``t``: the device copy of ``before``.  The host steps (spurious removal, stability) turn ``before`` into ``after``
    by zeroing whole columns; the same columns of ``t`` are zeroed on the device (in place) and ``t`` is returned."""
    changed = np.any(np.asarray(before) != np.asarray(after), axis=0)
    if changed.any():
        if np.any(np.asarray(after)[:, changed] != 0.0):
            raise RuntimeError("a host step changed a cluster matrix other than by zeroing columns")
        t[:, _torch().as_tensor(np.flatnonzero(changed), device=t.device)] = 0.0
    return t
