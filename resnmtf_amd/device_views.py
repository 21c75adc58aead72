"""Dense views that are ``torch`` tensors: a 2-D floating tensor on the engine's GPU is uploaded in
place (``Engine.set_view_device``: any of fp64 / fp32 / fp16 / bf16, any strides, no host copy, no fp64 staging image) and
is never converted to NumPy; a CPU tensor is handled as its NumPy array.  ``torch`` is never imported here: an object can
only be a tensor when the caller has imported it.

``RawDeviceView`` marks a device tensor whose non-negativity shift and column normalisation (``check_data``,
``R/utils.r:416,422``) are still to be done: ``problem.prepare(normalise=True)`` wraps a device tensor in it instead of
pre-processing it on the host, and the upload then runs them on the device (``raw=True``), as ``resnmtf_set_view_raw``
does for host data."""
from __future__ import annotations

import sys
import warnings

import numpy as np

OUTPUTS = ("numpy", "torch")


def _torch():
    return sys.modules.get("torch")


def is_tensor(x) -> bool:
    t = _torch()
    return t is not None and isinstance(x, t.Tensor)


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
    """A view that is uploaded from device memory: a CUDA tensor or a ``RawDeviceView``."""
    return isinstance(x, RawDeviceView) or (is_tensor(x) and x.device.type != "cpu")


def check_tensor(t, what: str = "view"):
    """The refusals that need no device: a tensor view is 2-D and floating."""
    if t.ndim != 2:
        raise ValueError(f"{what}: a tensor view must be 2-D, got {t.ndim} dimensions")
    if not t.dtype.is_floating_point:
        raise ValueError(f"{what}: a tensor view must have a floating dtype, got {t.dtype}")


def host_or_device(x, what: str = "view"):
    """A CPU tensor as the fp64 array of its values (after the checks); everything else as it is."""
    if is_tensor(x):
        check_tensor(x, what)
        if x.device.type == "cpu":
            return x.detach().to(_torch().float64).numpy()
    return x


def as_view(x, device_id: int = 0, what: str = "view"):
    """A dense view as the host layer keeps it: a CUDA tensor (or ``RawDeviceView``) as it is, after the checks -- 2-D,
    floating, on ``cuda:device_id`` (``ValueError`` otherwise) --, a CPU tensor as the fp64 array of its values, anything
    else as ``np.asarray(x, dtype=np.float64)``."""
    if isinstance(x, RawDeviceView):
        as_view(x.tensor, device_id, what)
        return x
    x = host_or_device(x, what)
    if not is_tensor(x):
        return np.asarray(x, dtype=np.float64)
    if x.device.type != "cuda" or x.device.index != int(device_id):
        raise ValueError(f"{what}: the tensor lives on {x.device}, the engine on cuda:{int(device_id)}")
    return x


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
