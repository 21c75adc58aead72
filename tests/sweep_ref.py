"""Host reference of ONE device sweep, step by step (test infrastructure; imports the oracle).

``step_reference`` follows ``update_matrices`` (R/update_steps.r:272-319) in its Gauss-Seidel order, but every step
takes the DEVICE's outputs of the steps before it as its inputs, so that each step's error is that step's own and a
failure names the kernel:

* F_v from the old F_v, S_v, G_v, lambda_v; the coupling terms read the other views' F: new for w < v, old for w > v;
* G_v from the device's new F_v (coupling: the other views' G, new for w < v, old for w > v);
* S_v from the device's new F_v and G_v (xi coupling: the other views' S, new for w < v, old for w > v);
* lambda_v and mu_v from the device's new F_v and G_v;
* the sweep's error (R/utils.r:157-166) from the device's new factors.

The arithmetic is the oracle's own ``update_f`` / ``update_g`` / ``update_s`` / ``update_lm`` / ``calculate_error``;
nothing is restated here.  ``x`` is the image the passes actually stream (``stream_image``): for the dense f32 views
``Engine.get_view``, which reads the Xt image (``Xt32``) while the X.G pass reads ``X32`` -- so a disagreement between
the two images shows up as an F-step failure.
"""
from __future__ import annotations

import numpy as np

from oracle import resnmtf_oracle as O

B16_SCALE = 8192.0      # RESNMTF_B16_SCALE: the fp16 passes split their factor operand b * 2^13 into two fp16 pieces


def step_reference(x, before, after, phi, xi, psi, row_names, col_names, data=None, row_indices=None, col_indices=None):
    """Reference of each step of one sweep.

    ``x[v]``: the streamed image of view v (fp64 matrix); ``before[v]`` / ``after[v]``: ``(F, S, G, lambda, mu)`` of the
    device before and after the sweep (``Engine.get_factors``); ``data[v]``: the fp64 upload (None: ``x``), which the
    device's ||X||^2 comes from.  Returns ``{"f", "g", "s", "lam", "mu": per-view lists, "err": per-view errors}``.

    The error is ``calculate_error`` on ``data`` plus the one term in which the device's trace form reads the image
    instead: ``2 <X - X~, F S G^T> / ||X||^2`` (zero when the image is the data)."""
    n_v = len(x)
    data = x if data is None else data
    ri = O.reorder_data(row_names) if row_indices is None else row_indices
    ci = O.reorder_data(col_names) if col_indices is None else col_indices
    f0 = [b[0] for b in before]; s0 = [b[1] for b in before]; g0 = [b[2] for b in before]
    lam0 = [b[3] for b in before]; mu0 = [b[4] for b in before]
    f1 = [a[0] for a in after]; s1 = [a[1] for a in after]; g1 = [a[2] for a in after]
    out = {"f": [], "g": [], "s": [], "lam": [], "mu": []}
    for v in range(n_v):
        fs = f1[:v] + f0[v:]
        gs = g1[:v] + g0[v:]
        ss = s1[:v] + s0[v:]
        out["f"].append(O.update_f(x[v], fs, s0[v], g0[v], lam0[v], phi, v, ri[v], row_names[v], row_names))
        out["g"].append(O.update_g(x[v], f1[v], s0[v], gs, mu0[v], psi, v, ci[v], col_names[v], col_names))
        out["s"].append(O.update_s(x[v], f1[v], ss, g1[v], xi, v))
        out["lam"].append(O.update_lm(lam0[v], f1[v]))
        out["mu"].append(O.update_lm(mu0[v], g1[v]))
    norms = np.array([np.linalg.norm(d, "fro") ** 2 for d in data])
    err = O.calculate_error(data, f1, s1, g1, norms)
    for v in range(n_v):
        if x[v] is not data[v]:
            err[v] += 2.0 * np.sum((data[v] - x[v]) * ((f1[v] @ s1[v]) @ g1[v].T)) / norms[v]
    out["err"] = err
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the 2-byte images (resnmtf_options.x_half): host emulation of max_entry_kernel + pack_half_kernel
# ---------------------------------------------------------------------------------------------------------------------
def half_scale(x32: np.ndarray, u16: bool) -> np.float32:
    """The per-view scale build_half_images chooses from the largest f32 entry: 16-bit integers 65535 / max (f32
    division), fp16 the power of two that puts the largest entry in [2^13, 2^14)."""
    mx = np.float32(np.max(x32)) if x32.size else np.float32(0.0)
    if not (mx > 0 and np.isfinite(mx)):
        return np.float32(1.0)
    if u16:
        return np.float32(np.float32(65535.0) / mx)
    _, ex = np.frexp(mx)
    return np.float32(np.ldexp(np.float32(1.0), 14 - int(ex)))


def quantise(x32: np.ndarray, scale: np.float32, u16: bool) -> np.ndarray:
    """pack_half_kernel on f32 entries: ``min(rint(x scale), 65535)`` as 16-bit integers, or round-to-nearest-even fp16
    of ``x scale`` (products in f32, as on the device)."""
    y = np.asarray(x32, dtype=np.float32) * np.float32(scale)
    if u16:
        return np.minimum(np.rint(y), np.float32(65535.0)).astype(np.uint16)
    return y.astype(np.float16)


def half_image(data: np.ndarray, u16: bool):
    """``(image, rel_error)``: the 2-byte image of the fp64 upload ``data`` with the scale taken back out (fp64), and
    ``|| X~ - X ||_F / || X ||_F`` as ``resnmtf_view_image_info`` measures it (X = the f32 image, ||X|| from the fp64
    upload).  The upload rounds ``data`` to f32 first (convert_x_kernel)."""
    x32 = np.asarray(data, dtype=np.float64).astype(np.float32)
    scale = half_scale(x32, u16)
    q = quantise(x32, scale, u16)
    img = q.astype(np.float64) / np.float64(scale)
    d = img - x32.astype(np.float64)
    rel = float(np.sqrt(np.sum(d * d) / np.sum(np.asarray(data, dtype=np.float64) ** 2)))
    return img, rel


def fp16_split(b: np.ndarray) -> np.ndarray:
    """The factor operand as pass_half_kernel (fp16 images) multiplies it: ``v = b 2^13`` in f32, ``hi = fp16(min(v,
    65504))``, ``lo = fp16(v - hi)``, value ``(hi + lo) / 2^13``.  22 bits while lo is a normal fp16 number (b >= 2^-16);
    below, lo is subnormal and the entry keeps an absolute error of up to 2^-38."""
    v = np.asarray(b, dtype=np.float64).astype(np.float32) * np.float32(B16_SCALE)
    hi = np.minimum(v, np.float32(65504.0)).astype(np.float16)
    lo = (v - hi.astype(np.float32)).astype(np.float16)
    return (hi.astype(np.float64) + lo.astype(np.float64)) / B16_SCALE


def stream_image(engine, v: int, data: np.ndarray, plan: dict) -> np.ndarray:
    """The matrix the passes of view v stream, as fp64: the device's f32 image (``get_view``), the sparse view's
    stored values rounded to f32 (densified), or the emulated 2-byte image (the f32 images are not read back then)."""
    if plan["image"] == "f32":
        return engine.get_view(v)
    if plan["image"] == "sparse":
        d = data.toarray() if hasattr(data, "toarray") else np.asarray(data)
        return d.astype(np.float32).astype(np.float64)
    return half_image(data, plan["image"] == "u16")[0]


# ---------------------------------------------------------------------------------------------------------------------
# the statistic and its mutants
# ---------------------------------------------------------------------------------------------------------------------
def rel_stat(got: np.ndarray, ref: np.ndarray):
    """``(max |got / ref - 1| over ref > 0, count of entries with ref == 0 but got != 0)``; a non-finite ``got`` where
    ``ref > 0`` is an infinite error (NaN would compare false against any bar)."""
    got = np.asarray(got, dtype=np.float64); ref = np.asarray(ref, dtype=np.float64)
    pos = ref > 0
    dev = np.abs(got[pos] / ref[pos] - 1.0)
    worst = float(np.max(np.where(np.isfinite(dev), dev, np.inf))) if pos.any() else 0.0
    return worst, int(np.count_nonzero(got[~pos]))
