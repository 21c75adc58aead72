"""The steps every entry point shares, written once: preparing a problem (names, shared-name maps, symmetrised
restrictions, pre-processing: ``prepare``), wiring an engine's view coupling (``couple`` over ``pair_table``), loading a
child engine from one that already holds the data (``load_child``), and assembling a ``res_nmtf_inner`` result
(``inner_result`` with ``reported_error``).  Imported at module top by ``api``, ``batched``, ``spurious`` and ``sharded``;
imports only ``naming`` and ``engine`` itself."""
from __future__ import annotations

from collections import namedtuple
from typing import Optional, Sequence

import numpy as np

from . import device_views, naming
from . import engine as _engine
from .engine import Engine


def svd_init(data: Sequence[np.ndarray], k_vec: Sequence[int], seed: Optional[int] = None, sigma: float = 0.05):
    """``init_mats_inner`` (``R/update_steps.r:78-125``) on the host, as in the reference
    (the initialisation is outside the accelerated loop).  The noise on S comes from NumPy's
    generator instead of ``MASS::mvrnorm`` + R's RNG: statistically, not bitwise, equivalent."""
    rng = np.random.default_rng(seed)
    init_f, init_s, init_g, init_lam, init_mu = [], [], [], [], []
    for x, k in zip(data, k_vec):
        u, d, vt = np.linalg.svd(x, full_matrices=False)
        f = np.abs(u[:, :k]); g = np.abs(vt.T[:, :k])
        s = np.abs(np.diag(d)[:k, :k]) + np.abs(rng.normal(0.0, np.sqrt(sigma), size=(k, k)))
        cf, cg = f.sum(axis=0), g.sum(axis=0)
        s = s * (cf * cg)[None, :]
        f = f / cf[None, :]; g = g / cg[None, :]
        init_f.append(f); init_s.append(s); init_g.append(g)
        init_lam.append(f.sum(axis=0)); init_mu.append(g.sum(axis=0))
    return init_f, init_s, init_g, init_lam, init_mu


def _raw_on_device(d):
    """A view in device memory whose pre-processing is left to its upload: a dense tensor as a ``RawDeviceView``, a
    sparse one as a raw ``SparseDeviceView`` (the tensor itself is left as it is)."""
    if isinstance(d, device_views.RawDeviceView):
        return d
    if isinstance(d, device_views.SparseDeviceView):
        return d.as_raw()
    if device_views.is_sparse_tensor(d):
        return device_views.SparseDeviceView(d, raw=True)
    return device_views.RawDeviceView(d)


# a problem as res_nmtf_inner receives it (R/main.r:225-249)
Prepared = namedtuple("Prepared", "data row_names col_names phi xi psi row_shared col_shared")


def prepare(data, phi, xi, psi, row_names, col_names, *, normalise: bool, symmetrise: bool) -> Prepared:
    """``apply_resnmtf``'s steps before the loop: ``give_names`` (``R/main.r:228``; only the shapes of ``data`` are
    read), the shared-name maps (``:230``), the restriction matrices -- symmetrised (``init_rest_mats``, ``:233-235``)
    or, with ``symmetrise=False``, taken as the symmetrised matrices they already are (None = zeros) -- and, with
    ``normalise``, the non-negativity shift and column normalisation on the host (``check_data``, ``:237``).  A CPU
    ``torch`` tensor is taken as its NumPy array; a tensor on a GPU is never brought to the host: with ``normalise`` it
    is wrapped in ``device_views.RawDeviceView`` (a sparse one in a raw ``device_views.SparseDeviceView``) and pre-processed
    on the device at its upload."""
    n_v = len(data)
    data = [device_views.host_or_device(d, f"view {v}") for v, d in enumerate(data)]
    rn, cn = naming.give_names(data, phi, psi, row_names, col_names)
    shared = naming.shared_names(rn), naming.shared_names(cn)
    if symmetrise:
        phi, psi, xi = (naming.init_rest_mats(m, n_v) for m in (phi, psi, xi))
    else:
        phi, psi, xi = (np.zeros((n_v, n_v)) if m is None else np.asarray(m, dtype=np.float64) for m in (phi, psi, xi))
    if normalise:
        data = [_raw_on_device(d) if device_views.is_device_view(d) else naming.check_data([d])[0] for d in data]
    return Prepared(list(data), rn, cn, phi, xi, psi, *shared)


def pair_table(names, shared=None) -> list:
    """``table[v][w]`` = the index pairs (``naming.index_pairs``) of the names views v and w share along one axis --
    ``(None, None)`` for NA -- and ``None`` on the diagonal.  ``shared``: the axis' shared-name map, built from the
    names when not given."""
    shared = naming.shared_names(names) if shared is None else shared
    return [[None if v == w else naming.index_pairs(names[v], names[w], shared[v].get(w)) for w in range(len(names))]
            for v in range(len(names))]


def couple(eng, row_names, col_names, row_shared=None, col_shared=None):
    """Hand ``eng`` the shared rows and columns of every ordered pair of views (nothing to do for one view)."""
    rows, cols = pair_table(row_names, row_shared), pair_table(col_names, col_shared)
    for v in range(len(row_names)):
        for w in range(len(row_names)):
            if v != w:
                eng.set_shared_rows(v, w, *rows[v][w])
                eng.set_shared_cols(v, w, *cols[v][w])


def _draw_shuffle(eng, v: int, src, shuffle_seed: int, shuffle_sparse: bool = False):
    """``shuffle_view`` (``R/obtain_bicl.r:11-22``) of ``src``'s view v into ``eng``'s view v, drawn and re-normalised
    on the device; redrawn while a row or a column of the shuffled matrix sums to zero (``:14-18``).  ``shuffle_sparse``
    (opt-in): a sparse view is shuffled as a sparse view (``Engine.shuffle_view_sparse_from``: the same draws, the same
    seeds, the same bound of 64); without it the library refuses it as before.  A sparse view with fewer stored entries
    than ``max(n, m)`` is refused before the first draw: every shuffle of it has an all-zero row or column."""
    draw = eng.shuffle_view_from
    if shuffle_sparse and src.sparse[v]:
        lines = max(src.n_rows[v], src.n_cols[v])
        stored = src.view_storage(v)[1]                 # (>= the number of positive entries)
        if stored < lines:
            raise ValueError(f"shuffle_view: view {v} stores {stored} entries, fewer than max(n, m) = {lines}: every shuffle "
                             "of it has an all-zero row or column, and the reference's shuffle_view (R/obtain_bicl.r:14-18) "
                             "would not terminate on this view")
        draw = eng.shuffle_view_sparse_from
    for attempt in range(64):
        draw(v, src, v, seed=(shuffle_seed + 7919 * attempt) * 1000003 + v)
        er, ec = eng.empty_lines(v)
        if not (er.any() or ec.any()):
            return
    raise RuntimeError("shuffle_view: every draw left an all-zero row or column")


def load_child(eng, src, seed: int, *, shuffle_seed: Optional[int] = None, samples=None, host_views=None, coupling=None,
               shuffle_sparse: bool = False, sparse_on_device: bool = False):
    """Fill ``eng`` from ``src``, an engine on the same device that holds the data: every view shuffled (with
    ``shuffle_seed``; sparse views only with ``shuffle_sparse``, ``_draw_shuffle``), sub-sampled (``samples = (row_samples, col_samples)``) or copied -- a sparse view is uploaded from
    ``host_views[v]`` instead, or with ``sparse_on_device`` (opt-in) sub-sampled / copied on the device as a sparse view
    (``Engine.subsample_view_sparse_from`` / ``copy_view_sparse_from``; ``host_views`` is then not read for it) -- then the
    device SVD init with ``seed + v``; ``sparse_on_device`` may also be one flag per view (a sparse view that came from
    device memory has no host copy and always takes the device route); at last ``coupling`` = (phi, xi, psi,
    row_names, col_names), or for shuffles none: no restrictions, uncoupled (``R/obtain_bicl.r:35-39``)."""
    for v in range(eng.n_views):
        if shuffle_seed is not None:
            _draw_shuffle(eng, v, src, shuffle_seed, shuffle_sparse)
        elif (sparse_on_device[v] if isinstance(sparse_on_device, (list, tuple)) else sparse_on_device) and src.sparse[v]:
            if samples is not None:
                eng.subsample_view_sparse_from(v, src, v, samples[0][v], samples[1][v])
            else:
                eng.copy_view_sparse_from(v, src, v)
        elif host_views is not None and host_views[v] is not None:
            eng.set_view_sparse(v, host_views[v], pre_processed=True)      # (sub-samples are not re-normalised)
        elif samples is not None:
            eng.subsample_view_from(v, src, v, samples[0][v], samples[1][v])
        else:
            eng.copy_view_from(v, src, v)
        eng.init_svd(v, seed=seed + v)
    if shuffle_seed is not None:
        eng.set_restrictions(None, None, None)
    else:
        eng.set_restrictions(*coupling[:3])
        couple(eng, *coupling[3:])


def shuffled_engines(src, k: int, num_repeats: int, seed: int = 0, max_iters: int = 100000, device_id: int = 0, *,
                     shuffle_sparse: bool = False) -> list:
    """``obtain_shuffled_f`` (``R/obtain_bicl.r:31-42``) drawn from the views an engine already holds on the device
    (``src``: a ``res_nmtf_inner`` engine or a stability repeat's sub-sample; no second upload): ``num_repeats`` engines,
    every view shuffled from ``src``'s and re-normalised, no restrictions, uncoupled, device SVD init, run to
    convergence -- the draws and seeds of ``shuffles_on_device(dev, k, num_repeats, seed=seed)``: repeat r initialises
    with ``seed + 1000 + r`` and shuffles with ``seed * 7919 + r + 1``.  The engines are returned open, with their
    factors on the device (``Engine.spurious_scores``); the caller closes them.  ``shuffle_sparse`` (opt-in): a sparse
    view of ``src`` is shuffled into a sparse view of the same capacity (mixed problems work view by view); without it
    the engines are dense and the library refuses a sparse source as before."""
    out = []
    nnz = [src.view_storage(v)[1] if shuffle_sparse and src.sparse[v] else None for v in range(src.n_views)]
    try:
        for r in range(num_repeats):
            eng = Engine(src.n_rows, src.n_cols, [k] * src.n_views, device_id=device_id, nnz=nnz)
            out.append(eng)
            load_child(eng, src, seed + 1000 + r, shuffle_seed=seed * 7919 + r + 1, shuffle_sparse=shuffle_sparse)
            eng.run(n_iters=None, tol=1.0e-6, max_iters=max_iters)
    except BaseException:
        for eng in out:
            eng.close()
        raise
    return out


def _draw_shuffle_fp64(x, v: int, shuffle_seed: int, device_id: int = 0, shuffle=None, shuffle_sparse=None):
    """``_draw_shuffle`` in double precision (DESIGN.md sections 27 and 30): ``shuffle_view`` (``R/obtain_bicl.r:11-22``) of
    the view ``x`` -- a host array or a dense tensor on the device through ``engine.fp64_shuffle``, a sparse view (a
    canonical ``scipy.sparse`` matrix or a ``SparseDeviceView``) through ``engine.fp64_shuffle_sparse`` --, re-normalised
    there, redrawn while a row or a column of the draw sums to zero (``:14-18``) -- the same draw seeds, the same bound of
    64.  A sparse view with fewer stored entries than ``max(n, m)`` is refused before the first draw, as ``_draw_shuffle``
    does.  Returns ``(the fp64 tensor on the device -- a ``sparse_csc`` one for a sparse view --, the draws made)``.
    ``shuffle`` replaces ``engine.fp64_shuffle``, ``shuffle_sparse`` ``engine.fp64_shuffle_sparse``: test hooks."""
    if device_views.is_sparse_device_view(x) or type(x).__module__.startswith("scipy.sparse"):
        if device_views.is_sparse_device_view(x):
            x = device_views.as_sparse_view(x, device_id, f"view {v}")
        lines, stored = max(int(x.shape[0]), int(x.shape[1])), int(x.nnz)        # (>= the number of positive entries)
        if stored < lines:
            raise ValueError(f"shuffle_view: view {v} stores {stored} entries, fewer than max(n, m) = {lines}: every shuffle "
                             "of it has an all-zero row or column, and the reference's shuffle_view (R/obtain_bicl.r:14-18) "
                             "would not terminate on this view")
        sparse_draw = shuffle_sparse or _engine.fp64_shuffle_sparse

        def draw(seed):
            return sparse_draw(x, seed, normalise=True, device_id=device_id)
    else:
        dense_draw = shuffle or _engine.fp64_shuffle

        def draw(seed):
            t, _, er, ec = dense_draw(x, seed, normalise=True, device_id=device_id)
            return t, er, ec
    for attempt in range(64):
        t, er, ec = draw((shuffle_seed + 7919 * attempt) * 1000003 + v)
        if not (np.any(er) or np.any(ec)):
            return t, attempt + 1
    raise RuntimeError("shuffle_view: every draw left an all-zero row or column")


def shuffled_fits_fp64(data, k: int, num_repeats: int, seed: int = 0, max_iters: int = 100000, device_id: int = 0, *,
                       shuffle=None, fit=None, keep=None, shuffle_sparse=None, fp64_init: bool = False) -> list:
    """``obtain_shuffled_f`` (``R/obtain_bicl.r:31-42``) in double precision (DESIGN.md sections 27 and 30): for every
    repeat r, each view of ``data`` (host arrays or dense tensors on ``cuda:device_id``, as the fp64 run received them; a
    sparse view as its canonical ``scipy.sparse`` matrix or its ``SparseDeviceView``) drawn by ``_draw_shuffle_fp64`` with
    ``shuffled_engines``' seeds -- the shuffle seed ``seed * 7919 + r + 1`` -- and the draws factorised by
    ``res_nmtf_inner(precision="fp64", fp64_device=True, output="torch", n_iters=None, spurious=False, seed=seed + 1000 +
    r)`` -- with a sparse draw among them also ``fp64_sparse_device=True``: the draw is factorised as the sparse device
    view it is --: no restrictions, uncoupled, from the device SVD start the f32 shuffle engine takes for the same draw, to
    convergence (``max_iters`` guards it); with ``fp64_init`` from ``engine.fp64_init_svd`` of the
    draw under the same seed, and no engine is built.  Returns the ``num_repeats`` lists of normalised F's per view as NumPy arrays --
    ``check_biclusters``' ``shuffled_f``; the draws of one repeat are the only shuffled copies alive, one per view.
    Test hooks: ``shuffle`` replaces ``engine.fp64_shuffle``, ``shuffle_sparse`` ``engine.fp64_shuffle_sparse``,
    ``fit(tensors, k, seed, max_iters, device_id)`` the factorisation (it returns the F's), ``keep(r, tensors, attempts)``
    sees every repeat's draws before they go."""
    views = list(data)
    n_v = len(views)
    if fit is None:
        def fit(tensors, k, seed, max_iters, device_id):
            from .api import res_nmtf_inner          # (lazy: api imports this module at its top)
            more = {"fp64_sparse_device": True} if any(device_views.is_sparse_tensor(t) for t in tensors) else {}
            if fp64_init:
                more["fp64_init"] = True
            res = res_nmtf_inner(tensors, None, None, None, None, None, [k] * n_v, None, None, None, None, spurious=False,
                                 seed=seed, max_iters=max_iters, device_id=device_id, precision="fp64", fp64_device=True,
                                 output="torch", **more)
            return res["output_f"]
    out = []
    for r in range(num_repeats):
        drawn = [_draw_shuffle_fp64(x, v, seed * 7919 + r + 1, device_id, shuffle, shuffle_sparse) for v, x in enumerate(views)]
        tensors = [t for t, _ in drawn]
        if keep is not None:
            keep(r, tensors, [a for _, a in drawn])
        fs = fit(tensors, k, seed + 1000 + r, max_iters, device_id)
        out.append([np.array(device_views.to_numpy(f), dtype=np.float64) for f in fs])
        del drawn, tensors, fs
    return out


def fit_fp64_on_device(tensors, k: int, phi, xi, psi, n_iters, num_repeats=5, spurious: bool = False, **kw) -> dict:
    """``res_nmtf_inner(precision="fp64", fp64_device=True, output="torch")`` of views that are fp64 tensors on the device,
    k biclusters per view, from the device's SVD start (shared maps from the names in ``kw``): the fit of a stability
    repeat in double precision (``batched.stability_repeat_fp64``); ``kw`` goes on to it."""
    from .api import res_nmtf_inner          # (lazy: api imports this module at its top)
    return res_nmtf_inner(tensors, None, None, None, None, None, [k] * len(tensors), phi, xi, psi, n_iters, num_repeats, spurious,
                          precision="fp64", fp64_device=True, output="torch", **kw)


def reported_error(errs, n_iters) -> float:
    """``R/main.r:126-130``: the mean of the last ten errors of a run to convergence, else the last error."""
    return float(np.mean(errs[-10:])) if n_iters is None else float(errs[-1])


_INNER_KEYS = ("output_f", "output_s", "output_g", "Error", "All_Error", "bisil", "row_clusters", "col_clusters",
               "lambda", "mu", "spurious", "init", "state", "tag", "extras")
_DEVICE_DATA_KEYS = ("output_f", "output_s", "output_g", "row_clusters", "col_clusters", "Error", "All_Error", "tag",
                     "extras", "row_names", "col_names", "init", "lambda", "mu", "data", "device_data", "spurious_check", "device_out")


def inner_result(output_f, output_s, output_g, errs=None, n_iters=None, *, lam=None, mu=None, device_data: bool = False,
                 data_on_device=None, **more) -> dict:
    """The result of ``res_nmtf_inner`` (``R/main.r:115-139``) with its keys in their fixed order -- ``device_data``:
    the order of ``DeviceData.factorise`` (clusters before the errors, no ``"bisil"``).  ``errs``: the error trace, which
    gives ``"Error"``; without it the ``no_clusts`` result.  ``lam``: ``"lambda"``; ``data_on_device``: the key
    ``"device_data"`` (the flag has the name); ``more``: the clusters, ``bisil`` and the optional keys.  A value that is None is left out (``"bisil"`` stays: None = not scored)."""
    vals = dict(more, output_f=output_f, output_s=output_s, output_g=output_g, mu=mu, **{"lambda": lam})
    if data_on_device is not None:
        vals["device_data"] = data_on_device
    if errs is not None:
        vals.update(Error=reported_error(errs, n_iters), All_Error=errs)
        if not device_data:
            vals.setdefault("bisil", None)
    keys = _DEVICE_DATA_KEYS if device_data else _INNER_KEYS
    if not set(vals) <= set(keys):
        raise TypeError(f"not keys of this result: {sorted(set(vals) - set(keys))}")
    return {key: vals[key] for key in keys if key in vals and (vals[key] is not None or key == "bisil")}
