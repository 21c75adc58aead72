"""Host-side mirror of the reference's two exported functions for the path this repository
accelerates: ``res_nmtf_inner`` (``R/main.r:32-140``) and ``apply_resnmtf``
(``R/main.r:214-335``).  Same argument names and meaning, same keys in the result; the
loop itself (update_matrices x T, calculate_error x T, normalisation_check, binary cluster
matrices) runs in the HIP library through the C-ABI.  R is not available in the build or
run environment, so this Python module is the tested stand-in for the thin R wrapper shown
in INTEGRATION.md.

Stability selection (``stability_check``, ``R/stability_analysis.r:302-338``) runs here too: the sub-samples are
gathered, factorised and scored (relevance) on the device, see ``stability_check``.

Spurious-bicluster removal exists as a post-step on a finished result (``check_biclusters`` / ``remove_spurious``,
from ``spurious.py``) and, with the keyword-only opt-in ``spurious_on_device=True``, inside the entry points below as
the reference runs it (``spurious=True``): in ``res_nmtf_inner`` before the bisilhouette, in every stability repeat
before its relevance and for every k of the sweep; the shuffled factorisations are drawn from the engine's own device
copy and scored on the device (``spurious.check_on_device``).  Without the opt-in ``spurious=True`` raises
``NotImplementedError`` as before.  On ``scipy.sparse`` views the removal needs the further opt-in
``shuffle_sparse=True``: their shuffles are drawn on the device as sparse views (``resnmtf_shuffle_view_sparse``).

Copies (the k sweep) and sub-samples (stability selection, its trimming probes included) of ``scipy.sparse`` views are
gathered on the host and uploaded, unless the keyword-only opt-in ``sparse_on_device=True`` is given: then they are made
on the device from the one upload (``resnmtf_copy_view_sparse``, ``resnmtf_subsample_count_sparse`` +
``resnmtf_subsample_view_sparse``).  Same clusters and factors; a sub-sample's ``data_norms`` is then summed from the f32
values the device holds, so ``All_Error`` of the stability repeats may move (tested bar: 1e-6 absolute; not at all when the data are
f32-representable); copies are bitwise.  No effect on dense data.

The bisilhouette score (``bisil``, ``R/obtain_bicl.r:189-199``) is an opt-in here: ``res_nmtf_inner(score_bisil=True)``
scores the result on the device (per-member silhouettes from ``resnmtf_bisil``, combined by ``bisil.py``), and
``apply_resnmtf(k_val=None, k_sweep=True)`` runs the reference's k sweep on it (``R/main.r:269-334``).  Sparse views
are scored only with the further opt-in ``bisil_sparse=True`` (``resnmtf_bisil_sparse``, from the CSC / CSR copies).
Its definition restates the published score (the R package's source is not available): parity with ``bisilhouette`` is
unpinned.
Without the opt-ins ``bisil`` stays ``None`` and ``k_val=None`` raises ``NotImplementedError``, as before.

Under ``precision="fp64"`` the score is computed in double precision on the numbers that were factorised
(``res_nmtf_inner(score_bisil=True, fp64_bisil=True)`` -> ``engine.fp64_bisil`` -> ``resnmtf_fp64_bisil``, no handle), and
``apply_resnmtf(precision="fp64")`` runs a known k or the k sweep on it; with the further opt-in
``fp64_bisil_sparse=True`` sparse views are scored too, stored sparse (``engine.fp64_bisil_sparse`` ->
``resnmtf_fp64_bisil_sparse``), and the fp64 k sweep runs on them.  Spurious-bicluster
removal runs there too with the opt-in ``fp64_spurious=True`` (beside ``spurious_on_device=True``): the shuffles are drawn
from the fp64 values (``engine.fp64_shuffle`` -> ``resnmtf_fp64_shuffle``, no handle) and factorised by the fp64 path
(``problem.shuffled_fits_fp64``).  Stability selection runs there with the opt-in
``fp64_stability=True`` (``stability_check(precision="fp64")``): the sub-samples are gathered from the fp64 values
(``engine.fp64_subsample`` -> ``resnmtf_fp64_subsample``, no handle), factorised by the fp64 path and scored from the
cluster tensors it leaves on the device (``engine.fp64_relevance`` -> ``resnmtf_fp64_relevance``).
With the further opt-in ``fp64_subsample_sparse=True`` the sub-samples of sparse views are gathered sparse
(``engine.fp64_subsample_sparse`` -> ``resnmtf_fp64_subsample_sparse``) and factorised as sparse device views (DESIGN.md
section 31).
"""
from __future__ import annotations

import warnings
from typing import Callable, Optional

import numpy as np

from . import batched, bisil, device_views, naming, sparse
from . import engine as _engine
from . import spurious as _spurious
from .engine import Engine
from .problem import couple, inner_result, prepare, svd_init  # noqa: F401  (svd_init: part of this module's surface)
from .spurious import check_biclusters, remove_spurious  # noqa: F401  (post-steps, R/obtain_bicl.r:113-188)

_DISTANCES = ("euclidean", "manhattan", "cosine")


def _as_list(x):
    if ((isinstance(x, np.ndarray) and x.ndim == 2) or sparse.is_sparse(x)
            or isinstance(x, (device_views.RawDeviceView, device_views.SparseDeviceView))):
        return [x]                      # check_lists, R/utils.r:313-316
    if device_views.is_tensor(x):       # one tensor is one view (never a list of its rows)
        (device_views.check_sparse_tensor if device_views.is_sparse_tensor(x) else device_views.check_tensor)(x)
        return [x]
    return list(x)


def _views(data, device_id: int = 0) -> list:
    """The views as fp64 arrays; a ``scipy.sparse`` view becomes a canonical CSC copy (``sparse.canonical_csc``: the
    caller's matrix is not modified) and stays sparse on the device (``resnmtf_create_sparse``); a ``torch`` tensor on
    ``cuda:device_id`` stays the tensor it is (``device_views.as_view``: 2-D, floating, on that device, else
    ``ValueError``; a CPU tensor becomes its fp64 array); a sparse tensor on that device becomes its
    ``device_views.SparseDeviceView`` and is a sparse view too (a CPU one: its ``scipy.sparse`` matrix)."""
    data = [device_views.host_or_device(d, f"view {v}") for v, d in enumerate(_as_list(data))]      # (a CPU sparse tensor: scipy)
    return [sparse.canonical_csc(d) if sparse.is_sparse(d) else device_views.as_view(d, device_id, f"view {v}")
            for v, d in enumerate(data)]


def _load_engine(eng: Engine, data, init_f, init_s, init_g, lam, mu, phi, xi, psi,
                 row_names, col_names, row_indices, column_indices, seed=None, device_factors=None):
    """``init_f is None``: the initial factors come from the device (``resnmtf_init_svd``).  ``device_factors[v]``
    (``device_views.factor_routes``): view v's initial factors are device tensors and go in through
    ``Engine.set_factors_device``."""
    for v in range(eng.n_views):
        if eng.owned[v]:
            if isinstance(data[v], device_views.SparseDeviceView):
                device_views.upload_sparse(eng, v, data[v], pre_processed=True)                        # (in place, taken as given)
            elif sparse.is_sparse(data[v]):
                eng.set_view_sparse(v, data[v], pre_processed=True)                                    # (already pre-processed)
            else:
                device_views.upload(eng, v, data[v])                                                   # (a tensor: in place)
        if init_f is None:
            eng.init_svd(v, seed=_seed(seed) + v)                          # update_steps.r:78-125
        elif device_factors is not None and device_factors[v]:
            eng.set_factors_device(v, init_f[v], init_s[v], init_g[v],
                                   None if lam is None else lam[v], None if mu is None else mu[v])
        else:
            eng.set_factors(v, init_f[v], init_s[v], init_g[v],
                            None if lam is None else device_views.to_numpy(lam[v]),
                            None if mu is None else device_views.to_numpy(mu[v]))
    eng.set_restrictions(phi, xi, psi)
    couple(eng, row_names, col_names, row_indices, column_indices)


def res_nmtf_inner(data, row_indices, column_indices,
                   init_f=None, init_s=None, init_g=None,
                   k_vec=None, phi=None, xi=None, psi=None,
                   n_iters=None, num_repeats=5, spurious=True, distance="euclidean",
                   no_clusts=False, *, row_names=None, col_names=None, device_id: int = 0,
                   max_iters: int = 100000, seed: Optional[int] = None, engine_opts: Optional[dict] = None,
                   host_init: bool = False, return_init: bool = False, score_bisil: bool = False,
                   spurious_on_device: bool = False, bisil_sparse: bool = False, shuffle_sparse: bool = False,
                   sparse_on_device: bool = False, output: str = "numpy", init_lm=None, return_state: bool = False,
                   post_on_device: bool = False, precision: str = "f32", fp64_sparse: bool = False,
                   fp64_device: bool = False, fp64_sparse_device: bool = False, fp64_bisil: bool = False,
                   fp64_spurious: bool = False, fp64_bisil_sparse: bool = False, fp64_shuffle_sparse: bool = False,
                   fp64_init: bool = False):
    """``res_nmtf_inner`` (``R/main.r:32-140``).

    ``data``: list of pre-processed (non-negative, column-normalised) matrices; ``row_indices[v][w]``
    / ``column_indices[v][w]``: shared names between views v and w or None (NA), as produced by
    ``naming.shared_names``; ``phi/xi/psi``: symmetrised restriction matrices (the reference's
    ``res_nmtf_inner`` needs them non-NULL, ``R/update_steps.r:150``); ``n_iters=None`` runs to
    convergence.  Keyword-only extras: ``row_names``/``col_names`` (the reference reads them off
    the matrices' dimnames), ``max_iters`` (a guard the reference lacks), ``seed`` for the SVD
    init noise, ``host_init`` (without explicit initial factors: ``False`` = ``init_mats_inner`` on
    the device, randomized top-k SVD on the pass kernels, milliseconds; ``True`` = NumPy's full SVD
    on the host as the reference's ``svd()``, seconds to minutes -- statistically equivalent),
    ``return_init`` (adds ``"init"``: the (F, S, G, lambda, mu) per view the loop started from), ``score_bisil``
    (``"bisil"`` holds the bisilhouette score of the result under ``distance``, computed on the device before the
    engine closes, ``bisil.score``; dense views only unless ``bisil_sparse``; default ``None`` as before),
    ``bisil_sparse`` (opt-in: ``score_bisil`` then scores sparse views too, from their CSC / CSR copies on the device,
    ``Engine.bisil_sparse`` -- bitwise the score of the densified view; no effect on dense views),
    ``spurious_on_device`` (with
    ``spurious=True``: ``obtain_biclusters(remove_spurious = TRUE)``, ``R/obtain_bicl.r:151-204`` -- ``num_repeats``
    shuffles of the engine's own views, to convergence, scored on the device, the flagged cluster columns zeroed through
    ``relations``, then ``bisil`` of the cleaned clusters; the result carries ``"spurious"`` as ``remove_spurious``
    does and equals ``remove_spurious(data, res_nmtf_inner(..., spurious=False, seed=seed), num_repeats, seed=seed)``:
    the shuffles use the spurious seed ``0 if seed is None else seed``, repeat r initialising with ``+ 1000 + r`` and
    shuffling with ``seed * 7919 + r + 1``, as ``check_biclusters`` derives them; dense views only unless
    ``shuffle_sparse``), ``shuffle_sparse`` (opt-in: the removal then runs on sparse views too -- each is shuffled on the
    device as a sparse view, ``Engine.shuffle_view_sparse_from``: the dense path's draw of the densified view, same seeds,
    same redraw rule; a view with fewer stored entries than ``max(n, m)`` raises ``ValueError``, no shuffle of it can pass
    the rule; pass the same flag to ``remove_spurious`` for the identity above; no effect on dense views),
    ``sparse_on_device`` (a no-op here by design, DESIGN.md section 10: accepted so that callers pass one set of flags to
    every entry point; this function uploads ``data`` itself and its spurious children are shuffles, which always draw
    from the engine's own handle, so it has no copy or sub-sample to route), ``output`` (``"numpy"``, or ``"torch"``:
    ``output_f`` / ``output_s`` / ``output_g`` / ``row_clusters`` / ``col_clusters`` are then fp64 ``torch`` tensors on
    ``cuda:device_id``, written there by ``Engine.finalise_device`` -- bitwise the NumPy result; the small values stay
    NumPy).

    A view may also be a 2-D floating ``torch`` tensor on ``cuda:device_id`` (fp64 / fp32 / fp16 / bf16, any strides;
    mixed freely with NumPy and ``scipy.sparse`` views): it is uploaded in place (``Engine.set_view_device``), bitwise
    as ``t.double().cpu().numpy()`` would be, and never converted to NumPy.  A CPU tensor is taken as its NumPy array.
    ``ValueError`` for a non-floating dtype, another device, or a tensor that is not 2-D; ``host_init=True`` without
    explicit initial factors raises ``NotImplementedError`` for such a view, as for a sparse one.

    A 2-D ``sparse_csc`` / ``sparse_csr`` / coalesced ``sparse_coo`` tensor on ``cuda:device_id`` is a SPARSE view
    (DESIGN.md section 16): uploaded from its own arrays (``Engine.set_view_sparse_device``, values taken as given), checked
    on the device -- its refusals surface as ``ResnmtfError`` --, bitwise the ``scipy.sparse`` view of the same values and
    never brought to the host.  Everything said of sparse views above holds for it; a CPU sparse tensor is taken as its
    ``scipy.sparse`` matrix.

    Initial factors may be ``torch`` tensors too.  Per view, ``init_f[v]``, ``init_s[v]`` and
    ``init_g[v]`` that are all tensors on ``cuda:device_id`` (2-D, fp64 / fp32 / fp16 / bf16, any strides) are read in
    place (``Engine.set_factors_device``), bitwise as ``t.double().cpu().numpy()`` would be; all three on the host (NumPy,
    or a CPU tensor, taken as its fp64 array) take the host route; a mix within one view, or a tensor on another
    device, is a ``ValueError`` before any engine exists.  ``init_lm`` (keyword-only): ``(lambdas, mus)``, one entry of
    k values per view, taken in place of ``colSums(init_f[v])`` / ``colSums(init_g[v])`` (``R/update_steps.r:55-56``);
    needs explicit initial factors.  ``return_state`` (keyword-only) adds ``"state"``: per view the raw ``(F, S, G, lambda,
    mu)`` after the last sweep -- ``Engine.get_factors`` with ``output="numpy"``, ``Engine.get_factors_device`` (fp64
    tensors on the device) with ``output="torch"``; with ``output="torch"``, ``"init"`` comes from the device as well.

    Resuming: a call given another call's ``"state"`` as ``init_f`` / ``init_s`` / ``init_g`` and ``init_lm`` continues it.
    With a fixed ``n_iters`` the two calls together are bit for bit the one uninterrupted call (``All_Error``
    concatenated, the state and the outputs).  In convergence mode (``n_iters=None``) the first stop test after a resume
    compares with 0, as that of any fresh run does (``R/main.r:53-54``): the previous mean error is not carried over, so
    the stop sweep can differ, and only when the uninterrupted run would have stopped on the first resumed sweep.

    ``post_on_device`` (keyword-only opt-in; needs ``output="torch"``, else ``ValueError``): the
    steps after the loop stay on the device.  ``Engine.finalise`` and ``Engine.get_factors`` are not called: F, S, G and
    the clusters come from ``Engine.finalise_device``, lambda and mu from ``Engine.get_factors_device`` (those two
    k-vectors are copied to the host: the result keeps its types); the removal is ``spurious.apply_removal_device`` (the
    k x k S copied to the host, the flagged columns zeroed in clones of the cluster tensors) and ``bisil`` is scored from
    the cleaned tensors (``Engine.bisil_device``: silhouettes and their combination on the device).  The result equals
    the same call without the flag key for key, bit for bit.

    ``precision`` (keyword-only; ``"f32"``, the default, is everything above, untouched; anything but ``"f32"`` or
    ``"fp64"`` is a ``ValueError``): ``"fp64"`` runs the loop through ``engine.fp64_run`` -- the
    reference's arithmetic in double on the whole device, at any size, k up to 64 and one k for all views, at most 8
    views.  Views are dense NumPy arrays or CPU tensors; restrictions and names as above; the initial state is the explicit factors
    (with ``init_lm`` if given), ``svd_init`` with ``host_init=True``, else the device's own SVD initialisation (an engine
    is built, loaded, initialised, read with ``get_factors`` and closed: the start ``return_init`` reports).  The result
    has the keys and types of the f32 call; ``return_init`` is honoured.  What needs a live handle is refused before any
    device work with a ``NotImplementedError`` naming the flag: ``spurious=True`` with ``spurious_on_device``,
    ``score_bisil``, ``output="torch"``, ``post_on_device``, ``return_state``, sparse views, views or factors in device
    memory.

    ``fp64_sparse`` (keyword-only opt-in; a no-op with ``precision="f32"``): with
    ``precision="fp64"``, ``scipy.sparse`` views (a CPU sparse tensor is taken as its SciPy matrix) are accepted,
    validated as on the f32 route, and stored and streamed sparse (``resnmtf_fp64_run_sparse``); dense and sparse views
    mix.  The initial state is the explicit factors (with ``init_lm``) or the device's SVD initialisation through a
    short-lived sparse engine; ``host_init=True`` without explicit factors raises ``NotImplementedError``, as on the f32
    route.  Sparse tensors in device memory stay refused (``fp64_sparse_device`` admits them), and without the flag sparse
    views are refused as before.

    ``fp64_device`` (keyword-only opt-in; a no-op with ``precision="f32"``): with
    ``precision="fp64"``, dense views, initial factors and ``init_lm`` may be ``torch`` tensors on ``cuda:device_id`` (read
    where they lie, ``resnmtf_fp64_run_device``: bitwise ``t.double().cpu().numpy()`` through the host route), and
    ``output="torch"`` and ``return_state`` (which needs ``output="torch"``, else ``ValueError``) are honoured: F, S, G,
    lambda, mu and the raw state stay on the device, and the cluster matrices are built there from F, G and S (bitwise the
    host's).  The device's SVD initialisation then stays on the device too: the short-lived engine is loaded with
    ``set_view_device`` and read with ``get_factors_device``.  Combines with ``fp64_sparse`` (host ``scipy.sparse`` views
    beside device dense views).  Still refused: ``score_bisil``, ``spurious_on_device``, ``post_on_device`` and sparse
    tensors in device memory.  Without the flag every refusal above stands word for word.

    ``fp64_sparse_device`` (keyword-only opt-in; a no-op with ``precision="f32"``): with
    ``precision="fp64"``, a 2-D ``sparse_csc`` / ``sparse_csr`` / coalesced ``sparse_coo`` tensor on ``cuda:device_id`` (or
    its ``device_views.SparseDeviceView``) is a sparse view of the fp64 path too, read where it lies
    (``resnmtf_fp64_run_sparse_device``): taken as pre-processed, checked and sorted on the device -- its refusals surface
    as ``ResnmtfError`` --, never brought to the host.  The result is bit for bit that of the ``scipy.sparse`` matrix of
    the same stored entries under ``fp64_sparse``, with one difference: an explicitly stored zero stays stored on this
    route, while ``sparse.canonical_csc`` drops it on the host route.  Such views mix with everything ``fp64_sparse`` and
    ``fp64_device`` admit.  Without explicit factors the start is the device's SVD initialisation through a short-lived
    sparse engine loaded with ``set_view_sparse_device(pre_processed=True)`` (read with ``get_factors_device`` under
    ``fp64_device``); ``host_init=True`` then raises the sparse views' ``NotImplementedError``.  ``return_init``,
    ``output="torch"`` and ``return_state`` behave as described above.  Without the flag every refusal above stands word
    for word, the one of sparse tensors under ``fp64_device=True`` included.

    ``fp64_bisil`` (keyword-only opt-in; a no-op with ``precision="f32"``): with
    ``precision="fp64"``, ``score_bisil`` is honoured: ``"bisil"`` is ``bisil.score`` of the result's clusters over
    ``engine.fp64_bisil`` -- the per-member silhouettes in double precision (``resnmtf_fp64_bisil``, no handle), computed
    on the views exactly as the run received them: a host view is uploaded once more for the scoring, a device tensor
    (``fp64_device``) is read where it lies.  The cluster matrices are brought to the host (n k + m k values per view)
    and the score is combined there.  Combines with ``fp64_device`` and ``output="torch"``.  A sparse view with
    ``score_bisil`` raises a ``NotImplementedError`` naming ``fp64_bisil`` and sparse views.
    ``fp64_bisil_sparse`` (keyword-only opt-in; read only with ``precision="fp64"``, ``score_bisil``
    and ``fp64_bisil=True``, a no-op everywhere else): the sparse views that ``fp64_sparse`` / ``fp64_sparse_device`` admit
    are scored too, through ``engine.fp64_bisil_sparse`` (``resnmtf_fp64_bisil_sparse``: bit for bit ``engine.fp64_bisil``
    of the densified view, without densifying it), dense views through ``engine.fp64_bisil`` as before, and the two
    combine in ``bisil.score``.  Mixed view lists and ``output="torch"`` work.  Without it the refusal above stands.
    ``fp64_spurious`` (keyword-only opt-in; a no-op with ``precision="f32"``): with
    ``precision="fp64"``, ``spurious=True`` and ``spurious_on_device=True`` the removal runs in double precision: after the
    run, ``check_biclusters(data, F, num_repeats, seed=seed, precision="fp64")`` on the views exactly as the run received
    them (host arrays or dense device tensors) -- every shuffle drawn by ``engine.fp64_shuffle`` and factorised by the
    fp64 path (``problem.shuffled_fits_fp64``) --, then the removal, then ``bisil`` of the cleaned clusters (with
    ``score_bisil`` and ``fp64_bisil``); the result carries ``"spurious"`` and equals ``remove_spurious(data,
    res_nmtf_inner(..., precision="fp64", spurious=False, seed=seed), num_repeats, seed=seed, precision="fp64")``.  A
    sparse view with it is refused by name (no fp64 sparse shuffle exists).  Without the flag every
    refusal above stands word for word.
    ``fp64_shuffle_sparse`` (keyword-only opt-in; read only with ``precision="fp64"`` and
    ``fp64_spurious=True``, a no-op everywhere else): the sparse views that ``fp64_sparse`` / ``fp64_sparse_device`` admit
    are shuffled sparse (``engine.fp64_shuffle_sparse`` -> ``resnmtf_fp64_shuffle_sparse``: the dense draw of the densified
    view at the stored positions, without densifying it) and the draws factorised as sparse device views; dense views go
    through ``engine.fp64_shuffle`` as before, and mixed view lists work.  The result equals ``remove_spurious(data, plain
    result, num_repeats, seed=seed, precision="fp64", fp64_shuffle_sparse=True)``.  Without it the refusal above stands.
    ``fp64_init`` (keyword-only opt-in; a no-op with ``precision="f32"``): read only where the fp64
    call builds its short-lived engine -- no explicit factors and ``host_init=False``.  The start then comes from
    ``engine.fp64_init_svd`` (``resnmtf_fp64_init_svd``: ``init_mats_inner``, ``R/update_steps.r:78-125``, on the fp64 values
    of the views, same seeds ``seed + v``) and no ``Engine`` is constructed: on the device under ``fp64_device``, from the
    sparse sources under ``fp64_sparse`` / ``fp64_sparse_device``.  ``return_init`` reports this start.  The flag passes on
    to the shuffled fits of ``fp64_spurious``.  Without it every call, result and refusal is what it was.
    """
    if precision not in ("f32", "fp64"):
        raise ValueError(f"precision must be 'f32' or 'fp64', got {precision!r}")
    if precision == "fp64":
        return _res_nmtf_inner_fp64(data, row_indices, column_indices, init_f, init_s, init_g, k_vec, phi, xi, psi, n_iters,
                                    spurious, distance, no_clusts, row_names=row_names, col_names=col_names,
                                    device_id=device_id, max_iters=max_iters, seed=seed, engine_opts=engine_opts,
                                    host_init=host_init, return_init=return_init, score_bisil=score_bisil,
                                    spurious_on_device=spurious_on_device, output=output, init_lm=init_lm,
                                    return_state=return_state, post_on_device=post_on_device, fp64_sparse=fp64_sparse,
                                    fp64_device=fp64_device, fp64_sparse_device=fp64_sparse_device, fp64_bisil=fp64_bisil,
                                    fp64_spurious=fp64_spurious, num_repeats=num_repeats, fp64_bisil_sparse=fp64_bisil_sparse,
                                    fp64_shuffle_sparse=fp64_shuffle_sparse, fp64_init=fp64_init)
    device_views.check_output(output)
    _check_post_on_device(post_on_device, output)
    data = _views(data, device_id)
    n_v = len(data)
    if k_vec is None:
        raise ValueError("k_vec is required")
    k_vec = [int(k) for k in np.atleast_1d(k_vec)]
    if len(k_vec) != n_v:
        raise ValueError("k_vec must be a vector of the same length as the number of views.")   # utils.r:440
    remove = bool(spurious) and not no_clusts
    _refuse_host_spurious(remove, spurious_on_device,
                          "spurious-bicluster removal (R/obtain_bicl.r:31-133) is outside the accelerated path; "
                          "pass spurious=False or do it on the R side (INTEGRATION.md).")
    _check_distance(distance)
    is_sp = [sparse.is_sparse_view(d) for d in data]
    if remove:
        _spurious.check_num_repeats(num_repeats)
        if any(is_sp) and not shuffle_sparse:
            raise NotImplementedError("spurious-bicluster removal needs shuffled views: device shuffles of sparse views "
                                      "are not supported")
    for v in range(n_v):
        if is_sp[v] and sparse.is_sparse(data[v]):      # (a sparse tensor in device memory: the device checks stand in)
            sparse.validate(data[v], f"view {v}")
    if score_bisil and any(is_sp) and not bisil_sparse:
        raise NotImplementedError("the bisilhouette score of sparse views is not supported (dense views only)")
    if any(is_sp) and host_init and (init_f is None or init_g is None or init_s is None):
        raise NotImplementedError("host_init=True (NumPy's dense SVD) is not available for sparse views; the device "
                                  "initialisation (host_init=False) works on them")
    if any(device_views.is_device_view(d) for d in data) and host_init and (init_f is None or init_g is None or init_s is None):
        raise NotImplementedError("host_init=True (NumPy's dense SVD) is not available for views in device memory; the "
                                  "device initialisation (host_init=False) works on them")
    phi, xi, psi = (np.zeros((n_v, n_v)) if m is None else np.asarray(m, dtype=np.float64) for m in (phi, xi, psi))
    row_names, col_names = naming.give_names(data, None, None, row_names, col_names)

    lam = mu = None
    if init_f is None or init_g is None or init_s is None:                                        # update_steps.r:41
        init_f = init_s = init_g = None
        if host_init:
            init_f, init_s, init_g, lam, mu = svd_init(data, k_vec, seed)
    device_factors = None
    if init_f is not None:
        init_f, init_s, init_g = _as_list(init_f), _as_list(init_s), _as_list(init_g)
        if lam is None:                           # (svd_init's own factors are host arrays)
            device_factors, init_f, init_s, init_g = device_views.factor_routes(init_f, init_s, init_g, device_id)
    if init_lm is not None:
        if init_f is None or lam is not None:
            raise ValueError("init_lm needs explicit initial factors (init_f, init_s and init_g)")
        lam, mu = device_views.check_init_lm(init_lm, n_v)

    eng = Engine([d.shape[0] for d in data], [d.shape[1] for d in data], k_vec, device_id=device_id,
                 nnz=[d.nnz if sp else None for d, sp in zip(data, is_sp)], **(engine_opts or {}))
    try:
        _load_engine(eng, data, init_f, init_s, init_g, lam, mu, phi, xi, psi,
                     row_names, col_names, row_indices, column_indices, seed=seed, device_factors=device_factors)
        raw_state = eng.get_factors_device if output == "torch" else eng.get_factors
        init_state = [raw_state(v) for v in range(n_v)] if return_init else None      # (F, S, G, lambda, mu) the loop starts from
        total_err = eng.run(n_iters=n_iters, tol=1.0e-6, max_iters=max_iters)
        state = [raw_state(v) for v in range(n_v)] if return_state else None          # ... and the one it ended in
        # per view: F, S, G, the binary clusters (main.r:110 + obtain_bicl.r:162-180), lambda, mu
        if post_on_device:               # everything of size n or m stays where it is; the two k-vectors come to the host
            out_f, out_s, out_g, row_cl, col_cl, lams, mus = (
                list(x) for x in zip(*[(*eng.finalise_device(v), *(device_views.to_numpy(t) for t in eng.get_factors_device(v)[3:]))
                                       for v in range(n_v)]))
            on_device = None
        else:
            out_f, out_s, out_g, row_cl, col_cl, lams, mus = (
                list(x) for x in zip(*[(*eng.finalise(v), *eng.get_factors(v)[3:]) for v in range(n_v)]))
            on_device = [eng.finalise_device(v) for v in range(n_v)] if output == "torch" else None
        check = (_spurious.check_on_device(eng, num_repeats, seed, max_iters=max_iters, device_id=device_id,
                                           shuffle_sparse=shuffle_sparse)
                 if remove else None)                                                             # obtain_bicl.r:151-188
        score_fn = ((lambda rc, cc: bisil.score(rc, cc, distance, engine=eng, sparse_views=bisil_sparse))
                    if score_bisil and not no_clusts else None)                                   # obtain_bicl.r:189-199
        cleaned = _remove_then_score({"output_s": out_s, "row_clusters": row_cl, "col_clusters": col_cl}, check, score_fn,
                                     on_device=post_on_device)
    finally:
        eng.close()
    # ("init": a test hook, the initial state the device built, for a reference run from the same start)
    if on_device is not None:        # the host steps above read the NumPy copies; what is returned lives on the device
        out_f, out_s, out_g = _device_outputs(on_device, row_cl, col_cl, cleaned)
    if no_clusts:                                                                                 # main.r:115-120
        return inner_result(out_f, out_s, out_g, init=init_state, state=state)
    # ("bisil": None unless score_bisil; bisil.py, parity with bisilhouette::bisilhouette unpinned)
    return inner_result(out_f, out_s, out_g, total_err, n_iters, bisil=cleaned.get("bisil"),
                        row_clusters=cleaned["row_clusters"], col_clusters=cleaned["col_clusters"], lam=lams, mu=mus,
                        spurious=cleaned.get("spurious"), init=init_state, state=state)


def _res_nmtf_inner_fp64(data, row_indices, column_indices, init_f, init_s, init_g, k_vec, phi, xi, psi, n_iters, spurious,
                         distance, no_clusts, *, row_names, col_names, device_id, max_iters, seed, engine_opts, host_init,
                         return_init, score_bisil, spurious_on_device, output, init_lm, return_state, post_on_device,
                         fp64_sparse: bool = False, fp64_device: bool = False, fp64_sparse_device: bool = False,
                         fp64_bisil: bool = False, runner: Optional[Callable] = None, sil: Optional[Callable] = None,
                         fp64_spurious: bool = False, num_repeats=5, checker: Optional[Callable] = None,
                         fp64_bisil_sparse: bool = False, fp64_shuffle_sparse: bool = False, fp64_init: bool = False):
    """``res_nmtf_inner(precision="fp64")``: the checks of the f32 call, the refusals of what needs a live handle, the
    initial state, then one ``engine.fp64_run`` (``runner`` replaces it: a test hook).  ``fp64_device``: views, factors
    and results may live in device memory (``res_nmtf_inner``'s docstring); the runner then also gets ``output`` and
    ``return_state``.  ``fp64_sparse_device``: a sparse tensor on ``cuda:device_id`` reaches the problem as its
    ``SparseDeviceView`` -- the same tensor, untouched.  ``fp64_bisil``: ``score_bisil`` is honoured through
    ``engine.fp64_bisil`` on the views as they arrived (``sil(v, rc, cc, distance)`` replaces it: a test hook);
    ``fp64_bisil_sparse``: a sparse view then goes to ``engine.fp64_bisil_sparse`` instead of being refused.
    ``fp64_spurious``: ``spurious=True`` with ``spurious_on_device`` is honoured through
    ``spurious.check_biclusters(..., precision="fp64")`` on the views as they arrived (``checker`` replaces it: a test
    hook), then ``_remove_then_score``; ``fp64_shuffle_sparse``: a sparse view is then shuffled sparse (section 30) instead
    of being refused, and the checker gets the flag.  ``fp64_init``: without explicit factors and ``host_init`` the start
    is ``engine.fp64_init_svd``'s (section 32) and no engine is built; the checker gets the flag."""
    def refuse(flag):
        raise NotImplementedError(f'precision="fp64": {flag} needs a live engine handle, which the fp64 path does not '
                                  'keep (it runs through resnmtf_fp64_run); use precision="f32" for it')
    device_views.check_output(output)
    remove = bool(spurious) and not no_clusts
    for flag, on in (("spurious_on_device", remove and spurious_on_device and not fp64_spurious),
                     ("score_bisil", score_bisil and not fp64_bisil),
                     ("post_on_device", post_on_device), ('output="torch"', output == "torch" and not fp64_device),
                     ("return_state", return_state and not fp64_device)):
        if on:
            refuse(flag)
    if return_state and output != "torch":
        raise ValueError("precision=\"fp64\": return_state=True needs output='torch' (the raw state is left on the device)")
    _refuse_host_spurious(remove, spurious_on_device,
                          "spurious-bicluster removal (R/obtain_bicl.r:31-133) is outside the accelerated path; "
                          "pass spurious=False or do it on the R side (INTEGRATION.md).")
    _check_distance(distance)
    views = []
    for v, d in enumerate(_as_list(data)):
        d = device_views.host_or_device(d, f"view {v}")      # (a CPU sparse tensor: its scipy.sparse matrix)
        if fp64_sparse and sparse.is_sparse(d):              # opt-in: stored and streamed sparse (resnmtf_fp64_run_sparse)
            d = sparse.canonical_csc(d)
            sparse.validate(d, f"view {v}")
            views.append(d)
            continue
        if fp64_sparse_device and device_views.is_sparse_device_view(d):      # opt-in: read where it lies (section 24)
            views.append(device_views.as_sparse_view(d, device_id, f"view {v}"))
            continue
        if sparse.is_sparse_view(d) or device_views.is_sparse_tensor(d):
            refuse(f"sparse views (view {v})")
        if device_views.is_device_view(d):
            if not (fp64_device and device_views.is_tensor(d)):
                refuse(f"views in device memory (view {v})")
            views.append(device_views.as_view(d, device_id, f"view {v}"))      # (checked; read where it lies)
            continue
        views.append(np.asarray(d, dtype=np.float64))
    data, n_v = views, len(views)
    is_sp = [sparse.is_sparse_view(d) for d in data]
    if remove:                                    # (here: spurious_on_device and fp64_spurious are set, or the call was refused)
        _spurious.check_num_repeats(num_repeats)
        if not fp64_shuffle_sparse:
            _spurious.refuse_sparse_fp64(data)
    score = bool(score_bisil) and not no_clusts                  # (here: fp64_bisil is set, or the call was refused above)
    if score and any(is_sp) and not fp64_bisil_sparse:
        raise NotImplementedError(f'precision="fp64": score_bisil with fp64_bisil=True scores dense views only; sparse views '
                                  f'(view {is_sp.index(True)}) are not supported by resnmtf_fp64_bisil')
    if any(device_views.is_device_view(d) and not is_sp[v] for v, d in enumerate(data)) and host_init and (init_f is None or init_g is None or init_s is None):
        raise NotImplementedError("host_init=True (NumPy's dense SVD) is not available for views in device memory; the "
                                  "device initialisation (host_init=False) works on them")
    if any(is_sp) and host_init and (init_f is None or init_g is None or init_s is None):
        raise NotImplementedError("host_init=True (NumPy's dense SVD) is not available for sparse views; the device "
                                  "initialisation (host_init=False) works on them")
    if k_vec is None:
        raise ValueError("k_vec is required")
    k_vec = [int(k) for k in np.atleast_1d(k_vec)]
    if len(k_vec) != n_v:
        raise ValueError("k_vec must be a vector of the same length as the number of views.")   # utils.r:440
    if len(set(k_vec)) != 1:
        raise ValueError('precision="fp64" takes one k for all views (resnmtf_fp64_run)')
    lam = mu = None
    if init_f is None or init_g is None or init_s is None:
        init_f = init_s = init_g = None
    else:
        init_f, init_s, init_g = _as_list(init_f), _as_list(init_s), _as_list(init_g)
        if not fp64_device and any(device_views.is_device_tensor(x) for x in (*init_f, *init_s, *init_g)):
            refuse("factors in device memory")
        _, init_f, init_s, init_g = device_views.factor_routes(init_f, init_s, init_g, device_id)
    if init_lm is not None:
        if init_f is None:
            raise ValueError("init_lm needs explicit initial factors (init_f, init_s and init_g)")
        lam, mu = device_views.check_init_lm(init_lm, n_v)
        if not fp64_device and any(device_views.is_device_tensor(x) for x in (*lam, *mu)):
            refuse("factors in device memory")
        if not fp64_device:
            lam, mu = [device_views.to_numpy(x) for x in lam], [device_views.to_numpy(x) for x in mu]
    phi, xi, psi = (np.zeros((n_v, n_v)) if m is None else np.asarray(m, dtype=np.float64) for m in (phi, xi, psi))
    row_names, col_names = naming.give_names(data, None, None, row_names, col_names)
    batched._check_group_limits(0, data, k_vec[0], batched.FP64_LIMITS)

    if init_f is None and host_init:
        init_f, init_s, init_g, lam, mu = svd_init(data, k_vec, seed)
    elif init_f is None and fp64_init:            # init_mats_inner on the fp64 values, without an engine (section 32)
        start = _engine.fp64_init_svd(data, k_vec[0], seed=_seed(seed), output="torch" if fp64_device else "numpy",
                                      device_id=device_id)
        init_f, init_s, init_g, lam, mu = (list(x) for x in zip(*start))
    elif init_f is None:                          # the device's own SVD initialisation: the start the f32 call reports
        more = {"nnz": [d.nnz if sp else None for d, sp in zip(data, is_sp)]} if any(is_sp) else {}      # (a short-lived sparse engine)
        eng = Engine([d.shape[0] for d in data], [d.shape[1] for d in data], k_vec, device_id=device_id, **more,
                     **(engine_opts or {}))
        try:
            _load_engine(eng, data, None, None, None, None, None, phi, xi, psi, row_names, col_names, row_indices,
                         column_indices, seed=seed)
            # (fp64_device: the start stays on the device and is handed straight to the run)
            start = eng.get_factors_device if fp64_device else eng.get_factors
            init_f, init_s, init_g, lam, mu = (list(x) for x in zip(*[start(v) for v in range(n_v)]))
        finally:
            eng.close()
    problem = {"data": data, "k": k_vec[0], "init_f": list(init_f), "init_s": list(init_s), "init_g": list(init_g),
               "init_lam": None if lam is None else list(lam), "init_mu": None if mu is None else list(mu),
               "phi": phi, "xi": xi, "psi": psi, "row_pairs": batched.pair_table(row_names, row_indices),
               "col_pairs": batched.pair_table(col_names, column_indices), "n_iters": n_iters}
    init_state = None
    if return_init:                               # (F, S, G, lambda, mu) the loop starts from; None lambda / mu: the colSums
        def held(a):                              # as the result holds it: an fp64 tensor on the device, or an fp64 array
            if output == "torch":
                import torch
                return (a.detach() if device_views.is_tensor(a) else torch.as_tensor(np.asarray(a, dtype=np.float64))).to(
                    device=torch.device("cuda", int(device_id)), dtype=torch.float64)
            return np.array(device_views.to_numpy(a.detach().double()) if device_views.is_tensor(a) else a, dtype=np.float64)
        init_state = []
        for v in range(n_v):
            f0, s0, g0 = held(init_f[v]), held(init_s[v]), held(init_g[v])
            init_state.append((f0, s0, g0, f0.sum(0) if lam is None or lam[v] is None else held(lam[v]),
                               g0.sum(0) if mu is None or mu[v] is None else held(mu[v])))
    more = {"output": output, "return_state": return_state} if fp64_device else {}
    out = (runner or _engine.fp64_run)(problem, tol=1.0e-6, max_iters=max_iters, device_id=device_id, **more)
    state = out.get("state") if return_state else None
    if no_clusts:                                                                                 # main.r:115-120
        return inner_result(out["f"], out["s"], out["g"], init=init_state, state=state)
    clusters = _binary_clusters_device if output == "torch" else batched._binary_clusters
    rcs, ccs = zip(*[clusters(f, g, s) for f, g, s in zip(out["f"], out["g"], out["s"])])
    check = None
    if remove:                                    # obtain_bicl.r:151-188, on the numbers that were factorised (section 27)
        flag = {"fp64_shuffle_sparse": True} if fp64_shuffle_sparse else {}      # (only then: every other call is the one it was)
        if fp64_init:
            flag["fp64_init"] = True
        check = (checker or _spurious.check_biclusters)(data, out["f"], num_repeats, seed=seed, device_id=device_id,
                                                        max_iters=max_iters, precision="fp64", **flag)
    score_fn = None
    if score:                                     # obtain_bicl.r:189-199, on the numbers that were factorised (section 26)
        if sil is None:
            def sil(v, rc, cc, distance):      # (a sparse view is here only with fp64_bisil_sparse: section 29)
                one = _engine.fp64_bisil_sparse if is_sp[v] else _engine.fp64_bisil
                return one(data[v], rc, cc, distance, device_id=device_id)

        def score_fn(rcs, ccs):
            return bisil.score([device_views.to_numpy(rc) for rc in rcs], [device_views.to_numpy(cc) for cc in ccs],
                               distance, sil=sil)
    cleaned = _remove_then_score({"output_s": out["s"], "row_clusters": list(rcs), "col_clusters": list(ccs)}, check, score_fn,
                                 on_device=output == "torch")
    return inner_result(out["f"], out["s"], out["g"], np.asarray(out["all_error"], dtype=np.float64), n_iters,
                        bisil=cleaned["bisil"], row_clusters=cleaned["row_clusters"], col_clusters=cleaned["col_clusters"],
                        lam=out["lambda"], mu=out["mu"], spurious=cleaned.get("spurious"), init=init_state, state=state)


def _binary_clusters_device(f, g, s):
    """``batched._binary_clusters`` of F, G and S in device memory, built there: the comparisons with 1/n and 1/m are
    exact, and ``argmax`` takes the first maximum of every S column as NumPy's does, so the matrices are bitwise the
    host's."""
    import torch
    rc = (f > 1.0 / f.shape[0]).to(torch.float64)
    cc = (g > 1.0 / g.shape[0]).to(torch.float64)
    return rc[:, torch.argmax(s, dim=0)], cc


def _device_outputs(on_device, row_cl, col_cl, cleaned: dict):
    """``output="torch"``: ``on_device`` holds ``Engine.finalise_device``'s five tensors per view, ``row_cl`` / ``col_cl``
    the NumPy clusters ``finalise`` gave and ``cleaned`` what the host steps made of them (spurious columns zeroed).
    Returns the F, S, G lists on the device and replaces ``cleaned``'s clusters by the tensors, the same columns zeroed."""
    for key, i, before in (("row_clusters", 3, row_cl), ("col_clusters", 4, col_cl)):
        cleaned[key] = [device_views.zero_columns_like(t[i], b, a) for t, b, a in zip(on_device, before, cleaned[key])]
    return tuple([t[i] for t in on_device] for i in range(3))


def _check_post_on_device(post_on_device: bool, output: str):
    if post_on_device and output != "torch":
        raise ValueError("post_on_device=True needs output='torch' (the steps after the loop then work on the device tensors).")


def _remove_then_score(res: dict, check: Optional[dict], score_fn: Optional[Callable], on_device: bool = False) -> dict:
    """R's order (``R/obtain_bicl.r:176-199``): with a ``check`` (``check_biclusters``' scores and thresholds) the
    removal first (``spurious.apply_removal``: copies, ``"spurious"`` added; ``on_device``: the clusters are tensors,
    ``spurious.apply_removal_device``), then ``"bisil"`` = ``score_fn(row_clusters, col_clusters)`` of the cleaned
    clusters (``None`` without a ``score_fn``).  Returns a new dict."""
    removal = _spurious.apply_removal_device if on_device else _spurious.apply_removal
    out = removal(res, check) if check is not None else dict(res)
    out["bisil"] = None if score_fn is None else score_fn(out["row_clusters"], out["col_clusters"])
    return out


def _number_biclusters(results) -> float:
    """``number_biclusters`` (``R/stability_analysis.r:92-97``): the sum of every row-cluster matrix; 0 for results
    without cluster matrices (``no_clusts``)."""
    return float(sum(_cluster_sum(rc) for rc in (results.get("row_clusters") or [])))


def _cluster_sum(rc) -> float:
    """The sum of a cluster matrix: a tensor in device memory is summed there in fp64 (0 / 1 entries: exact in any order),
    anything else on the host."""
    if device_views.is_device_tensor(rc):
        return float(rc.detach().double().sum().item())
    return float(np.asarray(device_views.to_numpy(rc)).sum())


def _refuse_host_spurious(wanted, spurious_on_device: bool, message: str):
    """``spurious=True`` runs only with the opt-in ``spurious_on_device``; ``message``: the caller's own refusal."""
    if wanted and not spurious_on_device:
        raise NotImplementedError(message)


def _check_distance(distance):
    if distance not in _DISTANCES:
        raise ValueError("distance must be one of 'euclidean', 'manhattan' or 'cosine'.")         # utils.r:425


def _check_common(n_iters, num_repeats, n_stability, distance, sample_rate, stab_thres):
    """What ``apply_resnmtf`` checks for a known k and for the k sweep alike (``R/utils.r:220-253``, ``:425``, ``:286-300``)."""
    for name, val in (("n_iters", n_iters), ("num_repeats", num_repeats), ("n_stability", n_stability)):
        if val is not None and (int(val) != val or val < 1):
            raise ValueError(f"{name} must be a positive integer.")
    _check_distance(distance)
    _check_stability_numbers(sample_rate, stab_thres)


def _seed(seed) -> int:
    return 0 if seed is None else int(seed)


def _check_stability_numbers(sample_rate, stab_thres):
    """``check_numeric`` (``R/utils.r:286-300``)."""
    if not isinstance(sample_rate, (int, float, np.integer, np.floating)) or isinstance(sample_rate, bool):
        raise ValueError("sample_rate must be a numeric.")
    if not isinstance(stab_thres, (int, float, np.integer, np.floating)) or isinstance(stab_thres, bool):
        raise ValueError("stab_thres must be a numeric.")
    if not 0 <= stab_thres <= 1:
        raise ValueError("stab_thres must be between 0 and 1.")
    if not 0 < sample_rate <= 1:
        raise ValueError("sample_rate must be greater than 0 and less than or equal to 1.")


def stability_check(data, results, k, phi, xi, psi, n_iters, spurious, num_repeats, no_clusts, distance,
                    sample_rate=0.9, n_stability=5, stab_thres=0.6, remove_unstable=True, *,
                    row_names=None, col_names=None, device_id: int = 0, seed: Optional[int] = None, group=None,
                    max_iters: int = 100000, return_repeats: bool = False, repeat_runner: Optional[Callable] = None,
                    spurious_on_device: bool = False, shuffle_sparse: bool = False, sparse_on_device: bool = False,
                    output: str = "numpy", precision: str = "f32", fp64_subsample_sparse: bool = False,
                    fp64_shuffle_sparse: bool = False, fp64_init: bool = False):
    """``stability_check`` (``R/stability_analysis.r:302-338``): ``n_stability`` factorisations of sub-samples
    (``sample_rate`` of the rows and columns, drawn and trimmed as ``stability_repeat`` does, ``:215-249``), each scored
    against ``results`` by ``relevance_results`` (``:45-67``) -- the gathers, the factorisations and the scoring run on
    the device (``batched.stability_relevance_on_device``); the repeats are sharded over the ranks of ``group`` when a
    process group is initialised, and the mean relevance does not depend on their number.

    ``data``: the pre-processed views the original factorisation used (as ``res_nmtf_inner`` receives them; the
    sub-samples are not re-normalised); ``phi`` / ``xi`` / ``psi``: the symmetrised restriction matrices;
    ``k``: the number of biclusters (a scalar or the reference's ``k_vec``).  Returns ``results`` itself when it has no
    biclusters (``no_clusts`` results included; the reference's message becomes a warning) or when a repeat could not
    be sampled; with ``remove_unstable=False`` ``{"res": results, "relevance": n_views x k array}``; else a copy of
    ``results`` whose row- and column-cluster columns with a mean relevance below ``stab_thres`` are zero (F, S, G
    untouched; ``results`` is not modified).  ``spurious=True`` inside the repeats needs the opt-in
    ``spurious_on_device=True``: every repeat then removes the spurious biclusters of its own sub-sample before its
    relevance is scored (``R/stability_analysis.r:254-266``; ``batched.stability_relevance_on_device``, spurious seed
    ``seed + 2000 + r`` for repeat r); without it, ``NotImplementedError`` as before.  On sparse views the removal needs
    the further opt-in ``shuffle_sparse=True``: the shuffles are drawn from each repeat's own sparse sub-sample handle
    and re-normalised (``Engine.shuffle_view_sparse_from``).  ``sparse_on_device=True`` (opt-in): the sub-samples of
    sparse views are probed, trimmed and gathered on the device (``resnmtf_subsample_view_sparse``) instead of on the
    host; same draws, clusters and factors, ``All_Error`` within 1e-6 absolute (module docstring).
    Keyword-only extras: names, ``device_id``, ``seed`` of the draws and the device SVD inits, ``group``,
    ``max_iters``; test hooks: ``return_repeats`` (adds ``"repeats"``: per repeat the trimmed draws, relevance and
    the sub-sample's own clusters -- under ``"stability"`` of a copy of the result), ``repeat_runner(r)`` (replaces
    one repeat; nothing touches the device); ``output``: ``"torch"`` returns the two cluster lists as fp64 ``torch``
    tensors on ``cuda:device_id`` (those of ``results`` when it holds tensors, with the unstable columns zeroed there),
    ``"numpy"`` as NumPy arrays.  The cluster matrices of a view that are both tensors on ``cuda:device_id`` are scored
    from there (``Engine.set_reference_clusters_device``) and are not turned into NumPy unless ``"numpy"`` asks for them;
    anything else is scored from NumPy copies.  The views may be ``torch`` tensors
    on that device, as for ``res_nmtf_inner``.

    ``precision`` (keyword-only; ``"f32"``, the default, is everything above, untouched).  ``"fp64"`` (DESIGN.md section
    28) runs the repeats in double precision without an f32 handle (``batched.stability_relevance_fp64``): the same draws
    for the same seed, every sub-sample gathered from the fp64 values of the views (``engine.fp64_subsample``),
    factorised by ``res_nmtf_inner(precision="fp64")`` and scored from the cluster tensors it leaves on the device
    (``engine.fp64_relevance``).  ``data``: dense host arrays or dense tensors on ``cuda:device_id``, pre-processed, as
    ``res_nmtf_inner`` receives them.  ``spurious=True`` with ``spurious_on_device=True`` is the fp64 removal inside every
    repeat (``fp64_spurious``); ``remove_unstable``, ``return_repeats``, ``repeat_runner`` and ``output`` work as above.
    A host view is copied to the device once and read there by every repeat.  Refused by name
    (``NotImplementedError``): a sparse view of any kind, a device tensor still to be shifted and normalised
    (``RawDeviceView``), ``group``, ``sparse_on_device``, ``shuffle_sparse``.
    ``fp64_subsample_sparse=True`` (keyword-only opt-in; read only under ``precision="fp64"``, a
    no-op everywhere else) admits views stored sparse -- ``scipy.sparse`` matrices (taken as their canonical CSC and
    uploaded once) and sparse tensors on ``cuda:device_id`` (read where they lie) --, mixed with dense ones at will: their
    sub-samples are gathered sparse (``engine.fp64_subsample_sparse``: bit for bit the dense gather of the densified view
    at the stored positions, and the same empty lines, so the trimmed lists are those of the dense route), stay sparse
    tensors on the device and are factorised as sparse device views.  ``spurious=True`` on a sparse view needs
    ``fp64_shuffle_sparse=True`` as well (keyword-only opt-in; read only under ``precision="fp64"``):
    the removal inside every repeat then shuffles the sparse sub-sample sparse; without it that combination is refused by
    name.  ``group``, ``sparse_on_device``, ``shuffle_sparse`` and a ``RawDeviceView`` stay refused as above, and without
    ``fp64_subsample_sparse`` so does every sparse view, word for word.
    """
    if precision not in ("f32", "fp64"):
        raise ValueError(f"precision must be 'f32' or 'fp64', got {precision!r}")
    device_views.check_output(output)
    if _number_biclusters(results) == 0:                                                          # :308-311
        warnings.warn("No biclusters detected!")
        return results
    if precision == "fp64":
        for flag, on in (("group", group is not None), ("sparse_on_device", sparse_on_device), ("shuffle_sparse", shuffle_sparse)):
            if on:
                raise NotImplementedError(f'stability_check(precision="fp64"): {flag} is not supported: the fp64 repeats run '
                                          'one after the other on dense views')
    _refuse_host_spurious(spurious, spurious_on_device,
                          "stability selection with spurious-bicluster removal inside its repeats "
                          "(R/stability_analysis.r:254-266) is outside the accelerated path; pass spurious=False")
    spurious_repeats = _spurious.check_num_repeats(num_repeats) if spurious else 0
    _check_stability_numbers(sample_rate, stab_thres)
    if int(n_stability) != n_stability or n_stability < 1:
        raise ValueError("n_stability must be a positive integer.")
    data = _views(data, device_id)
    n_v = len(data)
    if precision == "fp64":
        for v, d in enumerate(data):
            if isinstance(d, device_views.RawDeviceView):
                raise NotImplementedError(f'stability_check(precision="fp64"): a device tensor still to be shifted and '
                                          f'column-normalised (view {v}) is not supported: the route takes pre-processed '
                                          'dense views')
            if not (sparse.is_sparse_view(d) or device_views.is_sparse_device_view(d)):
                continue
            if not fp64_subsample_sparse:
                raise NotImplementedError(f'stability_check(precision="fp64"): a sparse view (view {v}) is not supported: '
                                          'resnmtf_fp64_subsample gathers dense views')
            if getattr(d, "raw", False):
                raise NotImplementedError(f'stability_check(precision="fp64"): a sparse device tensor still to be '
                                          f'column-normalised (view {v}) is not supported: the route takes pre-processed views')
            if spurious and not fp64_shuffle_sparse:
                raise NotImplementedError(f'stability_check(precision="fp64"): spurious=True on a sparse view (view {v}) is not '
                                          'supported without fp64_shuffle_sparse=True: the removal inside a repeat shuffles '
                                          'the sparse sub-sample (resnmtf_fp64_shuffle_sparse)')
    # host copies of the small cluster matrices for the scoring, unless both of a view's are on the engine's device (they
    # are then read in place); `given` keeps the caller's
    given = results
    kept = [all(device_views.on_engine_device(x, device_id) and x.dtype.is_floating_point for x in (rc, cc))
            for rc, cc in zip(results["row_clusters"], results["col_clusters"])]
    results = dict(results, row_clusters=[rc if on else device_views.to_numpy(rc) for rc, on in zip(results["row_clusters"], kept)],
                   col_clusters=[cc if on else device_views.to_numpy(cc) for cc, on in zip(results["col_clusters"], kept)])
    if (spurious_repeats and repeat_runner is None and not shuffle_sparse and precision != "fp64"       # (fp64: judged above)
            and any(sparse.is_sparse_view(d) for d in data)):
        raise NotImplementedError("spurious-bicluster removal needs shuffled views: device shuffles of sparse views "
                                  "are not supported")
    k = int(np.atleast_1d(k)[0])
    seed = _seed(seed)
    dev = None
    if precision == "fp64":
        if repeat_runner is None:
            row_names, col_names = naming.give_names(data, None, None, row_names, col_names)
        # (sparse views, admitted above, are recognised there: the call is the one it was)
        stab = batched.stability_relevance_fp64(data, results, k, int(n_stability), float(sample_rate), n_iters, seed, phi, xi,
                                                psi, row_names, col_names, max_iters, device_id,
                                                keep_clusters=return_repeats, spurious_repeats=spurious_repeats,
                                                runner=repeat_runner, **({"fp64_init": True} if fp64_init else {}))
    else:
        if repeat_runner is None:
            row_names, col_names = naming.give_names(data, None, None, row_names, col_names)
            dev = batched.DeviceData(data, phi, xi, psi, row_names, col_names, device_id=device_id, pre_processed=True)
        try:
            stab = batched.stability_relevance_on_device(dev, results, k, int(n_stability), float(sample_rate), n_iters,
                                                         seed, group, max_iters, keep_clusters=return_repeats,
                                                         runner=repeat_runner, spurious_repeats=spurious_repeats,
                                                         shuffle_sparse=shuffle_sparse,
                                                         **({"sparse_on_device": True} if sparse_on_device else {}))
        finally:
            if dev is not None:
                dev.close()
    if not stab["stability_performed"]:                                                          # :323-325
        warnings.warn("Unable to perform stability analysis due to sparsity of data.")
        return given
    relevance = stab["relevance"]
    if not remove_unstable:                                                                       # :328-329
        out = {"res": given, "relevance": relevance}
    else:                                                                                         # :330-337
        out = dict(given)
        for key in ("row_clusters", "col_clusters"):
            out[key] = []
            for i in range(n_v):
                drop = relevance[i] < stab_thres
                if kept[i] and output == "torch":       # stays on the device: a clone with the unstable columns zeroed there
                    out[key].append(_zero_columns_on_device(given[key][i], drop))
                    continue
                before = device_views.to_numpy(results[key][i])
                after = np.array(before, dtype=np.float64, copy=True)
                after[:, drop] = 0.0
                out[key].append(_cluster_output(given[key][i], before, after, output, device_id))
    if return_repeats:
        out = dict(out)
        out["stability"] = {"relevance": relevance, "repeats": stab["repeats"]}
    return out


def _zero_columns_on_device(t, drop: np.ndarray):
    """A clone of the device cluster matrix ``t`` whose columns ``drop`` are zero: what ``_cluster_output`` makes of its
    host copy (``zero_columns_like`` writes only the columns that change: those of ``drop`` that hold a non-zero entry)."""
    out = t.clone()
    cols = np.flatnonzero(np.asarray(drop) & (out != 0).any(dim=0).cpu().numpy())      # (k flags, not the matrix)
    if cols.size:
        import torch        # (the caller works with it)
        out[:, torch.as_tensor(cols, device=out.device)] = 0.0
    return out


def _cluster_output(given, before: np.ndarray, after: np.ndarray, output: str, device_id: int):
    """A cluster matrix of ``stability_check``'s result in the form ``output`` asks for: ``after`` is the host copy
    ``before`` of ``given`` with its unstable columns zeroed.  A tensor is cloned and the same columns zeroed on the device."""
    if output == "numpy":
        return after
    import torch        # (output="torch": the caller works with it)
    if device_views.is_tensor(given):
        return device_views.zero_columns_like(given.clone(), before, after)
    return torch.as_tensor(after, device=torch.device("cuda", int(device_id)))


def apply_resnmtf(data, init_f=None, init_s=None, init_g=None, k_val=None,
                  phi=None, xi=None, psi=None, n_iters=None, k_min=3, k_max=8,
                  distance="euclidean", spurious=True, num_repeats=5, no_clusts=False,
                  sample_rate=0.9, n_stability=5, stability=True, stab_thres=0.4,
                  remove_unstable=True, use_parallel=True, *, row_names=None, col_names=None,
                  device_id: int = 0, max_iters: int = 100000, seed: Optional[int] = None,
                  k_sweep: bool = False, return_sweep: bool = False, sweep_runner: Optional[Callable] = None,
                  spurious_on_device: bool = False, bisil_sparse: bool = False, shuffle_sparse: bool = False,
                  sparse_on_device: bool = False, output: str = "numpy", post_on_device: bool = False,
                  precision: str = "f32", score_bisil: bool = False, fp64_sparse: bool = False, fp64_device: bool = False,
                  fp64_sparse_device: bool = False, fp64_bisil: bool = False, fp64_spurious: bool = False,
                  fp64_stability: bool = False, fp64_bisil_sparse: bool = False, fp64_shuffle_sparse: bool = False,
                  fp64_subsample_sparse: bool = False, fp64_init: bool = False):
    """``apply_resnmtf`` (``R/main.r:214-335``) for a known ``k_val``: naming, shared-name maps, restriction
    symmetrisation, non-negativity shift and column normalisation on the host, then the device loop and -- with
    ``stability=True`` (the default) and ``spurious=False`` -- ``stability_check`` on the pre-processed data, as
    ``R/main.r:255-262`` does.  As at that call site, ``remove_unstable`` is NOT forwarded: ``stability_check``
    always runs with its default ``remove_unstable=True`` (unstable biclusters are zeroed whatever is passed here).
    ``stab_thres`` defaults to 0.4 here, against 0.6 in ``stability_check``.  ``stability=True`` with
    ``spurious=True`` is refused (spurious-bicluster removal is outside the accelerated path).

    ``k_val=None`` with the keyword-only opt-in ``k_sweep=True``: the reference's k sweep (``R/main.r:269-334``, see
    ``_sweep``): every k in ``k_min:k_max`` factorised from one upload (``batched.k_sweep_on_device``, seeds
    ``seed + k``), each result scored by ``bisil`` on the device, the first maximum kept, the range extended by one
    while its largest k scores best; then ``stability_check`` on the pick WITH ``remove_unstable`` forwarded
    (``R/main.r:324-332``, unlike the ``k_val`` branch).  The result is the picked ``res_nmtf_inner`` result.  Test
    hooks: ``return_sweep`` adds ``"k_sweep": {"k": [...], "bisil": [...]}``; ``sweep_runner(k)`` replaces one
    factorisation and its score (a result dict with ``"bisil"``; nothing touches the device).  Without ``k_sweep``,
    ``k_val=None`` raises ``NotImplementedError`` as before.

    ``spurious_on_device=True`` (keyword-only opt-in) lets ``spurious=True`` run: ``res_nmtf_inner(spurious=True,
    spurious_on_device=True)`` for the known k or for every k of the sweep (ranked by the bisilhouette of the cleaned
    clusters), and ``stability_check`` with the removal inside its repeats.  The reference's default pipeline is
    ``apply_resnmtf(data, k_sweep=True, spurious_on_device=True)``.

    ``bisil_sparse=True`` (keyword-only opt-in) lets the k sweep run on ``scipy.sparse`` views: they stay sparse on the
    device and every k is scored from their CSC / CSR copies (``Engine.bisil_sparse``), bitwise the score of the
    densified views; ``stability=True`` then works as it does for sparse views with a known ``k_val``.  No effect on
    dense data; ``spurious=True`` on sparse views stays refused (device shuffles of sparse views are not supported)
    unless ``shuffle_sparse`` is set too.

    ``shuffle_sparse=True`` (keyword-only opt-in) lets ``spurious=True`` run on ``scipy.sparse`` views: every shuffle of
    a sparse view is drawn on the device as a sparse view (``resnmtf_shuffle_view_sparse``: the dense path's draw of
    the densified view, DESIGN.md section 10 "Sparse shuffles"), in ``res_nmtf_inner``, for every k of the sweep and
    inside the stability repeats.  The reference's default pipeline on sparse data is ``apply_resnmtf(data,
    k_sweep=True, spurious_on_device=True, bisil_sparse=True, shuffle_sparse=True)``.  No effect on dense data.

    ``sparse_on_device=True`` (keyword-only opt-in): the copies of sparse views the k sweep makes for every k and the
    sub-samples of the stability repeats are made on the device from the one upload (``resnmtf_copy_view_sparse``,
    ``resnmtf_subsample_view_sparse``; DESIGN.md section 10 "Device copies and sub-samples") instead of gathered on the
    host and uploaded.  Same clusters, factors and stability outcome; ``All_Error`` of the repeats within 1e-6 absolute.  No
    effect on dense data.

    A view may be a 2-D floating ``torch`` tensor on ``cuda:device_id`` (``res_nmtf_inner``): it is never brought to the
    host -- its shift and column normalisation run on the device at every upload (``Engine.set_view_device(raw=True)``,
    the sums in the device's order, where ``check_data`` sums a host view in NumPy's).  ``output="torch"`` (keyword-only)
    returns ``output_f`` / ``output_s`` / ``output_g`` / ``row_clusters`` / ``col_clusters`` as fp64 ``torch`` tensors on
    that device (``Engine.finalise_device``); the small values stay NumPy.  With a ``k_val``, ``init_f`` / ``init_s`` /
    ``init_g`` may be ``torch`` tensors on that device too (``res_nmtf_inner``); the k sweep refuses
    explicit factors as before.

    ``post_on_device=True`` (keyword-only opt-in, needs ``output="torch"``): the steps after the
    loop stay on the device, in ``res_nmtf_inner`` and for every k of the sweep, the extension k's included
    (``DeviceData.factorise(post_on_device=True)``; removal and ``bisil`` from the tensors it returns).  Same result,
    bit for bit.

    ``precision`` (keyword-only; ``"f32"``, the default, is everything above, untouched, and ``score_bisil`` and the
    ``fp64_*`` flags are then not read; anything but ``"f32"`` or ``"fp64"`` is a ``ValueError``).  ``"fp64"`` (DESIGN.md
    section 26) runs ``res_nmtf_inner(precision="fp64")`` on the prepared data: with a ``k_val`` once, ``score_bisil`` and
    the ``fp64_sparse`` / ``fp64_device`` / ``fp64_sparse_device`` / ``fp64_bisil`` flags passed through; with
    ``k_val=None, k_sweep=True`` for every k of the reference's sweep, each scored in double precision
    (``score_bisil=True, fp64_bisil=True``, seed ``seed + k``, the correct shared maps for every k), the selection being
    ``_sweep`` as above with the cap ``min(ncol, 64)``; ``return_sweep`` and ``sweep_runner`` work as before.  Refused
    with a ``NotImplementedError`` naming the flag: ``stability=True`` (the repeats run on the f32 engine; mixing the two
    precisions is left for later), ``spurious=True``, sparse views in the sweep, and views in device memory (their
    pre-processing runs at an f32 engine's upload; pass pre-processed tensors to ``res_nmtf_inner``).
    ``fp64_spurious=True`` (keyword-only opt-in; a no-op with ``precision="f32"``) lets
    ``spurious=True`` run under ``"fp64"`` with ``spurious_on_device=True``: ``res_nmtf_inner(..., spurious=True,
    spurious_on_device=True, fp64_spurious=True)`` for the ``k_val``, or for every k of the sweep, the extension k's
    included, each with its own check at seed ``seed + k`` and ranked by the bisilhouette of its cleaned clusters --
    ``apply_resnmtf(data, precision="fp64", k_sweep=True, stability=False, spurious_on_device=True, fp64_spurious=True)``
    is the reference's default pipeline minus stability.  A sparse view with it is refused by name.
    ``fp64_stability=True`` (keyword-only opt-in; a no-op with ``precision="f32"``) lets
    ``stability=True`` run under ``"fp64"``: after the fit, ``stability_check(p.data, ..., precision="fp64")`` on the
    prepared data -- for a ``k_val`` with ``remove_unstable`` NOT forwarded (``R/main.r:255-262``), after the k sweep's pick
    with it forwarded (``:324-332``), exactly as the f32 function does; with ``spurious=True`` (which needs
    ``fp64_spurious`` as above) the removal runs inside every repeat.  A sparse view with it is refused by name.
    ``apply_resnmtf(data, precision="fp64", k_sweep=True, spurious_on_device=True, fp64_spurious=True,
    fp64_stability=True)`` is the reference's default pipeline.  Without the flag ``stability=True`` stays refused.
    ``fp64_bisil_sparse=True`` (keyword-only opt-in; a no-op with ``precision="f32"``) is passed
    through to ``res_nmtf_inner`` -- for the ``k_val`` and for every k of the sweep -- and lifts the refusal of sparse views
    in the fp64 k sweep: ``apply_resnmtf(data, precision="fp64", k_sweep=True, fp64_sparse=True, fp64_bisil_sparse=True,
    spurious=False, stability=False)`` selects k on ``scipy.sparse`` views, every k scored by
    ``engine.fp64_bisil_sparse``.
    ``fp64_shuffle_sparse=True`` (keyword-only opt-in; read only with ``precision="fp64"`` and
    ``fp64_spurious=True``, a no-op everywhere else) is passed through in the same way and lifts the refusal of a sparse
    view with ``fp64_spurious``: ``apply_resnmtf(data, precision="fp64", k_sweep=True, fp64_sparse=True,
    fp64_bisil_sparse=True, spurious_on_device=True, fp64_spurious=True, fp64_shuffle_sparse=True, stability=False)`` is the
    reference's default pipeline minus stability on ``scipy.sparse`` views, every k with its own check at ``seed + k``.
    ``fp64_subsample_sparse=True`` (keyword-only opt-in; read only with ``precision="fp64"`` and
    ``fp64_stability=True``, a no-op everywhere else) lifts the refusal of a sparse view with ``fp64_stability``: it is
    passed on to ``stability_check(precision="fp64")`` -- for a ``k_val`` and after the sweep's pick --, together with
    ``fp64_shuffle_sparse`` when that is set, and the sub-samples of ``scipy.sparse`` views are gathered, factorised and
    screened sparse.  ``apply_resnmtf(data, precision="fp64", k_sweep=True, fp64_sparse=True, fp64_bisil_sparse=True,
    spurious_on_device=True, fp64_spurious=True, fp64_shuffle_sparse=True, fp64_stability=True,
    fp64_subsample_sparse=True)`` is the reference's default pipeline in double precision on data that stays sparse end to
    end.
    Still refused by name: ``fp64_spurious`` on a sparse view without ``fp64_shuffle_sparse``, ``fp64_stability`` on a
    sparse view without ``fp64_subsample_sparse``, and views in device memory.
    ``fp64_init=True`` (keyword-only opt-in; a no-op with ``precision="f32"``) is passed on to every
    fit that would build a short-lived f32 engine for its start -- the ``k_val`` fit, every k of the sweep, the shuffled
    fits of the removal and the stability repeats --: each starts from ``engine.fp64_init_svd`` under the seed it had."""
    if precision not in ("f32", "fp64"):
        raise ValueError(f"precision must be 'f32' or 'fp64', got {precision!r}")
    if precision == "fp64":
        return _apply_fp64(data, init_f, init_s, init_g, k_val, phi, xi, psi, n_iters, k_min, k_max, distance, spurious,
                           num_repeats, no_clusts, sample_rate, n_stability, stability, stab_thres, row_names=row_names,
                           col_names=col_names, device_id=device_id, max_iters=max_iters, seed=seed, k_sweep=k_sweep,
                           return_sweep=return_sweep, sweep_runner=sweep_runner, output=output, score_bisil=score_bisil,
                           fp64_sparse=fp64_sparse, fp64_device=fp64_device, fp64_sparse_device=fp64_sparse_device,
                           fp64_bisil=fp64_bisil, fp64_spurious=fp64_spurious, spurious_on_device=spurious_on_device,
                           fp64_stability=fp64_stability, remove_unstable=remove_unstable,
                           fp64_bisil_sparse=fp64_bisil_sparse, fp64_shuffle_sparse=fp64_shuffle_sparse,
                           fp64_subsample_sparse=fp64_subsample_sparse, fp64_init=fp64_init)
    device_views.check_output(output)
    _check_post_on_device(post_on_device, output)
    on_dev = {"sparse_on_device": True} if sparse_on_device else {}      # (off: every call below is the earlier one)
    out_kw = {"output": output} if output != "numpy" else {}
    if post_on_device:
        out_kw["post_on_device"] = True
    data = _views(data, device_id)
    n_v = len(data)
    if k_val is None and k_sweep:
        return _apply_k_sweep(data, init_f, init_s, init_g, phi, xi, psi, n_iters, k_min, k_max, distance, spurious,
                              num_repeats, no_clusts, sample_rate, n_stability, stability, stab_thres, remove_unstable,
                              row_names=row_names, col_names=col_names, device_id=device_id, max_iters=max_iters,
                              seed=seed, return_sweep=return_sweep, sweep_runner=sweep_runner,
                              spurious_on_device=spurious_on_device, bisil_sparse=bisil_sparse,
                              shuffle_sparse=shuffle_sparse, **on_dev, **out_kw)
    if k_val is None:
        raise NotImplementedError("the k sweep (R/main.r:279-321) needs the bisilhouette score, which is "
                                  "outside the accelerated path; pass k_val")
    _refuse_host_spurious(stability and spurious and not no_clusts, spurious_on_device,
                          "stability selection with spurious-bicluster removal (R/obtain_bicl.r:31-133) is "
                          "outside the accelerated path; pass spurious=False (or stability=False and do the "
                          "removal on the R side, INTEGRATION.md)")
    _check_common(n_iters, num_repeats, n_stability, distance, sample_rate, stab_thres)
    k_vec = [int(np.atleast_1d(k_val)[0])] * n_v                                                  # main.r:226
    ranks = [d.shape[1] for d in data]
    if any(k < 1 for k in k_vec):
        raise ValueError("k_vec must be a vector of integers greater than 1.")                    # utils.r:437
    if any(k > r for k, r in zip(k_vec, ranks)):
        raise ValueError("k_vec must be a vector of integers less than or equal to the ranks of the views.")
    p = prepare(data, phi, xi, psi, row_names, col_names, normalise=True, symmetrise=True)        # main.r:228-237
    results = res_nmtf_inner(p.data, p.row_shared, p.col_shared, init_f, init_s, init_g, k_vec, p.phi, p.xi, p.psi,
                             n_iters, num_repeats, spurious, distance, no_clusts,
                             row_names=p.row_names, col_names=p.col_names, device_id=device_id, max_iters=max_iters,
                             seed=seed, spurious_on_device=spurious_on_device, shuffle_sparse=shuffle_sparse, **on_dev,
                             **out_kw)
    out_kw.pop("post_on_device", None)                                                            # (stability_check has no such step)
    if stability:                                                                                 # main.r:255-262
        results = stability_check(p.data, results, k_vec, p.phi, p.xi, p.psi, n_iters, spurious, num_repeats,
                                  no_clusts, distance, sample_rate, n_stability, stab_thres,
                                  row_names=p.row_names, col_names=p.col_names, device_id=device_id, seed=seed,
                                  max_iters=max_iters, spurious_on_device=spurious_on_device,
                                  shuffle_sparse=shuffle_sparse, **on_dev, **out_kw)
    return results


def _apply_fp64(data, init_f, init_s, init_g, k_val, phi, xi, psi, n_iters, k_min, k_max, distance, spurious, num_repeats,
                no_clusts, sample_rate, n_stability, stability, stab_thres, *, row_names, col_names, device_id, max_iters,
                seed, k_sweep, return_sweep, sweep_runner, output, score_bisil, fp64_sparse, fp64_device,
                fp64_sparse_device, fp64_bisil, fp64_spurious=False, spurious_on_device=False, fp64_stability=False,
                remove_unstable=True, fp64_bisil_sparse=False, fp64_shuffle_sparse=False, fp64_subsample_sparse=False,
                fp64_init=False):
    """``apply_resnmtf(precision="fp64")``: the checks of the f32 function, the refusals of what runs on the f32 engine,
    ``prepare``, then ``res_nmtf_inner(precision="fp64")`` -- once for a ``k_val``, or as ``run(k)`` of ``_sweep`` --, then
    with ``stability`` and ``fp64_stability`` ``stability_check(precision="fp64")`` on the prepared data."""
    def refuse(flag, why):
        raise NotImplementedError(f'apply_resnmtf(precision="fp64"): {flag} is not supported: {why}')
    device_views.check_output(output)
    data = _views(data, device_id)
    n_v = len(data)
    sweep = k_val is None and k_sweep
    if k_val is None and not k_sweep:
        raise NotImplementedError("the k sweep (R/main.r:279-321) needs the bisilhouette score, which is "
                                  "outside the accelerated path; pass k_val")
    _check_common(n_iters, num_repeats, n_stability, distance, sample_rate, stab_thres)
    if sweep:                                     # the checks of _apply_k_sweep, in its order
        _check_whole_number(k_min, "k_min")
        _check_whole_number(k_max, "k_max")
        if k_max <= k_min:
            raise ValueError("k_max must be greater than k_min.")                                 # utils.r:250-252
        k_min, k_max = int(k_min), int(k_max)
        if no_clusts:
            raise ValueError("the k sweep ranks the biclusters by their bisilhouette score: no_clusts=True has none")
    if stability and not fp64_stability:
        refuse("stability=True", "the stability repeats run on the f32 engine; pass stability=False")
    if (stability and not fp64_subsample_sparse
            and any(sparse.is_sparse_view(d) or device_views.is_sparse_device_view(d) for d in data)):
        refuse("a sparse view with fp64_stability", "resnmtf_fp64_subsample gathers dense views; pass stability=False")
    remove = bool(spurious) and not no_clusts
    if remove and not fp64_spurious:
        refuse("spurious=True", "spurious-bicluster removal runs on the f32 engine; pass spurious=False")
    _refuse_host_spurious(remove, spurious_on_device,
                          "spurious-bicluster removal (R/obtain_bicl.r:31-133) is outside the accelerated path; "
                          "pass spurious=False")
    if remove:
        _spurious.check_num_repeats(num_repeats)
        if any(sparse.is_sparse_view(d) for d in data) and not fp64_shuffle_sparse:
            refuse("a sparse view with fp64_spurious", "no fp64 sparse shuffle exists; pass spurious=False")
    if any(device_views.is_device_view(d) for d in data):
        refuse("a view in device memory", "its shift and column normalisation run at an f32 engine's upload; pass host "
               "arrays, or pre-processed tensors to res_nmtf_inner(precision=\"fp64\", fp64_device=True)")
    flags = {"fp64_sparse": fp64_sparse, "fp64_device": fp64_device, "fp64_sparse_device": fp64_sparse_device}
    common = {"device_id": device_id, "max_iters": max_iters, "output": output, "precision": "fp64", **flags}
    if remove:                                    # (only then: without the flag every call is the one it was)
        common.update(spurious_on_device=True, fp64_spurious=True)
        if fp64_shuffle_sparse:                   # (the same: passed through only when set)
            common.update(fp64_shuffle_sparse=True)
    if fp64_bisil_sparse:                         # (the same: passed through only when set)
        common.update(fp64_bisil_sparse=True)
    if fp64_init:                                 # (the same)
        common.update(fp64_init=True)

    def stab_kw(p):                               # the keywords of stability_check(precision="fp64") on the prepared data
        kw = {"row_names": p.row_names, "col_names": p.col_names, "device_id": device_id, "seed": seed, "max_iters": max_iters,
              "spurious_on_device": spurious_on_device, "output": output, "precision": "fp64"}
        if fp64_subsample_sparse:                 # (passed on only when set: without the flag every call is the one it was)
            kw["fp64_subsample_sparse"] = True
            if fp64_shuffle_sparse:
                kw["fp64_shuffle_sparse"] = True
        if fp64_init:
            kw["fp64_init"] = True
        return kw
    if not sweep:
        k_vec = [int(np.atleast_1d(k_val)[0])] * n_v                                              # main.r:226
        if any(k < 1 for k in k_vec):
            raise ValueError("k_vec must be a vector of integers greater than 1.")                # utils.r:437
        if any(k > d.shape[1] for k, d in zip(k_vec, data)):
            raise ValueError("k_vec must be a vector of integers less than or equal to the ranks of the views.")
        p = prepare(data, phi, xi, psi, row_names, col_names, normalise=True, symmetrise=True)    # main.r:228-237
        results = res_nmtf_inner(p.data, p.row_shared, p.col_shared, init_f, init_s, init_g, k_vec, p.phi, p.xi, p.psi, n_iters,
                                 num_repeats, spurious, distance, no_clusts, row_names=p.row_names, col_names=p.col_names,
                                 seed=seed, score_bisil=score_bisil, fp64_bisil=fp64_bisil, **common)
        if stability:                                                                             # main.r:255-262
            results = stability_check(p.data, results, k_vec, p.phi, p.xi, p.psi, n_iters, spurious, num_repeats, no_clusts,
                                      distance, sample_rate, n_stability, stab_thres, **stab_kw(p))
        return results
    if any(sparse.is_sparse_view(d) for d in data) and not fp64_bisil_sparse:
        refuse("a sparse view in the k sweep", "resnmtf_fp64_bisil scores dense views only; pass k_val (with fp64_sparse=True)")
    if init_f is not None or init_s is not None or init_g is not None:
        raise NotImplementedError("the k sweep starts every k from the device's SVD initialisation; explicit initial "
                                  "factors are not supported with k_val=None")
    cap = min(min(d.shape[1] for d in data), 64)
    if k_max > cap:
        raise ValueError("k_vec must be a vector of integers less than or equal to the ranks of the views.")
    seed = _seed(seed)
    p = prepare(data, phi, xi, psi, row_names, col_names, normalise=True, symmetrise=True)        # main.r:228-237

    # every k, the extra ones included, with the correct shared maps (R's extension loop passes NULL ones,
    # R/main.r:305-309)
    def run(k):
        return res_nmtf_inner(p.data, p.row_shared, p.col_shared, None, None, None, [k] * n_v, p.phi, p.xi, p.psi, n_iters,
                              num_repeats, remove, distance, False, row_names=p.row_names, col_names=p.col_names,
                              seed=seed + k, score_bisil=True, fp64_bisil=True, **common)

    ks, scores, results, pick = _sweep(sweep_runner or run, k_min, k_max, cap)
    results = results[pick]                                                                       # main.r:313-314
    if stability:                                                                                 # main.r:324-332
        results = stability_check(p.data, results, [ks[pick]] * n_v, p.phi, p.xi, p.psi, n_iters, spurious, num_repeats,
                                  no_clusts, distance, sample_rate, n_stability, stab_thres, remove_unstable, **stab_kw(p))
    if return_sweep:
        results = dict(results)
        results["k_sweep"] = {"k": ks, "bisil": scores}
    return results


def _check_whole_number(x, name):
    """``check_whole_number`` (``R/utils.r:220-227``)."""
    if not isinstance(x, (int, float, np.integer, np.floating)) or isinstance(x, bool):
        raise ValueError(f"{name} must be a numeric.")
    if np.floor(x) != x or x <= 0:
        raise ValueError(f"{name} must be a positive integer.")


def _sweep(run: Callable, k_min: int, k_max: int, cap: int, initial: Optional[list] = None):
    """The selection of ``R/main.r:269-318``: ``run(k)`` -> a result with ``"bisil"`` for every k in
    ``k_min:k_max`` (or ``initial``, those results already computed), the first maximum (``which.max``), then one more
    k while the pick is the largest k scored.
    The reference would stop with an error once k + 1 exceeds a view's column count; here the range stops at ``cap``
    (``min(ncol of the views, 64)``) with a warning and the best so far is kept.  Returns (ks, scores, results, pick)."""
    ks = list(range(k_min, k_max + 1))
    results = list(initial) if initial is not None else [run(k) for k in ks]
    scores = [float(r["bisil"]) for r in results]
    pick = int(np.argmax(scores))                                                                 # main.r:291 (first max)
    while ks[pick] == ks[-1]:                                                                     # main.r:295-312
        if ks[-1] + 1 > cap:
            warnings.warn(f"the k sweep stops at k = {ks[-1]}: k + 1 would exceed min(ncol of the views, 64) = {cap}; "
                          "the best k so far is kept")
            break
        ks.append(ks[-1] + 1)
        results.append(run(ks[-1]))
        scores.append(float(results[-1]["bisil"]))
        pick = int(np.argmax(scores))
    return ks, scores, results, pick


def _apply_k_sweep(data, init_f, init_s, init_g, phi, xi, psi, n_iters, k_min, k_max, distance, spurious, num_repeats,
                   no_clusts, sample_rate, n_stability, stability, stab_thres, remove_unstable, *, row_names, col_names,
                   device_id, max_iters, seed, return_sweep, sweep_runner, spurious_on_device=False, bisil_sparse=False,
                   shuffle_sparse=False, sparse_on_device=False, output="numpy", post_on_device=False):
    """``apply_resnmtf`` with ``k_val = NULL`` (``R/main.r:269-334``); see ``apply_resnmtf``."""
    n_v = len(data)
    on_dev = {"sparse_on_device": True} if sparse_on_device else {}
    out_kw = {"output": output} if output != "numpy" else {}
    post_kw = {"post_on_device": True} if post_on_device else {}
    _check_common(n_iters, num_repeats, n_stability, distance, sample_rate, stab_thres)
    _check_whole_number(k_min, "k_min")
    _check_whole_number(k_max, "k_max")
    if k_max <= k_min:
        raise ValueError("k_max must be greater than k_min.")                                     # utils.r:250-252
    k_min, k_max = int(k_min), int(k_max)
    _refuse_host_spurious(spurious and not no_clusts, spurious_on_device,
                          "spurious-bicluster removal (R/obtain_bicl.r:31-133) is outside the accelerated "
                          "path; pass spurious=False")
    spurious_repeats = _spurious.check_num_repeats(num_repeats) if spurious and not no_clusts else 0
    if no_clusts:
        raise ValueError("the k sweep ranks the biclusters by their bisilhouette score: no_clusts=True has none")
    if any(sparse.is_sparse_view(d) for d in data):
        if not bisil_sparse:
            raise NotImplementedError("the k sweep scores with the bisilhouette, which is not supported for sparse views "
                                      "(dense views only); pass k_val")
        if spurious_repeats and not shuffle_sparse:
            raise NotImplementedError("spurious-bicluster removal needs shuffled views: device shuffles of sparse views "
                                      "are not supported")
    if init_f is not None or init_s is not None or init_g is not None:
        raise NotImplementedError("the k sweep starts every k from the device's SVD initialisation; explicit initial "
                                  "factors are not supported with k_val=None")
    cap = min(min(d.shape[1] for d in data), 64)
    if k_max > cap:
        raise ValueError("k_vec must be a vector of integers less than or equal to the ranks of the views.")
    seed = _seed(seed)
    p = prepare(data, phi, xi, psi, row_names, col_names, normalise=True, symmetrise=True)        # main.r:228-237
    dev = None
    try:
        if sweep_runner is None:
            dev = batched.DeviceData(p.data, p.phi, p.xi, p.psi, p.row_names, p.col_names, device_id=device_id,
                                     pre_processed=True)

            def scored(r):                                  # a res_nmtf_inner result with its bisil (main.r:131-139)
                cleaned = _remove_then_score({key: r[key] for key in ("output_s", "row_clusters", "col_clusters")},
                                             r.get("spurious_check"),
                                             lambda rc, cc: bisil.score(rc, cc, distance, engine=dev.base,
                                                                        sparse_views=bisil_sparse),
                                             on_device=post_on_device)
                out = (r["output_f"], r["output_s"], r["output_g"])
                if r.get("device_out") is not None and not post_on_device:      # output="torch": what is returned lives on the device
                    out = _device_outputs(r["device_out"], r["row_clusters"], r["col_clusters"], cleaned)
                return inner_result(*out, r["All_Error"], n_iters,
                                    bisil=cleaned["bisil"], row_clusters=cleaned["row_clusters"],
                                    col_clusters=cleaned["col_clusters"], lam=r["lambda"], mu=r["mu"],
                                    spurious=cleaned.get("spurious"))

            # every k, the extra ones included, with the correct shared-column maps (R's extension loop passes NULL
            # ones, R/main.r:305-309)
            def run(k):
                return scored(dev.factorise(k, n_iters, seed + k, max_iters=max_iters, tag=f"k={k}", return_lm=True,
                                            spurious_repeats=spurious_repeats, spurious_seed=seed + k,
                                            shuffle_sparse=shuffle_sparse, **on_dev, **out_kw, **post_kw))

            initial = [scored(r) for r in batched.k_sweep_on_device(dev, k_min, k_max, n_iters, seed,       # main.r:279-290
                                                                    max_iters=max_iters, return_lm=True,
                                                                    spurious_repeats=spurious_repeats,
                                                                    shuffle_sparse=shuffle_sparse, **on_dev, **out_kw,
                                                                    **post_kw)]
        else:
            run, initial = sweep_runner, None
        ks, scores, results, pick = _sweep(run, k_min, k_max, cap, initial)
    finally:
        if dev is not None:
            dev.close()
    results = results[pick]                                                                       # main.r:313-314
    if stability:                                                                                 # main.r:324-332
        results = stability_check(p.data, results, [ks[pick]] * n_v, p.phi, p.xi, p.psi, n_iters, spurious, num_repeats,
                                  no_clusts, distance, sample_rate, n_stability, stab_thres, remove_unstable,
                                  row_names=p.row_names, col_names=p.col_names, device_id=device_id, seed=seed,
                                  max_iters=max_iters, spurious_on_device=spurious_on_device,
                                  shuffle_sparse=shuffle_sparse, **on_dev, **out_kw)
    if return_sweep:
        results = dict(results)
        results["k_sweep"] = {"k": ks, "bisil": scores}
    return results
