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
``NotImplementedError`` as before.

The bisilhouette score (``bisil``, ``R/obtain_bicl.r:189-199``) is an opt-in here: ``res_nmtf_inner(score_bisil=True)``
scores the result on the device (per-member silhouettes from ``resnmtf_bisil``, combined by ``bisil.py``), and
``apply_resnmtf(k_val=None, k_sweep=True)`` runs the reference's k sweep on it (``R/main.r:269-334``).  Its definition
restates the published score (the R package's source is not available): parity with ``bisilhouette`` is unpinned.
Without the opt-ins ``bisil`` stays ``None`` and ``k_val=None`` raises ``NotImplementedError``, as before.
"""
from __future__ import annotations

import warnings
from typing import Callable, Dict, List, Optional, Sequence

import numpy as np

from . import bisil, naming, sparse
from . import spurious as _spurious
from .engine import Engine
from .spurious import check_biclusters, remove_spurious  # noqa: F401  (post-steps, R/obtain_bicl.r:113-188)

_DISTANCES = ("euclidean", "manhattan", "cosine")


def _as_list(x):
    if isinstance(x, np.ndarray) and x.ndim == 2:
        return [x]                      # check_lists, R/utils.r:313-316
    if sparse.is_sparse(x):
        return [x]
    return list(x)


def _views(data) -> list:
    """The views as fp64 arrays; a ``scipy.sparse`` view becomes a canonical CSC copy (``sparse.canonical_csc``: the
    caller's matrix is not modified) and stays sparse on the device (``resnmtf_create_sparse``)."""
    return [sparse.canonical_csc(d) if sparse.is_sparse(d) else np.asarray(d, dtype=np.float64) for d in _as_list(data)]


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


def _load_engine(eng: Engine, data, init_f, init_s, init_g, lam, mu, phi, xi, psi,
                 row_names, col_names, row_indices, column_indices, seed=None):
    """``init_f is None``: the initial factors come from the device (``resnmtf_init_svd``)."""
    n_v = eng.n_views
    for v in range(n_v):
        if eng.owned[v]:
            if sparse.is_sparse(data[v]):
                eng.set_view_sparse(v, data[v], pre_processed=True)                                    # (already pre-processed)
            else:
                eng.set_view(v, data[v])
        if init_f is None:
            eng.init_svd(v, seed=(0 if seed is None else int(seed)) + v)                          # update_steps.r:78-125
        else:
            eng.set_factors(v, init_f[v], init_s[v], init_g[v],
                            None if lam is None else lam[v], None if mu is None else mu[v])
    eng.set_restrictions(phi, xi, psi)
    for v in range(n_v):
        for w in range(n_v):
            if w == v:
                continue
            if n_v > 1:
                iv, iw = naming.index_pairs(row_names[v], row_names[w], row_indices[v].get(w))
                eng.set_shared_rows(v, w, iv, iw)
                iv, iw = naming.index_pairs(col_names[v], col_names[w], column_indices[v].get(w))
                eng.set_shared_cols(v, w, iv, iw)


def res_nmtf_inner(data, row_indices, column_indices,
                   init_f=None, init_s=None, init_g=None,
                   k_vec=None, phi=None, xi=None, psi=None,
                   n_iters=None, num_repeats=5, spurious=True, distance="euclidean",
                   no_clusts=False, *, row_names=None, col_names=None, device_id: int = 0,
                   max_iters: int = 100000, seed: Optional[int] = None, engine_opts: Optional[dict] = None,
                   host_init: bool = False, return_init: bool = False, score_bisil: bool = False,
                   spurious_on_device: bool = False):
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
    engine closes, ``bisil.score``; dense views only; default ``None`` as before), ``spurious_on_device`` (with
    ``spurious=True``: ``obtain_biclusters(remove_spurious = TRUE)``, ``R/obtain_bicl.r:151-204`` -- ``num_repeats``
    shuffles of the engine's own views, to convergence, scored on the device, the flagged cluster columns zeroed through
    ``relations``, then ``bisil`` of the cleaned clusters; the result carries ``"spurious"`` as ``remove_spurious``
    does and equals ``remove_spurious(data, res_nmtf_inner(..., spurious=False, seed=seed), num_repeats, seed=seed)``:
    the shuffles use the spurious seed ``0 if seed is None else seed``, repeat r initialising with ``+ 1000 + r`` and
    shuffling with ``seed * 7919 + r + 1``, as ``check_biclusters`` derives them; dense views only).
    """
    data = _views(data)
    n_v = len(data)
    if k_vec is None:
        raise ValueError("k_vec is required")
    k_vec = [int(k) for k in np.atleast_1d(k_vec)]
    if len(k_vec) != n_v:
        raise ValueError("k_vec must be a vector of the same length as the number of views.")   # utils.r:440
    if not no_clusts and spurious and not spurious_on_device:
        raise NotImplementedError(
            "spurious-bicluster removal (R/obtain_bicl.r:31-133) is outside the accelerated path; "
            "pass spurious=False or do it on the R side (INTEGRATION.md).")
    remove = bool(spurious) and not no_clusts
    if distance not in _DISTANCES:
        raise ValueError("distance must be one of 'euclidean', 'manhattan' or 'cosine'.")         # utils.r:425
    is_sp = [sparse.is_sparse(d) for d in data]
    if remove:
        _spurious.check_num_repeats(num_repeats)
        if any(is_sp):
            raise NotImplementedError("spurious-bicluster removal needs shuffled views: device shuffles of sparse views "
                                      "are not supported")
    for v in range(n_v):
        if is_sp[v]:
            sparse.validate(data[v], f"view {v}")
    if score_bisil and any(is_sp):
        raise NotImplementedError("the bisilhouette score of sparse views is not supported (dense views only)")
    if any(is_sp) and host_init and (init_f is None or init_g is None or init_s is None):
        raise NotImplementedError("host_init=True (NumPy's dense SVD) is not available for sparse views; the device "
                                  "initialisation (host_init=False) works on them")
    phi = np.zeros((n_v, n_v)) if phi is None else np.asarray(phi, dtype=np.float64)
    xi = np.zeros((n_v, n_v)) if xi is None else np.asarray(xi, dtype=np.float64)
    psi = np.zeros((n_v, n_v)) if psi is None else np.asarray(psi, dtype=np.float64)
    if row_names is None or col_names is None:
        rn, cn = naming.give_names(data, None, None)
        row_names = row_names or rn
        col_names = col_names or cn
    if row_indices is None:
        row_indices = naming.shared_names(row_names)
    if column_indices is None:
        column_indices = naming.shared_names(col_names)

    lam = mu = None
    if init_f is None or init_g is None or init_s is None:                                        # update_steps.r:41
        init_f = init_s = init_g = None
        if host_init:
            init_f, init_s, init_g, lam, mu = svd_init(data, k_vec, seed)
    if init_f is not None:
        init_f, init_s, init_g = _as_list(init_f), _as_list(init_s), _as_list(init_g)

    eng = Engine([d.shape[0] for d in data], [d.shape[1] for d in data], k_vec, device_id=device_id,
                 **(engine_opts or {}), **({"nnz": [d.nnz if sp else None for d, sp in zip(data, is_sp)]} if any(is_sp) else {}))
    try:
        _load_engine(eng, data, init_f, init_s, init_g, lam, mu, phi, xi, psi,
                     row_names, col_names, row_indices, column_indices, seed=seed)
        init_state = [eng.get_factors(v) for v in range(n_v)] if return_init else None      # (F, S, G, lambda, mu) the loop starts from
        total_err = eng.run(n_iters=n_iters, tol=1.0e-6, max_iters=max_iters)
        out_f, out_s, out_g, row_cl, col_cl, lams, mus = [], [], [], [], [], [], []
        for v in range(n_v):
            f, s, g, rc, cc = eng.finalise(v)                                                     # main.r:110 + obtain_bicl.r:162-180
            out_f.append(f); out_s.append(s); out_g.append(g); row_cl.append(rc); col_cl.append(cc)
            _, _, _, lv, mv = eng.get_factors(v)
            lams.append(lv); mus.append(mv)
        check = None
        if remove:                                                                                # obtain_bicl.r:151-188
            check = _spurious.check_on_device(eng, num_repeats, seed, max_iters=max_iters, device_id=device_id)
        score_fn = None
        if score_bisil and not no_clusts:                                                         # obtain_bicl.r:189-199
            score_fn = lambda rc, cc: bisil.score(rc, cc, distance, engine=eng)             # noqa: E731
        cleaned = _remove_then_score({"output_s": out_s, "row_clusters": row_cl, "col_clusters": col_cl}, check, score_fn)
    finally:
        eng.close()
    row_cl, col_cl, score = cleaned["row_clusters"], cleaned["col_clusters"], cleaned.get("bisil")
    if no_clusts:                                                                                 # main.r:115-120
        res = {"output_f": out_f, "output_s": out_s, "output_g": out_g}
        if return_init:
            res["init"] = init_state
        return res
    if n_iters is None:
        error = float(np.mean(total_err[-10:]))                                                   # main.r:127
    else:
        error = float(total_err[-1])                                                              # main.r:129
    res = {
        "output_f": out_f, "output_s": out_s, "output_g": out_g,
        "Error": error, "All_Error": total_err,
        "bisil": score,           # None unless score_bisil (bisil.py; parity with bisilhouette::bisilhouette unpinned)
        "row_clusters": row_cl, "col_clusters": col_cl,
        "lambda": lams, "mu": mus,
    }
    if "spurious" in cleaned:
        res["spurious"] = cleaned["spurious"]
    if return_init:               # (test hook: the initial state the device built, for a reference run from the same start)
        res["init"] = init_state
    return res


def _remove_then_score(res: dict, check: Optional[dict], score_fn: Optional[Callable]) -> dict:
    """R's order (``R/obtain_bicl.r:176-199``): with a ``check`` (``check_biclusters``' scores and thresholds) the
    removal first (``spurious.apply_removal``: copies, ``"spurious"`` added), then ``"bisil"`` = ``score_fn(row_clusters,
    col_clusters)`` of the cleaned clusters (``None`` without a ``score_fn``).  Returns a new dict."""
    out = _spurious.apply_removal(res, check) if check is not None else dict(res)
    out["bisil"] = None if score_fn is None else score_fn(out["row_clusters"], out["col_clusters"])
    return out


def _number_biclusters(results) -> float:
    """``number_biclusters`` (``R/stability_analysis.r:92-97``): the sum of every row-cluster matrix; 0 for results
    without cluster matrices (``no_clusts``)."""
    return float(sum(np.asarray(rc).sum() for rc in (results.get("row_clusters") or [])))


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
                    spurious_on_device: bool = False):
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
    ``seed + 2000 + r`` for repeat r); without it, ``NotImplementedError`` as before.
    Keyword-only extras: names, ``device_id``, ``seed`` of the draws and the device SVD inits, ``group``,
    ``max_iters``; test hooks: ``return_repeats`` (adds ``"repeats"``: per repeat the trimmed draws, relevance and
    the sub-sample's own clusters -- under ``"stability"`` of a copy of the result), ``repeat_runner(r)`` (replaces
    one repeat; nothing touches the device).
    """
    if _number_biclusters(results) == 0:                                                          # :308-311
        warnings.warn("No biclusters detected!")
        return results
    if spurious and not spurious_on_device:
        raise NotImplementedError("stability selection with spurious-bicluster removal inside its repeats "
                                  "(R/stability_analysis.r:254-266) is outside the accelerated path; pass spurious=False")
    spurious_repeats = _spurious.check_num_repeats(num_repeats) if spurious else 0
    _check_stability_numbers(sample_rate, stab_thres)
    if int(n_stability) != n_stability or n_stability < 1:
        raise ValueError("n_stability must be a positive integer.")
    data = _views(data)
    n_v = len(data)
    k = int(np.atleast_1d(k)[0])
    seed = 0 if seed is None else int(seed)
    from . import batched
    dev = None
    if repeat_runner is None:
        if row_names is None or col_names is None:
            rn, cn = naming.give_names(data, None, None, row_names, col_names)
            row_names = row_names or rn
            col_names = col_names or cn
        dev = batched.DeviceData(data, phi, xi, psi, row_names, col_names, device_id=device_id, pre_processed=True)
    try:
        stab = batched.stability_relevance_on_device(dev, results, k, int(n_stability), float(sample_rate), n_iters,
                                                     seed, group, max_iters, keep_clusters=return_repeats,
                                                     runner=repeat_runner, spurious_repeats=spurious_repeats)
    finally:
        if dev is not None:
            dev.close()
    if not stab["stability_performed"]:                                                          # :323-325
        warnings.warn("Unable to perform stability analysis due to sparsity of data.")
        return results
    relevance = stab["relevance"]
    if not remove_unstable:                                                                       # :328-329
        out = {"res": results, "relevance": relevance}
    else:                                                                                         # :330-337
        out = dict(results)
        out["row_clusters"] = [np.array(rc, dtype=np.float64, copy=True) for rc in results["row_clusters"]]
        out["col_clusters"] = [np.array(cc, dtype=np.float64, copy=True) for cc in results["col_clusters"]]
        for i in range(n_v):
            drop = relevance[i] < stab_thres
            out["row_clusters"][i][:, drop] = 0.0
            out["col_clusters"][i][:, drop] = 0.0
    if return_repeats:
        out = dict(out)
        out["stability"] = {"relevance": relevance, "repeats": stab["repeats"]}
    return out


def apply_resnmtf(data, init_f=None, init_s=None, init_g=None, k_val=None,
                  phi=None, xi=None, psi=None, n_iters=None, k_min=3, k_max=8,
                  distance="euclidean", spurious=True, num_repeats=5, no_clusts=False,
                  sample_rate=0.9, n_stability=5, stability=True, stab_thres=0.4,
                  remove_unstable=True, use_parallel=True, *, row_names=None, col_names=None,
                  device_id: int = 0, max_iters: int = 100000, seed: Optional[int] = None,
                  k_sweep: bool = False, return_sweep: bool = False, sweep_runner: Optional[Callable] = None,
                  spurious_on_device: bool = False):
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
    ``apply_resnmtf(data, k_sweep=True, spurious_on_device=True)``."""
    data = _views(data)
    n_v = len(data)
    if k_val is None and k_sweep:
        return _apply_k_sweep(data, init_f, init_s, init_g, phi, xi, psi, n_iters, k_min, k_max, distance, spurious,
                              num_repeats, no_clusts, sample_rate, n_stability, stability, stab_thres, remove_unstable,
                              row_names=row_names, col_names=col_names, device_id=device_id, max_iters=max_iters,
                              seed=seed, return_sweep=return_sweep, sweep_runner=sweep_runner,
                              spurious_on_device=spurious_on_device)
    if k_val is None:
        raise NotImplementedError("the k sweep (R/main.r:279-321) needs the bisilhouette score, which is "
                                  "outside the accelerated path; pass k_val")
    if stability and spurious and not no_clusts and not spurious_on_device:
        raise NotImplementedError("stability selection with spurious-bicluster removal (R/obtain_bicl.r:31-133) is "
                                  "outside the accelerated path; pass spurious=False (or stability=False and do the "
                                  "removal on the R side, INTEGRATION.md)")
    for name, val in (("n_iters", n_iters), ("num_repeats", num_repeats), ("n_stability", n_stability)):
        if val is not None and (int(val) != val or val < 1):
            raise ValueError(f"{name} must be a positive integer.")                               # utils.r:220-253
    _check_stability_numbers(sample_rate, stab_thres)                                             # utils.r:286-300
    k_vec = [int(np.atleast_1d(k_val)[0])] * n_v                                                  # main.r:226
    ranks = [d.shape[1] for d in data]
    if any(k < 1 for k in k_vec):
        raise ValueError("k_vec must be a vector of integers greater than 1.")                    # utils.r:437
    if any(k > r for k, r in zip(k_vec, ranks)):
        raise ValueError("k_vec must be a vector of integers less than or equal to the ranks of the views.")
    rn, cn = naming.give_names(data, phi, psi, row_names, col_names)                              # main.r:228
    row_idx, col_idx = naming.shared_names(rn), naming.shared_names(cn)                           # main.r:230
    phi_m = naming.init_rest_mats(phi, n_v)                                                       # main.r:233-235
    psi_m = naming.init_rest_mats(psi, n_v)
    xi_m = naming.init_rest_mats(xi, n_v)
    data = naming.check_data(data)                                                                # main.r:237
    results = res_nmtf_inner(data, row_idx, col_idx, init_f, init_s, init_g, k_vec, phi_m, xi_m, psi_m,
                             n_iters, num_repeats, spurious, distance, no_clusts,
                             row_names=rn, col_names=cn, device_id=device_id, max_iters=max_iters, seed=seed,
                             spurious_on_device=spurious_on_device)
    if stability:                                                                                 # main.r:255-262
        results = stability_check(data, results, k_vec, phi_m, xi_m, psi_m, n_iters, spurious, num_repeats,
                                  no_clusts, distance, sample_rate, n_stability, stab_thres,
                                  row_names=rn, col_names=cn, device_id=device_id, seed=seed,
                                  max_iters=max_iters, spurious_on_device=spurious_on_device)
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
                   device_id, max_iters, seed, return_sweep, sweep_runner, spurious_on_device=False):
    """``apply_resnmtf`` with ``k_val = NULL`` (``R/main.r:269-334``); see ``apply_resnmtf``."""
    n_v = len(data)
    for name, val in (("n_iters", n_iters), ("num_repeats", num_repeats), ("n_stability", n_stability)):
        if val is not None and (int(val) != val or val < 1):
            raise ValueError(f"{name} must be a positive integer.")                               # utils.r:220-253
    _check_whole_number(k_min, "k_min")
    _check_whole_number(k_max, "k_max")
    if k_max <= k_min:
        raise ValueError("k_max must be greater than k_min.")                                     # utils.r:250-252
    k_min, k_max = int(k_min), int(k_max)
    if distance not in _DISTANCES:
        raise ValueError("distance must be one of 'euclidean', 'manhattan' or 'cosine'.")         # utils.r:425
    _check_stability_numbers(sample_rate, stab_thres)                                             # utils.r:286-300
    if spurious and not no_clusts and not spurious_on_device:
        raise NotImplementedError("spurious-bicluster removal (R/obtain_bicl.r:31-133) is outside the accelerated "
                                  "path; pass spurious=False")
    spurious_repeats = _spurious.check_num_repeats(num_repeats) if spurious and not no_clusts else 0
    if no_clusts:
        raise ValueError("the k sweep ranks the biclusters by their bisilhouette score: no_clusts=True has none")
    if any(sparse.is_sparse(d) for d in data):
        raise NotImplementedError("the k sweep scores with the bisilhouette, which is not supported for sparse views "
                                  "(dense views only); pass k_val")
    if init_f is not None or init_s is not None or init_g is not None:
        raise NotImplementedError("the k sweep starts every k from the device's SVD initialisation; explicit initial "
                                  "factors are not supported with k_val=None")
    cap = min(min(d.shape[1] for d in data), 64)
    if k_max > cap:
        raise ValueError("k_vec must be a vector of integers less than or equal to the ranks of the views.")
    seed = 0 if seed is None else int(seed)
    rn, cn = naming.give_names(data, phi, psi, row_names, col_names)                              # main.r:228
    phi_m = naming.init_rest_mats(phi, n_v)                                                       # main.r:233-235
    psi_m = naming.init_rest_mats(psi, n_v)
    xi_m = naming.init_rest_mats(xi, n_v)
    data = naming.check_data(data)                                                                # main.r:237
    dev = None
    try:
        if sweep_runner is None:
            from . import batched
            dev = batched.DeviceData(data, phi_m, xi_m, psi_m, rn, cn, device_id=device_id, pre_processed=True)

            def scored(r):                                  # a res_nmtf_inner result with its bisil (main.r:131-139)
                out = {key: r[key] for key in ("output_f", "output_s", "output_g", "Error", "All_Error")}
                cleaned = _remove_then_score({key: r[key] for key in ("output_s", "row_clusters", "col_clusters")},
                                             r.get("spurious_check"),
                                             lambda rc, cc: bisil.score(rc, cc, distance, engine=dev.base))
                out["bisil"] = cleaned["bisil"]
                out.update({key: cleaned[key] for key in ("row_clusters", "col_clusters")})
                out.update({key: r[key] for key in ("lambda", "mu")})
                if "spurious" in cleaned:
                    out["spurious"] = cleaned["spurious"]
                return out

            # every k, the extra ones included, with the correct shared-column maps (R's extension loop passes NULL
            # ones, R/main.r:305-309)
            def run(k):
                return scored(dev.factorise(k, n_iters, seed + k, max_iters=max_iters, tag=f"k={k}", return_lm=True,
                                            spurious_repeats=spurious_repeats, spurious_seed=seed + k))

            initial = [scored(r) for r in batched.k_sweep_on_device(dev, k_min, k_max, n_iters, seed,       # main.r:279-290
                                                                    max_iters=max_iters, return_lm=True,
                                                                    spurious_repeats=spurious_repeats)]
        else:
            run, initial = sweep_runner, None
        ks, scores, results, pick = _sweep(run, k_min, k_max, cap, initial)
    finally:
        if dev is not None:
            dev.close()
    results = results[pick]                                                                       # main.r:313-314
    if stability:                                                                                 # main.r:324-332
        results = stability_check(data, results, [ks[pick]] * n_v, phi_m, xi_m, psi_m, n_iters, spurious, num_repeats,
                                  no_clusts, distance, sample_rate, n_stability, stab_thres, remove_unstable,
                                  row_names=rn, col_names=cn, device_id=device_id, seed=seed, max_iters=max_iters,
                                  spurious_on_device=spurious_on_device)
    if return_sweep:
        results = dict(results)
        results["k_sweep"] = {"k": ks, "bisil": scores}
    return results
