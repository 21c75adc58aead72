"""Spurious-bicluster removal (``obtain_biclusters(..., remove_spurious = TRUE)``, ``R/obtain_bicl.r:151-204``) as a
post-step on a finished ``res_nmtf_inner`` / ``apply_resnmtf`` result, in the way ``stability_check`` is one for
stability selection:

1. ``num_repeats`` factorisations of shuffled views (``obtain_shuffled_f``, ``:31-42``) on the device
   (``batched.shuffles_on_device``; sharded over the ranks of an initialised process group);
2. per view, the Jensen-Shannon scores (``jsd_calc``, ``R/utils.r:95-106``) of the shuffled F columns against each
   other (``get_thresholds``, ``:80-102``) and of the result's F columns against them (``check_biclusters``,
   ``:113-133``), all on the device in one ``resnmtf_jsd_pairs`` call;
3. on the host: the mean, the mode of ``stats::density`` of the null scores (``density_mode``), the means of the scores
   and the removal rule (``:176-188``).

The loops the reference writes in R stay in R's order; DESIGN.md section 11.

Inside the pipeline (the opt-in ``spurious_on_device=True`` of ``res_nmtf_inner``, ``stability_check`` and
``apply_resnmtf``) the same check runs on a live engine instead (``check_on_device``): the shuffles are drawn from the
engine's own device copy (``problem.shuffled_engines``) and ``resnmtf_spurious_scores`` gathers and scores the pool on
the device; only the K scores and the null scores come back for ``thresholds``.
"""
from __future__ import annotations

import copy
from typing import Callable, Optional

import numpy as np

from . import device_views, sparse
from .engine import jsd_pairs
from .problem import shuffled_engines, shuffled_fits_fp64


# ---------------------------------------------------------------------------------------------
# stats::density with its defaults, for the mode of the null scores (a few hundred to a few
# hundred thousand values, once per view: host work)
# ---------------------------------------------------------------------------------------------
def _seq(frm: float, to: float, n: int) -> np.ndarray:
    """``seq.int(from, to, length.out = n)`` (R's symmetric form)."""
    i = np.arange(n, dtype=np.float64)
    by = (to - frm) / (n - 1)
    out = np.where(i < n // 2, frm + i * by, to - (n - 1 - i) * by)
    out[0], out[-1] = frm, to
    return out


def _dnorm(x: np.ndarray, sigma: float) -> np.ndarray:
    """``stats::dnorm(x, 0, sigma)``, with nmath's accurate branch for |x| / sigma >= 5."""
    v = np.abs(x / sigma)
    out = 0.398942280401432677939946059934 * np.exp(-0.5 * v * v) / sigma
    far = v >= 5
    if far.any():
        x1 = np.ldexp(np.rint(np.ldexp(v[far], 16)), -16)
        x2 = v[far] - x1
        out[far] = 0.398942280401432677939946059934 / sigma * (np.exp(-0.5 * x1 * x1) * np.exp((-0.5 * x2 - x1) * x2))
    out[v > np.sqrt(-2 * np.log(2) * (-1021 + 1 - 53))] = 0.0
    return out


def bw_nrd0(x: np.ndarray) -> float:
    """``stats::bw.nrd0``: 0.9 min(sd, IQR / 1.34) n^-0.2 with its fallbacks (type-7 quartiles)."""
    x = np.asarray(x, dtype=np.float64)
    if len(x) < 2:
        raise ValueError("need at least 2 data points")
    m = np.sum(x) / len(x)
    m = m + np.sum(x - m) / len(x)                      # R's refined mean: a constant vector gets sd = 0 exactly
    hi = float(np.sqrt(np.sum((x - m) ** 2) / (len(x) - 1)))
    q25, q75 = np.quantile(x, [0.25, 0.75], method="linear")
    lo = min(hi, float(q75 - q25) / 1.34)
    if lo == 0:
        lo = hi or abs(float(x[0])) or 1.0
    return 0.9 * lo * len(x) ** (-0.2)


def density(x, n: int = 512, cut: float = 3.0):
    """``stats::density(x)`` with the defaults (gaussian kernel, ``bw.nrd0``, ``from = min - cut bw``, ``to = max + cut
    bw``), R <= 4.3's coordinates: ``BinDist`` on [lo, up] = [from - 4 bw, to + 4 bw], the circular convolution with
    the kernel sampled at spacing 2 (up - lo) / (2n - 1) -- here as the equal direct Toeplitz sum (the binned mass has
    an all-zero upper half) -- clamped at 0 and interpolated onto ``seq(from, to, length.out = n)``.  Returns (x, y)."""
    x = np.asarray(x, dtype=np.float64)
    nx = len(x)
    bw = bw_nrd0(x)
    frm, to = float(x.min()) - cut * bw, float(x.max()) + cut * bw
    lo, up = frm - 4 * bw, to + 4 * bw
    xpos = (x - lo) / ((up - lo) / (n - 1))
    ix = np.floor(xpos).astype(np.int64)
    fx = xpos - ix
    w = 1.0 / nx
    y = np.zeros(n + 1)
    inner = (ix >= 0) & (ix <= n - 2)
    np.add.at(y, ix[inner], w * (1 - fx[inner]))
    np.add.at(y, ix[inner] + 1, w * fx[inner])
    np.add.at(y, np.zeros(int(np.sum(ix == -1)), dtype=np.int64), w * fx[ix == -1])
    np.add.at(y, np.full(int(np.sum(ix == n - 1)), n - 1, dtype=np.int64), w * (1 - fx[ix == n - 1]))
    y = y[:n]
    by = 2 * (up - lo) / (2 * n - 1)
    kern = _dnorm(np.arange(n) * by, bw)
    conv = np.maximum(0.0, kern[np.abs(np.arange(n)[:, None] - np.arange(n)[None, :])] @ y)
    xords, xout = _seq(lo, up, n), _seq(frm, to, n)
    j = np.clip(np.searchsorted(xords, xout, side="right"), 1, n - 1)      # xords[j - 1] <= v < xords[j] (approx's interval)
    i = j - 1
    yout = conv[i] + (conv[j] - conv[i]) * ((xout - xords[i]) / (xords[j] - xords[i]))
    yout = np.where(xout == xords[j], conv[j], np.where(xout == xords[i], conv[i], yout))
    return xout, yout


def density_mode(scores) -> float:
    """``dens <- stats::density(scores); dens$x[which.max(dens$y)]`` (the first maximum)."""
    x, y = density(scores)
    return float(x[int(np.argmax(y))])


# ---------------------------------------------------------------------------------------------
# the pair lists, in R's order
# ---------------------------------------------------------------------------------------------
def pool_pairs(K: int, R: int):
    """The pairs of one view over the column pool ``cbind(F_i, f_1[[i]], ..., f_R[[i]])`` (F column k = k, shuffle r's
    column m = K + r K + m): ``null`` in ``calculate_f_shuffle_jsd``'s order (j = 1..R-1, k, l = j+1..R, m; K^2 R(R-1)/2
    pairs) and ``score`` in ``check_biclusters``' (F column k against the R K columns of ``cbind(f_1..f_R)``)."""
    null = [(K + j * K + k, K + l * K + m) for j in range(R - 1) for k in range(K) for l in range(j + 1, R) for m in range(K)]
    score = [(k, K + y) for k in range(K) for y in range(R * K)]
    return np.array(null, dtype=np.int32).reshape(-1, 2), np.array(score, dtype=np.int32).reshape(-1, 2)


def _check_factors(mats, what):
    for i, m in enumerate(mats):
        if not np.all(np.isfinite(m)):
            raise ValueError(f"{what} of view {i} has non-finite entries")


def check_biclusters(data, output_f, num_repeats: int = 5, *, seed: Optional[int] = None, device_id: int = 0,
                     group=None, max_iters: int = 100000, shuffled_f=None, jsd: Optional[Callable] = None,
                     grouped: bool = False, shuffle_sparse: bool = False, precision: str = "f32",
                     fp64_shuffle_sparse: bool = False, fp64_init: bool = False) -> dict:
    """``check_biclusters`` (``R/obtain_bicl.r:113-133``) with ``get_thresholds`` (``:80-102``): returns
    ``{"score": n_views x K, "avg_threshold": n_views, "max_threshold": n_views}``.

    ``data``: the pre-processed views (as ``res_nmtf_inner`` receives them); ``output_f``: the result's F per view.  The
    ``num_repeats`` shuffled factorisations run on the device to convergence (``n_iters`` is not forwarded by the
    reference either; ``max_iters`` guards them), drawn from ``seed``, sharded over ``group``'s ranks; the scores come
    from ``resnmtf_jsd_pairs``.  Test hooks: ``shuffled_f`` (a list of ``num_repeats`` lists of per-view F matrices:
    no factorisation) and ``jsd(cols, pairs) -> scores`` (replaces the device scorer).  ``grouped=True``: the shuffled
    factorisations are ``batched.shuffled_jobs(data, K, num_repeats, seed)`` -- shuffled on the host, re-normalised
    (``check_data``), to convergence -- run in one ``batched.run_jobs_grouped`` call (fp64, one workgroup per job)
    instead of ``shuffles_on_device``; ``group`` is then not used.  At the default 5 repeats this is slower than the
    default path (the grouped kernel is latency-bound per job): it buys fp64 shuffled fits, not
    speed.  ``shuffle_sparse=True`` (opt-in): ``scipy.sparse`` views are shuffled as sparse views on the device
    (``resnmtf_shuffle_view_sparse``: the dense path's draws of the densified views, DESIGN.md section 10 "Sparse
    shuffles"); without it they are refused as before, and with ``grouped`` they stay refused.
    ``precision="fp64"`` (opt-in): the shuffled F's are ``problem.shuffled_fits_fp64(data, K,
    num_repeats, seed)`` -- every view drawn in double precision from the view as given (``engine.fp64_shuffle``: a host
    array, or a dense tensor on ``cuda:device_id`` read where it lies) and factorised by the fp64 path; the scorer, the
    thresholds and the result are the same.  Sparse views, ``grouped`` and ``group`` are refused with it.
    ``fp64_shuffle_sparse=True`` (opt-in; read only with ``precision="fp64"``): a sparse view -- a
    ``scipy.sparse`` matrix, taken as its canonical CSC, or a sparse tensor on ``cuda:device_id`` read where it lies -- is
    drawn by ``engine.fp64_shuffle_sparse`` and its draws are factorised as sparse device views; dense views as before.
    ``fp64_init=True`` (opt-in; read only with ``precision="fp64"``): every shuffled fit starts from
    ``engine.fp64_init_svd`` of its draws instead of a short-lived f32 engine, with the same seeds."""
    if precision not in ("f32", "fp64"):
        raise ValueError(f"precision must be 'f32' or 'fp64', got {precision!r}")
    if precision == "fp64":
        return _check_biclusters_fp64(data, output_f, num_repeats, seed=seed, device_id=device_id, group=group,
                                      max_iters=max_iters, shuffled_f=shuffled_f, jsd=jsd, grouped=grouped,
                                      shuffle_sparse=fp64_shuffle_sparse, fp64_init=fp64_init)
    R = check_num_repeats(num_repeats)
    views = list(data) if not (isinstance(data, np.ndarray) and data.ndim == 2) and not sparse.is_sparse(data) else [data]
    if any(sparse.is_sparse(d) for d in views):
        if not shuffle_sparse:
            raise NotImplementedError("spurious-bicluster removal needs shuffled views: device shuffles of sparse views are "
                                      "not supported")
        if grouped and shuffled_f is None:
            raise NotImplementedError("the grouped path takes dense views only; sparse views are shuffled on the device "
                                      "(grouped=False)")
    views = [sparse.canonical_csc(d) if sparse.is_sparse(d) else np.asarray(d, dtype=np.float64) for d in views]
    output_f, K = _checked_output_f([d.shape for d in views], output_f, R)
    if shuffled_f is None:
        from . import batched      # (lazy: batched imports this module at its top for check_on_device and the removal)
        seed = 0 if seed is None else int(seed)
        if grouped:
            reps = batched.run_jobs_grouped(batched.shuffled_jobs(views, K, R, seed=seed), device_id=device_id,
                                            pre_processed=False, max_iters=max_iters)
        else:
            dev = batched.DeviceData(views, device_id=device_id, pre_processed=True)
            try:
                reps = batched.shuffles_on_device(dev, K, R, n_iters=None, seed=seed, group=group, max_iters=max_iters,
                                                  shuffle_sparse=shuffle_sparse)
            finally:
                dev.close()
        shuffled_f = [rep["output_f"] for rep in reps]
    return _score_against_shuffles(output_f, shuffled_f, R, jsd, device_id)


def _checked_output_f(shapes, output_f, R: int):
    """The result's F per view as fp64 arrays (a tensor is downloaded), checked against the views' shapes: (F's, K)."""
    output_f = [np.asarray(device_views.to_numpy(f), dtype=np.float64) for f in output_f]
    n_v = len(shapes)
    if len(output_f) != n_v:
        raise ValueError("output_f must hold one F per view")
    K = output_f[0].shape[1]
    for i, f in enumerate(output_f):
        if f.ndim != 2 or f.shape != (shapes[i][0], K):
            raise ValueError(f"output_f[{i}] must be {shapes[i][0]} x {K}")
        if f.shape[0] < 2:
            raise ValueError("views need at least 2 rows (bw.nrd0 needs two data points)")
    _check_null_count(K, R)
    _check_factors(output_f, "output_f")
    return output_f, K


def _check_biclusters_fp64(data, output_f, num_repeats, *, seed, device_id, group, max_iters, shuffled_f, jsd, grouped,
                           shuffle_sparse: bool = False, fp64_init: bool = False) -> dict:
    """``check_biclusters(precision="fp64")``: the views as the fp64 run received them, the shuffled F's from
    ``problem.shuffled_fits_fp64``, then the scoring every route shares.  ``shuffle_sparse``
    (``fp64_shuffle_sparse``): sparse views are admitted, a ``scipy.sparse`` one as its canonical CSC.  ``fp64_init``: passed
    on to the shuffled fits, and only when it is set."""
    R = check_num_repeats(num_repeats)
    if grouped or group is not None:
        raise ValueError('precision="fp64": the shuffled fits run through resnmtf_fp64_run, one after another; grouped and '
                         'group do not apply')
    views = ([data] if (isinstance(data, np.ndarray) and data.ndim == 2) or sparse.is_sparse(data) or device_views.is_tensor(data)
             else list(data))
    views = [device_views.host_or_device(d, f"view {v}") for v, d in enumerate(views)]
    if not shuffle_sparse:
        refuse_sparse_fp64(views)
    views = [device_views.as_view(d, device_id, f"view {v}") for v, d in enumerate(views)]
    views = [sparse.canonical_csc(d) if sparse.is_sparse(d) else d for d in views]
    if any(isinstance(d, device_views.RawDeviceView) or getattr(d, "raw", False) for d in views):
        raise ValueError('precision="fp64": the views are taken as pre-processed; a RawDeviceView is not')
    output_f, K = _checked_output_f([tuple(d.shape) for d in views], output_f, R)
    if shuffled_f is None:
        flag = {"fp64_init": True} if fp64_init else {}
        shuffled_f = shuffled_fits_fp64(views, K, R, 0 if seed is None else int(seed), max_iters=max_iters, device_id=device_id,
                                        **flag)
    return _score_against_shuffles(output_f, shuffled_f, R, jsd, device_id)


def refuse_sparse_fp64(views):
    """``fp64_spurious`` / ``precision="fp64"`` with a sparse view of any kind: refused by name."""
    for v, d in enumerate(views):
        if sparse.is_sparse_view(d) or device_views.is_sparse_tensor(d) or isinstance(d, device_views.SparseDeviceView):
            raise NotImplementedError(f'precision="fp64": spurious-bicluster removal in double precision (fp64_spurious) shuffles '
                                      f'dense views only; a sparse view (view {v}) is not supported: no fp64 sparse shuffle exists')


def _score_against_shuffles(output_f, shuffled_f, R: int, jsd, device_id: int) -> dict:
    """The scores and thresholds of checked F's against ``shuffled_f`` (``R`` lists of one F per view)."""
    n_v, K = len(output_f), output_f[0].shape[1]
    if len(shuffled_f) != R or any(len(fs) != n_v for fs in shuffled_f):
        raise ValueError("shuffled_f must hold num_repeats lists of one F per view")
    shuffled_f = [[np.asarray(f, dtype=np.float64) for f in fs] for fs in shuffled_f]
    for fs in shuffled_f:
        for i, f in enumerate(fs):
            if f.shape != output_f[i].shape:
                raise ValueError(f"shuffled F of view {i} must be {output_f[i].shape[0]} x {K}")
        _check_factors(fs, "a shuffled F")
    if jsd is None:
        jsd = lambda cols, pairs: jsd_pairs(cols, pairs, device_id=device_id)    # noqa: E731
    null_p, score_p = pool_pairs(K, R)
    rows = []
    for i in range(n_v):
        pool = np.concatenate([output_f[i]] + [fs[i] for fs in shuffled_f], axis=1)
        vals = np.asarray(jsd(pool, np.concatenate([null_p, score_p])), dtype=np.float64)
        rows.append(_view_check(i, vals[len(null_p):].reshape(K, R * K), vals[:len(null_p)]))
    return _check_result(rows)


def check_num_repeats(num_repeats) -> int:
    if isinstance(num_repeats, bool) or int(num_repeats) != num_repeats or num_repeats < 2:
        raise ValueError("num_repeats must be an integer >= 2 (the reference indexes a second shuffled repeat)")
    return int(num_repeats)


def _check_null_count(K: int, R: int):
    if K * K * R * (R - 1) // 2 < 2:
        raise ValueError("a single null score (K = 1, num_repeats = 2): stats::density needs two")


def _view_check(i: int, scores, null):
    """View i's (score row, avg threshold, max threshold) from its null scores and its K scores -- or the K x (R K)
    single scores they are the row means of (``:125-128``) -- all of which must be finite."""
    scores = np.asarray(scores, dtype=np.float64)
    if not (np.all(np.isfinite(scores)) and np.all(np.isfinite(null))):
        raise ValueError(f"view {i}: a Jensen-Shannon score is not finite (a density summed to zero; R gives NaN "
                         "here and check_biclusters cannot continue)")
    return (scores if scores.ndim == 1 else scores.mean(axis=1), *thresholds(null))


def _check_result(rows) -> dict:
    score, avg, mx = zip(*rows)
    return {"score": np.array(score, dtype=np.float64), "avg_threshold": np.array(avg), "max_threshold": np.array(mx)}


def thresholds(null):
    """``get_thresholds`` (``:97-99``) of one view's null scores: (their mean, the mode of ``stats::density``)."""
    null = np.asarray(null, dtype=np.float64)
    return float(np.mean(null)), density_mode(null)


def check_on_device(eng, num_repeats: int, seed: Optional[int] = None, *, max_iters: int = 100000,
                    device_id: int = 0, shuffle_sparse: bool = False) -> dict:
    """``check_biclusters`` of the factorisation an engine holds (its F on the device, as ``finalise`` normalises it)
    against ``num_repeats`` shuffles of the engine's own views: ``problem.shuffled_engines(eng, K, num_repeats, seed)``
    -- the draws of ``check_biclusters(data, F, num_repeats, seed=seed)`` -- scored per view by
    ``resnmtf_spurious_scores``; the thresholds on the host.  Bitwise ``check_biclusters``' result for the same data,
    F and seed.  Returns ``{"score", "avg_threshold", "max_threshold"}``.  ``shuffle_sparse``: passed on to
    ``shuffled_engines`` (sparse views of ``eng`` shuffled as sparse views)."""
    n_v, K = eng.n_views, eng.k[0]
    R = check_num_repeats(num_repeats)
    if any(k != K for k in eng.k):
        raise ValueError("every view needs the same k (the reference's k_vec is one k repeated)")
    _check_null_count(K, R)
    shuffles = shuffled_engines(eng, K, R, 0 if seed is None else int(seed), max_iters=max_iters, device_id=device_id,
                                shuffle_sparse=shuffle_sparse)
    try:
        return _check_result([_view_check(i, *eng.spurious_scores(i, shuffles)) for i in range(n_v)])
    finally:
        for sh in shuffles:
            sh.close()


def removal_flags(check: dict) -> np.ndarray:
    """The removal rule ``score < max_threshold | score == 0`` (``R/obtain_bicl.r:182-183``): n_views x K, by F column."""
    score = np.asarray(check["score"], dtype=np.float64)
    mx = np.asarray(check["max_threshold"], dtype=np.float64)
    return (score < mx[:, None]) | (score == 0)


def apply_removal(results: dict, check: dict) -> dict:
    """The removal of ``obtain_biclusters`` (``R/obtain_bicl.r:176-188``) for a ``check``: view i's cluster columns
    ``relations`` (``which.max`` of every S column) flagged by ``removal_flags`` are zeroed in copies of
    ``row_clusters`` and ``col_clusters``.  Returns a copy of ``results`` with ``"spurious"``: ``check`` plus
    ``"removed"``, the n_views x K mask of the zeroed cluster columns."""
    out = dict(results)
    out["row_clusters"] = [np.array(rc, dtype=np.float64, copy=True) for rc in results["row_clusters"]]
    out["col_clusters"] = [np.array(cc, dtype=np.float64, copy=True) for cc in results["col_clusters"]]
    removed = []
    for i in range(len(out["row_clusters"])):
        relations = np.argmax(np.asarray(results["output_s"][i]), axis=0)        # apply(S, 2, which.max)
        indices = (check["score"][i] < check["max_threshold"][i]) | (check["score"][i] == 0)
        new = indices[relations]
        out["row_clusters"][i][:, new] = 0.0
        out["col_clusters"][i][:, new] = 0.0
        removed.append(new)
    out["spurious"] = dict(copy.deepcopy(check), removed=np.array(removed, dtype=bool))
    return out


def apply_removal_device(results: dict, check: dict) -> dict:
    """``apply_removal`` for cluster matrices that are ``torch`` tensors (``post_on_device``): the
    same ``removed`` mask -- ``relations`` from the k x k S, copied to the host when it is a tensor --, the flagged
    columns zeroed in clones of the cluster tensors where they live; nothing of size n or m is copied to the host and
    the inputs are not written.  ``"spurious"`` is the entry ``apply_removal`` returns."""
    out = dict(results)
    out["row_clusters"], out["col_clusters"], removed = [], [], []
    for i, (rc, cc) in enumerate(zip(results["row_clusters"], results["col_clusters"])):
        relations = np.argmax(np.asarray(device_views.to_numpy(results["output_s"][i])), axis=0)   # apply(S, 2, which.max)
        indices = (check["score"][i] < check["max_threshold"][i]) | (check["score"][i] == 0)
        new = indices[relations]
        rc, cc = rc.clone(), cc.clone()
        cols = np.flatnonzero(new)
        if cols.size:
            for t in (rc, cc):
                t[:, t.new_tensor(cols, dtype=device_views._torch().long)] = 0.0
        out["row_clusters"].append(rc)
        out["col_clusters"].append(cc)
        removed.append(new)
    out["spurious"] = dict(copy.deepcopy(check), removed=np.array(removed, dtype=bool))
    return out


def remove_spurious(data, results: dict, num_repeats: int = 5, *, grouped: bool = False, **kwargs) -> dict:
    """The removal step of ``obtain_biclusters`` (``R/obtain_bicl.r:176-188``) on a ``res_nmtf_inner(spurious=False)``
    / ``apply_resnmtf(spurious=False, stability=False)`` result: with ``check = check_biclusters(data,
    results["output_f"], num_repeats, **kwargs)``, view i's cluster columns ``relations`` (``which.max`` of every S
    column) flagged by ``score < max_threshold | score == 0`` are zeroed in ``row_clusters`` and ``col_clusters``.
    Returns a copy (F, S, G unchanged; ``results`` is not modified) with ``"spurious"``: ``check`` plus ``"removed"``,
    the n_views x K mask of the zeroed cluster columns.  ``grouped`` is passed on to ``check_biclusters``, and so is
    every other keyword -- ``precision="fp64"`` among them (the shuffles drawn and factorised in
    double precision).  A result whose cluster matrices are tensors (``output="torch"``) is cleaned where it lives
    (``apply_removal_device``)."""
    if not results.get("row_clusters") or not results.get("col_clusters"):
        raise ValueError("results has no cluster matrices (a no_clusts result): nothing to remove")
    _check_factors([device_views.to_numpy(s) for s in results["output_s"]], "output_s")
    check = check_biclusters(data, results["output_f"], num_repeats, grouped=grouped, **kwargs)
    if any(device_views.is_tensor(c) for c in results["row_clusters"]):      # (an output="torch" result: removed where it lives)
        return apply_removal_device(results, check)
    return apply_removal(results, check)
