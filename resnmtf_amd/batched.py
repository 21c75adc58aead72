"""Batched driver for the repeated factorisations around the hot path.

The reference calls ``res_nmtf_inner`` many times per ``apply_resnmtf``: once per candidate k
(``R/main.r:279-321``), ``num_repeats`` times on shuffled data for spurious-bicluster removal
(``R/obtain_bicl.r:31-42``) and ``n_stability`` times on sub-samples (``R/stability_analysis.r:215-278``)
-- 36 to 66 independent factorisations.  They share nothing, so they are replicas: this module
builds the job lists with the reference's own sampling rules and runs them, sharded round-robin
over the ranks of a ``torch.distributed`` process group when there is one (one process per GPU, no
collective in the data path; the results are gathered as Python objects at the end).

Stability selection is scored here too: ``stability_relevance_on_device`` runs the repeats of ``stability_check``
and reduces each sub-sample's factorisation to its relevance values on the device (``resnmtf_relevance``);
``stability_relevance_fp64`` does the same in double precision without a handle (``resnmtf_fp64_subsample``, the fp64
run, ``resnmtf_fp64_relevance``), over the same draws and the same trimming loop.  What is
NOT here: the other scores computed from the factorisations -- the bisilhouette (``bisil.py``, scored on
``DeviceData.base`` by the k sweep of ``api.apply_resnmtf``) and the JSD scores (``spurious.py``).

Sparse views (``scipy.sparse``) stay sparse on the device.  Their copies (k sweep) and sub-samples (stability repeats,
the trimming probes included) are gathered on the host and uploaded, unless the keyword-only opt-in
``sparse_on_device=True`` is passed down (``DeviceData.child`` / ``factorise`` / ``stability_repeat``,
``k_sweep_on_device``, ``stability_relevance_on_device``): then they are made on the device from ``DeviceData.base``
(``resnmtf_copy_view_sparse``, ``resnmtf_subsample_count_sparse`` + ``resnmtf_subsample_view_sparse``) and the results
are those of the host route, except that a sub-sample's ``data_norms`` is summed from the f32 values the device holds
(DESIGN.md section 10 "Device copies and sub-samples").
"""
from __future__ import annotations

import contextlib
from collections import namedtuple
from dataclasses import dataclass, field
from typing import Callable, Dict, List, Optional, Sequence

import numpy as np

from . import device_views, naming, sparse, spurious
from . import engine as _engine
from ._lib import GROUP_MAX_K, GROUP_MAX_VIEW_ENTRIES, GROUP_MAX_VIEWS, MAX_K
from .engine import Engine, group_run
from .problem import (fit_fp64_on_device, inner_result, load_child, pair_table, prepare,  # noqa: F401  (shuffled_engines:
                      reported_error, shuffled_engines, svd_init)                         # part of this module's surface)


@dataclass
class Job:
    """One independent factorisation: the arguments of ``apply_resnmtf`` with a known k."""
    data: List[np.ndarray]
    k_val: int
    phi: Optional[np.ndarray] = None
    xi: Optional[np.ndarray] = None
    psi: Optional[np.ndarray] = None
    n_iters: Optional[int] = None
    seed: int = 0
    row_names: Optional[List[List[str]]] = None
    col_names: Optional[List[List[str]]] = None
    tag: str = ""
    extras: Dict = field(default_factory=dict)


def shuffle_view(x: np.ndarray, rng: np.random.Generator) -> np.ndarray:
    """``shuffle_view`` (``R/obtain_bicl.r:11-22``): all entries permuted uniformly, redrawn while a
    row or a column sums to zero."""
    x = np.asarray(x, dtype=np.float64)
    while True:
        messed = rng.permutation(x.ravel()).reshape(x.shape)
        if not ((messed.sum(axis=0) == 0).any() or (messed.sum(axis=1) == 0).any()):
            return messed


def subsample_views(data: Sequence[np.ndarray], sample_rate: float, rng: np.random.Generator,
                    row_names: Optional[Sequence[Sequence[str]]] = None,
                    col_names: Optional[Sequence[Sequence[str]]] = None, max_attempts: int = 20):
    """The sampling of ``stability_repeat`` (``R/stability_analysis.r:215-249`` with ``initial_shuffle``
    ``:111-132`` and ``sample_view`` ``:156-193``): view 1 draws ``floor(dim * sample_rate)`` rows and
    columns without replacement; a later view re-uses view 1's draw along every axis on which it
    has view 1's extent, else draws its own; all-zero rows / columns of a sub-sample are dropped
    (from every earlier view sharing that draw).  The sub-samples are NOT re-normalised (Appendix
    B11).  Returns ``(new_data, row_samples, col_samples, new_row_names, new_col_names)`` or ``None``
    after ``max_attempts`` failures (the reference prints and gives up at 20, ``:223-226``)."""
    data = [np.asarray(d, dtype=np.float64) for d in data]
    n_v = len(data)
    dim_1 = data[0].shape
    for _ in range(max_attempts - 1):
        rows: List[np.ndarray] = [None] * n_v
        cols: List[np.ndarray] = [None] * n_v
        new: List[np.ndarray] = [None] * n_v
        rows[0] = rng.choice(dim_1[0], int(dim_1[0] * sample_rate), replace=False)           # :230
        cols[0] = rng.choice(dim_1[1], int(dim_1[1] * sample_rate), replace=False)           # :231
        new[0] = data[0][np.ix_(rows[0], cols[0])]
        if (new[0].sum(axis=0) == 0).any() or (new[0].sum(axis=1) == 0).any():               # :233-240
            keep_c = new[0].sum(axis=0) != 0; keep_r = new[0].sum(axis=1) != 0
            rows[0] = rows[0][keep_r]; cols[0] = cols[0][keep_c]
            new[0] = data[0][np.ix_(rows[0], cols[0])]
        for i in range(1, n_v):
            dims = data[i].shape
            same_r, same_c = dims[0] == dim_1[0], dims[1] == dim_1[1]
            rows[i] = rows[0] if same_r else rng.choice(dims[0], int(dims[0] * sample_rate), replace=False)   # :114-118
            cols[i] = cols[0] if same_c else rng.choice(dims[1], int(dims[1] * sample_rate), replace=False)   # :119-123
            new[i] = data[i][np.ix_(rows[i], cols[i])]
            if (new[i].sum(axis=0) == 0).any() or (new[i].sum(axis=1) == 0).any():           # :165-190
                keep_c = new[i].sum(axis=0) != 0; keep_r = new[i].sum(axis=1) != 0
                for p in (range(i + 1) if same_r else [i]):
                    rows[p] = rows[p][keep_r]
                for p in (range(i + 1) if same_c else [i]):
                    cols[p] = cols[p][keep_c]
                for p in range(i + 1):
                    new[p] = data[p][np.ix_(rows[p], cols[p])]
        if all((d.sum(axis=0) != 0).all() and (d.sum(axis=1) != 0).all() for d in new):      # test_cond
            rn = None if row_names is None else [[row_names[v][t] for t in rows[v]] for v in range(n_v)]
            cn = None if col_names is None else [[col_names[v][t] for t in cols[v]] for v in range(n_v)]
            return new, rows, cols, rn, cn
    return None


# ---------------------------------------------------------------------------------------------
# job lists
# ---------------------------------------------------------------------------------------------
def k_sweep_jobs(data, k_min: int = 3, k_max: int = 8, phi=None, xi=None, psi=None, n_iters=None, seed: int = 0,
                 row_names=None, col_names=None) -> List[Job]:
    """The factorisations of the k sweep, ``R/main.r:270-290`` (one per k in ``k_min:k_max``; the
    reference then scores them with the bisilhouette and may extend the range, ``:291-312``)."""
    return [Job(list(data), k, phi, xi, psi, n_iters, seed + k, row_names, col_names, tag=f"k={k}")
            for k in range(k_min, k_max + 1)]


def shuffled_jobs(data, n_clusts: int, num_repeats: int = 5, seed: int = 0, n_iters=None) -> List[Job]:
    """``obtain_shuffled_f`` (``R/obtain_bicl.r:31-42``): ``num_repeats`` factorisations of
    independently shuffled copies of every view -- no restrictions, fresh names
    (``temp_row_*``, ``:19-20``), so the views are uncoupled."""
    rng = np.random.default_rng(seed)
    return [Job([shuffle_view(x, rng) for x in data], n_clusts, None, None, None, n_iters, seed + 1000 + r,
                tag=f"shuffle={r}") for r in range(num_repeats)]


def stability_jobs(data, k: int, n_stability: int = 5, sample_rate: float = 0.9, phi=None, xi=None, psi=None,
                   n_iters=None, seed: int = 0, row_names=None, col_names=None) -> List[Job]:
    """The factorisations of ``stability_check`` (``R/stability_analysis.r:305-323``): one per
    repeat on a sub-sample drawn by ``subsample_views``; the draws are kept in ``extras`` for the
    relevance computation (on the device: ``stability_relevance_on_device``).  Repeats whose sampling fails are skipped, as the reference
    does (``stability_performed = FALSE``)."""
    rng = np.random.default_rng(seed)
    data = [np.asarray(d, dtype=np.float64) for d in data]
    row_names, col_names = naming.give_names(data, phi, psi, row_names, col_names)
    jobs = []
    for r in range(n_stability):
        s = subsample_views(data, sample_rate, rng, row_names, col_names)
        if s is None:
            continue
        new, rows, cols, rn, cn = s
        jobs.append(Job(new, k, phi, xi, psi, n_iters, seed + 2000 + r, rn, cn, tag=f"stability={r}",
                        extras={"row_samples": rows, "col_samples": cols}))
    return jobs


# ---------------------------------------------------------------------------------------------
# execution
# ---------------------------------------------------------------------------------------------
def run_job(job: Job, device_id: int = 0, pre_processed: bool = False, return_init: bool = False) -> dict:
    """One factorisation through the accelerated path: naming, symmetrisation and (unless
    ``pre_processed``) non-negativity shift + normalisation as ``apply_resnmtf`` does, device-side SVD
    initialisation, the loop, finalise."""
    from . import api      # (lazy: api imports this module at its top for DeviceData and the repeats)
    p = prepare([np.asarray(d, dtype=np.float64) for d in job.data], job.phi, job.xi, job.psi, job.row_names, job.col_names,
                normalise=not pre_processed, symmetrise=True)
    res = api.res_nmtf_inner(p.data, p.row_shared, p.col_shared, None, None, None, [job.k_val] * len(p.data), p.phi, p.xi,
                             p.psi, job.n_iters, spurious=False, row_names=p.row_names, col_names=p.col_names,
                             device_id=device_id, seed=job.seed, return_init=return_init)
    res["tag"] = job.tag
    res["extras"] = job.extras
    return res


def run_jobs(jobs: Sequence[Job], device_id: int = 0, group=None, runner: Optional[Callable] = None,
             pre_processed: bool = False) -> List[dict]:
    """Run independent jobs; with an initialised ``torch.distributed`` group of W ranks, rank r runs
    jobs r, r + W, ... on its GPU and every rank returns the complete list in job order.  ``runner``
    replaces ``run_job`` (the CPU tests inject a stand-in)."""
    runner = runner or (lambda job: run_job(job, device_id=device_id, pre_processed=pre_processed))
    rank, world, dist = 0, 1, None
    try:
        import torch.distributed as dist_mod
        if dist_mod.is_available() and dist_mod.is_initialized():
            dist = dist_mod
            rank, world = dist.get_rank(group), dist.get_world_size(group)
    except ImportError:
        pass
    mine = {i: runner(jobs[i]) for i in range(rank, len(jobs), world)}
    if world == 1:
        return [mine[i] for i in range(len(jobs))]
    gathered: List[Optional[dict]] = [None] * world
    dist.all_gather_object(gathered, mine, group=group)
    merged: Dict[int, dict] = {}
    for part in gathered:
        merged.update(part)
    return [merged[i] for i in range(len(jobs))]


# ---------------------------------------------------------------------------------------------
# many small jobs in one launch: one workgroup per job, fp64 (resnmtf_group_run)
# ---------------------------------------------------------------------------------------------
GroupLimits = namedtuple("GroupLimits", "path max_views max_k max_view_entries")
GROUPED_LIMITS = GroupLimits("grouped", GROUP_MAX_VIEWS, GROUP_MAX_K, GROUP_MAX_VIEW_ENTRIES)      # resnmtf_group_run
FP64_LIMITS = GroupLimits("fp64", GROUP_MAX_VIEWS, MAX_K, None)                                    # resnmtf_fp64_run: no cap on n * m


def _check_group_limits(i: int, data, k: int, limits: GroupLimits = GROUPED_LIMITS):
    if len(data) > limits.max_views:
        raise ValueError(f"job {i}: the {limits.path} path takes at most {limits.max_views} views, got {len(data)}")
    if not 1 <= k <= limits.max_k:
        raise ValueError(f"job {i}: the {limits.path} path takes 1 <= k <= {limits.max_k}, got k = {k}")
    for v, x in enumerate(data):
        n, m = x.shape
        if k > n or k > m:
            raise ValueError(f"job {i}: k = {k} exceeds a dimension of view {v} ({n} x {m})")
        if limits.max_view_entries is not None and n * m > limits.max_view_entries:
            raise ValueError(f"job {i}: view {v} has {n * m} entries, above the {limits.path} path's 2^22; use run_jobs")


def prepare_grouped_job(job: Job, i: int = 0, pre_processed: bool = False, init=None,
                        limits: GroupLimits = GROUPED_LIMITS, allow_sparse: bool = False) -> dict:
    """The problem ``engine.group_run`` receives for one job, prepared as ``run_job`` prepares it for the engine:
    names, shared-name index pairs, symmetrised restrictions, ``check_data`` unless ``pre_processed``, and the initial
    factors ``init`` = (F, S, G[, lambda, mu]) per view or, when None, ``api.svd_init(data, k_vec, job.seed)`` on the
    host.  Sparse views and jobs over the kernel's limits are refused here; ``limits`` names the path and its caps
    (``GROUPED_LIMITS``, the default, or ``FP64_LIMITS`` for ``engine.fp64_run``).  ``allow_sparse`` (opt-in, the fp64
    path alone: DESIGN.md section 22): ``scipy.sparse`` views pass -- canonical CSC copies, validated
    (``sparse.validate``) and pre-processed as on the f32 route -- and need an explicit ``init`` (NumPy's dense SVD is
    not available for them); sparse tensors in device memory stay refused."""
    sparse_views = [d for d in job.data if sparse.is_sparse_view(d)]
    if sparse_views:
        if not (allow_sparse and all(sparse.is_sparse(d) for d in sparse_views)):
            raise NotImplementedError(f"job {i}: the {limits.path} path takes dense views only; run sparse views with run_jobs")
        if init is None:
            raise NotImplementedError(f"job {i}: the host SVD initialisation (NumPy's dense SVD) is not available for sparse "
                                      "views; pass init = (F, S, G[, lambda, mu])")
    data = [sparse.canonical_csc(d) if sparse.is_sparse(d) else np.asarray(d, dtype=np.float64) for d in job.data]
    if any(d.ndim != 2 for d in data):
        raise ValueError(f"job {i}: every view must be a matrix")
    n_v, k = len(data), int(job.k_val)
    _check_group_limits(i, data, k, limits)
    for v, d in enumerate(data):
        if sparse.is_sparse(d):
            sparse.validate(d, f"view {v}")
    p = prepare(data, job.phi, job.xi, job.psi, job.row_names, job.col_names, normalise=not pre_processed, symmetrise=True)
    data = p.data
    if init is None:
        init = svd_init(data, [k] * n_v, job.seed)
    init = list(init)
    if len(init) not in (3, 5):
        raise ValueError(f"job {i}: an initial state is (F, S, G) or (F, S, G, lambda, mu) per view")
    f0, s0, g0 = init[0], init[1], init[2]
    lam0 = init[3] if len(init) > 3 else None
    mu0 = init[4] if len(init) > 4 else None
    for what, mats, shape in (("F", f0, lambda n, m: (n, k)), ("S", s0, lambda n, m: (k, k)), ("G", g0, lambda n, m: (m, k)),
                              ("lambda", lam0, lambda n, m: (k,)), ("mu", mu0, lambda n, m: (k,))):
        if mats is None:
            continue
        if len(mats) != n_v:
            raise ValueError(f"job {i}: the initial {what} must hold one entry per view")
        for v, (a, x) in enumerate(zip(mats, data)):
            want = shape(*x.shape)
            if np.shape(a) != want:
                raise ValueError(f"job {i}, view {v}: the initial {what} has shape {np.shape(a)}, expected {want}")
    return {"data": data, "k": k, "init_f": list(f0), "init_s": list(s0), "init_g": list(g0),
            "init_lam": None if lam0 is None else list(lam0), "init_mu": None if mu0 is None else list(mu0),
            "phi": p.phi, "xi": p.xi, "psi": p.psi, "row_pairs": pair_table(p.row_names, p.row_shared),
            "col_pairs": pair_table(p.col_names, p.col_shared), "n_iters": job.n_iters,
            "row_names": p.row_names, "col_names": p.col_names}


def _binary_clusters(f, g, s):
    """``R/obtain_bicl.r:162-180`` with ``remove_spurious = FALSE``: thresholds 1/n and 1/m, row clusters re-ordered by
    the first maximum of every S column."""
    rc = (f > 1.0 / f.shape[0]).astype(np.float64)
    cc = (g > 1.0 / g.shape[0]).astype(np.float64)
    return rc[:, np.argmax(s, axis=0)], cc


def run_jobs_grouped(jobs: Sequence[Job], device_id: int = 0, pre_processed: bool = False, inits=None,
                     max_iters: int = 100000, group_runner: Optional[Callable] = None) -> List[dict]:
    """Run independent jobs in one ``resnmtf_group_run`` call: every job in its own workgroup, fp64 throughout, from
    ``inits[i]`` = (F, S, G[, lambda, mu]) per view when given, else from ``api.svd_init`` on the host with the job's
    seed.  Returns, in job order, the keys ``run_job`` returns (``bisil`` None).  Every job is prepared and checked
    (dense views only, at most 8 views, 1 <= k <= 32, n * m <= 2^22 per view) before any device work.
    ``group_runner(problems, tol=, max_iters=, device_id=)`` replaces ``engine.group_run`` (a test hook)."""
    jobs = list(jobs)
    if inits is not None and len(inits) != len(jobs):
        raise ValueError("inits must hold one initial state per job")
    for i, job in enumerate(jobs):                    # refusals first, before any SVD or device work
        if any(sparse.is_sparse_view(d) for d in job.data):
            raise NotImplementedError(f"job {i}: the grouped path takes dense views only; run sparse views with run_jobs")
        _check_group_limits(i, [np.asarray(d) for d in job.data], int(job.k_val))
    problems = [prepare_grouped_job(job, i, pre_processed, None if inits is None else inits[i]) for i, job in enumerate(jobs)]
    outs = (group_runner or group_run)(problems, tol=1.0e-6, max_iters=max_iters, device_id=device_id)
    results = []
    for job, out in zip(jobs, outs):
        rcs, ccs = zip(*[_binary_clusters(f, g, s) for f, g, s in zip(out["f"], out["g"], out["s"])])
        results.append(inner_result(out["f"], out["s"], out["g"], np.asarray(out["all_error"], dtype=np.float64), job.n_iters,
                                    row_clusters=list(rcs), col_clusters=list(ccs), lam=out["lambda"], mu=out["mu"], tag=job.tag,
                                    extras=job.extras))
    return results


def run_job_fp64(job: Job, device_id: int = 0, pre_processed: bool = False, init=None, max_iters: int = 100000,
                 runner: Optional[Callable] = None, sparse: bool = False) -> dict:
    """One job through the device-wide fp64 path (``engine.fp64_run``): prepared as
    ``prepare_grouped_job`` prepares it -- dense views only, at most 8 views, 1 <= k <= 64, no cap on n * m -- from
    ``init`` = (F, S, G[, lambda, mu]) per view or, when None, ``api.svd_init`` on the host with the job's seed.
    Returns the keys ``run_job`` returns (``bisil`` None).  ``runner(problem, tol=, max_iters=, device_id=)`` replaces
    ``engine.fp64_run`` (a test hook); every refusal comes before it is called.  ``sparse`` (opt-in, DESIGN.md section
    22): ``scipy.sparse`` views are accepted and reach the runner as canonical CSC matrices, pre-processed as on the f32
    route; they need an explicit ``init``."""
    problem = prepare_grouped_job(job, 0, pre_processed, init, limits=FP64_LIMITS, allow_sparse=bool(sparse))
    out = (runner or _engine.fp64_run)(problem, tol=1.0e-6, max_iters=max_iters, device_id=device_id)
    rcs, ccs = zip(*[_binary_clusters(f, g, s) for f, g, s in zip(out["f"], out["g"], out["s"])])
    return inner_result(out["f"], out["s"], out["g"], np.asarray(out["all_error"], dtype=np.float64), job.n_iters,
                        row_clusters=list(rcs), col_clusters=list(ccs), lam=out["lambda"], mu=out["mu"], tag=job.tag,
                        extras=job.extras)


# ---------------------------------------------------------------------------------------------
# the same job kinds with the data resident on the device: one upload, copies / shuffles drawn there
# ---------------------------------------------------------------------------------------------
Child = namedtuple("Child", "eng row_names col_names samples host_views")


class DeviceData:
    """The pre-processed views of one data set, uploaded once (``resnmtf_set_view_raw``) and kept for
    any number of factorisations (``resnmtf_copy_view`` / ``resnmtf_shuffle_view``).  At c2 size an
    upload costs ~45 ms of PCIe + conversion, 500 sweeps ~23 ms: re-uploading per job would dominate.

    ``pre_processed=True`` (opt-in) takes the data as ``res_nmtf_inner`` receives them: the views are uploaded exactly
    as given (``resnmtf_set_view``, no shift, no normalisation) and ``phi`` / ``xi`` / ``psi`` are the symmetrised
    matrices, used as they are -- the form ``stability_check`` gets both in (``R/main.r:255-262``; its sub-samples are
    not re-normalised).

    A dense view may be a 2-D floating ``torch`` tensor on ``cuda:device_id``: it is uploaded in place
    (``resnmtf_set_view_device``, with the shift and the normalisation unless ``pre_processed``), bitwise as its values
    widened on the host would be, and never converted to NumPy; a ``device_views.RawDeviceView`` is pre-processed at
    its upload either way (what ``prepare(normalise=True)`` makes of a device tensor)."""

    def __init__(self, data, phi=None, xi=None, psi=None, row_names=None, col_names=None, device_id: int = 0,
                 pre_processed: bool = False):
        # sparse views (scipy.sparse) stay sparse: a canonical, pre-processed CSC copy on the host, from which the
        # sub-samples are gathered, and a sparse view on the device
        # A sparse tensor in device memory has no host copy: self.sp holds its marker (device_views.SparseDeviceView:
        # shape and nnz), the device checks stand in for sparse.validate, the device normalises at the base upload, and
        # its copies and sub-samples are made on the device whatever sparse_on_device says.
        data = [device_views.host_or_device(d, f"view {v}") for v, d in enumerate(data)]
        self.sp = [device_views.as_sparse_view(d, device_id, f"view {v}") if device_views.is_sparse_device_view(d) else
                   (None if not sparse.is_sparse(d) else (sparse.canonical_csc(d) if pre_processed else sparse.check_data_one(d)))
                   for v, d in enumerate(data)]
        for v, c in enumerate(self.sp):
            if pre_processed and c is not None and not self._sp_device(v):
                sparse.validate(c)
        data = [device_views.as_view(d, device_id, f"view {v}") if c is None else c for v, (d, c) in enumerate(zip(data, self.sp))]
        self.data_shapes = [tuple(d.shape) for d in data]
        n_v = len(data)
        # (not pre_processed: the device shifts and normalises the dense views, set_view_raw below)
        p = prepare(data, phi, xi, psi, row_names, col_names, normalise=False, symmetrise=not pre_processed)
        self.rn, self.cn, self.phi, self.xi, self.psi = p.row_names, p.col_names, p.phi, p.xi, p.psi
        self.device_id = device_id
        self.base = Engine([s[0] for s in self.data_shapes], [s[1] for s in self.data_shapes], [2] * n_v, device_id=device_id,
                           nnz=[None if c is None else c.nnz for c in self.sp])
        self.was_negative = [False] * n_v
        for v in range(n_v):
            if self._sp_device(v):
                device_views.upload_sparse(self.base, v, self.sp[v], pre_processed=pre_processed)      # (the device normalises)
            elif self.sp[v] is not None:
                self.base.set_view_sparse(v, self.sp[v], pre_processed=True)      # (normalised on the host: self.sp)
            else:           # (a host array: set_view / set_view_raw; a tensor: set_view_device, in place)
                self.was_negative[v] = device_views.upload(self.base, v, data[v], raw=not pre_processed)

    def close(self):
        self.base.close()

    def _sp_device(self, v: int) -> bool:
        """View ``v`` is a sparse view that came from device memory: ``self.sp[v]`` is its marker, not a host copy."""
        return isinstance(self.sp[v], device_views.SparseDeviceView)

    def _trim_samples(self, samples, max_rounds: int = 20, *, sparse_on_device: bool = False, counts: Optional[dict] = None):
        """``sample_view`` / ``stability_repeat`` (``R/stability_analysis.r:165-190``, ``:233-240``): all-zero rows and
        columns of a sub-sample are dropped -- from every earlier view that shares the draw (equal extent along that
        axis) -- and the sub-samples gathered again, until none is left.  The emptiness test runs on the device
        (``resnmtf_view_empty_lines``), on probes that hold only the data; a sparse view's sub-sample is gathered on the
        host instead, or with ``sparse_on_device`` (opt-in) probed like a dense one: the count of its stored entries
        (``Engine.subsample_count_sparse``), a sparse probe of that capacity, ``subsample_view_sparse_from``.  Returns the
        trimmed draws or ``None``.  ``counts``: a dict of the caller's that receives, per sparse view probed on the
        device, ``(rows, cols, stored entries)`` of its last probe (``child`` sizes its engine from them)."""
        def probe_view(i, rows_i, cols_i):
            if self.sp[i] is not None and (sparse_on_device or self._sp_device(i)):
                count = self.base.subsample_count_sparse(i, rows_i, cols_i)
                if counts is not None:
                    counts[i] = (rows_i, cols_i, count)
                with Engine([len(rows_i)], [len(cols_i)], [2], device_id=self.device_id, nnz=[count]) as probe:
                    probe.subsample_view_sparse_from(0, self.base, i, rows_i, cols_i)
                    return probe.empty_lines(0)
            if self.sp[i] is not None:              # sparse view: the sub-sample is gathered on the host
                _, er, ec = sparse.subsample(self.sp[i], rows_i, cols_i)
                return er, ec
            with Engine([len(rows_i)], [len(cols_i)], [2], device_id=self.device_id) as probe:
                probe.subsample_view_from(0, self.base, i, rows_i, cols_i)
                return probe.empty_lines(0)

        return trim_samples(self.data_shapes, samples, probe_view, max_rounds)

    def _subsample_count(self, v: int, rows, cols, counts: dict) -> int:
        """The stored entries of the sub-sample of sparse view ``v``: the count ``_trim_samples`` left in ``counts`` for
        its last probe when that probe had these lists (a view trimmed through a later one is counted again), else a
        count."""
        seen = counts.get(v)
        if seen is not None and np.array_equal(seen[0], rows) and np.array_equal(seen[1], cols):
            return seen[2]
        return self.base.subsample_count_sparse(v, rows, cols)

    @contextlib.contextmanager
    def child(self, k: int, seed: int = 0, shuffle_seed: Optional[int] = None, samples=None, *, shuffle_sparse: bool = False,
              sparse_on_device: bool = False):
        """An engine with k biclusters per view, loaded from ``self.base`` and closed on exit: the views copied -- or
        shuffled as ``obtain_shuffled_f`` does (``shuffle_seed``: no restrictions, uncoupled), or sub-sampled as
        ``stability_repeat`` does (``samples = (row_samples, col_samples)``: trimmed first, ``_trim_samples``; not
        re-normalised, names carried over) -- and SVD-initialised on the device (``problem.load_child``).  Yields
        ``Child(eng, row_names, col_names, samples, host_views)``: the names in use, the trimmed samples, what was uploaded
        of a sparse view -- or ``None`` when the trimming fails (``R/stability_analysis.r:223-226``).  ``shuffle_sparse``
        (opt-in): with ``shuffle_seed`` the sparse views are shuffled on the device as sparse views
        (``resnmtf_shuffle_view_sparse``); without it they are refused.  ``sparse_on_device`` (opt-in): the sparse views
        are copied (``resnmtf_copy_view_sparse``) or sub-sampled (``resnmtf_subsample_view_sparse``, the trimming
        included) from ``self.base`` on the device instead of gathered on the host and uploaded; the new engine's view
        is sized from ``base.view_storage`` or from the sub-sample's count, and ``host_views[v]`` is ``None`` for it
        (``Engine.get_view_sparse`` reads the same f32-rounded matrix).  Shuffles are not affected."""
        n_v = len(self.data_shapes)
        shapes, rn, cn = self.data_shapes, self.rn, self.cn
        counts = {}
        if samples is not None:
            samples = self._trim_samples(samples, sparse_on_device=sparse_on_device, counts=counts)
            if samples is None:
                yield None
                return
            shapes = [(len(samples[0][v]), len(samples[1][v])) for v in range(n_v)]
            rn = [[self.rn[v][t] for t in samples[0][v]] for v in range(n_v)]
            cn = [[self.cn[v][t] for t in samples[1][v]] for v in range(n_v)]
        if shuffle_seed is not None and any(c is not None for c in self.sp) and not shuffle_sparse:
            raise NotImplementedError("device shuffles of sparse views are not supported")
        # sparse views: the whole view or its sub-sample, gathered on the host
        on_device = [(sparse_on_device or self._sp_device(v)) and shuffle_seed is None and c is not None for v, c in enumerate(self.sp)]
        host_views = [None if c is None or on_device[v] else
                      (c if samples is None else sparse.subsample(c, samples[0][v], samples[1][v])[0])
                      for v, c in enumerate(self.sp)]
        nnz = [None if hv is None else hv.nnz for hv in host_views]
        for v in range(n_v):
            if on_device[v]:
                nnz[v] = self.base.view_storage(v)[1] if samples is None else self._subsample_count(v, samples[0][v], samples[1][v], counts)
        more = {"sparse_on_device": True} if any(on_device) else {}      # (off: the calls are exactly the earlier ones)
        if any(on_device) and not sparse_on_device:
            more = {"sparse_on_device": on_device}                        # (view by view: scipy.sparse views keep the host route)
        with Engine([s[0] for s in shapes], [s[1] for s in shapes], [k] * n_v, device_id=self.device_id, nnz=nnz) as eng:
            load_child(eng, self.base, seed, shuffle_seed=shuffle_seed, samples=samples, host_views=host_views,
                       coupling=(self.phi, self.xi, self.psi, rn, cn), shuffle_sparse=shuffle_sparse, **more)
            yield Child(eng, rn, cn, samples, host_views)

    def factorise(self, k: int, n_iters: Optional[int] = None, seed: int = 0, shuffle_seed: Optional[int] = None,
                  max_iters: int = 100000, tag: str = "", samples=None, return_init: bool = False,
                  return_data: bool = False, return_lm: bool = False, spurious_repeats: int = 0,
                  spurious_seed: int = 0, *, shuffle_sparse: bool = False, sparse_on_device: bool = False,
                  output: str = "numpy", post_on_device: bool = False) -> dict:
        """One factorisation with k biclusters per view of the views copied, shuffled (``shuffle_seed``) or sub-sampled
        (``samples``) on the device (``child``): device SVD init, loop, finalise.  With ``samples`` whose trimming
        fails: ``{"stability_performed": False, "tag"}``.
        ``return_init`` / ``return_data`` add the initial (F, S, G, lambda, mu) per view and the device's copy of the
        data actually factorised (fp32 precision) to the result: what a reference run needs to start from the same place.
        ``return_lm`` adds ``"lambda"`` / ``"mu"`` per view (the keys of a ``res_nmtf_inner`` result, for the k sweep of
        ``apply_resnmtf``).  ``spurious_repeats`` = R >= 2: the scores of ``check_biclusters`` against R shuffles of
        this factorisation's own device copy (``spurious.check_on_device`` with ``spurious_seed``) as
        ``"spurious_check"`` (the caller removes).  ``shuffle_sparse`` (opt-in): sparse views are shuffled as sparse
        views, by ``shuffle_seed`` and by the spurious check alike; ``return_data`` of a shuffled sparse view stays
        refused with ``output="numpy"`` (the host holds no copy of the shuffle: ``Engine.get_view_sparse`` reads it without
        densifying).
        ``sparse_on_device`` (opt-in): sparse views are copied / sub-sampled on the device (``child``); ``return_data``
        then reads them back (``Engine.get_view_sparse``: the same f32-rounded matrix).  ``output="torch"`` adds
        ``"device_out"``: per view ``Engine.finalise_device``'s five tensors (the other keys stay NumPy), and with
        ``return_data`` ``"device_data"``: per view the device's copy of the data factorised, left on the device -- a
        dense fp32 tensor (``Engine.get_view_device``) or a ``sparse_csc`` tensor (``Engine.get_view_sparse_device``).  A
        shuffled sparse view is then not refused: its entry of ``"data"`` is ``None`` and ``"device_data"`` holds the
        shuffle.  ``post_on_device`` (opt-in, needs ``output="torch"``, else ``ValueError``):
        ``Engine.finalise`` and ``Engine.get_factors`` are not called -- ``output_f`` / ``output_s`` / ``output_g`` /
        ``row_clusters`` / ``col_clusters`` ARE ``finalise_device``'s tensors and ``"lambda"`` / ``"mu"`` come from
        ``get_factors_device`` (the two k-vectors copied to the host); same values, bit for bit."""
        n_v = len(self.data_shapes)
        device_views.check_output(output)
        if post_on_device and output != "torch":
            raise ValueError("post_on_device=True needs output='torch' (the steps after the loop then work on the device tensors).")
        shuffled_sparse = shuffle_seed is not None and any(c is not None for c in self.sp)
        if return_data and shuffled_sparse and output != "torch":
            raise NotImplementedError("return_data of a shuffled sparse view is not supported (it would densify the shuffle)")
        with self.child(k, seed, shuffle_seed, samples, shuffle_sparse=shuffle_sparse, sparse_on_device=sparse_on_device) as ch:
            if ch is None:
                return {"stability_performed": False, "tag": tag}
            eng = ch.eng
            init_state = [eng.get_factors(v) for v in range(n_v)] if return_init else None
            # (sparse views: the host copy rounded to f32, as the device holds the values)
            data_used = ([None if shuffled_sparse and self.sp[v] is not None else
                          ch.host_views[v].toarray().astype(np.float32).astype(np.float64) if ch.host_views[v] is not None
                          else (eng.get_view_sparse(v).toarray() if self.sp[v] is not None else eng.get_view(v))
                          for v in range(n_v)] if return_data else None)
            data_dev = ([eng.get_view_sparse_device(v) if self.sp[v] is not None else eng.get_view_device(v) for v in range(n_v)]
                        if return_data and output == "torch" else None)
            errs = eng.run(n_iters=n_iters, tol=1.0e-6, max_iters=max_iters)
            check = (spurious.check_on_device(eng, spurious_repeats, spurious_seed, max_iters=max_iters,
                                              device_id=self.device_id, shuffle_sparse=shuffle_sparse)
                     if spurious_repeats else None)
            if post_on_device:           # nothing of size n or m is downloaded
                fin = fin_dev = [eng.finalise_device(v) for v in range(n_v)]
                lms = ([[device_views.to_numpy(t) for t in eng.get_factors_device(v)[3:]] for v in range(n_v)]
                       if return_lm else None)
            else:
                fin = [eng.finalise(v) for v in range(n_v)]
                fin_dev = [eng.finalise_device(v) for v in range(n_v)] if output == "torch" else None
                lms = [eng.get_factors(v)[3:] for v in range(n_v)] if return_lm else None
        f, s, g, rc, cc = (list(x) for x in zip(*fin))
        return inner_result(f, s, g, errs, n_iters, device_data=True, row_clusters=rc, col_clusters=cc, tag=tag,
                            extras={} if ch.samples is None else {"row_samples": ch.samples[0], "col_samples": ch.samples[1]},
                            row_names=ch.row_names, col_names=ch.col_names, init=init_state,
                            lam=lms and [lm[0] for lm in lms], mu=lms and [lm[1] for lm in lms], data=data_used,
                            data_on_device=data_dev,
                            spurious_check=check, device_out=fin_dev)

    def stability_repeat(self, k: int, n_iters: Optional[int], seed: int, samples, max_iters: int = 100000, tag: str = "",
                         keep_clusters: bool = False, spurious_repeats: int = 0, spurious_seed: int = 0, *,
                         shuffle_sparse: bool = False, sparse_on_device: bool = False) -> dict:
        """One repeat of ``stability_check`` (``R/stability_analysis.r:215-278``): the sub-sample ``samples`` factorised
        (``child``) and, instead of finalise, its clusters scored against the reference clusters set on ``self.base``
        (``resnmtf_relevance``, ``:268-276``) -- the result holds the n_views x k ``"relevance"`` matrix and no factors,
        or ``{"stability_performed": False, "tag"}`` when the trimming fails.  ``keep_clusters`` adds the sub-sample's
        own binary clusters (a test hook: they cost a finalise download).  ``spurious_repeats`` = R >= 2: the cluster
        columns flagged against R shuffles of the sub-sample (``spurious.check_on_device`` with ``spurious_seed``) are
        removed before the scoring (``resnmtf_relevance_masked``, ``:254-276``) and the kept clusters are the cleaned
        ones.  ``shuffle_sparse`` (opt-in): the shuffles of a sparse view are drawn from the repeat's own sparse
        sub-sample handle (gathered on the host as before) and re-normalised, as for dense views.  ``sparse_on_device``
        (opt-in): the sparse sub-sample is probed, trimmed and gathered on the device (``child``); the shuffles keep
        drawing from the repeat's own handle."""
        n_v = len(self.data_shapes)
        with self.child(k, seed, samples=samples, sparse_on_device=sparse_on_device) as ch:
            if ch is None:
                return {"stability_performed": False, "tag": tag}
            eng, (rows, cols) = ch.eng, ch.samples
            errs = eng.run(n_iters=n_iters, tol=1.0e-6, max_iters=max_iters)
            check = (spurious.check_on_device(eng, spurious_repeats, spurious_seed, max_iters=max_iters,
                                              device_id=self.device_id, shuffle_sparse=shuffle_sparse)
                     if spurious_repeats else None)
            if check is None:
                rel = [eng.relevance(v, self.base, v, rows[v], cols[v]) for v in range(n_v)]
            else:
                flags = spurious.removal_flags(check)
                rel = [eng.relevance_masked(v, self.base, v, rows[v], cols[v], flags[v]) for v in range(n_v)]
            res = {"stability_performed": True, "relevance": np.stack(rel), "Error": reported_error(errs, n_iters),
                   "All_Error": errs, "tag": tag, "extras": {"row_samples": rows, "col_samples": cols}}
            if keep_clusters:
                fin = [eng.finalise(v) for v in range(n_v)]
                kept = {"output_s": [f[1] for f in fin], "row_clusters": [f[3] for f in fin], "col_clusters": [f[4] for f in fin]}
                if check is not None:
                    kept = spurious.apply_removal(kept, check)
                res["row_clusters"], res["col_clusters"] = kept["row_clusters"], kept["col_clusters"]
        return res


def k_sweep_on_device(dev: DeviceData, k_min: int = 3, k_max: int = 8, n_iters=None, seed: int = 0, group=None,
                      max_iters: int = 100000, return_lm: bool = False, spurious_repeats: int = 0, *,
                      shuffle_sparse: bool = False, sparse_on_device: bool = False, output: str = "numpy",
                      post_on_device: bool = False) -> List[dict]:
    """The factorisations of the k sweep (``R/main.r:279-290``) from one upload; sharded round-robin over
    the ranks of an initialised process group (every rank holds its own ``DeviceData``).  ``spurious_repeats``: each
    k's result carries its ``"spurious_check"`` (``DeviceData.factorise``, spurious seed ``seed + k``).
    ``sparse_on_device`` (opt-in): every k copies the sparse views from ``dev.base`` on the device
    (``resnmtf_copy_view_sparse``) instead of uploading the host CSC again.  ``output`` / ``post_on_device``:
    ``DeviceData.factorise``."""
    more = {"sparse_on_device": True} if sparse_on_device else {}
    if output != "numpy":
        more["output"] = output
    if post_on_device:
        more["post_on_device"] = True
    ks = list(range(k_min, k_max + 1))
    return run_jobs(ks, group=group, runner=lambda k: dev.factorise(k, n_iters, seed + k, max_iters=max_iters, tag=f"k={k}",
                                                                    return_lm=return_lm, spurious_repeats=spurious_repeats,
                                                                    spurious_seed=seed + k, shuffle_sparse=shuffle_sparse, **more))


def shuffles_on_device(dev: DeviceData, n_clusts: int, num_repeats: int = 5, n_iters=None, seed: int = 0, group=None,
                       max_iters: int = 100000, *, shuffle_sparse: bool = False) -> List[dict]:
    """``obtain_shuffled_f`` (``R/obtain_bicl.r:31-42``) with the shuffles drawn on the device (``shuffle_sparse``:
    sparse views shuffled as sparse views, ``DeviceData.child``)."""
    reps = list(range(num_repeats))
    return run_jobs(reps, group=group,
                    runner=lambda r: dev.factorise(n_clusts, n_iters, seed + 1000 + r, shuffle_seed=seed * 7919 + r + 1,
                                                   max_iters=max_iters, tag=f"shuffle={r}", shuffle_sparse=shuffle_sparse))


def stability_on_device(dev: DeviceData, k: int, n_stability: int = 5, sample_rate: float = 0.9, n_iters=None, seed: int = 0,
                        group=None, *, sparse_on_device: bool = False) -> List[dict]:
    """The factorisations of ``stability_check`` (``R/stability_analysis.r:305-323``): the draws follow
    ``subsample_views`` (shared draws for equal extents), the sub-samples are gathered on the device; all-zero rows /
    columns of a sub-sample -- the pre-processed data are non-negative, not positive: ``make_non_neg`` leaves a zero
    at every shifted column's minimum and sparse inputs stay sparse -- are dropped as the reference does
    (``DeviceData._trim_samples``); a repeat whose sampling fails returns ``stability_performed = False``.
    ``sparse_on_device`` (opt-in): sparse views are probed, trimmed and sub-sampled on the device (``DeviceData.child``)."""
    more = {"sparse_on_device": True} if sparse_on_device else {}
    draws = stability_draws(dev.data_shapes, n_stability, sample_rate, seed)
    return run_jobs(list(range(n_stability)), group=group,
                    runner=lambda r: dev.factorise(k, n_iters, seed + 2000 + r, samples=draws[r], tag=f"stability={r}", **more))


def stability_draws(shapes, n_stability: int, sample_rate: float, seed: int = 0):
    """The untrimmed draws of the ``n_stability`` repeats, ``[(row_samples, col_samples)]``: view 1 draws
    ``floor(dim * sample_rate)`` rows and columns, a later view re-uses view 1's draw along an axis of equal extent
    (``R/stability_analysis.r:111-132``, ``:230-231``)."""
    rng = np.random.default_rng(seed)
    draws = []
    for _ in range(n_stability):
        rows, cols = [], []
        for v, (n, m) in enumerate(shapes):
            same_r = v > 0 and n == shapes[0][0]
            same_c = v > 0 and m == shapes[0][1]
            rows.append(rows[0] if same_r else rng.choice(n, int(n * sample_rate), replace=False))      # :114-118, :230
            cols.append(cols[0] if same_c else rng.choice(m, int(m * sample_rate), replace=False))      # :119-123, :231
        draws.append((rows, cols))
    return draws


def trim_samples(shapes, samples, probe: Callable, max_rounds: int = 20):
    """``sample_view`` / ``stability_repeat`` (``R/stability_analysis.r:165-190``, ``:233-240``): all-zero rows and
    columns of a sub-sample are dropped -- from every earlier view that shares the draw (equal extent along that axis)
    -- and the sub-samples probed again, until none is left.  ``probe(i, rows, cols)`` returns the boolean masks
    ``(empty_rows, empty_cols)`` of view i's sub-sample at these lists; which route answers it is the caller's (the f32
    engine's probes: ``DeviceData._trim_samples``; ``engine.fp64_subsample``: ``stability_relevance_fp64``).  Returns the
    trimmed ``(rows, cols)`` or ``None`` (a sub-sample below 2 x 2, or no fixed point after ``max_rounds``)."""
    n_v = len(shapes)
    rows = [np.asarray(r).copy() for r in samples[0]]; cols = [np.asarray(c).copy() for c in samples[1]]
    for _ in range(max_rounds):
        changed = False
        for i in range(n_v):
            if len(rows[i]) < 2 or len(cols[i]) < 2:
                return None
            er, ec = probe(i, rows[i], cols[i])
            if er.any() or ec.any():
                changed = True
                same_r = shapes[i][0] == shapes[0][0]
                same_c = shapes[i][1] == shapes[0][1]
                for p in (range(i + 1) if same_r else [i]):            # :168-174
                    if len(rows[p]) == len(er):
                        rows[p] = rows[p][~er]
                for p in (range(i + 1) if same_c else [i]):            # :175-181
                    if len(cols[p]) == len(ec):
                        cols[p] = cols[p][~ec]
        if not changed:
            return rows, cols
    return None


def mean_relevance(repeats: Sequence[dict], n_stability: int) -> Optional[np.ndarray]:
    """``stability_check``'s reduction (``R/stability_analysis.r:315-327``): the repeats' n_views x k relevance
    matrices summed on the host in repeat order, then divided by ``n_stability`` -- the same additions in the same
    order whatever the number of ranks that computed them.  ``None`` when a repeat was not performed (the reference
    then returns the results unchanged)."""
    total = None
    for rep in repeats:
        if not rep.get("stability_performed", True):
            return None
        rel = np.asarray(rep["relevance"], dtype=np.float64)
        total = (np.zeros_like(rel) if total is None else total) + rel
    return total / n_stability


def stability_relevance_on_device(dev: Optional[DeviceData], results: dict, k: int, n_stability: int = 5,
                                  sample_rate: float = 0.9, n_iters=None, seed: int = 0, group=None,
                                  max_iters: int = 100000, keep_clusters: bool = False,
                                  runner: Optional[Callable] = None, spurious_repeats: int = 0, *,
                                  shuffle_sparse: bool = False, sparse_on_device: bool = False) -> dict:
    """The repeats of ``stability_check`` (``R/stability_analysis.r:302-334``) with their scoring on the device:
    ``results``' binary clusters are set once on ``dev.base`` (``resnmtf_set_reference_clusters``; a view whose two cluster
    matrices are ``torch`` tensors on the engine's GPU: ``resnmtf_set_reference_clusters_device``, read in place), repeat r
    factorises the sub-sample of ``stability_draws`` (trimmed as ``stability_on_device`` does) up to the end of the loop
    and returns its n_views x k relevance (``resnmtf_relevance``) -- no factor leaves the device.  The repeats are
    sharded round-robin over the ranks of an initialised process group (``run_jobs``; every rank holds its own
    ``DeviceData`` and the same ``results``) and reduced by ``mean_relevance``.  ``runner(r)`` replaces the
    repeat (the CPU tests inject a stand-in; ``dev`` is then not used).  Returns ``{"stability_performed",
    "relevance" (None when not performed), "repeats"}``.  ``spurious_repeats`` = R >= 2: every repeat removes its
    spurious biclusters before it is scored (``R/stability_analysis.r:254-266``), against R shuffles of its own
    sub-sample drawn with the spurious seed ``seed + 2000 + r`` -- the repeat's own factorisation seed, so that repeat r
    equals ``remove_spurious(sub_data, sub_result, R, seed=seed + 2000 + r)``; per repeat only the k-sized flags, scores
    and the null scores cross to the host.  ``sparse_on_device`` (opt-in): the repeats probe, trim and gather the sparse
    views' sub-samples on the device (``DeviceData.stability_repeat``)."""
    if runner is None:
        more = {"sparse_on_device": True} if sparse_on_device else {}
        n_v = len(dev.data_shapes)
        for v in range(n_v):
            rc, cc = results["row_clusters"][v], results["col_clusters"][v]
            if all(device_views.is_tensor(x) and device_views.on_engine_device(x, dev.device_id) for x in (rc, cc)):
                dev.base.set_reference_clusters_device(v, rc, cc)
            else:
                dev.base.set_reference_clusters(v, rc, cc)
        draws = stability_draws(dev.data_shapes, n_stability, sample_rate, seed)

        def runner(r):
            return dev.stability_repeat(k, n_iters, seed + 2000 + r, draws[r], max_iters=max_iters, tag=f"stability={r}",
                                        keep_clusters=keep_clusters, spurious_repeats=spurious_repeats,
                                        spurious_seed=seed + 2000 + r, shuffle_sparse=shuffle_sparse, **more)
    repeats = run_jobs(list(range(n_stability)), group=group, runner=runner)
    rel = mean_relevance(repeats, n_stability)
    return {"stability_performed": rel is not None, "relevance": rel, "repeats": repeats}


def stability_repeat_fp64(data, results, k: int, n_iters, seed: int, samples, phi, xi, psi, row_names, col_names,
                          max_iters: int = 100000, device_id: int = 0, tag: str = "", keep_clusters: bool = False,
                          spurious_repeats: int = 0, return_init: bool = False, fp64_init: bool = False) -> dict:
    """One repeat of ``stability_check`` (``R/stability_analysis.r:215-278``) in double precision:
    the draws ``samples`` trimmed (``trim_samples`` with ``engine.fp64_subsample`` as the probe), every view's sub-sample
    an fp64 tensor on the device (``resnmtf_fp64_subsample``: the fp64 values, not re-normalised, names carried over; the
    tensor of the view's last probe, whose lists are the trimmed ones, is the one factorised: one gather per view when
    nothing is trimmed), factorised by ``res_nmtf_inner(precision="fp64", fp64_device=True, output="torch")`` at ``seed`` --
    with ``spurious_repeats`` = R >= 2 its spurious biclusters removed there (``fp64_spurious``, spurious seed ``seed``) --
    and the cluster tensors it leaves scored against ``results``' clusters (``engine.fp64_relevance``; tensors on the
    device are read in place).  Returns ``DeviceData.stability_repeat``'s dict, or ``{"stability_performed": False,
    "tag"}`` when the trimming fails.  ``keep_clusters`` adds the sub-sample's (cleaned) clusters as NumPy arrays,
    ``return_init`` the start of the factorisation (test hooks).
    A view of ``data`` that is stored sparse (``stability_check`` admits it with
    ``fp64_subsample_sparse=True``) is probed by ``engine.fp64_subsample_sparse`` instead: its sub-sample is a
    ``sparse_csc`` tensor on the device, the same rule holds for it (the tensor of the last probe is the sub-sample), and the
    fit then also gets ``fp64_sparse_device=True`` -- with ``spurious_repeats`` also ``fp64_shuffle_sparse=True`` -- so that
    it is factorised, and its draws are shuffled, as the sparse device view it is.  Dense and sparse views mix; without a
    sparse view every call is the one it was.  ``fp64_init``: the fit starts from
    ``engine.fp64_init_svd`` of the sub-samples at ``seed`` instead of a short-lived f32 engine; passed on only when set."""
    n_v = len(data)
    shapes = [tuple(int(s) for s in d.shape) for d in data]
    stored_sparse = [sparse.is_sparse_view(d) for d in data]
    last = {}                                     # per view: the lists and the tensor of its latest probe (one alive per view)

    def probe(i, rows_i, cols_i):
        gather = _engine.fp64_subsample_sparse if stored_sparse[i] else _engine.fp64_subsample
        t, er, ec = gather(data[i], rows_i, cols_i, device_id)
        last[i] = (rows_i, cols_i, t)
        return er, ec
    trimmed = trim_samples(shapes, samples, probe)
    if trimmed is None:
        return {"stability_performed": False, "tag": tag}
    rows, cols = trimmed
    # trim_samples ends with a round in which every view was probed and nothing changed: each view's latest probe had
    # the final lists, so its tensor is the sub-sample to factorise and nothing is gathered twice
    assert all(np.array_equal(last[v][0], rows[v]) and np.array_equal(last[v][1], cols[v]) for v in range(n_v))
    subs = [last[v][2] for v in range(n_v)]
    last.clear()
    rn = [[row_names[v][t] for t in rows[v]] for v in range(n_v)]
    cn = [[col_names[v][t] for t in cols[v]] for v in range(n_v)]
    more = {"return_init": True} if return_init else {}
    if spurious_repeats:
        more.update(spurious_on_device=True, fp64_spurious=True)
    if any(stored_sparse):                        # (only then: without a sparse sub-sample the fit is the call it was)
        more.update(fp64_sparse_device=True)
        if spurious_repeats:
            more.update(fp64_shuffle_sparse=True)
    if fp64_init:
        more.update(fp64_init=True)
    res = fit_fp64_on_device(subs, k, phi, xi, psi, n_iters, spurious_repeats if spurious_repeats else 5, bool(spurious_repeats),
                             row_names=rn, col_names=cn, device_id=device_id, max_iters=max_iters, seed=seed, **more)
    del subs
    rel = [_engine.fp64_relevance(res["row_clusters"][v], res["col_clusters"][v], results["row_clusters"][v],
                                  results["col_clusters"][v], rows[v], cols[v], device_id) for v in range(n_v)]
    out = {"stability_performed": True, "relevance": np.stack(rel), "Error": res["Error"], "All_Error": res["All_Error"],
           "tag": tag, "extras": {"row_samples": rows, "col_samples": cols}}
    if keep_clusters:
        out["row_clusters"] = [device_views.to_numpy(t) for t in res["row_clusters"]]
        out["col_clusters"] = [device_views.to_numpy(t) for t in res["col_clusters"]]
    if return_init:
        out["init"] = res["init"]
    return out


def stability_relevance_fp64(data, results: dict, k: int, n_stability: int, sample_rate: float, n_iters, seed: int, phi, xi,
                             psi, row_names, col_names, max_iters: int = 100000, device_id: int = 0,
                             keep_clusters: bool = False, spurious_repeats: int = 0, runner: Optional[Callable] = None,
                             fp64_init: bool = False) -> dict:
    """``stability_relevance_on_device`` in double precision: the repeats of ``stability_check``
    without an f32 handle.  ``data``: the pre-processed dense views, host arrays or tensors on ``cuda:device_id``.  The
    draws are ``stability_draws(shapes, n_stability, sample_rate, seed)`` -- the f32 route's for the same seed --, repeat
    r is ``stability_repeat_fp64`` at the seed ``seed + 2000 + r`` (with ``spurious_repeats`` also its spurious seed, the
    f32 route's convention), one after the other (no process group), and the reduction is ``mean_relevance``.
    ``runner(r)`` replaces the repeat (the CPU tests inject a stand-in; nothing then touches the device).  Returns
    ``{"stability_performed", "relevance" (None when not performed), "repeats"}``.  A host view is copied to the device
    once, as an fp64 tensor (``engine.fp64_device_view``), and every probe and gather of every repeat reads that copy in
    place -- one source copy per view, as ``DeviceData`` keeps one; a tensor already there is read where it lies.
    A view stored sparse (a ``scipy.sparse`` matrix, a sparse tensor on the device or its
    ``SparseDeviceView``) is uploaded once as a ``sparse_csc`` tensor of its canonical CSC
    (``engine.fp64_sparse_device_view``), or read where it lies, and its sub-samples stay sparse
    (``stability_repeat_fp64``)."""
    if runner is None:
        shapes = [tuple(int(s) for s in d.shape) for d in data]
        draws = stability_draws(shapes, n_stability, sample_rate, seed)
        sources = [_engine.fp64_sparse_device_view(d, device_id) if sparse.is_sparse_view(d) else _engine.fp64_device_view(d, device_id)
                   for d in data]

        def runner(r):
            return stability_repeat_fp64(sources, results, k, n_iters, seed + 2000 + r, draws[r], phi, xi, psi, row_names,
                                         col_names, max_iters=max_iters, device_id=device_id, tag=f"stability={r}",
                                         keep_clusters=keep_clusters, spurious_repeats=spurious_repeats,
                                         **({"fp64_init": True} if fp64_init else {}))
    repeats = [runner(r) for r in range(n_stability)]
    rel = mean_relevance(repeats, n_stability)
    return {"stability_performed": rel is not None, "relevance": rel, "repeats": repeats}
