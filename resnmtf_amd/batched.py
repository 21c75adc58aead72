"""Batched driver for the repeated factorisations around the hot path.

The reference calls ``res_nmtf_inner`` many times per ``apply_resnmtf``: once per candidate k
(``R/main.r:279-321``), ``num_repeats`` times on shuffled data for spurious-bicluster removal
(``R/obtain_bicl.r:31-42``) and ``n_stability`` times on sub-samples (``R/stability_analysis.r:215-278``)
-- 36 to 66 independent factorisations.  They share nothing, so they are replicas: this module
builds the job lists with the reference's own sampling rules and runs them, sharded round-robin
over the ranks of a ``torch.distributed`` process group when there is one (one process per GPU, no
collective in the data path; the results are gathered as Python objects at the end).

Stability selection is scored here too: ``stability_relevance_on_device`` runs the repeats of ``stability_check``
and reduces each sub-sample's factorisation to its relevance values on the device (``resnmtf_relevance``).  What is
NOT here: the other scores computed from the factorisations -- the bisilhouette (``bisil.py``, scored on
``DeviceData.base`` by the k sweep of ``api.apply_resnmtf``) and the JSD scores (``spurious.py``).
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Callable, Dict, List, Optional, Sequence

import numpy as np


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
    from . import naming
    rng = np.random.default_rng(seed)
    data = [np.asarray(d, dtype=np.float64) for d in data]
    if row_names is None or col_names is None:
        rn, cn = naming.give_names(data, phi, psi, row_names, col_names)
        row_names = row_names or rn
        col_names = col_names or cn
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
    from . import api, naming
    data = [np.asarray(d, dtype=np.float64) for d in job.data]
    n_v = len(data)
    rn, cn = naming.give_names(data, job.phi, job.psi, job.row_names, job.col_names)
    row_idx, col_idx = naming.shared_names(rn), naming.shared_names(cn)
    phi = naming.init_rest_mats(job.phi, n_v); psi = naming.init_rest_mats(job.psi, n_v); xi = naming.init_rest_mats(job.xi, n_v)
    if not pre_processed:
        data = naming.check_data(data)
    res = api.res_nmtf_inner(data, row_idx, col_idx, None, None, None, [job.k_val] * n_v, phi, xi, psi,
                             job.n_iters, spurious=False, row_names=rn, col_names=cn, device_id=device_id,
                             seed=job.seed, return_init=return_init)
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
def _check_group_limits(i: int, data, k: int):
    from ._lib import GROUP_MAX_K, GROUP_MAX_VIEW_ENTRIES, GROUP_MAX_VIEWS
    if len(data) > GROUP_MAX_VIEWS:
        raise ValueError(f"job {i}: the grouped path takes at most {GROUP_MAX_VIEWS} views, got {len(data)}")
    if not 1 <= k <= GROUP_MAX_K:
        raise ValueError(f"job {i}: the grouped path takes 1 <= k <= {GROUP_MAX_K}, got k = {k}")
    for v, x in enumerate(data):
        n, m = x.shape
        if k > n or k > m:
            raise ValueError(f"job {i}: k = {k} exceeds a dimension of view {v} ({n} x {m})")
        if n * m > GROUP_MAX_VIEW_ENTRIES:
            raise ValueError(f"job {i}: view {v} has {n * m} entries, above the grouped path's 2^22; use run_jobs")


def prepare_grouped_job(job: Job, i: int = 0, pre_processed: bool = False, init=None) -> dict:
    """The problem ``engine.group_run`` receives for one job, prepared as ``run_job`` prepares it for the engine:
    names, shared-name index pairs, symmetrised restrictions, ``check_data`` unless ``pre_processed``, and the initial
    factors ``init`` = (F, S, G[, lambda, mu]) per view or, when None, ``api.svd_init(data, k_vec, job.seed)`` on the
    host.  Sparse views and jobs over the kernel's limits are refused here."""
    from . import api, naming, sparse
    if any(sparse.is_sparse(d) for d in job.data):
        raise NotImplementedError(f"job {i}: the grouped path takes dense views only; run sparse views with run_jobs")
    data = [np.asarray(d, dtype=np.float64) for d in job.data]
    if any(d.ndim != 2 for d in data):
        raise ValueError(f"job {i}: every view must be a matrix")
    n_v, k = len(data), int(job.k_val)
    _check_group_limits(i, data, k)
    rn, cn = naming.give_names(data, job.phi, job.psi, job.row_names, job.col_names)
    row_idx, col_idx = naming.shared_names(rn), naming.shared_names(cn)
    phi = naming.init_rest_mats(job.phi, n_v); psi = naming.init_rest_mats(job.psi, n_v); xi = naming.init_rest_mats(job.xi, n_v)
    if not pre_processed:
        data = naming.check_data(data)
    if init is None:
        init = api.svd_init(data, [k] * n_v, job.seed)
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
    row_pairs = [[None if v == w else naming.index_pairs(rn[v], rn[w], row_idx[v].get(w)) for w in range(n_v)] for v in range(n_v)]
    col_pairs = [[None if v == w else naming.index_pairs(cn[v], cn[w], col_idx[v].get(w)) for w in range(n_v)] for v in range(n_v)]
    return {"data": data, "k": k, "init_f": list(f0), "init_s": list(s0), "init_g": list(g0),
            "init_lam": None if lam0 is None else list(lam0), "init_mu": None if mu0 is None else list(mu0),
            "phi": phi, "xi": xi, "psi": psi, "row_pairs": row_pairs, "col_pairs": col_pairs, "n_iters": job.n_iters,
            "row_names": rn, "col_names": cn}


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
    from . import sparse
    jobs = list(jobs)
    if inits is not None and len(inits) != len(jobs):
        raise ValueError("inits must hold one initial state per job")
    for i, job in enumerate(jobs):                    # refusals first, before any SVD or device work
        if any(sparse.is_sparse(d) for d in job.data):
            raise NotImplementedError(f"job {i}: the grouped path takes dense views only; run sparse views with run_jobs")
        _check_group_limits(i, [np.asarray(d) for d in job.data], int(job.k_val))
    problems = [prepare_grouped_job(job, i, pre_processed, None if inits is None else inits[i]) for i, job in enumerate(jobs)]
    if group_runner is None:
        from .engine import group_run as group_runner
    outs = group_runner(problems, tol=1.0e-6, max_iters=max_iters, device_id=device_id)
    results = []
    for job, out in zip(jobs, outs):
        errs = np.asarray(out["all_error"], dtype=np.float64)
        error = float(np.mean(errs[-10:])) if job.n_iters is None else float(errs[-1])      # R/main.r:126-130
        rcs, ccs = zip(*[_binary_clusters(f, g, s) for f, g, s in zip(out["f"], out["g"], out["s"])])
        results.append({"output_f": out["f"], "output_s": out["s"], "output_g": out["g"], "Error": error,
                        "All_Error": errs, "bisil": None, "row_clusters": list(rcs), "col_clusters": list(ccs),
                        "lambda": out["lambda"], "mu": out["mu"], "tag": job.tag, "extras": job.extras})
    return results


# ---------------------------------------------------------------------------------------------
# the same job kinds with the data resident on the device: one upload, copies / shuffles drawn there
# ---------------------------------------------------------------------------------------------
def _draw_shuffle(eng, v: int, src, shuffle_seed: int):
    """``shuffle_view`` (``R/obtain_bicl.r:11-22``) of ``src``'s view v into ``eng``'s view v, drawn and re-normalised
    on the device; redrawn while a row or a column of the shuffled matrix sums to zero (``:14-18``)."""
    for attempt in range(64):
        eng.shuffle_view_from(v, src, v, seed=(shuffle_seed + 7919 * attempt) * 1000003 + v)
        er, ec = eng.empty_lines(v)
        if not (er.any() or ec.any()):
            return
    raise RuntimeError("shuffle_view: every draw left an all-zero row or column")


def shuffled_engines(src, k: int, num_repeats: int, seed: int = 0, max_iters: int = 100000, device_id: int = 0) -> list:
    """``obtain_shuffled_f`` (``R/obtain_bicl.r:31-42``) drawn from the views an engine already holds on the device
    (``src``: a ``res_nmtf_inner`` engine or a stability repeat's sub-sample; no second upload): ``num_repeats`` engines,
    every view shuffled from ``src``'s and re-normalised, no restrictions, uncoupled, device SVD init, run to
    convergence -- the draws and seeds of ``shuffles_on_device(dev, k, num_repeats, seed=seed)``: repeat r initialises
    with ``seed + 1000 + r`` and shuffles with ``seed * 7919 + r + 1``.  The engines are returned open, with their
    factors on the device (``Engine.spurious_scores``); the caller closes them."""
    from .engine import Engine
    n_v = src.n_views
    out = []
    try:
        for r in range(num_repeats):
            eng = Engine(src.n_rows, src.n_cols, [k] * n_v, device_id=device_id)
            out.append(eng)
            for v in range(n_v):
                _draw_shuffle(eng, v, src, seed * 7919 + r + 1)
                eng.init_svd(v, seed=seed + 1000 + r + v)
            eng.set_restrictions(None, None, None)          # R/obtain_bicl.r:35-39: apply_resnmtf without phi/xi/psi
            eng.run(n_iters=None, tol=1.0e-6, max_iters=max_iters)
    except BaseException:
        for eng in out:
            eng.close()
        raise
    return out


class DeviceData:
    """The pre-processed views of one data set, uploaded once (``resnmtf_set_view_raw``) and kept for
    any number of factorisations (``resnmtf_copy_view`` / ``resnmtf_shuffle_view``).  At c2 size an
    upload costs ~45 ms of PCIe + conversion, 500 sweeps ~23 ms: re-uploading per job would dominate.

    ``pre_processed=True`` (opt-in) takes the data as ``res_nmtf_inner`` receives them: the views are uploaded exactly
    as given (``resnmtf_set_view``, no shift, no normalisation) and ``phi`` / ``xi`` / ``psi`` are the symmetrised
    matrices, used as they are -- the form ``stability_check`` gets both in (``R/main.r:255-262``; its sub-samples are
    not re-normalised)."""

    def __init__(self, data, phi=None, xi=None, psi=None, row_names=None, col_names=None, device_id: int = 0,
                 pre_processed: bool = False):
        from . import naming, sparse
        from .engine import Engine
        # sparse views (scipy.sparse) stay sparse: a canonical, pre-processed CSC copy on the host, from which the
        # sub-samples are gathered, and a sparse view on the device
        self.sp = [None if not sparse.is_sparse(d) else (sparse.canonical_csc(d) if pre_processed else sparse.check_data_one(d))
                   for d in data]
        if pre_processed:
            for c in self.sp:
                if c is not None:
                    sparse.validate(c)
        data = [d if c is None else c for d, c in zip(data, self.sp)]
        self.data_shapes = [tuple(d.shape) if c is not None else np.asarray(d).shape for d, c in zip(data, self.sp)]
        n_v = len(data)
        self.rn, self.cn = naming.give_names([d if c is not None else np.asarray(d) for d, c in zip(data, self.sp)], phi, psi,
                                             row_names, col_names)
        if pre_processed:
            self.phi, self.xi, self.psi = (np.zeros((n_v, n_v)) if m is None else np.asarray(m, dtype=np.float64)
                                           for m in (phi, xi, psi))
        else:
            self.phi = naming.init_rest_mats(phi, n_v); self.xi = naming.init_rest_mats(xi, n_v); self.psi = naming.init_rest_mats(psi, n_v)
        self.device_id = device_id
        nnz = [None if c is None else c.nnz for c in self.sp] if any(c is not None for c in self.sp) else None
        self.base = Engine([s[0] for s in self.data_shapes], [s[1] for s in self.data_shapes], [2] * n_v, device_id=device_id,
                           nnz=nnz)
        if pre_processed:
            for v in range(n_v):
                if self.sp[v] is not None:
                    self.base.set_view_sparse(v, self.sp[v], pre_processed=True)
                else:
                    self.base.set_view(v, np.asarray(data[v], dtype=np.float64))
            self.was_negative = [False] * n_v
        else:
            self.was_negative = [False if self.sp[v] is not None else self.base.set_view_raw(v, np.asarray(data[v], dtype=np.float64))
                                 for v in range(n_v)]
            for v in range(n_v):
                if self.sp[v] is not None:
                    self.base.set_view_sparse(v, self.sp[v], pre_processed=True)      # (normalised on the host: self.sp)

    def close(self):
        self.base.close()

    def _trim_samples(self, samples, max_rounds: int = 20):
        """``sample_view`` / ``stability_repeat`` (``R/stability_analysis.r:165-190``, ``:233-240``): all-zero rows and
        columns of a sub-sample are dropped -- from every earlier view that shares the draw (equal extent along that
        axis) -- and the sub-samples gathered again, until none is left.  The emptiness test runs on the device
        (``resnmtf_view_empty_lines``), on probes that hold only the data.  Returns the trimmed draws or ``None``."""
        from .engine import Engine
        n_v = len(self.data_shapes)
        rows = [np.asarray(r).copy() for r in samples[0]]; cols = [np.asarray(c).copy() for c in samples[1]]
        for _ in range(max_rounds):
            changed = False
            for i in range(n_v):
                if len(rows[i]) < 2 or len(cols[i]) < 2:
                    return None
                probe = None
                if self.sp[i] is not None:          # sparse view: the sub-sample is gathered on the host
                    from . import sparse
                    _, er, ec = sparse.subsample(self.sp[i], rows[i], cols[i])
                else:
                    probe = Engine([len(rows[i])], [len(cols[i])], [2], device_id=self.device_id)
                if probe is not None:
                    try:
                        probe.subsample_view_from(0, self.base, i, rows[i], cols[i])
                        er, ec = probe.empty_lines(0)
                    finally:
                        probe.close()
                if er.any() or ec.any():
                    changed = True
                    same_r = self.data_shapes[i][0] == self.data_shapes[0][0]
                    same_c = self.data_shapes[i][1] == self.data_shapes[0][1]
                    for p in (range(i + 1) if same_r else [i]):            # :168-174
                        if len(rows[p]) == len(er):
                            rows[p] = rows[p][~er]
                    for p in (range(i + 1) if same_c else [i]):            # :175-181
                        if len(cols[p]) == len(ec):
                            cols[p] = cols[p][~ec]
            if not changed:
                return rows, cols
        return None

    def factorise(self, k: int, n_iters: Optional[int] = None, seed: int = 0, shuffle_seed: Optional[int] = None,
                  max_iters: int = 100000, tag: str = "", samples=None, return_init: bool = False,
                  return_data: bool = False, relevance: bool = False, keep_clusters: bool = False,
                  return_lm: bool = False, spurious_repeats: int = 0, spurious_seed: int = 0) -> dict:
        """One factorisation with k biclusters per view: views copied -- or, with ``shuffle_seed``, shuffled as
        ``obtain_shuffled_f`` does (no restrictions, fresh names; redrawn while a row or a column of the shuffled
        matrix sums to zero, ``R/obtain_bicl.r:14-18``), or, with ``samples = (row_samples, col_samples)``,
        sub-sampled as ``stability_repeat`` does (not re-normalised, names carried over; all-zero rows / columns
        dropped first, ``_trim_samples``) -- on the device, device SVD init, loop, finalise.
        ``return_init`` / ``return_data`` add the initial (F, S, G, lambda, mu) per view and the device's copy of the
        data actually factorised (fp32 precision) to the result: what a reference run needs to start from the same place.
        ``relevance`` (with ``samples``): instead of finalise, score the sub-sample's clusters against the reference
        clusters set on ``self.base`` (``resnmtf_relevance``, ``R/stability_analysis.r:268-276``) -- the result holds
        the n_views x k ``"relevance"`` matrix and no factors; ``keep_clusters`` adds the sub-sample's own binary
        clusters (a test hook: they cost a finalise download).  ``return_lm`` adds ``"lambda"`` / ``"mu"`` per view (the
        keys of a ``res_nmtf_inner`` result, for the k sweep of ``apply_resnmtf``).  ``spurious_repeats`` = R >= 2: the
        scores of ``check_biclusters`` against R shuffles of this factorisation's own device copy
        (``spurious.check_on_device`` with ``spurious_seed``) -- with ``relevance``, the flagged cluster columns are
        removed before the scoring (``resnmtf_relevance_masked``, ``R/stability_analysis.r:254-276``) and the kept
        clusters are the cleaned ones; else the result holds the check as ``"spurious_check"`` (the caller removes)."""
        from . import naming
        from .engine import Engine
        n_v = len(self.data_shapes)
        if samples is not None:
            samples = self._trim_samples(samples)
            if samples is None:
                return {"stability_performed": False, "tag": tag}          # R/stability_analysis.r:223-226
        shapes = self.data_shapes if samples is None else [(len(samples[0][v]), len(samples[1][v])) for v in range(n_v)]
        rn, cn = self.rn, self.cn
        if samples is not None:
            rn = [[self.rn[v][t] for t in samples[0][v]] for v in range(n_v)]
            cn = [[self.cn[v][t] for t in samples[1][v]] for v in range(n_v)]
        shuffled = shuffle_seed is not None
        host_views = [None] * n_v          # sparse views: what is uploaded (the whole view or its sub-sample), gathered on the host
        if any(c is not None for c in self.sp):
            if shuffled:
                raise NotImplementedError("device shuffles of sparse views are not supported")
            from . import sparse
            for v in range(n_v):
                if self.sp[v] is not None:
                    host_views[v] = self.sp[v] if samples is None else sparse.subsample(self.sp[v], samples[0][v], samples[1][v])[0]
        nnz = [None if hv is None else hv.nnz for hv in host_views] if any(hv is not None for hv in host_views) else None
        eng = Engine([s[0] for s in shapes], [s[1] for s in shapes], [k] * n_v, device_id=self.device_id, nnz=nnz)
        try:
            for v in range(n_v):
                if shuffled:
                    _draw_shuffle(eng, v, self.base, shuffle_seed)
                elif host_views[v] is not None:
                    eng.set_view_sparse(v, host_views[v], pre_processed=True)      # (sub-samples are not re-normalised)
                elif samples is not None:
                    eng.subsample_view_from(v, self.base, v, samples[0][v], samples[1][v])
                else:
                    eng.copy_view_from(v, self.base, v)
                eng.init_svd(v, seed=seed + v)
            if shuffled:
                eng.set_restrictions(None, None, None)          # R/obtain_bicl.r:35-39: apply_resnmtf without phi/xi/psi
            else:
                eng.set_restrictions(self.phi, self.xi, self.psi)
                rs, cs = naming.shared_names(rn), naming.shared_names(cn)
                for v in range(n_v):
                    for w in range(n_v):
                        if v != w:
                            eng.set_shared_rows(v, w, *naming.index_pairs(rn[v], rn[w], rs[v].get(w)))
                            eng.set_shared_cols(v, w, *naming.index_pairs(cn[v], cn[w], cs[v].get(w)))
            init_state = [eng.get_factors(v) for v in range(n_v)] if return_init else None
            # (sparse views: the host copy rounded to f32, as the device holds the values)
            data_used = ([host_views[v].toarray().astype(np.float32).astype(np.float64) if host_views[v] is not None
                          else eng.get_view(v) for v in range(n_v)] if return_data else None)
            errs = eng.run(n_iters=n_iters, tol=1.0e-6, max_iters=max_iters)
            check = None
            if spurious_repeats:
                from . import spurious
                check = spurious.check_on_device(eng, spurious_repeats, spurious_seed, max_iters=max_iters,
                                                  device_id=self.device_id)
            if relevance and check is not None:
                flags = spurious.removal_flags(check)
                rel = np.stack([eng.relevance_masked(v, self.base, v, samples[0][v], samples[1][v], flags[v])
                                for v in range(n_v)])
                fin = None
                if keep_clusters:
                    fin = [eng.finalise(v) for v in range(n_v)]
                    cleaned = spurious.apply_removal({"output_s": [f[1] for f in fin], "row_clusters": [f[3] for f in fin],
                                                      "col_clusters": [f[4] for f in fin]}, check)
                    fin = [(None, None, None, rc, cc) for rc, cc in zip(cleaned["row_clusters"], cleaned["col_clusters"])]
            elif relevance:
                rel = np.stack([eng.relevance(v, self.base, v, samples[0][v], samples[1][v]) for v in range(n_v)])
                fin = [eng.finalise(v) for v in range(n_v)] if keep_clusters else None
            else:
                fin = [eng.finalise(v) for v in range(n_v)]
                lms = [eng.get_factors(v)[3:] for v in range(n_v)] if return_lm else None
        finally:
            eng.close()
        error = float(np.mean(errs[-10:])) if n_iters is None else float(errs[-1])           # R/main.r:126-130
        if relevance:
            res = {"stability_performed": True, "relevance": rel, "Error": error, "All_Error": errs, "tag": tag,
                   "extras": {"row_samples": samples[0], "col_samples": samples[1]}}
            if keep_clusters:
                res["row_clusters"] = [f[3] for f in fin]
                res["col_clusters"] = [f[4] for f in fin]
            return res
        res = {"output_f": [f[0] for f in fin], "output_s": [f[1] for f in fin], "output_g": [f[2] for f in fin],
               "row_clusters": [f[3] for f in fin], "col_clusters": [f[4] for f in fin],
               "Error": error, "All_Error": errs, "tag": tag,
               "extras": {} if samples is None else {"row_samples": samples[0], "col_samples": samples[1]},
               "row_names": rn, "col_names": cn}
        if return_init:
            res["init"] = init_state
        if return_lm:
            res["lambda"] = [lm[0] for lm in lms]
            res["mu"] = [lm[1] for lm in lms]
        if return_data:
            res["data"] = data_used
        if check is not None:
            res["spurious_check"] = check
        return res


def k_sweep_on_device(dev: DeviceData, k_min: int = 3, k_max: int = 8, n_iters=None, seed: int = 0, group=None,
                      max_iters: int = 100000, return_lm: bool = False, spurious_repeats: int = 0) -> List[dict]:
    """The factorisations of the k sweep (``R/main.r:279-290``) from one upload; sharded round-robin over
    the ranks of an initialised process group (every rank holds its own ``DeviceData``).  ``spurious_repeats``: each
    k's result carries its ``"spurious_check"`` (``DeviceData.factorise``, spurious seed ``seed + k``)."""
    ks = list(range(k_min, k_max + 1))
    return run_jobs(ks, group=group, runner=lambda k: dev.factorise(k, n_iters, seed + k, max_iters=max_iters, tag=f"k={k}",
                                                                    return_lm=return_lm, spurious_repeats=spurious_repeats,
                                                                    spurious_seed=seed + k))


def shuffles_on_device(dev: DeviceData, n_clusts: int, num_repeats: int = 5, n_iters=None, seed: int = 0, group=None,
                       max_iters: int = 100000) -> List[dict]:
    """``obtain_shuffled_f`` (``R/obtain_bicl.r:31-42``) with the shuffles drawn on the device."""
    reps = list(range(num_repeats))
    return run_jobs(reps, group=group,
                    runner=lambda r: dev.factorise(n_clusts, n_iters, seed + 1000 + r, shuffle_seed=seed * 7919 + r + 1,
                                                   max_iters=max_iters, tag=f"shuffle={r}"))


def stability_on_device(dev: DeviceData, k: int, n_stability: int = 5, sample_rate: float = 0.9, n_iters=None, seed: int = 0,
                        group=None) -> List[dict]:
    """The factorisations of ``stability_check`` (``R/stability_analysis.r:305-323``): the draws follow
    ``subsample_views`` (shared draws for equal extents), the sub-samples are gathered on the device; all-zero rows /
    columns of a sub-sample -- the pre-processed data are non-negative, not positive: ``make_non_neg`` leaves a zero
    at every shifted column's minimum and sparse inputs stay sparse -- are dropped as the reference does
    (``DeviceData._trim_samples``); a repeat whose sampling fails returns ``stability_performed = False``."""
    draws = stability_draws(dev.data_shapes, n_stability, sample_rate, seed)
    return run_jobs(list(range(n_stability)), group=group,
                    runner=lambda r: dev.factorise(k, n_iters, seed + 2000 + r, samples=draws[r], tag=f"stability={r}"))


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
                                  runner: Optional[Callable] = None, spurious_repeats: int = 0) -> dict:
    """The repeats of ``stability_check`` (``R/stability_analysis.r:302-334``) with their scoring on the device:
    ``results``' binary clusters are uploaded once onto ``dev.base`` (``resnmtf_set_reference_clusters``), repeat r
    factorises the sub-sample of ``stability_draws`` (trimmed as ``stability_on_device`` does) up to the end of the loop
    and returns its n_views x k relevance (``resnmtf_relevance``) -- no factor leaves the device.  The repeats are
    sharded round-robin over the ranks of an initialised process group (``run_jobs``; every rank holds its own
    ``DeviceData`` and the same ``results``) and reduced by ``mean_relevance``.  ``runner(r)`` replaces the
    repeat (the CPU tests inject a stand-in; ``dev`` is then not used).  Returns ``{"stability_performed",
    "relevance" (None when not performed), "repeats"}``.  ``spurious_repeats`` = R >= 2: every repeat removes its
    spurious biclusters before it is scored (``R/stability_analysis.r:254-266``), against R shuffles of its own
    sub-sample drawn with the spurious seed ``seed + 2000 + r`` -- the repeat's own factorisation seed, so that repeat r
    equals ``remove_spurious(sub_data, sub_result, R, seed=seed + 2000 + r)``; per repeat only the k-sized flags, scores
    and the null scores cross to the host."""
    if runner is None:
        n_v = len(dev.data_shapes)
        for v in range(n_v):
            dev.base.set_reference_clusters(v, results["row_clusters"][v], results["col_clusters"][v])
        draws = stability_draws(dev.data_shapes, n_stability, sample_rate, seed)

        def runner(r):
            return dev.factorise(k, n_iters, seed + 2000 + r, max_iters=max_iters, samples=draws[r], relevance=True,
                                 keep_clusters=keep_clusters, tag=f"stability={r}", spurious_repeats=spurious_repeats,
                                 spurious_seed=seed + 2000 + r)
    repeats = run_jobs(list(range(n_stability)), group=group, runner=runner)
    rel = mean_relevance(repeats, n_stability)
    return {"stability_performed": rel is not None, "relevance": rel, "repeats": repeats}
