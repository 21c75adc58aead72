"""The Python layer around the engine (no GPU): its shared steps are written once (``resnmtf_amd/problem.py``), and
every path that loads a coupled problem hands the engine the same restriction matrices and the same index pairs."""
import ast
import inspect
import os
import re

import numpy as np
import pytest

from resnmtf_amd import api, batched, problem, sharded, synth
from test_group_host import _coupled_job, _RecordingEngine

PKG = os.path.dirname(os.path.abspath(problem.__file__))


def _sources(skip=("engine.py",)):
    return {name: open(os.path.join(PKG, name)).read() for name in sorted(os.listdir(PKG))
            if name.endswith(".py") and name not in skip}


def _functions_containing(pattern):
    """(file, innermost function) of every source line that matches ``pattern``, docstrings and comments aside."""
    found = set()
    for name, src in _sources().items():
        tree = ast.parse(src)
        docs = set()
        for node in ast.walk(tree):
            if isinstance(node, (ast.FunctionDef, ast.ClassDef, ast.Module)) and ast.get_docstring(node, clean=False) is not None:
                docs.update(range(node.body[0].lineno, node.body[0].end_lineno + 1))
        funcs = [n for n in ast.walk(tree) if isinstance(n, ast.FunctionDef)]
        for no, line in enumerate(src.splitlines(), 1):
            if no in docs or not re.search(pattern, line.split("#")[0]):
                continue
            inside = [f for f in funcs if f.lineno <= no <= f.end_lineno]
            found.add((name, max(inside, key=lambda f: f.lineno).name if inside else "<module>"))
    return found


def test_the_coupling_is_wired_in_one_function():
    assert _functions_containing(r"set_shared_rows\(") == {("problem.py", "couple")}
    assert _functions_containing(r"set_shared_cols\(") == {("problem.py", "couple")}


def test_the_reported_error_is_written_once():
    hits = [(name, no) for name, src in _sources().items() for no, line in enumerate(src.splitlines(), 1) if "[-10:]" in line]
    assert len(hits) == 1 and hits[0][0] == "problem.py", hits


def test_restrictions_are_symmetrised_by_prepare_alone():
    assert _functions_containing(r"(?<!def )init_rest_mats\(") == {("problem.py", "prepare")}


# the function-level imports of a sibling module that remain, each with the cycle it breaks
LAZY_SIBLING_IMPORTS = {
    ("batched.py", "run_job", "api"): "api imports batched at its top (DeviceData, the repeats); run_job calls api.res_nmtf_inner",
    ("spurious.py", "check_biclusters", "batched"): "batched imports spurious at its top (check_on_device, the removal); "
                                                    "check_biclusters runs its shuffles through batched",
}


def test_siblings_are_imported_at_module_top():
    found = set()
    for name in ("api.py", "batched.py", "spurious.py"):
        tree = ast.parse(open(os.path.join(PKG, name)).read())
        for fn in (n for n in ast.walk(tree) if isinstance(n, ast.FunctionDef)):
            for node in ast.walk(fn):
                if isinstance(node, ast.ImportFrom) and node.level > 0:
                    found.update((name, fn.name, node.module or a.name) for a in node.names)
    assert found == set(LAZY_SIBLING_IMPORTS)


def test_factorise_returns_one_kind_of_result():
    params = inspect.signature(batched.DeviceData.factorise).parameters
    assert "relevance" not in params and "keep_clusters" not in params
    assert {"k", "n_iters", "seed", "shuffle_seed", "max_iters", "tag", "samples", "return_init", "return_data", "return_lm",
            "spurious_repeats", "spurious_seed"} <= set(params)
    assert "keep_clusters" in inspect.signature(batched.DeviceData.stability_repeat).parameters


def test_inner_result_keeps_both_key_orders():
    f = s = g = rc = cc = [np.ones((2, 2))]
    errs = np.arange(12.0)
    full = problem.inner_result(f, s, g, errs, None, row_clusters=rc, col_clusters=cc, lam=[1], mu=[2], spurious={}, init=[0],
                                tag="t", extras={})
    assert list(full) == ["output_f", "output_s", "output_g", "Error", "All_Error", "bisil", "row_clusters", "col_clusters",
                          "lambda", "mu", "spurious", "init", "tag", "extras"]
    assert full["Error"] == np.mean(errs[2:]) and full["bisil"] is None
    assert problem.inner_result(f, s, g, errs, 12, row_clusters=rc, col_clusters=cc, lam=[1], mu=[2])["Error"] == 11.0
    dev = problem.inner_result(f, s, g, errs, 3, device_data=True, row_clusters=rc, col_clusters=cc, tag="", extras={},
                               row_names=[["a"]], col_names=[["b"]], init=[0], lam=[1], mu=[2], data=[0], spurious_check={})
    assert list(dev) == ["output_f", "output_s", "output_g", "row_clusters", "col_clusters", "Error", "All_Error", "tag", "extras",
                         "row_names", "col_names", "init", "lambda", "mu", "data", "spurious_check"]
    assert list(problem.inner_result(f, s, g, init=None)) == ["output_f", "output_s", "output_g"]
    with pytest.raises(TypeError):
        problem.inner_result(f, s, g, errs, 3, relevance=1)


class _RecordingChild(_RecordingEngine):
    """The recording engine with what ``DeviceData`` needs on top: raw uploads, device copies, ``with``."""

    def set_view_raw(self, v, x):
        self.views[v] = np.array(x, dtype=np.float64)
        return bool((self.views[v] < 0).any())

    def copy_view_from(self, v, other, v_src=0):
        self.views[v] = other.views[v_src]

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def test_every_path_loads_the_same_coupling(monkeypatch):
    """The three-view job with an NA pair and unsymmetrised restrictions, loaded through ``api.res_nmtf_inner``,
    ``DeviceData.factorise``, ``sharded.make_hip_engine`` and ``prepare_grouped_job``: the same restriction matrices
    and, for every ordered pair of views, the same index pairs."""
    job = _coupled_job(3, n_iters=5)
    n_v = len(job.data)
    for mod in (api, batched, sharded):
        monkeypatch.setattr(mod, "Engine", _RecordingChild)
    loads = {}

    with pytest.warns(UserWarning, match="non-negative"):
        batched.run_job(job)
    loads["api.res_nmtf_inner"] = _RecordingEngine.last

    dev = batched.DeviceData(job.data, job.phi, job.xi, job.psi, job.row_names, job.col_names)
    res = dev.factorise(job.k_val, job.n_iters, job.seed)
    loads["DeviceData.factorise"] = _RecordingEngine.last
    assert loads["DeviceData.factorise"] is not dev.base and res["row_names"] == job.row_names

    with pytest.warns(UserWarning, match="non-negative"):
        p = problem.prepare(job.data, job.phi, job.xi, job.psi, job.row_names, job.col_names, normalise=True, symmetrise=True)
    init = problem.svd_init(p.data, [job.k_val] * n_v, job.seed)
    prob = synth.Problem(p.data, init[0], init[1], init[2], p.phi, p.xi, p.psi, job.k_val, row_names=p.row_names,
                         col_names=p.col_names, extras={"shapes": [d.shape for d in p.data]})
    loads["sharded.make_hip_engine"] = sharded.make_hip_engine(prob, [True] * n_v, 0, stream=1).e

    with pytest.warns(UserWarning, match="non-negative"):
        grouped = batched.prepare_grouped_job(job)

    assert not np.array_equal(job.phi, grouped["phi"]) and grouped["row_pairs"][0][2] == (None, None)
    assert any(grouped["row_pairs"][v][w][0] is not None for v in range(n_v) for w in range(n_v) if v != w)
    for name, eng in loads.items():
        for got, want in zip(eng.rest, (grouped["phi"], grouped["xi"], grouped["psi"])):
            np.testing.assert_array_equal(got, want, err_msg=name)
        assert set(eng.rows) == set(eng.cols) == {(v, w) for v in range(n_v) for w in range(n_v) if v != w}, name
        for loaded, table in ((eng.rows, grouped["row_pairs"]), (eng.cols, grouped["col_pairs"])):
            for (v, w), (iv, iw) in loaded.items():
                wv, ww = table[v][w]
                if wv is None:
                    assert iv is None and iw is None, name
                else:
                    np.testing.assert_array_equal(iv, wv, err_msg=name)
                    np.testing.assert_array_equal(iw, ww, err_msg=name)
