"""The launch plan of small handles, one per branch of the host layer's planning, against a recorded table.

``tests/golden/plan_table.json`` holds ``Engine.view_plan(v)`` of every view of every case below, as the library computed
it on an MI355X before the host layer described the F side and the G side of a view once (``struct Side``).  The plan is a
pure function of the shapes, the options and the CU count, so any later change of the host layer has to reproduce it entry
by entry -- or change the table on purpose.  Creating a handle (and ``prepare`` where the chain fields matter) is all a
case does; no sweep runs.

Re-record (on the device, with the build whose plans are to be pinned)::

    python tests/test_gpu_view_plan_table.py --record [--lib path/to/libresnmtf_hip.so]
"""
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
TABLE = os.path.join(ROOT, "tests", "golden", "plan_table.json")


def _case(name, shapes, k, prepare=False, owned=None, couple=False, sparse=False, **opts):
    return dict(name=name, shapes=shapes, k=k, prepare=prepare, owned=owned, couple=couple, sparse=sparse, opts=opts)


# shapes: (n, m) per view; couple: phi / psi = 1 between all views that share their rows / columns (identity maps)
CASES = [
    _case("k5_resident", [(200, 136)], 5, prepare=True),
    _case("k16_streamed_pingpong", [(4160, 136)], 16, target_workgroups=64),
    _case("k16_streamed_both", [(4160, 4100)], 16, target_workgroups=64),
    _case("k32_wide", [(200, 264)], 32),
    _case("k48_wide", [(200, 264)], 48),
    _case("k64_wide", [(200, 264)], 64, prepare=True),
    _case("k64_wide_big", [(2100, 1300)], 64),
    _case("k32_xcd_order", [(2100, 1300)], 32, xcd_order=True),
    _case("k32_f32_mfma", [(200, 264)], 32, bf16_split=2),
    _case("k64_f32_mfma", [(1100, 520)], 64, bf16_split=2),
    _case("k16_mode_b", [(200, 136)], 16, kk_mode=2),
    _case("k32_mode_a", [(200, 264)], 32, kk_mode=1),
    _case("k64_mode_a_big", [(2100, 1300)], 64, kk_mode=1),
    _case("k8_waves4", [(520, 330)], 8, pass_waves=4),
    _case("k8_waves16", [(520, 330)], 8, pass_waves=16),
    _case("k8_splits_forced", [(1500, 700)], 8, pass_splits_xg=3, pass_splits_xtf=5),
    _case("k32_splits_forced", [(1500, 700)], 32, pass_splits_xg=2, pass_splits_xtf=3),
    _case("k8_fp16", [(520, 330)], 8, x_half=1, upload=True),
    _case("k8_u16", [(520, 330)], 8, x_half=2, upload=True),
    _case("k8_u16_unroll6", [(520, 330)], 8, x_half=2, half_unroll=6),
    _case("k8_no_pitch_pad", [(200, 136)], 8, no_pitch_pad=True),
    _case("k8_lds_pad", [(200, 136)], 8, pass_lds_pad_kb=16),
    _case("k8_fused_updates", [(200, 136)], 8, prepare=True, fuse_updates=1),
    _case("k5_sparse_before_upload", [(300, 200)], 5, sparse=True),
    _case("k5_sparse_uploaded", [(300, 200)], 5, sparse=True, upload=True, prepare=True),
    _case("k40_sparse_uploaded", [(300, 200)], 40, sparse=True, upload=True),
    _case("k5_short_rows", [(40, 300)], 5, prepare=True),          # n < 64 < m
    _case("k5_short_cols", [(300, 40)], 5, prepare=True),          # m < 64 < n
    _case("k32_short_rows", [(40, 300)], 32),
    _case("k32_short_cols", [(300, 40)], 32),
    _case("two_views_chain", [(200, 136), (200, 72)], 5, prepare=True, couple=True),
    _case("two_views_chain_split_slabs", [(200, 3000), (200, 2500)], 5, prepare=True, couple=True, pass_splits_xg=3),
    _case("two_views_replicate_f", [(200, 136), (200, 72)], 5, prepare=True, couple=True, replicate_f=True),
    _case("three_views_replicate_f", [(200, 136), (200, 72), (200, 100)], 5, prepare=True, couple=True, replicate_f=True),
    _case("three_views_no_f_chain", [(200, 136), (200, 72), (200, 100)], 5, prepare=True, couple=True, replicate_f=True,
          no_f_chain=True),
    _case("replicate_gs_mixed", [(200, 136), (200, 136), (200, 136)], 5, prepare=True, couple=True, owned=[True, False, True],
          replicate_f=True, replicate_gs=True),
    _case("replicate_gs_mixed_k32", [(200, 136), (200, 136)], 32, prepare=True, couple=True, owned=[False, True],
          replicate_f=True, replicate_gs=True),
    _case("slice_chains_one_rank", [(200, 136)], 5, prepare=True, owned=[True], replicate_f=True, replicate_gs=True, slice_chains=True,
          slice_index=0, slice_count=1),
    _case("slice_chains_one_rank_k64", [(200, 136)], 64, prepare=True, owned=[True], replicate_f=True, replicate_gs=True, slice_chains=True,
          slice_index=0, slice_count=1),
    _case("five_views_chain8", [(200, 136), (200, 72), (200, 100), (200, 64), (200, 90)], 5, prepare=True, couple=True,
          owned=[True, True, False, True, False], replicate_f=True),
    _case("five_views_owned", [(200, 136), (200, 72), (200, 100), (200, 64), (200, 90)], 5, prepare=True, couple=True),
]


def _sparse_view(rng, n, m):
    import scipy.sparse as sp
    x = rng.random((n, m)) * (rng.random((n, m)) < 0.08)
    x[rng.integers(0, n, m), np.arange(m)] += 0.5            # no empty column
    x[7, :] = rng.random(m)                                  # one dense row among sparse ones: a block of its own
    return sp.csc_matrix(x)


def build(case, seed=0):
    """The engine of a case, with data / factors / couplings as far as the case asks for them."""
    from resnmtf_amd.engine import Engine
    rng = np.random.default_rng(seed)
    shapes, k, opts = case["shapes"], case["k"], dict(case["opts"])
    upload = opts.pop("upload", False) or case["prepare"]
    V = len(shapes)
    kw = dict(opts)
    if case["owned"] is not None:
        kw["owned"] = case["owned"]
    if case["sparse"]:
        kw["nnz"] = [n * m for n, m in shapes]
    e = Engine([n for n, _ in shapes], [m for _, m in shapes], [k] * V, **kw)
    owned = case["owned"] or [True] * V
    for v, (n, m) in enumerate(shapes):
        if upload and owned[v]:
            if case["sparse"]:
                e.set_view_sparse(v, _sparse_view(rng, n, m))
            else:
                e.set_view(v, rng.random((n, m)) + 0.01)
        if case["prepare"]:
            e.set_factors(v, rng.random((n, k)) + 0.1, rng.random((k, k)) + 0.1, rng.random((m, k)) + 0.1)
    if case["couple"]:
        w = np.ones((V, V)) - np.eye(V)
        rows_shared = len({n for n, _ in shapes}) == 1
        cols_shared = len({m for _, m in shapes}) == 1
        e.set_restrictions(phi=w if rows_shared else None, xi=0.5 * w, psi=w if cols_shared else None)
        for v in range(V):
            for u in range(V):
                if u == v:
                    continue
                if rows_shared:
                    e.set_shared_rows(v, u, np.arange(shapes[v][0]), np.arange(shapes[v][0]))
                if cols_shared:
                    e.set_shared_cols(v, u, np.arange(shapes[v][1]), np.arange(shapes[v][1]))
    if case["prepare"]:
        e.prepare()
        e.synchronize()
    return e


def plans_of(case):
    with build(case) as e:
        return [e.view_plan(v) for v in range(len(case["shapes"]))]


def _cu_count():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _plain(plans):
    return json.loads(json.dumps(plans))      # tuples -> lists, as the table holds them


@pytest.mark.gpu
def test_gpu_view_plan_table():
    with open(TABLE) as f:
        table = json.load(f)
    if _cu_count() != table["cu_count"]:
        pytest.skip(f"the table was recorded on {table['cu_count']} CUs, this device has {_cu_count()}")
    assert [c["name"] for c in CASES] == list(table["plans"]), "the cases and the recorded table differ: re-record on purpose"
    for case in CASES:
        got = _plain(plans_of(case))
        want = table["plans"][case["name"]]
        for v, (g, w) in enumerate(zip(got, want)):
            diff = {key: (w[key], g[key]) for key in w if g[key] != w[key]}
            assert g == w, f"{case['name']}, view {v}: (recorded, now) {diff}"
        assert len(got) == len(want)
        print(f"[plan table] {case['name']}: {len(got)} view(s) equal")


if __name__ == "__main__":
    if "--record" not in sys.argv:
        sys.exit("usage: python tests/test_gpu_view_plan_table.py --record [--lib path/to/libresnmtf_hip.so]")
    if "--lib" in sys.argv:
        from resnmtf_amd import _lib
        _lib.LIB_PATH = os.path.abspath(sys.argv[sys.argv.index("--lib") + 1])
    out = {"cu_count": _cu_count(), "plans": {c["name"]: _plain(plans_of(c)) for c in CASES}}
    with open(TABLE, "w") as f:
        json.dump(out, f, indent=1, sort_keys=False)
        f.write("\n")
    print(f"recorded {len(CASES)} cases on {out['cu_count']} CUs -> {TABLE}")
