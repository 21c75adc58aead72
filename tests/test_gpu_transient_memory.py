"""Transient device memory comes back: every entry point that takes a workspace on the device
for the length of one call -- the uploads, the view-to-view routes, the SVD initialisation, the scoring entries -- leaves
the device's free memory where it found it, after a successful call and after a refused one alike.  One round calls each
of them once; the free memory of the device is read after each of three rounds that follow a warm-up round."""
import numpy as np
import pytest

from resnmtf_amd import engine
from resnmtf_amd._lib import ResnmtfError
from resnmtf_amd.engine import Engine

from subsample_ref import random_csc

pytestmark = pytest.mark.gpu

# Bytes by which the readings of the three rounds may differ.  Measured on e47f27a ("Take dense views from device memory;
# optionally leave results there"), where every free was still written by hand: the three readings were equal.
ALLOWED_DIFFERENCE = 0


def test_free_device_memory_is_the_same_after_every_round():
    import torch
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(5)
    n, m, k = 60, 40, 3
    x = rng.random((n, m)) + 0.05
    x_thin = rng.random((n, 12)) + 0.05
    xs = random_csc(n, m, 0.3, 10)
    rows = rng.permutation(n)[:50].astype(np.int32)
    cols = rng.permutation(m)[:30].astype(np.int32)
    twice = rows.copy(); twice[7] = twice[3]
    rc = np.zeros((n, k)); rc[np.arange(n), np.arange(n) % k] = 1.0          # three biclusters with rows and columns
    cc = np.zeros((m, k)); cc[np.arange(m), np.arange(m) % k] = 1.0
    jsd_cols = rng.random((n, 4))
    jsd_pairs = np.array([[0, 1], [2, 3], [0, 3]], dtype=np.int32)
    t32 = torch.tensor(x, dtype=torch.float32, device=dev)                  # (the only torch allocation: before the rounds)

    def sparse(shape, nnz):
        return Engine([shape[0]], [shape[1]], [k], nnz=[nnz])

    with Engine([n], [m], [k]) as d, Engine([n], [12], [k]) as thin, Engine([n], [m], [10]) as slab, \
            Engine([n], [m], [k]) as d_to, Engine([50], [30], [k]) as d_sub, Engine([n], [m], [k]) as sh1, \
            Engine([n], [m], [k]) as sh2, sparse((n, m), xs.nnz) as s, sparse((n, m), xs.nnz) as s_to, \
            sparse((n, m), xs.nnz - 1) as s_short:
        s.set_view_sparse(0, xs)
        count = s.subsample_count_sparse(0, rows, cols)
        assert count > 1
        with sparse((50, 30), count) as s_sub, sparse((50, 30), count - 1) as s_sub_short:

            def one_round(seed):
                # ---- uploads
                assert d.set_view_raw(0, x) is False
                d.set_view_device(0, t32, raw=True)
                thin.set_view_raw(0, x_thin)
                slab.set_view_raw(0, x)
                s.set_view_sparse(0, xs)
                # ---- view to view, dense and sparse
                d_to.copy_view_from(0, d, 0)
                d_to.shuffle_view_from(0, d, 0, seed=seed)
                d_sub.subsample_view_from(0, d, 0, rows, cols)
                s_to.copy_view_sparse_from(0, s, 0)
                s_to.shuffle_view_sparse_from(0, s, 0, seed=seed)
                assert s.subsample_count_sparse(0, rows, cols) == count
                s_sub.subsample_view_sparse_from(0, s, 0, rows, cols)
                # ---- SVD initialisation: the view's own slabs, the thin route, temporary slabs, a sparse view
                for eng in (d, thin, slab, s, d_sub):
                    eng.init_svd(0, seed=seed)
                assert np.isfinite(d.run(1)).all()
                # ---- scoring
                d.finalise(0)
                d.set_reference_clusters(0, rc, cc)
                assert np.isfinite(d_sub.relevance(0, d, 0, rows, cols)).all()
                d.bisil(0, rc, cc)
                s.bisil_sparse(0, rc, cc)
                assert np.isfinite(engine.jsd_pairs(jsd_cols, jsd_pairs)).all()
                for i, sh in enumerate((sh1, sh2)):
                    sh.shuffle_view_from(0, d, 0, seed=seed + 1 + i)
                    sh.init_svd(0, seed=seed)
                    sh.run(1)
                score, null = d.spurious_scores(0, [sh1, sh2])
                assert np.isfinite(score).all() and np.isfinite(null).all()
                # ---- refusals raised after device work has begun, or right before it
                with pytest.raises(ResnmtfError, match=f"holds {count} stored entries, above the destination's nnz capacity {count - 1}"):
                    s_sub_short.subsample_view_sparse_from(0, s, 0, rows, cols)
                with pytest.raises(ResnmtfError, match="capacity"):
                    s_short.shuffle_view_sparse_from(0, s, 0, seed=seed)
                with pytest.raises(ResnmtfError, match="occurs twice"):
                    s_sub.subsample_view_sparse_from(0, s, 0, twice, cols)

            one_round(1)                                                   # warm-up: graphs, error buffers, plans
            free = []
            for r in range(3):
                one_round(2 + r)
                free.append(torch.cuda.mem_get_info(dev)[0])
            print("free device memory after the three rounds:", free)
            assert max(free) - min(free) <= ALLOWED_DIFFERENCE, free
