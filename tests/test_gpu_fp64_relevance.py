"""relevance_results of cluster matrices in device memory (resnmtf_fp64_relevance):
engine.fp64_relevance bit for bit stability_ref.relevance_counts (and relevance_sets at the small shapes), at the
parametrisation of the f32 twin (test_gpu_stability.test_relevance_bitwise_equals_restatement) plus k != k_ref; the crafted
empty sides and the self-reference; clusters of every dtype and layout; the reference from the host and from the device;
and the refusals, the lowest entry other than 0 / 1 named."""
import ctypes as C

import numpy as np
import pytest

from resnmtf_amd import _lib, engine
from resnmtf_amd.engine import ResnmtfError
from stability_ref import relevance_counts, relevance_sets

pytestmark = pytest.mark.gpu


def _torch_dev():
    import torch
    return torch, torch.device("cuda", 0)


def _clusters(rng, n, k, p=0.35, empty=()):
    c = (rng.random((n, k)) < p).astype(np.float64)
    for j in empty:
        c[:, j] = 0.0
    return c


# the f32 twin's shapes (k = k_ref), k = 64 at an odd extent, and k != k_ref both ways
@pytest.mark.parametrize("k,kr,n,m,N,M", [(1, 1, 40, 30, 50, 40), (3, 3, 150, 90, 170, 100), (3, 3, 64, 65, 64, 65),
                                          (16, 16, 700, 300, 800, 333), (64, 64, 1000, 200, 1111, 222), (64, 64, 129, 70, 129, 70),
                                          (2, 5, 40, 30, 50, 40), (7, 3, 150, 90, 170, 100), (64, 1, 129, 70, 140, 70),
                                          (1, 64, 65, 63, 70, 64)])
def test_relevance_bitwise_equals_restatement(k, kr, n, m, N, M):
    torch, dev = _torch_dev()
    rng = np.random.default_rng(1000 * k + n + kr)
    rc_ref = _clusters(rng, N, kr, empty=(kr - 1,) if kr > 2 else ())
    cc_ref = _clusters(rng, M, kr)
    refs = {"host": (rc_ref, cc_ref), "device": (torch.as_tensor(rc_ref, device=dev), torch.as_tensor(cc_ref, device=dev)),
            "mixed": (torch.as_tensor(rc_ref, device=dev).float(), np.asfortranarray(cc_ref))}
    for trial in range(3):
        rc = _clusters(rng, n, k, empty=(1,) if k > 2 else ())
        cc = _clusters(rng, m, k)
        rows = rng.choice(N, n, replace=False)
        cols = rng.choice(M, m, replace=False)
        want = relevance_counts(rc, cc, rc_ref[rows], cc_ref[cols])
        assert want.shape == (kr,)
        for name, (tr, tc) in refs.items():
            got = engine.fp64_relevance(torch.as_tensor(rc, device=dev), torch.as_tensor(cc, device=dev), tr, tc, rows, cols)
            assert got.tobytes() == want.tobytes(), (name, got, want)
        if max(k, kr) <= 5 and n * m <= 4000:
            assert np.array_equal(want, relevance_sets(rc, cc, rc_ref[rows], cc_ref[cols]))
    again = engine.fp64_relevance(torch.as_tensor(rc, device=dev), torch.as_tensor(cc, device=dev), *refs["device"], rows, cols)
    assert again.tobytes() == want.tobytes()


@pytest.mark.parametrize("dtype", ["float64", "float32", "float16", "bfloat16"])
def test_clusters_of_every_dtype_strided_and_expanded(dtype):
    torch, dev = _torch_dev()
    rng = np.random.default_rng(5)
    n, m, N, M, k, kr = 150, 90, 170, 100, 4, 3
    rc, cc = _clusters(rng, n, k), _clusters(rng, m, k)
    rc_ref, cc_ref = _clusters(rng, N, kr), _clusters(rng, M, kr)
    rows, cols = rng.choice(N, n, replace=False), rng.choice(M, m, replace=False)
    want = relevance_counts(rc, cc, rc_ref[rows], cc_ref[cols])
    dt = getattr(torch, dtype)

    def forms(a):
        t = torch.as_tensor(a, device=dev).to(dt)
        big = torch.zeros((2 * a.shape[0], 3 * a.shape[1] + 1), dtype=dt, device=dev)
        big[::2, 1::3] = t
        return [t.contiguous(), t.t().contiguous().t(), big[::2, 1::3]]

    for a, b in zip(forms(rc), forms(cc)):
        for tr, tc in zip(forms(rc_ref), forms(cc_ref)):
            got = engine.fp64_relevance(a, b, tr, tc, rows, cols)
            assert got.tobytes() == want.tobytes()
    # one column expanded over k: every cluster of the sub-sample is the same
    col = torch.as_tensor(rc[:, :1], device=dev).to(dt)
    got = engine.fp64_relevance(col.expand(n, k), forms(cc)[0], rc_ref, cc_ref, rows, cols)
    want = relevance_counts(np.repeat(rc[:, :1], k, axis=1), cc, rc_ref[rows], cc_ref[cols])
    assert got.tobytes() == want.tobytes()


def test_crafted_empty_sides_and_self_reference():
    torch, dev = _torch_dev()
    rng = np.random.default_rng(3)
    n, m, k = 96, 80, 4
    rows, cols = np.arange(n), np.arange(m)
    rc, cc = _clusters(rng, n, k), _clusters(rng, m, k)
    rc_ref, cc_ref = _clusters(rng, n, k), _clusters(rng, m, k)
    dev_t = lambda a: torch.as_tensor(a, device=dev)      # noqa: E731
    zero = np.zeros((n, k))
    assert np.array_equal(engine.fp64_relevance(dev_t(zero), dev_t(cc), rc_ref, cc_ref, rows, cols), np.zeros(k))   # m_0 = 0, n_0 != 0
    assert np.array_equal(engine.fp64_relevance(dev_t(zero), dev_t(cc), zero, cc_ref, rows, cols), np.ones(k))      # both empty
    assert np.array_equal(engine.fp64_relevance(dev_t(rc), dev_t(cc), dev_t(zero), cc_ref, rows, cols), np.zeros(k))  # n_0 = 0
    # the reference's members all outside the sub-sample: the GATHERED true_r is empty
    far = np.zeros((n + 5, k)); far[n:] = 1.0
    assert np.array_equal(engine.fp64_relevance(dev_t(rc), dev_t(cc), far, cc_ref, rows, cols), np.zeros(k))
    # reference = the sub-sample itself (identity draws): 1 for a non-empty bicluster
    rc[:, 2] = 0.0
    got = engine.fp64_relevance(dev_t(rc), dev_t(cc), dev_t(rc), dev_t(cc), rows, cols)
    assert got.tobytes() == relevance_counts(rc, cc, rc, cc).tobytes()
    nonempty = (rc.sum(0) > 0) & (cc.sum(0) > 0)
    assert not nonempty.all() and np.array_equal(got, np.where(nonempty, 1.0, 0.0))


def test_an_entry_other_than_0_or_1_is_refused_with_its_position():
    torch, dev = _torch_dev()
    rng = np.random.default_rng(9)
    n, m, k = 70, 50, 3
    rows, cols = np.arange(n), np.arange(m)
    good = {"row_c": _clusters(rng, n, k), "col_c": _clusters(rng, m, k), "true_r": _clusters(rng, n, k), "true_c": _clusters(rng, m, k)}
    order = ["row_c", "col_c", "true_r", "true_c"]
    for which, (r, c, value) in (("row_c", (69, 2, 0.5)), ("col_c", (0, 0, 2.0)), ("true_r", (33, 1, -1.0)), ("true_c", (20, 0, float("nan")))):
        for ref_on_device in (True, False):
            mats = {key: a.copy() for key, a in good.items()}
            mats[which][r, c] = value
            mats[which][min(r + 1, mats[which].shape[0] - 1), k - 1] = 3.0        # a later offender: not the one named
            args = [torch.as_tensor(mats[key], device=dev) if (i < 2 or ref_on_device) else mats[key] for i, key in enumerate(order)]
            name = which if which in ("row_c", "col_c") else (which + "_dev" if ref_on_device else which)
            with pytest.raises(ResnmtfError) as err:
                engine.fp64_relevance(*args, rows, cols)
            first = min([(c, r), (k - 1, min(r + 1, mats[which].shape[0] - 1))])       # column-major order
            assert f"{name} entries must be 0 or 1 (row {first[1]}, column {first[0]})" in str(err.value), str(err.value)
    got = engine.fp64_relevance(*[torch.as_tensor(good[key], device=dev) for key in order], rows, cols)
    assert got.tobytes() == relevance_counts(*[good[key] for key in order]).tobytes()


def _call(n=12, m=9, n_sub=5, m_sub=4, k=3, k_ref=2, rows=None, cols=None, struct_size=None, device_id=0, null=(), patch=None):
    """resnmtf_fp64_relevance through ctypes with sound device clusters and host references; ``patch(job)`` edits the job.
    Returns (code, text, the relevance buffer pre-filled with sentinels)."""
    import torch
    dev = torch.device("cuda", 0)
    lib = _lib.load()
    ns, ms, kk, kr = max(n_sub, 1), max(m_sub, 1), min(max(k, 1), 64), min(max(k_ref, 1), 64)
    rc = torch.ones((kk, ns), dtype=torch.float64, device=dev)        # column-major ns x kk
    cc = torch.ones((kk, ms), dtype=torch.float64, device=dev)
    tr = np.asfortranarray(np.ones((max(n, 1), kr)))
    tc = np.asfortranarray(np.ones((max(m, 1), kr)))
    ri = np.arange(ns, dtype=np.int32) if rows is None else np.asarray(rows, dtype=np.int32)
    ci = np.arange(ms, dtype=np.int32) if cols is None else np.asarray(cols, dtype=np.int32)
    rel = np.full(64, -7.25)
    job = _lib.Fp64RelevanceJob()
    job.struct_size = C.sizeof(job) if struct_size is None else struct_size
    job.n, job.m, job.n_sub, job.m_sub, job.k, job.k_ref = n, m, n_sub, m_sub, k, k_ref
    job.row_c = _lib.DeviceMatrix(rc.data_ptr(), 0, 1, ns)
    job.col_c = _lib.DeviceMatrix(cc.data_ptr(), 0, 1, ms)
    job.true_r, job.true_c = tr.ctypes.data_as(C.POINTER(C.c_double)), tc.ctypes.data_as(C.POINTER(C.c_double))
    job.rows, job.cols = ri.ctypes.data_as(C.POINTER(C.c_int)), ci.ctypes.data_as(C.POINTER(C.c_int))
    job.relevance = rel.ctypes.data_as(C.POINTER(C.c_double))
    for name in null:
        setattr(job, name, None)
    if patch is not None:
        patch(job, rc)
    code = lib.resnmtf_fp64_relevance(device_id, C.byref(job))
    text = (lib.resnmtf_last_error(None) or b"").decode()
    torch.cuda.synchronize()
    return code, text, rel


def test_the_other_refusals_leave_the_result_untouched():
    hostbuf = np.ones((5, 3))

    def two_places(job, rc):
        job.true_r_dev = _lib.DeviceMatrix(rc.data_ptr(), 0, 1, 5)

    def bad_dtype(job, rc):
        job.row_c.dtype = 4

    def bad_stride(job, rc):
        job.col_c.row_stride = -1

    def host_clusters(job, rc):
        job.row_c.ptr = hostbuf.ctypes.data

    def beyond(job, rc):
        job.col_c.col_stride = 1 << 40

    for kw, match in ((dict(struct_size=8), "struct_size mismatch"), (dict(n=0), "view dimensions must be positive"),
                      (dict(n_sub=13), "n_sub must be in [1, n]"), (dict(m_sub=0), "m_sub must be in [1, m]"),
                      (dict(k=0), "k must be in [1, 64]"), (dict(k=65), "k must be in [1, 64]"),
                      (dict(k_ref=65), "k_ref must be in [1, 64]"), (dict(null=("rows",)), "rows / cols are NULL"),
                      (dict(null=("relevance",)), "relevance is NULL"),
                      (dict(null=("true_r",)), "true_r is given in no place"), (dict(patch=two_places), "true_r is given in two places"),
                      (dict(null=("true_c",)), "true_c is given in no place"),
                      (dict(patch=bad_dtype), "row_c: unknown dtype"), (dict(patch=bad_stride), "col_c: strides must be >= 0"),
                      (dict(rows=[0, 1, 12, 3, 4]), "rows[2] = 12 is out of range [0, 12)"),
                      (dict(cols=[1, 0, 1, 2]), "cols[2] = 1 occurs twice"),
                      (dict(patch=host_clusters), "row_c is not device memory of device 0"),
                      (dict(patch=beyond), "col_c reaches beyond its allocation"),
                      (dict(device_id=99), "device_id out of range")):
        code, text, rel = _call(**kw)
        assert code == 1 and match in text, (kw, code, text)
        assert (rel == -7.25).all()
    assert _lib.load().resnmtf_fp64_relevance(0, None) == 1
    code, _, rel = _call()
    assert code == 0 and np.array_equal(rel[:2], np.ones(2)) and (rel[2:] == -7.25).all()       # all-ones clusters: identical biclusters
