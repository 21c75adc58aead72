"""ctypes binding of libresnmtf_hip.so (the C-ABI declared in include/resnmtf_hip.h).

The shared library is built in-tree by ``__graft_entry__.build()`` /
``python -m resnmtf_amd.build``.  There is deliberately no fallback: if the library is
missing, or no gfx950 device is usable, every compute entry point raises.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libresnmtf_hip.so")

OK = 0
ERR_NAMES = {1: "INVALID", 2: "NO_DEVICE", 3: "HIP", 4: "ALLOC", 5: "STATE"}
FACTOR_F, FACTOR_G, FACTOR_S, FACTOR_FBLOCK, FACTOR_FBLOCK_ALL = 0, 1, 2, 3, 4
FACTOR_GBLOCK, FACTOR_GBLOCK_ALL, FACTOR_SBLOCK, FACTOR_SBLOCK_ALL = 5, 6, 7, 8
PHASE_F, PHASE_G, PHASE_S, PHASE_F_ALL, PHASE_LOCAL_SWEEP = 0, 1, 2, 3, 4
PHASE_XTF, PHASE_G_ALL, PHASE_XG, PHASE_S_ALL = 5, 6, 7, 8
PHASE_SLICE_F, PHASE_SLICE_XTF, PHASE_SLICE_G, PHASE_SLICE_XG = 9, 10, 11, 12
FACTOR_U_SEND, FACTOR_U_RECV, FACTOR_FNEW_SEND, FACTOR_FNEW_RECV = 9, 10, 11, 12
FACTOR_T_SEND, FACTOR_T_RECV, FACTOR_GNEW_SEND, FACTOR_GNEW_RECV, FACTOR_F_SLICE, FACTOR_G_SLICE = 13, 14, 15, 16, 17, 18
TIMED_KINDS = ("xg", "xtf", "f_chain", "g_chain", "s_chain", "pack")
DTYPE_F64, DTYPE_F32, DTYPE_F16, DTYPE_BF16 = 0, 1, 2, 3      # RESNMTF_DTYPE_* (resnmtf_set_view_device)
SPARSE_CSC, SPARSE_CSR, SPARSE_COO = 0, 1, 2                   # RESNMTF_SPARSE_* (resnmtf_set_view_sparse_device)
INDEX_I32, INDEX_I64 = 0, 1                                   # RESNMTF_INDEX_*
ABI_VERSION = 2
MAX_K = 64


class ResnmtfError(RuntimeError):
    def __init__(self, code: int, text: str):
        super().__init__(f"resnmtf_hip error {code} ({ERR_NAMES.get(code, '?')}): {text}")
        self.code = code


class Options(C.Structure):
    _fields_ = [
        ("struct_size", C.c_int), ("device_id", C.c_int), ("stream", C.c_void_p),
        ("use_graph", C.c_int), ("check_every", C.c_int), ("target_workgroups", C.c_int),
        ("time_kernels", C.c_int), ("pass_waves", C.c_int), ("pass_splits_xg", C.c_int),
        ("pass_splits_xtf", C.c_int), ("pass_lds_pad_kb", C.c_int), ("update_blocks", C.c_int),
        ("no_pitch_pad", C.c_int), ("kk_mode", C.c_int), ("bf16_split", C.c_int), ("replicate_f", C.c_int),
        ("no_f_chain", C.c_int), ("x_half", C.c_int), ("half_unroll", C.c_int), ("replicate_gs", C.c_int),
        ("wait_mode", C.c_int), ("slice_chains", C.c_int), ("slice_index", C.c_int), ("slice_count", C.c_int),
        ("slice_p2p", C.c_int), ("xcd_order", C.c_int), ("fuse_updates", C.c_int),
    ]


class PassTiming(C.Structure):
    _fields_ = [
        ("xg_ms_total", C.c_double), ("xtf_ms_total", C.c_double),
        ("xg_launches", C.c_longlong), ("xtf_launches", C.c_longlong),
        ("xg_bytes", C.c_double), ("xtf_bytes", C.c_double),
        ("xg_flops", C.c_double), ("xtf_flops", C.c_double),
    ]


class ViewPlan(C.Structure):
    """``resnmtf_view_plan_info`` (include/resnmtf_hip.h): [0] = the X.G pass, [1] = the Xt.F pass."""
    _fields_ = [
        ("struct_size", C.c_int), ("k", C.c_int), ("kp", C.c_int), ("nt", C.c_int), ("image", C.c_int), ("kk_mode", C.c_int),
        ("half_unroll", C.c_int),
        ("wide", C.c_int * 2), ("xcd_order", C.c_int * 2), ("waves", C.c_int * 2), ("unroll", C.c_int * 2),
        ("pingpong", C.c_int * 2), ("nsplit", C.c_int * 2), ("rows_per_split", C.c_int * 2), ("rows", C.c_int * 2),
        ("rows_pad", C.c_int * 2),
        ("short_last", C.c_int * 2), ("ntiles", C.c_int * 2), ("tiles_per_wg", C.c_int * 2), ("aux_splits", C.c_int * 2),
        ("sparse_blocks", C.c_int * 2), ("pitch_pad", C.c_int), ("lds_pad_kb", C.c_int),
        ("prepared", C.c_int), ("f_chain_hoisted", C.c_int), ("f_chain_views", C.c_int), ("f_chain_one_slab", C.c_int),
    ]


class UpdatePlan(C.Structure):
    """``resnmtf_update_plan_info`` (include/resnmtf_hip.h): [0] = the F update, [1] = the G update."""
    _fields_ = [
        ("struct_size", C.c_int), ("prepared", C.c_int), ("k", C.c_int), ("kp", C.c_int), ("threads", C.c_int),
        ("rows_per_group", C.c_int), ("emit", C.c_int), ("mm64", C.c_int), ("packk", C.c_int),
        ("restricted", C.c_int * 2), ("n_couple", C.c_int * 2), ("couple_bucket", C.c_int * 2),
        ("n_identity_maps", C.c_int * 2), ("n_index_maps", C.c_int * 2), ("sigma_is_zero", C.c_int * 2),
        ("nsplit", C.c_int * 2), ("split_bucket", C.c_int * 2), ("rows_per_block", C.c_int * 2), ("nblk", C.c_int * 2),
        ("last_block_rows", C.c_int * 2), ("route", C.c_int * 2), ("s_restricted", C.c_int), ("s_n_couple", C.c_int),
    ]


_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int)
_h = C.c_void_p

GROUP_MAX_VIEWS = 8
GROUP_MAX_K = 32
GROUP_MAX_VIEW_ENTRIES = 1 << 22
FP64_PLAN_INTS = 12        # RESNMTF_FP64_PLAN_INTS
_MV = GROUP_MAX_VIEWS


class GroupJob(C.Structure):
    """``resnmtf_group_job`` (include/resnmtf_hip.h)."""
    _fields_ = [
        ("struct_size", C.c_int), ("n_views", C.c_int), ("k", C.c_int), ("n_iters", C.c_int),
        ("n_rows", C.c_int * _MV), ("n_cols", C.c_int * _MV),
        ("x", _dp * _MV), ("f0", _dp * _MV), ("s0", _dp * _MV), ("g0", _dp * _MV),
        ("lambda0", _dp * _MV), ("mu0", _dp * _MV),
        ("phi", _dp), ("xi", _dp), ("psi", _dp),
        ("row_count", (C.c_int * _MV) * _MV), ("row_idx_v", (_ip * _MV) * _MV), ("row_idx_w", (_ip * _MV) * _MV),
        ("col_count", (C.c_int * _MV) * _MV), ("col_idx_v", (_ip * _MV) * _MV), ("col_idx_w", (_ip * _MV) * _MV),
        ("f_out", _dp * _MV), ("s_out", _dp * _MV), ("g_out", _dp * _MV),
        ("lambda_out", _dp * _MV), ("mu_out", _dp * _MV),
        ("all_error", _dp), ("err_capacity", C.c_int), ("iters_done", _ip),
    ]


FP64_SPARSE_PLAN_INTS = 8  # RESNMTF_FP64_SPARSE_PLAN_INTS


class Fp64SparseView(C.Structure):
    """``resnmtf_fp64_sparse_view`` (include/resnmtf_hip.h): the canonical CSC of one view; all NULL = a dense view."""
    _fields_ = [("col_ptr", C.POINTER(C.c_longlong)), ("row_idx", _ip), ("values", _dp)]


class Fp64Sparse(C.Structure):
    """``resnmtf_fp64_sparse`` (include/resnmtf_hip.h)."""
    _fields_ = [("struct_size", C.c_int), ("view", Fp64SparseView * _MV)]


class DeviceMatrix(C.Structure):
    """``resnmtf_device_matrix`` (include/resnmtf_hip.h): a strided matrix in device memory, strides in elements."""
    _fields_ = [("ptr", C.c_void_p), ("dtype", C.c_int), ("row_stride", C.c_longlong), ("col_stride", C.c_longlong)]


_dm = C.POINTER(DeviceMatrix)


class Fp64Device(C.Structure):
    """``resnmtf_fp64_device`` (include/resnmtf_hip.h): what ``resnmtf_fp64_run_device`` reads from, and writes to, device
    memory -- views and initial factors as ``DeviceMatrix``, results and raw state as device ``double*``."""
    _fields_ = ([("struct_size", C.c_int), ("stream", C.c_void_p)] +
                [(name, DeviceMatrix * _MV) for name in ("x", "f0", "s0", "g0", "lambda0", "mu0")] +
                [(name, C.c_void_p * _MV) for name in ("f_out", "s_out", "g_out", "lambda_out", "mu_out",
                                                      "state_f", "state_s", "state_g", "state_lambda", "state_mu")])


class Fp64SparseDeviceView(C.Structure):
    """``resnmtf_fp64_sparse_device_view`` (include/resnmtf_hip.h): the arrays of one sparse view in device memory, as
    ``resnmtf_set_view_sparse_device`` takes them; all zero = the view comes from elsewhere."""
    _fields_ = [("layout", C.c_int), ("index_type", C.c_int), ("dtype", C.c_int), ("ptr_or_rows", C.c_void_p),
                ("idx_or_cols", C.c_void_p), ("values", C.c_void_p), ("nnz", C.c_longlong)]


class Fp64SparseDevice(C.Structure):
    """``resnmtf_fp64_sparse_device`` (include/resnmtf_hip.h): the sparse views ``resnmtf_fp64_run_sparse_device`` reads
    from device memory."""
    _fields_ = [("struct_size", C.c_int), ("stream", C.c_void_p), ("view", Fp64SparseDeviceView * _MV)]


FP64_BISIL_PLAN_INTS = 5   # RESNMTF_FP64_BISIL_PLAN_INTS


class Fp64BisilJob(C.Structure):
    """``resnmtf_fp64_bisil_job`` (include/resnmtf_hip.h): X in host memory (``x``) or in device memory (``x_dev`` read
    after ``stream``), the host 0 / 1 cluster matrices and the host outputs of ``resnmtf_fp64_bisil``."""
    _fields_ = [("struct_size", C.c_int), ("n", C.c_int), ("m", C.c_int), ("k", C.c_int), ("metric", C.c_int),
                ("x", _dp), ("x_dev", DeviceMatrix), ("stream", C.c_void_p),
                ("row_clusters", _dp), ("col_clusters", _dp), ("row_sil", _dp), ("col_sil", _dp)]


class Fp64BisilSparseJob(C.Structure):
    """``resnmtf_fp64_bisil_sparse_job`` (include/resnmtf_hip.h): the view as host CSC arrays (``x``) or as sparse arrays in
    device memory (``x_dev`` read after ``stream``), the host 0 / 1 cluster matrices and the host outputs of
    ``resnmtf_fp64_bisil_sparse``."""
    _fields_ = [("struct_size", C.c_int), ("n", C.c_int), ("m", C.c_int), ("k", C.c_int), ("metric", C.c_int),
                ("x", Fp64SparseView), ("x_dev", Fp64SparseDeviceView), ("stream", C.c_void_p),
                ("row_clusters", _dp), ("col_clusters", _dp), ("row_sil", _dp), ("col_sil", _dp)]


class Fp64ShuffleJob(C.Structure):
    """``resnmtf_fp64_shuffle_job`` (include/resnmtf_hip.h): X in host memory (``x``) or in device memory (``x_dev``), the
    caller's device array ``out`` (n m doubles, written after ``stream``) and the host outputs of ``resnmtf_fp64_shuffle``."""
    _fields_ = [("struct_size", C.c_int), ("n", C.c_int), ("m", C.c_int), ("normalise", C.c_int), ("seed", C.c_ulonglong),
                ("x", _dp), ("x_dev", DeviceMatrix), ("stream", C.c_void_p), ("out", C.c_void_p),
                ("was_negative", _ip), ("n_empty_rows", _ip), ("n_empty_cols", _ip),
                ("row_mask", C.POINTER(C.c_ubyte)), ("col_mask", C.POINTER(C.c_ubyte))]


class Fp64ShuffleSparseJob(C.Structure):
    """``resnmtf_fp64_shuffle_sparse_job`` (include/resnmtf_hip.h): the view as host CSC arrays (``x``) or as sparse arrays
    in device memory (``x_dev`` read after ``stream``), the caller's three device arrays of the draw's canonical CSC and the
    host outputs of ``resnmtf_fp64_shuffle_sparse``."""
    _fields_ = [("struct_size", C.c_int), ("n", C.c_int), ("m", C.c_int), ("normalise", C.c_int), ("seed", C.c_ulonglong),
                ("x", Fp64SparseView), ("x_dev", Fp64SparseDeviceView), ("stream", C.c_void_p),
                ("out_col_ptr", C.c_void_p), ("out_row_idx", C.c_void_p), ("out_values", C.c_void_p),
                ("n_empty_rows", _ip), ("n_empty_cols", _ip),
                ("row_mask", C.POINTER(C.c_ubyte)), ("col_mask", C.POINTER(C.c_ubyte))]


FP64_SUBSAMPLE_PLAN_INTS = 6   # RESNMTF_FP64_SUBSAMPLE_PLAN_INTS


class Fp64SubsampleJob(C.Structure):
    """``resnmtf_fp64_subsample_job`` (include/resnmtf_hip.h): the host index lists, X in host memory (``x``) or in device
    memory (``x_dev``), the caller's device array ``out`` (n_sub m_sub doubles, written after ``stream``) and the host
    outputs of ``resnmtf_fp64_subsample``."""
    _fields_ = [("struct_size", C.c_int), ("n", C.c_int), ("m", C.c_int), ("n_sub", C.c_int), ("m_sub", C.c_int),
                ("rows", _ip), ("cols", _ip), ("x", _dp), ("x_dev", DeviceMatrix), ("stream", C.c_void_p), ("out", C.c_void_p),
                ("n_empty_rows", _ip), ("n_empty_cols", _ip),
                ("row_mask", C.POINTER(C.c_ubyte)), ("col_mask", C.POINTER(C.c_ubyte))]


class Fp64SubsampleSparseJob(C.Structure):
    """``resnmtf_fp64_subsample_sparse_job`` (include/resnmtf_hip.h): the host index lists, the view as host CSC arrays
    (``x``) or as sparse arrays in device memory (``x_dev`` read after ``stream``), the caller's three device arrays of the
    sub-sample's canonical CSC with their capacity (all NULL and 0: count mode) and the host outputs of
    ``resnmtf_fp64_subsample_sparse``."""
    _fields_ = [("struct_size", C.c_int), ("n", C.c_int), ("m", C.c_int), ("n_sub", C.c_int), ("m_sub", C.c_int),
                ("rows", _ip), ("cols", _ip), ("x", Fp64SparseView), ("x_dev", Fp64SparseDeviceView), ("stream", C.c_void_p),
                ("out_col_ptr", C.c_void_p), ("out_row_idx", C.c_void_p), ("out_values", C.c_void_p),
                ("out_capacity", C.c_longlong), ("nnz_sub", C.POINTER(C.c_longlong)),
                ("n_empty_rows", _ip), ("n_empty_cols", _ip),
                ("row_mask", C.POINTER(C.c_ubyte)), ("col_mask", C.POINTER(C.c_ubyte))]


class Fp64RelevanceJob(C.Structure):
    """``resnmtf_fp64_relevance_job`` (include/resnmtf_hip.h): the sub-sample's cluster matrices in device memory, the
    reference's in host memory (``true_r`` / ``true_c``) or in device memory (``true_r_dev`` / ``true_c_dev``), the host index
    lists and the host result of ``resnmtf_fp64_relevance``."""
    _fields_ = [("struct_size", C.c_int), ("n", C.c_int), ("m", C.c_int), ("n_sub", C.c_int), ("m_sub", C.c_int),
                ("k", C.c_int), ("k_ref", C.c_int), ("row_c", DeviceMatrix), ("col_c", DeviceMatrix),
                ("true_r", _dp), ("true_c", _dp), ("true_r_dev", DeviceMatrix), ("true_c_dev", DeviceMatrix),
                ("rows", _ip), ("cols", _ip), ("stream", C.c_void_p), ("relevance", _dp)]


class Fp64Init(C.Structure):
    """``resnmtf_fp64_init`` (include/resnmtf_hip.h): the seeds, sigma and n_power of ``resnmtf_fp64_init_svd``, the five
    outputs per view (host pointers, or device pointers with ``outputs_on_device``), and the optional host outputs: the k
    leading singular values and the signed basis."""
    _fields_ = ([("struct_size", C.c_int), ("n_power", C.c_int), ("outputs_on_device", C.c_int), ("sigma", C.c_double),
                 ("seed", C.c_ulonglong * _MV)] +
                [(name, C.c_void_p * _MV) for name in ("f0", "s0", "g0", "lambda0", "mu0")] +
                [(name, _dp * _MV) for name in ("singular_values", "basis_u", "basis_v", "basis_d")] +
                [("basis_n_d", _ip * _MV)])


# name -> (restype, argtypes); must list every symbol include/resnmtf_hip.h declares
SIGNATURES = {
    "resnmtf_abi_version": (C.c_int, []),
    "resnmtf_device_count": (C.c_int, []),
    "resnmtf_default_options": (None, [C.POINTER(Options)]),
    "resnmtf_last_error": (C.c_char_p, [_h]),
    "resnmtf_create": (C.c_int, [C.c_int, _ip, _ip, _ip, _ip, C.POINTER(Options), C.POINTER(_h)]),
    "resnmtf_destroy": (C.c_int, [_h]),
    "resnmtf_create_sparse": (C.c_int, [C.c_int, _ip, _ip, _ip, _ip, C.POINTER(C.c_longlong), C.POINTER(Options), C.POINTER(_h)]),
    "resnmtf_set_view_csc": (C.c_int, [_h, C.c_int, C.POINTER(C.c_longlong), _ip, _dp, C.c_int]),
    "resnmtf_view_storage": (C.c_int, [_h, C.c_int, _ip, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]),
    "resnmtf_shuffle_view_sparse": (C.c_int, [_h, C.c_int, _h, C.c_int, C.c_ulonglong, C.c_int]),
    "resnmtf_subsample_count_sparse": (C.c_int, [_h, C.c_int, C.c_int, _ip, C.c_int, _ip, C.POINTER(C.c_longlong)]),
    "resnmtf_subsample_view_sparse": (C.c_int, [_h, C.c_int, _h, C.c_int, _ip, _ip]),
    "resnmtf_copy_view_sparse": (C.c_int, [_h, C.c_int, _h, C.c_int]),
    "resnmtf_get_view_csc": (C.c_int, [_h, C.c_int, C.POINTER(C.c_longlong), _ip, _dp]),
    "resnmtf_set_view": (C.c_int, [_h, C.c_int, _dp]),
    "resnmtf_set_view_raw": (C.c_int, [_h, C.c_int, _dp, _ip]),
    "resnmtf_set_view_device": (C.c_int, [_h, C.c_int, C.c_void_p, C.c_int, C.c_longlong, C.c_longlong, C.c_int, _ip, C.c_void_p]),
    "resnmtf_set_view_sparse_device": (C.c_int, [_h, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_longlong, C.c_int,
                                                 C.c_void_p]),
    "resnmtf_copy_view": (C.c_int, [_h, C.c_int, _h, C.c_int]),
    "resnmtf_shuffle_view": (C.c_int, [_h, C.c_int, _h, C.c_int, C.c_ulonglong, C.c_int]),
    "resnmtf_subsample_view": (C.c_int, [_h, C.c_int, _h, C.c_int, _ip, _ip]),
    "resnmtf_view_empty_lines": (C.c_int, [_h, C.c_int, _ip, _ip, C.POINTER(C.c_ubyte), C.POINTER(C.c_ubyte)]),
    "resnmtf_get_view": (C.c_int, [_h, C.c_int, _dp]),
    "resnmtf_get_view_device": (C.c_int, [_h, C.c_int, C.c_void_p, C.c_int, C.c_longlong, C.c_longlong, C.c_void_p]),
    "resnmtf_get_view_sparse_device": (C.c_int, [_h, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "resnmtf_set_factors": (C.c_int, [_h, C.c_int, _dp, _dp, _dp, _dp, _dp]),
    "resnmtf_set_factors_device": (C.c_int, [_h, C.c_int, _dm, _dm, _dm, _dm, _dm, C.c_void_p]),
    "resnmtf_init_svd": (C.c_int, [_h, C.c_int, C.c_ulonglong, C.c_double, C.c_int, _dp]),
    "resnmtf_init_svd_basis": (C.c_int, [_h, C.c_int, C.c_ulonglong, C.c_double, C.c_int, _dp, _dp, _dp, _dp, _ip]),
    "resnmtf_set_restrictions": (C.c_int, [_h, _dp, _dp, _dp]),
    "resnmtf_set_shared_rows": (C.c_int, [_h, C.c_int, C.c_int, C.c_int, _ip, _ip]),
    "resnmtf_set_shared_cols": (C.c_int, [_h, C.c_int, C.c_int, C.c_int, _ip, _ip]),
    "resnmtf_run": (C.c_int, [_h, C.c_int, C.c_double, C.c_int, _dp, C.c_int, _ip]),
    "resnmtf_get_factors": (C.c_int, [_h, C.c_int, _dp, _dp, _dp, _dp, _dp]),
    "resnmtf_get_factors_device": (C.c_int, [_h, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "resnmtf_finalise": (C.c_int, [_h, C.c_int, _dp, _dp, _dp, _dp, _dp]),
    "resnmtf_finalise_device": (C.c_int, [_h, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "resnmtf_set_reference_clusters": (C.c_int, [_h, C.c_int, C.c_int, _dp, _dp]),
    "resnmtf_set_reference_clusters_device": (C.c_int, [_h, C.c_int, C.c_int, _dm, _dm, C.c_void_p]),
    "resnmtf_relevance": (C.c_int, [_h, C.c_int, _h, C.c_int, _ip, _ip, _dp]),
    "resnmtf_relevance_masked": (C.c_int, [_h, C.c_int, _h, C.c_int, _ip, _ip, C.POINTER(C.c_ubyte), _dp]),
    "resnmtf_jsd_pairs": (C.c_int, [C.c_int, C.c_int, C.c_int, _dp, C.c_int, _ip, _dp]),
    "resnmtf_jsd_stages": (C.c_int, [C.c_int, C.c_int, C.c_int, _dp, C.c_int, _ip, _dp, _dp, _dp, _dp]),
    "resnmtf_spurious_scores": (C.c_int, [_h, C.c_int, C.POINTER(_h), C.c_int, _dp, _dp]),
    "resnmtf_group_run": (C.c_int, [C.c_int, C.c_int, C.POINTER(GroupJob), C.c_double, C.c_int]),
    "resnmtf_fp64_run": (C.c_int, [C.c_int, C.POINTER(GroupJob), C.c_double, C.c_int]),
    "resnmtf_fp64_plan": (C.c_int, [C.c_int, C.c_int, C.c_int, _ip]),
    "resnmtf_fp64_run_sparse": (C.c_int, [C.c_int, C.POINTER(GroupJob), C.POINTER(Fp64Sparse), C.c_double, C.c_int]),
    "resnmtf_fp64_sparse_plan": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_longlong), _ip, _ip]),
    "resnmtf_fp64_run_device": (C.c_int, [C.c_int, C.POINTER(GroupJob), C.POINTER(Fp64Sparse), C.POINTER(Fp64Device), C.c_double,
                                          C.c_int]),
    "resnmtf_fp64_run_sparse_device": (C.c_int, [C.c_int, C.POINTER(GroupJob), C.POINTER(Fp64Sparse), C.POINTER(Fp64Device),
                                                 C.POINTER(Fp64SparseDevice), C.c_double, C.c_int]),
    "resnmtf_fp64_bisil": (C.c_int, [C.c_int, C.POINTER(Fp64BisilJob)]),
    "resnmtf_fp64_bisil_plan": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_longlong, C.c_longlong, _ip]),
    "resnmtf_fp64_bisil_sparse": (C.c_int, [C.c_int, C.POINTER(Fp64BisilSparseJob)]),
    "resnmtf_fp64_shuffle": (C.c_int, [C.c_int, C.POINTER(Fp64ShuffleJob)]),
    "resnmtf_fp64_shuffle_sparse": (C.c_int, [C.c_int, C.POINTER(Fp64ShuffleSparseJob)]),
    "resnmtf_fp64_subsample": (C.c_int, [C.c_int, C.POINTER(Fp64SubsampleJob)]),
    "resnmtf_fp64_subsample_sparse": (C.c_int, [C.c_int, C.POINTER(Fp64SubsampleSparseJob)]),
    "resnmtf_fp64_subsample_plan": (C.c_int, [C.c_longlong, C.c_longlong, _ip]),
    "resnmtf_fp64_relevance": (C.c_int, [C.c_int, C.POINTER(Fp64RelevanceJob)]),
    "resnmtf_fp64_init_svd": (C.c_int, [C.c_int, C.POINTER(GroupJob), C.POINTER(Fp64Sparse), C.POINTER(Fp64Device),
                                        C.POINTER(Fp64SparseDevice), C.POINTER(Fp64Init)]),
    "resnmtf_bisil": (C.c_int, [_h, C.c_int, C.c_int, _dp, _dp, C.c_int, _dp, _dp]),
    "resnmtf_bisil_sparse": (C.c_int, [_h, C.c_int, C.c_int, _dp, _dp, C.c_int, _dp, _dp]),
    "resnmtf_bisil_device": (C.c_int, [_h, C.c_int, C.c_int, _dm, _dm, C.c_int, C.c_void_p, C.c_void_p, _dp, C.c_void_p]),
    "resnmtf_reserve_sweeps":(C.c_int, [_h, C.c_int]),
    "resnmtf_prepare": (C.c_int, [_h]),
    "resnmtf_phase": (C.c_int, [_h, C.c_int, C.c_int, C.c_int]),
    "resnmtf_factor_device_ptr": (C.c_int, [_h, C.c_int, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]),
    "resnmtf_view_errors": (C.c_int, [_h, C.c_int, C.c_int, C.c_int, _dp]),
    "resnmtf_synchronize": (C.c_int, [_h]),
    "resnmtf_pass_timings": (C.c_int, [_h, C.POINTER(PassTiming), C.c_int]),
    "resnmtf_view_image_info": (C.c_int, [_h, C.c_int, _ip, _dp]),
    "resnmtf_view_plan": (C.c_int, [_h, C.c_int, C.POINTER(ViewPlan)]),
    "resnmtf_update_plan": (C.c_int, [_h, C.c_int, C.POINTER(UpdatePlan)]),
    "resnmtf_kernel_timings": (C.c_int, [_h, _dp, C.POINTER(C.c_longlong), C.c_int]),
    "resnmtf_set_stop_tolerance": (C.c_int, [_h, C.c_double]),
    "resnmtf_loop_state": (C.c_int, [_h, _ip, _ip, _ip]),
    "resnmtf_slice_info": (C.c_int, [_h, _ip, _ip]),
    "resnmtf_p2p_export": (C.c_int, [_h, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "resnmtf_p2p_import": (C.c_int, [_h, C.c_int, C.c_void_p, C.c_size_t]),
    "resnmtf_p2p_selftest": (C.c_int, [_h, C.c_int]),
}

_lib = None


def _pin_hip_runtime():
    """One HIP runtime per process.  PyTorch wheels bundle their own ``libamdhip64.so`` (+ HSA runtime); this library is
    linked against the system's.  Whichever is loaded first serves both (same SONAME) -- and if it is the system's,
    a later ``import torch`` finds no device ("No HIP GPUs are available": its own HSA runtime comes up beside a foreign
    HIP).  So when torch is installed but not yet imported, its copy is loaded here first; without torch (an R process
    calling the C-ABI) the system's runtime is used as linked."""
    import importlib.util
    import sys
    if "torch" in sys.modules:
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.submodule_search_locations:
        return
    cand = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
    if os.path.exists(cand):
        try:
            C.CDLL(cand, mode=C.RTLD_GLOBAL)
        except OSError:
            pass


def load() -> C.CDLL:
    """Load the in-tree HIP library; raises ImportError loudly when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    _pin_hip_runtime()
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} not found: build it with `python -m resnmtf_amd.build` "
            "(hipcc --offload-arch=gfx950).  resnmtf_amd has no CPU fallback.")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError if the symbol is missing
        fn.restype = res
        fn.argtypes = args
    if lib.resnmtf_abi_version() != ABI_VERSION:
        raise ImportError("libresnmtf_hip.so ABI version mismatch")
    _lib = lib
    return lib
