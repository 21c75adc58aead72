// Device-wide fp64 factorisation (DESIGN.md sections 21 to 25): the host side of resnmtf_fp64_run, resnmtf_fp64_run_sparse,
// resnmtf_fp64_run_device, resnmtf_fp64_run_sparse_device and the two plan queries, and their kernels, which come in
// through resnmtf_fp64.hip.inc, resnmtf_fp64_sparse.hip.inc (sparse views), resnmtf_fp64_device.hip.inc (views and factors
// from device memory) and resnmtf_fp64_sparse_device.hip.inc (sparse views from device memory).  A translation unit of its
// own: the kernels get a code object of their own and leave the main unit's device code as it was.
//
// What needs no device -- where each view's data are (F64Source), the layout of the job's one buffer, the CSC check, the
// CSR build and the struct checks -- is resnmtf_fp64_job.h, plain C++.  This file holds what asks the runtime: the pointer
// checks, the launch sequence of a sweep (fp64_enqueue_sweep), the owner of a run's stream and memory (F64Run) and the
// stages fp64_run_impl calls in order, one body for all four entries.  The job checks and the error text are the main
// unit's (resnmtf_internal.h): these entries and resnmtf_group_run refuse the same things with the same texts.
//
// resnmtf_fp64_bisil (section 26), at the end of the file, scores a result in double precision: its kernels are
// resnmtf_fp64_bisil.hip.inc, its index lists, chunk rule and workspace resnmtf_bisil_plan.h (plain C++, shared with the
// main unit's resnmtf_bisil), its owner F64BisilRun.  resnmtf_fp64_bisil_sparse (section 29), right after it, scores a
// sparse view through the same launches (fp64_bisil_enqueue, its gather step a parameter): its one kernel is
// resnmtf_fp64_bisil_sparse.hip.inc, its rank tables and workspace resnmtf_bisil_plan.h.
//
// resnmtf_fp64_shuffle (section 27), after it, draws shuffle_view of a view in double precision: its kernels are
// resnmtf_fp64_shuffle.hip.inc, its permutation resnmtf_feistel.h (plain C++, shared with the main unit's shuffles), its
// struct checks and workspace resnmtf_fp64_shuffle_job.h (plain C++), its owner F64CallRun.
//
// resnmtf_fp64_subsample and resnmtf_fp64_relevance (section 28), after it, are what a stability repeat needs around a
// factorisation in double precision: the sub-sample of a view with its empty lines (resnmtf_fp64_subsample.hip.inc) and
// the relevance of cluster matrices in device memory (resnmtf_fp64_relevance.hip.inc); their struct checks, index-list
// checks, form chooser and workspaces are resnmtf_fp64_subsample_job.h (plain C++).  The three handle-free entries share
// one owner of a call's stream and buffers, F64CallRun, and one header of pointer / extent helpers, resnmtf_fp64_extent.h.
//
// resnmtf_fp64_shuffle_sparse (section 30), last, draws shuffle_view of a view stored sparse: its kernels are
// resnmtf_fp64_shuffle_sparse.hip.inc, its struct checks, extents and workspace resnmtf_fp64_shuffle_sparse_job.h (plain
// C++); the source comes in through the run's own checks (fp64_check_csc / fp64_build_sparse_device_view) and the
// destination is sorted by the same canonicaliser; its owners are F64Transient and F64CallRun.
//
// resnmtf_fp64_subsample_sparse (section 31), last, gathers the sub-sample of a stability repeat from a view stored
// sparse: its kernels are resnmtf_fp64_subsample_sparse.hip.inc, its struct checks, extents, workspace and transient byte
// count resnmtf_fp64_subsample_sparse_job.h (plain C++); the source comes in and the kept entries are sorted as in section
// 30, the lists are checked as in section 28; its owners are F64Transient and F64CallRun.
//
// resnmtf_fp64_init_svd (section 32), last, is init_mats_inner (R/update_steps.r:78-125) for every view of a job in double
// precision: the randomized subspace iteration of the main unit's resnmtf_init_svd on the fp64 values.  Its views come in
// through the run's checks and uploads (fp64_checks with F64Job::start_only, fp64_upload_view), its products, SpMM and
// Gram partials are the run's kernels, its own kernels are resnmtf_fp64_init.hip.inc, its L x L factorisations
// resnmtf_small_linalg.h (plain C++, shared with the main unit); its owners are F64Run, one buffer per view, and F64Block.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "resnmtf_hip.h"
#include "resnmtf_internal.h"
#include "resnmtf_fp64_job.h"
#include "resnmtf_fp64.hip.inc"
#include "resnmtf_fp64_sparse.hip.inc"
#include "resnmtf_fp64_device.hip.inc"
#include "resnmtf_fp64_sparse_device.hip.inc"
#include "resnmtf_bisil_plan.h"
#include "resnmtf_fp64_bisil.hip.inc"
#include "resnmtf_fp64_bisil_sparse.hip.inc"
#include "resnmtf_feistel.h"
#include "resnmtf_fp64_shuffle_job.h"
#include "resnmtf_fp64_shuffle.hip.inc"
#include "resnmtf_fp64_shuffle_sparse_job.h"
#include "resnmtf_fp64_shuffle_sparse.hip.inc"
#include "resnmtf_fp64_subsample_job.h"
#include "resnmtf_fp64_subsample.hip.inc"
#include "resnmtf_fp64_relevance.hip.inc"
#include "resnmtf_fp64_subsample_sparse_job.h"
#include "resnmtf_fp64_subsample_sparse.hip.inc"
#include "resnmtf_small_linalg.h"
#include "resnmtf_fp64_init.hip.inc"

namespace {
// one sweep of update_matrices (R/update_steps.r:272-319, views in index order) and the error of every view; the mean
// error of the sweep lands in the error history at `it`
void fp64_enqueue_sweep(hipStream_t st, const resnmtf_group_job& j, const F64Layout& L, double* buf, int it) {
  const int V = L.V, k = L.k, KP = L.KP;
  const int* ibuf = reinterpret_cast<const int*>(buf);
  double* kkA = buf + L.kk;
  double* kkB = kkA + (size_t)k * k;
  double* kkC = kkB + (size_t)k * k;
  double* kkD = kkC + (size_t)k * k;
  const bool psi_zero = fp64_all_zero(j.psi, V), xi_zero = fp64_all_zero(j.xi, V);
  for (int v = 0; v < V; ++v) {
    const F64View& w = L.vw[v];
    double* F = buf + w.f;
    double* G = buf + w.g;
    F64KKArgs kk{};
    kk.k = k; kk.V = V; kk.v = v;
    kk.kkA = kkA; kk.kkB = kkB; kk.kkC = kkC; kk.kkD = kkD;
    kk.S = buf + L.s; kk.lam = buf + L.lam + (size_t)v * k; kk.mu = buf + L.mu + (size_t)v * k;
    kk.cf = buf + L.cf + (size_t)v * k; kk.cg = buf + L.cg + (size_t)v * k;
    kk.norms = buf + L.norms; kk.errs = buf + L.errs; kk.err_out = buf + L.err + it;
    for (int side = 0; side < 2; ++side) {
      const bool g_form = side == 1;
      const int n = g_form ? w.m : w.n, m = g_form ? w.n : w.m;           // rows of the factor updated / of the other
      double* P = g_form ? G : F;
      const double* O = g_form ? F : G;
      const int gram_blk = (m + F64_GRAM_ROWS - 1) / F64_GRAM_ROWS;
      F64GramArgs ga{};
      ga.A[0] = O; ga.B[0] = O; ga.part[0] = buf + L.part0; ga.len = m; ga.k = k;
      hipLaunchKernelGGL(fp64_gram_kernel, dim3(gram_blk, 1), dim3(F64_THREADS), 0, st, ga);            // O^T O
      kk.mode = g_form ? F64_KK_SIDE_G : F64_KK_SIDE_F;
      kk.part_a = buf + L.part0; kk.nblk_a = gram_blk;
      hipLaunchKernelGGL(fp64_kk_kernel, dim3(1), dim3(F64_THREADS), 0, st, kk);
      if (w.sparse()) {                        // the operand row-major, then the SpMM over the lines of this side
        fp64_spmm(st, KP, g_form ? w.sxtf : w.sxg, reinterpret_cast<const long long*>(buf + (g_form ? w.cptr : w.rptr)),
                  reinterpret_cast<const int*>(buf + (g_form ? w.cidx : w.ridx)), buf + (g_form ? w.cval : w.rval), O, m, k,
                  buf + L.ot, n, g_form ? w.ldm : w.ldn, buf + L.slab);
      } else {
        fp64_product(st, KP, g_form ? w.xtf : w.xg, buf + (g_form ? w.xt : w.x), g_form ? w.ldm : w.ldn, O, m, k,
                     g_form ? w.npad : w.mpad, buf + L.slab);
      }
      F64UpdArgs u{};
      u.n = n; u.k = k; u.KP = KP; u.V = V;
      u.nsplit = w.sparse() ? (g_form ? w.sxtf.splits : w.sxg.splits) : (g_form ? w.xtf.splits : w.xg.splits);
      u.ldx = g_form ? w.ldm : w.ldn;
      u.slab = buf + L.slab; u.P = P; u.xo = buf + L.scratch; u.ps = buf + L.scratch2;
      u.S = buf + L.s + (size_t)v * k * k; u.W = kkB; u.lm = g_form ? kk.mu : kk.lam;
      const double* R = g_form ? j.psi : j.phi;
      u.rsum = fp64_col_sum(R, V, v);
      u.unrestricted = g_form ? (psi_zero ? 1 : 0) : (u.rsum == 0.0 ? 1 : 0);     // :190 / :152
      for (int x = 0; x < V; ++x) {
        u.r[x] = R ? R[x + (size_t)v * V] : 0.0;
        const long long mo = g_form ? L.cmap[v][x] : L.rmap[v][x];
        u.map[x] = mo >= 0 ? ibuf + mo : nullptr;
        u.Pw[x] = buf + (g_form ? L.vw[x].g : L.vw[x].f);
        u.nw[x] = g_form ? L.vw[x].m : L.vw[x].n;
      }
      u.colpart = buf + (g_form ? L.colg : L.colf);
      const int upd_blk = (n + F64_UPD_ROWS - 1) / F64_UPD_ROWS;
      if (g_form) hipLaunchKernelGGL(fp64_update_kernel<true>, dim3(upd_blk), dim3(F64_UPD_ROWS), 0, st, u);
      else hipLaunchKernelGGL(fp64_update_kernel<false>, dim3(upd_blk), dim3(F64_UPD_ROWS), 0, st, u);
    }
    // update_s (:220-240): (F^T X) G from the X^T F the G update kept, and G^T G of the new G; then update_lm
    const int gblk = (w.m + F64_GRAM_ROWS - 1) / F64_GRAM_ROWS;
    F64GramArgs gs{};
    gs.A[0] = buf + L.scratch; gs.B[0] = G; gs.part[0] = buf + L.part0;
    gs.A[1] = G; gs.B[1] = G; gs.part[1] = buf + L.part1;
    gs.len = w.m; gs.k = k;
    hipLaunchKernelGGL(fp64_gram_kernel, dim3(gblk, 2), dim3(F64_THREADS), 0, st, gs);
    if (w.sparse()) {                          // the three k x k matrices of the trace-form error, before update_s reuses kkA
      F64KKSparseArgs ks{};
      ks.k = k; ks.V = V; ks.v = v;
      ks.part_a = buf + L.part0; ks.nblk_a = gblk; ks.part_b = buf + L.part1; ks.nblk_b = gblk;
      ks.kkA = kkA; ks.slot = buf + L.slots + (size_t)v * 3 * k * k;
      fp64_kk_sparse(st, false, ks);
    }
    kk.mode = F64_KK_S;
    kk.part_a = buf + L.part0; kk.nblk_a = gblk; kk.part_b = buf + L.part1; kk.nblk_b = gblk;
    kk.col_f = buf + L.colf; kk.nblk_f = (w.n + F64_UPD_ROWS - 1) / F64_UPD_ROWS;
    kk.col_g = buf + L.colg; kk.nblk_g = (w.m + F64_UPD_ROWS - 1) / F64_UPD_ROWS;
    kk.xi_zero = xi_zero ? 1 : 0;
    kk.xsum = fp64_col_sum(j.xi, V, v);
    for (int x = 0; x < V; ++x) kk.xi[x] = j.xi ? j.xi[x + (size_t)v * V] : 0.0;
    hipLaunchKernelGGL(fp64_kk_kernel, dim3(1), dim3(F64_THREADS), 0, st, kk);
  }
  for (int v = 0; v < V; ++v) {            // calculate_error (R/utils.r:157-166) of every view, after all updates (:316-319)
    const F64View& w = L.vw[v];
    if (w.sparse()) {                          // the trace form, all k x k (section 22): no pass over X
      F64KKSparseArgs ks{};
      ks.k = k; ks.V = V; ks.v = v;
      ks.slot = buf + L.slots + (size_t)v * 3 * k * k; ks.t0 = kkB; ks.t1 = kkC;
      ks.S = buf + L.s + (size_t)v * k * k;
      ks.norms = buf + L.norms; ks.errs = buf + L.errs; ks.err_out = buf + L.err + it;
      fp64_kk_sparse(st, true, ks);
      continue;
    }
    hipLaunchKernelGGL(fp64_fs_kernel, dim3((w.n + F64_UPD_ROWS - 1) / F64_UPD_ROWS), dim3(F64_UPD_ROWS), 0, st,
                       (const double*)(buf + w.f), (const double*)(buf + L.s + (size_t)v * k * k), w.n, k, buf + L.scratch2);
    fp64_resid(st, KP, w.res, buf + w.x, w.ldn, buf + L.scratch2, w.n, buf + w.g, w.m, k, buf + L.spart);
    F64KKArgs kk{};
    kk.mode = F64_KK_ERR; kk.k = k; kk.V = V; kk.v = v;
    kk.part_a = buf + L.spart; kk.nblk_a = w.res.tiles * w.res.splits;
    kk.S = buf + L.s; kk.norms = buf + L.norms; kk.errs = buf + L.errs; kk.err_out = buf + L.err + it;
    hipLaunchKernelGGL(fp64_kk_kernel, dim3(1), dim3(F64_THREADS), 0, st, kk);
  }
}

// ---- what the device routes refuse by asking the runtime, before any allocation or launch ----
inline size_t fp64_dtype_bytes(int dtype) { return dtype == RESNMTF_DTYPE_F64 ? 8 : dtype == RESNMTF_DTYPE_F32 ? 4 : 2; }
// true when [p, p + bytes) is device memory of device_id and inside its allocation; a host pointer makes
// hipPointerGetAttributes fail (or report host memory, by version): both are "no", and the sticky error is cleared
bool fp64_on_device(int device_id, const void* p, size_t bytes, bool& beyond) {
  beyond = false;
  hipPointerAttribute_t attr;
  std::memset(&attr, 0, sizeof(attr));
  if (hipPointerGetAttributes(&attr, p) != hipSuccess) { (void)hipGetLastError(); return false; }
  if (attr.type != hipMemoryTypeDevice || attr.device != device_id) return false;
  hipDeviceptr_t base = nullptr;
  size_t size = 0;
  if (hipMemGetAddressRange(&base, &size, const_cast<void*>(p)) != hipSuccess) { (void)hipGetLastError(); return true; }
  const char* lo = static_cast<const char*>(static_cast<const void*>(base));
  beyond = static_cast<const char*>(p) + bytes > lo + size;
  return !beyond;
}

// the refusals that ask the runtime: every pointer of the struct is device memory of device_id and every matrix stays
// inside its allocation
std::string fp64_check_device_pointers(int device_id, const resnmtf_group_job& j, const resnmtf_fp64_device& d, const F64DeviceUse& use) {
  const int V = j.n_views, k = j.k;
  auto refusal = [&](int v, const char* name, bool beyond) {
    return "view " + std::to_string(v) + ": dev->" + name +
           (beyond ? " reaches beyond its allocation (too short for the shape and strides given)"
                   : " is not device memory of device " + std::to_string(device_id));
  };
  for (int v = 0; v < V; ++v) {
    const size_t n = (size_t)j.n_rows[v], m = (size_t)j.n_cols[v], kk = (size_t)k;
    struct In { const char* name; const resnmtf_device_matrix* a; size_t rows, cols; };
    const In in[6] = {{"x", &d.x[v], n, m}, {"f0", &d.f0[v], n, kk}, {"s0", &d.s0[v], kk, kk}, {"g0", &d.g0[v], m, kk},
                      {"lambda0", &d.lambda0[v], kk, 1}, {"mu0", &d.mu0[v], kk, 1}};
    for (const In& f : in) {
      if (!f.a->ptr) continue;
      const size_t last = (f.rows - 1) * (size_t)f.a->row_stride + (f.cols - 1) * (size_t)f.a->col_stride;
      bool beyond = false;
      if (!fp64_on_device(device_id, f.a->ptr, (last + 1) * fp64_dtype_bytes(f.a->dtype), beyond)) return refusal(v, f.name, beyond);
    }
    for (int f = 0; f < 2 * F64_OUT_SET; ++f) {
      if (!(f < F64_OUT_SET ? use.out : use.state)) continue;
      const F64OutField& o = F64_OUT_FIELDS[f];
      bool beyond = false;
      if (!fp64_on_device(device_id, o.ptr(d, v), o.count(n, m, kk) * sizeof(double), beyond)) return refusal(v, o.name, beyond);
    }
  }
  return "";
}

// the refusals that ask the runtime: every array is device memory of device_id and holds its element count
std::string fp64_check_sparse_device_pointers(int device_id, const resnmtf_group_job& j, const resnmtf_fp64_sparse_device& d, const F64Source* src) {
  for (int v = 0; v < j.n_views; ++v) {
    if (src[v] != F64Source::DeviceSparse) continue;
    const resnmtf_fp64_sparse_device_view& c = d.view[v];
    const bool coo = c.layout == RESNMTF_SPARSE_COO, csc = c.layout == RESNMTF_SPARSE_CSC;
    const size_t ib = c.index_type == RESNMTF_INDEX_I64 ? 8 : 4, nnz = (size_t)c.nnz;
    const size_t lines = (size_t)(csc ? j.n_cols[v] : j.n_rows[v]);
    struct Arr { const char* name; const void* p; size_t count, elem; };
    const Arr arrs[3] = {{"ptr_or_rows", c.ptr_or_rows, coo ? nnz : lines + 1, ib}, {"idx_or_cols", c.idx_or_cols, nnz, ib},
                         {"values", c.values, nnz, fp64_dtype_bytes(c.dtype)}};
    for (const Arr& a : arrs) {
      if (!a.p) continue;                    // (NULL only where nnz = 0 allows it)
      bool beyond = false;
      if (!fp64_on_device(device_id, a.p, a.count * a.elem, beyond))
        return "view " + std::to_string(v) + ": spd->view." + a.name +
               (beyond ? " is shorter than its element count (" + std::to_string(a.count) + " elements of " + std::to_string(a.elem) + " bytes)"
                       : " is not device memory of device " + std::to_string(device_id));
    }
  }
  return "";
}

// The owner of the transient device memory of the sparse device views: free device memory is asked before each
// allocation, a refusal leaves RESNMTF_ERR_ALLOC's text and nullptr; everything still held is freed on the way out.
class F64Transient {
 public:
  explicit F64Transient(const char* name = "fp64_run") : name_(name) {}   // `name` heads its refusals
  F64Transient(const F64Transient&) = delete;
  F64Transient& operator=(const F64Transient&) = delete;
  ~F64Transient() { release_all(); }
  void* take(size_t bytes) {
    bytes = std::max<size_t>(bytes, 8);
    size_t free_b = 0, total_b = 0;
    hipError_t e = hipMemGetInfo(&free_b, &total_b);
    void* p = nullptr;
    if (e == hipSuccess && bytes <= free_b) e = hipMalloc(&p, bytes);
    if (e != hipSuccess || !p) {
      (void)hipGetLastError();
      resnmtf_set_create_error(std::string(name_) + ": " + std::to_string(bytes) + " bytes asked for (the canonical arrays of a sparse view in device memory), " +
                               std::to_string(free_b) + " free on the device");
      return nullptr;
    }
    held_.push_back(p);
    return p;
  }
  template <class T>
  T* take_n(size_t count) { return static_cast<T*>(take(count * sizeof(T))); }
  void release(const void* p) {
    for (void*& q : held_)
      if (q && q == p) { (void)hipFree(q); q = nullptr; }
  }
  void release_all() {
    for (void*& q : held_)
      if (q) { (void)hipFree(q); q = nullptr; }
    held_.clear();
  }
  // (the sort's temporary storage, asked for by the main unit: remembered, so that release_sort_storage() can free it)
  static void* alloc(void* self, size_t bytes) {
    F64Transient* t = static_cast<F64Transient*>(self);
    return t->sort_storage_ = t->take(bytes);
  }
  void release_sort_storage() { release(sort_storage_); sort_storage_ = nullptr; }
 private:
  const char* name_;
  std::vector<void*> held_;
  void* sort_storage_ = nullptr;
};

// what the build of one sparse device view leaves in transient memory until the job's buffer holds it
struct F64SpdView {
  long long *cptr = nullptr, *rptr = nullptr;
  int *cidx = nullptr, *ridx = nullptr;
  const double* cval = nullptr;
  const long long* perm = nullptr;
};

// View v of spd, n x m: checked and sorted on stream st (resnmtf_sparse_device_canonical), its longest row and column
// reduced on the device; `sh` as fp64_check_csc fills it for the same canonical CSC.  Peak transient memory: five 8-byte
// arrays of nnz, two 4-byte ones, the two pointer arrays, 24 bytes of flags and rocPRIM's storage; on return the two
// key arrays, the spare payload array and that storage are free again.  RESNMTF_OK, or the code to return with the
// error text set; `name` heads the texts of runtime failures.
int fp64_build_sparse_device_view(hipStream_t st, F64Transient& tr, int v, const resnmtf_fp64_sparse_device_view& c, int n, int m,
                                  F64SpdView& out, F64SparseShape& sh, const char* name = "fp64_run") {
  resnmtf_sparse_device_build b{};
  b.layout = c.layout; b.index_type = c.index_type; b.dtype = c.dtype; b.n = n; b.m = m; b.nnz = c.nnz;
  b.ptr_or_rows = c.ptr_or_rows; b.idx_or_cols = c.idx_or_cols; b.values = c.values;
  const size_t nnz = (size_t)c.nnz;
  unsigned long long* words = tr.take_n<unsigned long long>(3);        // the two flag words, then the two longest-line ints
  if (!words) return RESNMTF_ERR_ALLOC;
  b.flags = words;
  int* longest = reinterpret_cast<int*>(words + 2);
  if (nnz > 0) {
    for (auto& p : b.key) if (!(p = tr.take_n<unsigned long long>(nnz))) return RESNMTF_ERR_ALLOC;
    for (auto& p : b.pay) if (!(p = tr.take_n<long long>(nnz))) return RESNMTF_ERR_ALLOC;
    if (!(b.cptr = tr.take_n<long long>((size_t)m + 1)) || !(b.rptr = tr.take_n<long long>((size_t)n + 1)) ||
        !(b.cidx = tr.take_n<int>(nnz)) || !(b.ridx = tr.take_n<int>(nnz)))
      return RESNMTF_ERR_ALLOC;
  }
  std::string why;
  const int rc = resnmtf_sparse_device_canonical(st, b, &F64Transient::alloc, &tr, why);
  if (rc == RESNMTF_ERR_INVALID) resnmtf_set_create_error("view " + std::to_string(v) + ": " + why);
  if (rc == RESNMTF_ERR_HIP) resnmtf_set_create_error(std::string(name) + ": view " + std::to_string(v) + ": " + why);
  if (rc != RESNMTF_OK) return rc;
  sh.nnz = nnz; sh.longest_row = sh.longest_col = 0;
  if (nnz == 0) return RESNMTF_OK;           // (zero pointers: the zeros of the job's buffer)
  int host_longest[2] = {0, 0};
  hipError_t e = hipMemsetAsync(longest, 0, 2 * sizeof(int), st);
  if (e == hipSuccess) {
    fp64_spd_longest(st, b.rptr, n, b.cptr, m, longest);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(host_longest, longest, sizeof(host_longest), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) {
    resnmtf_set_create_error(std::string(name) + ": view " + std::to_string(v) + ": " + hipGetErrorString(e));
    return RESNMTF_ERR_HIP;
  }
  sh.longest_row = host_longest[0]; sh.longest_col = host_longest[1];
  out.cptr = b.cptr; out.rptr = b.rptr; out.cidx = b.cidx; out.ridx = b.ridx; out.cval = b.csc_values; out.perm = b.csr_perm;
  for (const void* p : {(const void*)b.key[0], (const void*)b.key[1], (const void*)b.pay[0], (const void*)b.pay[1], (const void*)b.pay[2]})
    if (p != (const void*)out.cval && p != (const void*)out.perm) tr.release(p);
  tr.release_sort_storage();
  return RESNMTF_OK;
}

int fp64_run_impl(int device_id, const resnmtf_group_job* job, const resnmtf_fp64_sparse* sp, const resnmtf_fp64_device* dev,
                  const resnmtf_fp64_sparse_device* spd, double tol, int max_iters);
}  // namespace

extern "C" {

int resnmtf_fp64_sparse_plan(int n_rows, int n_cols, int k, const long long* col_ptr, const int* row_idx, int* out) {
  auto bad = [](const std::string& msg) { resnmtf_set_create_error(msg); return RESNMTF_ERR_INVALID; };
  if (!out) return bad("out is NULL");
  if (n_rows < 1 || n_cols < 1) return bad("view dimensions must be positive");
  if (k < 1 || k > RESNMTF_MAX_K) return bad("k must be in [1, 64]");
  if (k > n_rows || k > n_cols) return bad("k exceeds a view dimension (R/utils.r:444,449)");
  F64SparseShape sh;
  const std::string why = fp64_check_csc(n_rows, n_cols, col_ptr, row_idx, nullptr, sh);
  if (!why.empty()) return bad(why);
  const int KP = f64_kp(k);
  const F64SparsePlan xg = f64_plan_sparse(sh.longest_row), xtf = f64_plan_sparse(sh.longest_col);
  const int vals[RESNMTF_FP64_SPARSE_PLAN_INTS] = {KP, xg.splits, (int)xg.piece, (int)xg.longest, xtf.splits, (int)xtf.piece,
                                                   (int)xtf.longest, 64 / f64_sp_group(KP)};
  std::memcpy(out, vals, sizeof(vals));
  return RESNMTF_OK;
}

int resnmtf_fp64_run(int device_id, const resnmtf_group_job* job, double tol, int max_iters) {
  return fp64_run_impl(device_id, job, nullptr, nullptr, nullptr, tol, max_iters);
}

int resnmtf_fp64_run_sparse(int device_id, const resnmtf_group_job* job, const resnmtf_fp64_sparse* sp, double tol,
                            int max_iters) {
  return fp64_run_impl(device_id, job, sp, nullptr, nullptr, tol, max_iters);
}

int resnmtf_fp64_run_device(int device_id, const resnmtf_group_job* job, const resnmtf_fp64_sparse* sp,
                            const resnmtf_fp64_device* dev, double tol, int max_iters) {
  return fp64_run_impl(device_id, job, sp, dev, nullptr, tol, max_iters);
}

// res_nmtf_inner (R/main.r:32-140) with sparse views that are already in device memory (R/utils.r:416-419 densifies a sparse
// Matrix; these arrays stand for that matrix): resnmtf_fp64_run_device's body, the views of spd checked and sorted on the
// device first
int resnmtf_fp64_run_sparse_device(int device_id, const resnmtf_group_job* job, const resnmtf_fp64_sparse* sp,
                                   const resnmtf_fp64_device* dev, const resnmtf_fp64_sparse_device* spd, double tol, int max_iters) {
  return fp64_run_impl(device_id, job, sp, dev, spd, tol, max_iters);
}

int resnmtf_fp64_plan(int n_rows, int n_cols, int k, int* out) {
  auto bad = [](const std::string& msg) { resnmtf_set_create_error(msg); return RESNMTF_ERR_INVALID; };
  if (!out) return bad("out is NULL");
  if (n_rows < 1 || n_cols < 1) return bad("view dimensions must be positive");
  if (k < 1 || k > RESNMTF_MAX_K) return bad("k must be in [1, 64]");
  if (k > n_rows || k > n_cols) return bad("k exceeds a view dimension (R/utils.r:444,449)");
  const F64ProductPlan xg = f64_plan_product(n_rows, n_cols), xtf = f64_plan_product(n_cols, n_rows);
  const F64ProductPlan res = f64_plan_resid(n_rows, n_cols);
  const int vals[RESNMTF_FP64_PLAN_INTS] = {f64_kp(k), xg.tiles, xg.splits, xg.chunk, xtf.tiles, xtf.splits, xtf.chunk,
                                            res.tiles, res.splits, res.chunk, (int)f64_ld(n_rows), (int)f64_ld(n_cols)};
  std::memcpy(out, vals, sizeof(vals));
  return RESNMTF_OK;
}

}  // extern "C"

namespace {
// resnmtf_fp64_run (sp == nullptr), resnmtf_fp64_run_sparse (dev == nullptr), resnmtf_fp64_run_device (spd == nullptr) and
// resnmtf_fp64_run_sparse_device: one body.  Without a sparse view every step below is resnmtf_fp64_run's own -- the same
// layout, the same launches, the same bits --, without dev every step is resnmtf_fp64_run_sparse's, and without spd every
// step is resnmtf_fp64_run_device's.  The body is a sequence of stages over the job as the caller described it (F64Job)
// and what the run owns on the device (F64Run).

// the job of one call: the caller's structs, each view's source resolved once, and what the checks and the layout derive
struct F64Job {
  int device_id;
  const resnmtf_group_job& j;
  const resnmtf_fp64_sparse* sp;
  const resnmtf_fp64_device* dev;
  const resnmtf_fp64_sparse_device* spd;
  double tol;
  int max_iters;
  F64Source src[RESNMTF_GROUP_MAX_VIEWS];
  F64DeviceUse use;                         // the factors and the outputs in device memory (resnmtf_fp64_run_device)
  F64SparseShape shapes[RESNMTF_GROUP_MAX_VIEWS];
  F64Layout L;
  bool start_only = false;                  // resnmtf_fp64_init_svd: the views alone; the job holds no factors and no run outputs
  bool any(F64Source s) const { return std::find(src, src + RESNMTF_GROUP_MAX_VIEWS, s) != src + RESNMTF_GROUP_MAX_VIEWS; }
};

int fp64_bad(const std::string& msg) { resnmtf_set_create_error(msg); return RESNMTF_ERR_INVALID; }

// What a run holds on the device: its stream, the job's buffer and the transient arrays of the sparse device views.  On
// every way out the destructor waits for the stream and destroys it, then frees the buffer, then the transient arrays.
class F64Run {
 public:
  F64Run() = default;
  F64Run(const F64Run&) = delete;
  F64Run& operator=(const F64Run&) = delete;
  ~F64Run() {
    if (st) { (void)hipStreamSynchronize(st); (void)hipStreamDestroy(st); }
    if (buf) (void)hipFree(buf);
  }
  // a failed runtime call: its text, RESNMTF_ERR_HIP; the destructor does the rest
  int fail(hipError_t e, const char* what = "fp64_run: ") {
    resnmtf_set_create_error(std::string(what) + hipGetErrorString(e));
    return RESNMTF_ERR_HIP;
  }
  double* at(size_t off) { return host.data() + (off - host_begin); }     // `off` of the buffer, in the host copy

  hipStream_t st = nullptr;
  double* buf = nullptr;
  F64SpdView spdv[RESNMTF_GROUP_MAX_VIEWS];  // the sparse device views, in transient memory until the buffer holds them
  std::vector<double> host;                 // the host copy of [out_begin, out_end): the initial state in, the results out
  size_t host_begin = 0;
  int it = 0;                               // sweeps done
  F64Transient transient;
};

// the run's stream waits for what the caller's stream holds so far
hipError_t wait_for_caller(hipStream_t st, void* caller_stream) {
  hipEvent_t ev = nullptr;
  hipError_t e = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
  if (e != hipSuccess) return e;
  e = hipEventRecord(ev, static_cast<hipStream_t>(caller_stream));
  if (e == hipSuccess) e = hipStreamWaitEvent(st, ev, 0);
  (void)hipEventDestroy(ev);                // (released once the recorded work completes)
  return e;
}

// everything that is refused before the device is touched, in the order the header documents, and the device chosen
int fp64_checks(F64Job& J) {
  const resnmtf_group_job& j = J.j;
  fp64_resolve_sources(J.sp, J.dev, J.spd, J.src);
  // a shape no device holds is refused on its byte count before the data behind it is read
  if (fp64_shapes_ok(j)) {
    const long double img = fp64_image_bytes(j, J.src);
    if (img >= 0x1p58L) {
      char text[160];
      std::snprintf(text, sizeof(text), "fp64_run: more than %.0Lf bytes asked for (the fp64 images of the views alone)", img);
      resnmtf_set_create_error(text);
      return RESNMTF_ERR_ALLOC;
    }
  }
  if (J.spd) {                              // (first: a view in two places or in none is named with all four of them)
    const std::string why = fp64_check_sparse_device_struct(j, J.sp, J.dev, *J.spd);
    if (!why.empty()) return fp64_bad(why);
  }
  if (J.dev) {
    const std::string why = fp64_check_device_struct(j, *J.dev, J.src, J.use);
    if (!why.empty()) return fp64_bad(why);
  }
  if (const char* why = resnmtf_check_fp64_job(j, J.max_iters, fp64_x_elsewhere(J.src), J.start_only ? ~0u : J.use.factors,
                                               J.start_only || J.use.out))
    return fp64_bad(why);
  for (int v = j.n_views; v < RESNMTF_GROUP_MAX_VIEWS; ++v)
    if (J.src[v] == F64Source::HostCsc) return fp64_bad("a sparse view is given beyond n_views");
  if (J.dev) {
    const std::string why = fp64_check_device_pointers(J.device_id, j, *J.dev, J.use);
    if (!why.empty()) return fp64_bad(why);
  }
  if (J.any(F64Source::DeviceSparse)) {
    const std::string why = fp64_check_sparse_device_pointers(J.device_id, j, *J.spd, J.src);
    if (!why.empty()) return fp64_bad(why);
  }
  for (int v = 0; v < j.n_views; ++v) {
    if (J.src[v] != F64Source::HostCsc) continue;
    const resnmtf_fp64_sparse_view& c = J.sp->view[v];
    if (!c.values) return fp64_bad("view " + std::to_string(v) + ": values is NULL");
    const std::string why = fp64_check_csc(j.n_rows[v], j.n_cols[v], c.col_ptr, c.row_idx, c.values, J.shapes[v]);
    if (!why.empty()) return fp64_bad("view " + std::to_string(v) + ": " + why);
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) { resnmtf_set_create_error("no HIP device"); return RESNMTF_ERR_NO_DEVICE; }
  if (J.device_id < 0 || J.device_id >= ndev) return fp64_bad("device_id out of range");
  const hipError_t e = hipSetDevice(J.device_id);
  if (e != hipSuccess) { resnmtf_set_create_error(std::string("hipSetDevice: ") + hipGetErrorString(e)); return RESNMTF_ERR_HIP; }
  return RESNMTF_OK;
}

// the run's own stream, ordered after the caller's work where the caller has a stream (dev and spd name the same one)
int fp64_open_stream(const F64Job& J, F64Run& run) {
  hipError_t e = hipStreamCreateWithFlags(&run.st, hipStreamNonBlocking);
  if (e != hipSuccess) { run.st = nullptr; return run.fail(e, "hipStreamCreate: "); }
  if (J.dev || J.spd) e = wait_for_caller(run.st, J.spd ? J.spd->stream : J.dev->stream);
  return e == hipSuccess ? RESNMTF_OK : run.fail(e);
}

// the sparse views in device memory (section 24): the layout needs their longest lines, so their canonical arrays are
// built first, in transient memory, on the run's own stream, and copied into the job's buffer once that exists
int fp64_build_sparse_device_views(F64Job& J, F64Run& run) {
  int rc = RESNMTF_OK;
  for (int v = 0; v < J.j.n_views && rc == RESNMTF_OK; ++v)
    if (J.src[v] == F64Source::DeviceSparse)
      rc = fp64_build_sparse_device_view(run.st, run.transient, v, J.spd->view[v], J.j.n_rows[v], J.j.n_cols[v], run.spdv[v], J.shapes[v]);
  return rc;
}

// the layout, then the job's one buffer if the device has room for it, zero-filled
int fp64_allocate(F64Job& J, F64Run& run) {
  const resnmtf_group_job& j = J.j;
  fp64_layout(j, j.n_iters > 0 ? std::min(j.n_iters, J.max_iters) : J.max_iters, J.L, J.src, J.shapes);
  const size_t bytes = J.L.total * sizeof(double);
  size_t free_b = 0, total_b = 0;
  hipError_t e = hipMemGetInfo(&free_b, &total_b);
  if (e != hipSuccess) return run.fail(e);
  if (bytes > free_b) {
    resnmtf_set_create_error("fp64_run: " + std::to_string(bytes) + " bytes asked for (two fp64 images of every view, factors, slabs), " +
                     std::to_string(free_b) + " free on the device");
    return RESNMTF_ERR_ALLOC;
  }
  void* p = nullptr;
  e = hipMalloc(&p, std::max<size_t>(bytes, 8));
  if (e != hipSuccess) {
    resnmtf_set_create_error(std::string("fp64_run: ") + hipGetErrorString(e) + " (" + std::to_string(bytes) + " bytes asked for)");
    return e == hipErrorOutOfMemory ? RESNMTF_ERR_ALLOC : RESNMTF_ERR_HIP;
  }
  run.buf = static_cast<double*>(p);
  e = hipMemsetAsync(run.buf, 0, bytes, run.st);
  if (e == hipSuccess) e = hipStreamSynchronize(run.st);
  return e == hipSuccess ? RESNMTF_OK : run.fail(e);
}

// where the CSC and the CSR copy of a sparse view lie in a device buffer, in doubles from its start (section 22's storage)
struct F64SparseAt { size_t cptr, cval, cidx, rptr, rval, ridx; };

// a checked host CSC (n x m, nnz entries) into `buf`: the CSC arrays as given, and the CSR copy built here; blocking copies
hipError_t fp64_upload_host_csc(double* buf, const F64SparseAt& at, int n, int m, size_t nnz, const resnmtf_fp64_sparse_view& c) {
  std::vector<long long> rp;
  std::vector<int> ci;
  std::vector<double> rv;
  fp64_csr_from_csc(n, m, c.col_ptr, c.row_idx, c.values, rp, ci, rv);
  hipError_t e = hipMemcpy(buf + at.cptr, c.col_ptr, ((size_t)m + 1) * sizeof(long long), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(buf + at.rptr, rp.data(), rp.size() * sizeof(long long), hipMemcpyHostToDevice);
  if (nnz > 0) {
    if (e == hipSuccess) e = hipMemcpy(buf + at.cval, c.values, nnz * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(buf + at.cidx, c.row_idx, nnz * sizeof(int), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(buf + at.rval, rv.data(), nnz * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(buf + at.ridx, ci.data(), nnz * sizeof(int), hipMemcpyHostToDevice);
  }
  return e;
}

// the canonical arrays of a sparse device view (section 24; nnz >= 1) into `buf`, device to device on `st`, the CSR values
// gathered in fp64
hipError_t fp64_copy_spd_view(hipStream_t st, double* buf, const F64SparseAt& at, int n, int m, size_t nnz, const F64SpdView& c) {
  hipError_t e = hipMemcpyAsync(buf + at.cptr, c.cptr, ((size_t)m + 1) * sizeof(long long), hipMemcpyDeviceToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(buf + at.rptr, c.rptr, ((size_t)n + 1) * sizeof(long long), hipMemcpyDeviceToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(buf + at.cval, c.cval, nnz * sizeof(double), hipMemcpyDeviceToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(buf + at.cidx, c.cidx, nnz * sizeof(int), hipMemcpyDeviceToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(buf + at.ridx, c.ridx, nnz * sizeof(int), hipMemcpyDeviceToDevice, st);
  if (e == hipSuccess) {
    fp64_spd_gather(st, c.perm, c.cval, (long long)nnz, buf + at.rval);
    e = hipGetLastError();
  }
  return e;
}

// view v into the buffer, by where it comes from (`img`: the staging vector of the host dense views)
hipError_t fp64_upload_view(const F64Job& J, F64Run& run, int v, std::vector<double>& img) {
  const F64View& w = J.L.vw[v];
  double* buf = run.buf;
  hipStream_t st = run.st;
  hipError_t e = hipSuccess;
  const F64SparseAt at{w.cptr, w.cval, w.cidx, w.rptr, w.rval, w.ridx};
  switch (w.src) {
    case F64Source::DeviceSparse:           // from device memory (section 24); nnz = 0: the zeros of the memset are the view
      return w.nnz == 0 ? e : fp64_copy_spd_view(st, buf, at, w.n, w.m, w.nnz, run.spdv[v]);
    case F64Source::HostCsc:                // the CSC arrays as given, and the CSR copy built here
      return fp64_upload_host_csc(buf, at, w.n, w.m, w.nnz, J.sp->view[v]);
    case F64Source::DeviceDense:            // from device memory: one read, both images, no staging (section 23)
      fp64_images(st, J.dev->x[v], w.n, w.m, buf + w.x, w.ldn, buf + w.xt, w.ldm);
      return hipGetLastError();
    case F64Source::HostDense: {            // the two padded images through the staging vector
      const double* x = J.j.x[v];
      const size_t n = (size_t)w.n, m = (size_t)w.m;
      img.assign(w.ldn * w.mpad, 0.0);
      for (size_t c = 0; c < m; ++c) std::memcpy(&img[c * w.ldn], x + c * n, n * sizeof(double));
      e = hipMemcpy(buf + w.x, img.data(), img.size() * sizeof(double), hipMemcpyHostToDevice);
      if (e != hipSuccess) return e;
      img.assign(w.ldm * w.npad, 0.0);
      for (size_t c = 0; c < m; ++c)
        for (size_t i = 0; i < n; ++i) img[c + i * w.ldm] = x[i + c * n];
      return hipMemcpy(buf + w.xt, img.data(), img.size() * sizeof(double), hipMemcpyHostToDevice);
    }
  }
  return e;
}

// the views in index order; once the buffer holds the sparse device views, their transient arrays go
int fp64_upload_views(const F64Job& J, F64Run& run) {
  std::vector<double> img;
  hipError_t e = hipSuccess;
  for (int v = 0; v < J.L.V && e == hipSuccess; ++v) e = fp64_upload_view(J, run, v, img);
  if (e == hipSuccess && J.any(F64Source::DeviceSparse)) {
    e = hipStreamSynchronize(run.st);
    run.transient.release_all();
  }
  return e == hipSuccess ? RESNMTF_OK : run.fail(e);
}

// F, G, S, lambda and mu of every view: from the job through the host copy, or from device memory by kernels on the stream
int fp64_upload_state(const F64Job& J, F64Run& run) {
  const resnmtf_group_job& j = J.j;
  const F64Layout& L = J.L;
  const int V = L.V, k = L.k;
  double* buf = run.buf;
  hipError_t e = hipSuccess;
  run.host.assign(L.out_end - L.out_begin, 0.0);
  run.host_begin = L.out_begin;
  for (int v = 0; v < V; ++v) {
    if ((J.use.factors >> v) & 1u) continue;  // (from device memory, below)
    const size_t n = (size_t)L.vw[v].n, m = (size_t)L.vw[v].m;
    std::memcpy(run.at(L.vw[v].f), j.f0[v], n * k * sizeof(double));
    std::memcpy(run.at(L.vw[v].g), j.g0[v], m * k * sizeof(double));
    std::memcpy(run.at(L.s + (size_t)v * k * k), j.s0[v], (size_t)k * k * sizeof(double));
    for (int c = 0; c < k; ++c) {                                         // explicit init: colSums (R/update_steps.r:55-56)
      double cf = 0.0, cg = 0.0;
      if (!j.lambda0[v]) for (size_t i = 0; i < n; ++i) cf += j.f0[v][i + (size_t)c * n];
      if (!j.mu0[v]) for (size_t i = 0; i < m; ++i) cg += j.g0[v][i + (size_t)c * m];
      *run.at(L.lam + (size_t)v * k + c) = j.lambda0[v] ? j.lambda0[v][c] : cf;
      *run.at(L.mu + (size_t)v * k + c) = j.mu0[v] ? j.mu0[v][c] : cg;
    }
  }
  if (!J.use.factors) {
    e = hipMemcpy(buf + L.out_begin, run.host.data(), run.host.size() * sizeof(double), hipMemcpyHostToDevice);
    return e == hipSuccess ? RESNMTF_OK : run.fail(e);
  }
  for (int v = 0; v < V && e == hipSuccess; ++v) {                         // the host views' pieces alone
    if ((J.use.factors >> v) & 1u) continue;
    const size_t fg = ((size_t)L.vw[v].n + L.vw[v].m) * k;                 // F and G of a view are neighbours
    const size_t pieces[4][2] = {{L.vw[v].f, fg}, {L.s + (size_t)v * k * k, (size_t)k * k}, {L.lam + (size_t)v * k, (size_t)k},
                                 {L.mu + (size_t)v * k, (size_t)k}};
    for (int p = 0; p < 4 && e == hipSuccess; ++p)
      e = hipMemcpy(buf + pieces[p][0], run.at(pieces[p][0]), pieces[p][1] * sizeof(double), hipMemcpyHostToDevice);
  }
  for (int v = 0; v < V && e == hipSuccess; ++v) {                         // the others are written by kernels on the stream
    if (!((J.use.factors >> v) & 1u)) continue;
    const F64View& w = L.vw[v];
    const resnmtf_fp64_device& d = *J.dev;
    double* lam = buf + L.lam + (size_t)v * k;
    double* mu = buf + L.mu + (size_t)v * k;
    fp64_factors_in(run.st, d.f0[v], w.n, k, buf + w.f);
    fp64_factors_in(run.st, d.s0[v], k, k, buf + L.s + (size_t)v * k * k);
    fp64_factors_in(run.st, d.g0[v], w.m, k, buf + w.g);
    for (int side = 0; side < 2; ++side) {                                 // given: a k x 1 matrix (col_stride is not read)
      resnmtf_device_matrix vec = side ? d.mu0[v] : d.lambda0[v];
      vec.col_stride = vec.row_stride;
      if (vec.ptr) fp64_factors_in(run.st, vec, k, 1, side ? mu : lam);
    }
    if (!d.lambda0[v].ptr || !d.mu0[v].ptr)                                // not given: colSums (R/update_steps.r:55-56)
      hipLaunchKernelGGL(fp64_colsum_seq_kernel, dim3(2), dim3(64), 0, run.st, (const double*)(buf + w.f), w.n,
                         d.lambda0[v].ptr ? nullptr : lam, (const double*)(buf + w.g), w.m, d.mu0[v].ptr ? nullptr : mu, k);
    e = hipGetLastError();
  }
  return e == hipSuccess ? RESNMTF_OK : run.fail(e);
}

// the shared-row and shared-column maps of every view pair, -1 where a line has no partner
int fp64_upload_maps(const F64Job& J, F64Run& run) {
  const resnmtf_group_job& j = J.j;
  const F64Layout& L = J.L;
  if (L.total <= L.maps) return RESNMTF_OK;
  std::vector<int> maps((L.total - L.maps) * 2, -1);
  const size_t ibase = L.maps * 2;
  for (int v = 0; v < L.V; ++v)
    for (int w = 0; w < L.V; ++w) {
      if (L.rmap[v][w] >= 0)
        for (int p = 0; p < j.row_count[v][w]; ++p) maps[(size_t)L.rmap[v][w] - ibase + j.row_idx_v[v][w][p]] = j.row_idx_w[v][w][p];
      if (L.cmap[v][w] >= 0)
        for (int p = 0; p < j.col_count[v][w]; ++p) maps[(size_t)L.cmap[v][w] - ibase + j.col_idx_v[v][w][p]] = j.col_idx_w[v][w][p];
    }
  const hipError_t e = hipMemcpy(run.buf + L.maps, maps.data(), maps.size() * sizeof(int), hipMemcpyHostToDevice);
  return e == hipSuccess ? RESNMTF_OK : run.fail(e);
}

// ||X_v||_F^2 as norm()^2 (R/main.r:48)
int fp64_norms(const F64Job& J, F64Run& run) {
  const F64Layout& L = J.L;
  double* buf = run.buf;
  for (int v = 0; v < L.V; ++v) {
    const F64View& w = L.vw[v];
    // (a sparse view: over the CSC values, the image's non-zeros in entry order)
    const size_t total = w.sparse() ? w.nnz : w.ldn * w.mpad;
    const int nb = (int)((total + F64_NORM_CHUNK - 1) / F64_NORM_CHUNK);
    if (nb > 0)
      hipLaunchKernelGGL(fp64_norm_kernel, dim3(nb), dim3(F64_THREADS), 0, run.st, (const double*)(buf + (w.sparse() ? w.cval : w.x)),
                         total, buf + L.spart);
    F64KKArgs kk{};
    kk.mode = F64_KK_NORM; kk.k = L.k; kk.V = L.V; kk.v = v; kk.part_a = buf + L.spart; kk.nblk_a = nb;
    kk.S = buf + L.s; kk.norms = buf + L.norms; kk.errs = buf + L.errs; kk.err_out = buf + L.err;
    hipLaunchKernelGGL(fp64_kk_kernel, dim3(1), dim3(F64_THREADS), 0, run.st, kk);
  }
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? RESNMTF_OK : run.fail(e);
}

// the loop of R/main.r:53-80.  A fixed count is enqueued whole; in convergence mode the 8-byte mean error comes back
// after every sweep and the host applies the stop rule, so the state on the device is the stop sweep's own
int fp64_loop(const F64Job& J, F64Run& run) {
  double err_temp = 0.0;
  while (run.it < J.L.cap) {
    fp64_enqueue_sweep(run.st, J.j, J.L, run.buf, run.it);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return run.fail(e);
    ++run.it;
    if (J.j.n_iters == 0) {
      double mean = 0.0;
      e = hipMemcpyAsync(&mean, run.buf + J.L.err + (run.it - 1), sizeof(double), hipMemcpyDeviceToHost, run.st);
      if (e == hipSuccess) e = hipStreamSynchronize(run.st);
      if (e != hipSuccess) return run.fail(e);
      const double diff = std::fabs(mean - err_temp);
      err_temp = mean;
      if (!(diff > J.tol)) break;
    }
  }
  return RESNMTF_OK;
}

// view v's five pieces into one set of dev's arrays (0: the results, 1: the raw state), device to device on the stream
hipError_t fp64_copy_out(const F64Job& J, F64Run& run, int v, int set) {
  const F64View& w = J.L.vw[v];
  hipError_t e = hipSuccess;
  for (int f = set * F64_OUT_SET; f < (set + 1) * F64_OUT_SET && e == hipSuccess; ++f) {
    const F64OutField& o = F64_OUT_FIELDS[f];
    e = hipMemcpyAsync(o.ptr(*J.dev, v), run.buf + fp64_piece_offset(J.L, v, o.piece),
                       o.count((size_t)w.n, (size_t)w.m, (size_t)J.L.k) * sizeof(double), hipMemcpyDeviceToDevice, run.st);
  }
  return e;
}

// the raw state, as a later call resumes from it; normalisation_check (R/utils.r:176-195); the normalised results to
// device memory and to the host, the error history and the sweep count
int fp64_results_out(const F64Job& J, F64Run& run) {
  const resnmtf_group_job& j = J.j;
  const F64Layout& L = J.L;
  const int V = L.V, k = L.k;
  double* buf = run.buf;
  hipError_t e = hipSuccess;
  if (J.use.state)
    for (int v = 0; v < V; ++v)
      if ((e = fp64_copy_out(J, run, v, 1)) != hipSuccess) return run.fail(e);
  for (int v = 0; v < V; ++v) {
    const F64View& w = L.vw[v];
    const size_t total = ((size_t)w.n + w.m + k) * k;
    const int nb = (int)std::min<size_t>((total + F64_THREADS - 1) / F64_THREADS, 4096);
    hipLaunchKernelGGL(fp64_normalise_kernel, dim3(nb), dim3(F64_THREADS), 0, run.st, buf + w.f, buf + w.g,
                       buf + L.s + (size_t)v * k * k, (const double*)(buf + L.cf + (size_t)v * k),
                       (const double*)(buf + L.cg + (size_t)v * k), w.n, w.m, k);
  }
  e = hipGetLastError();
  std::vector<double> errs((size_t)run.it);
  bool to_host = !J.use.out;                // with device outputs the host copy is made only for a host pointer that is set
  for (int v = 0; v < V; ++v) {
    if (J.use.out && e == hipSuccess) e = fp64_copy_out(J, run, v, 0);
    to_host = to_host || j.f_out[v] || j.s_out[v] || j.g_out[v] || j.lambda_out[v] || j.mu_out[v];
  }
  if (e == hipSuccess && to_host)
    e = hipMemcpyAsync(run.host.data(), buf + L.out_begin, run.host.size() * sizeof(double), hipMemcpyDeviceToHost, run.st);
  if (e == hipSuccess && run.it > 0) e = hipMemcpyAsync(errs.data(), buf + L.err, errs.size() * sizeof(double), hipMemcpyDeviceToHost, run.st);
  if (e == hipSuccess) e = hipStreamSynchronize(run.st);
  if (e != hipSuccess) return run.fail(e);
  for (int v = 0; v < V; ++v) {            // (a host pointer may be NULL only beside device outputs)
    if (j.f_out[v]) std::memcpy(j.f_out[v], run.at(L.vw[v].f), (size_t)L.vw[v].n * k * sizeof(double));
    if (j.g_out[v]) std::memcpy(j.g_out[v], run.at(L.vw[v].g), (size_t)L.vw[v].m * k * sizeof(double));
    if (j.s_out[v]) std::memcpy(j.s_out[v], run.at(L.s + (size_t)v * k * k), (size_t)k * k * sizeof(double));
    if (j.lambda_out[v]) std::memcpy(j.lambda_out[v], run.at(L.lam + (size_t)v * k), (size_t)k * sizeof(double));
    if (j.mu_out[v]) std::memcpy(j.mu_out[v], run.at(L.mu + (size_t)v * k), (size_t)k * sizeof(double));
  }
  for (int t = 0; t < run.it; ++t) j.all_error[t] = errs[(size_t)t];
  *j.iters_done = run.it;
  return RESNMTF_OK;
}

int fp64_run_impl(int device_id, const resnmtf_group_job* job, const resnmtf_fp64_sparse* sp, const resnmtf_fp64_device* dev,
                  const resnmtf_fp64_sparse_device* spd, double tol, int max_iters) {
  // (the struct sizes first: nothing of sp or spd is read before them, and they are the first refusal of their entries)
  if (sp && sp->struct_size != (int)sizeof(resnmtf_fp64_sparse)) return fp64_bad("resnmtf_fp64_sparse struct_size mismatch");
  if (spd && spd->struct_size != (int)sizeof(resnmtf_fp64_sparse_device)) return fp64_bad("resnmtf_fp64_sparse_device struct_size mismatch");
  if (!job) return fp64_bad("job is NULL");
  if (max_iters < 1) return fp64_bad("max_iters must be >= 1");
  if (!std::isfinite(tol)) return fp64_bad("tol must be finite");
  F64Job J{device_id, *job, sp, dev, spd, tol, max_iters, {}, {}, {}, {}};
  F64Run run;                               // (no runtime call before fp64_open_stream; everything it holds goes on return)
  int rc = fp64_checks(J);
  if (rc == RESNMTF_OK) rc = fp64_open_stream(J, run);
  if (rc == RESNMTF_OK) rc = fp64_build_sparse_device_views(J, run);
  if (rc == RESNMTF_OK) rc = fp64_allocate(J, run);
  if (rc == RESNMTF_OK) rc = fp64_upload_views(J, run);
  if (rc == RESNMTF_OK) rc = fp64_upload_state(J, run);
  if (rc == RESNMTF_OK) rc = fp64_upload_maps(J, run);
  if (rc == RESNMTF_OK) rc = fp64_norms(J, run);
  if (rc == RESNMTF_OK) rc = fp64_loop(J, run);
  if (rc == RESNMTF_OK) rc = fp64_results_out(J, run);
  return rc;
}
}  // namespace

// ---- resnmtf_fp64_bisil: the silhouettes of R/obtain_bicl.r:189-199 on the fp64 values of X ----
namespace {
// What a call holds on the device: its stream and its one buffer.  On every way out the destructor waits for the stream
// and destroys it, then frees the buffer.
class F64BisilRun {
 public:
  F64BisilRun() = default;
  F64BisilRun(const F64BisilRun&) = delete;
  F64BisilRun& operator=(const F64BisilRun&) = delete;
  ~F64BisilRun() {
    if (st) { (void)hipStreamSynchronize(st); (void)hipStreamDestroy(st); }
    if (buf) (void)hipFree(buf);
  }
  int fail(hipError_t e, const char* what = "fp64_bisil: ") {
    resnmtf_set_create_error(std::string(what) + hipGetErrorString(e));
    return RESNMTF_ERR_HIP;
  }
  hipStream_t st = nullptr;
  double* buf = nullptr;
};

// the launches of every side and active bicluster on the run's stream.  gather(sd, feat, nf, upts, n_u, upad, G) enqueues
// what fills the restricted block G of side sd -- the gather of a dense X (resnmtf_fp64_bisil), the zero-fill and scatter
// of a sparse one (resnmtf_fp64_bisil_sparse) -- and returns the runtime's answer; the rest is one text for both.
template <class Gather>
hipError_t fp64_bisil_enqueue(hipStream_t st, Gather&& gather, int n, int m, int k, int metric,
                              const BisilHostLists& L, const F64BisilPlan& plan, const F64BisilMeta& M, double* buf) {
  double* G = buf;
  double* norm2 = buf + plan.norm2;
  double* partial = buf + plan.partial;
  double* sil = buf + plan.sil;
  const unsigned long long* dmeta = reinterpret_cast<const unsigned long long*>(buf + plan.meta);
  const int* dints = reinterpret_cast<const int*>(dmeta);
  hipError_t e = hipMemsetAsync(norm2, 0, plan.upad_max * sizeof(double), st);
  for (int sd = 0; sd < 2 && e == hipSuccess; ++sd) {
    const BisilHostSide& s = L.side[sd];
    const int n_u = (int)s.upts.size(), upad = (n_u + F64_BISIL_TILE - 1) / F64_BISIL_TILE * F64_BISIL_TILE;
    const int n_pts = sd == 0 ? n : m;
    const unsigned long long* umask = dmeta + M.mask[sd];
    const int* upts = dints + M.pts[sd];
    double* out = sil + (sd == 0 ? 0 : (size_t)n * k);
    for (int j = 0; j < k && e == hipSuccess; ++j) {
      if (!((L.active >> j) & 1ull)) continue;
      const int nf = L.side[1 - sd].cnt[j], n_mem = s.cnt[j];
      const int* feat = dints + M.feat[sd][j];
      const int* mpos = dints + M.mpos[sd][j];
      if ((e = gather(sd, feat, nf, upts, n_u, upad, G)) != hipSuccess) break;
      if (metric == F64_BISIL_COSINE)
        hipLaunchKernelGGL(fp64_bisil_norm_kernel, dim3((upad + 255) / 256), dim3(256), 0, st, (const double*)G, nf, upad, norm2);
      const dim3 grid((n_mem + F64_BISIL_TILE - 1) / F64_BISIL_TILE, plan.chunks[sd][j]);
      fp64_bisil_dist(metric, plan.kq, grid, st, G, nf, upad, n_u, mpos, n_mem, umask, norm2, k, plan.chunk_tiles[sd][j], partial);
      hipLaunchKernelGGL(fp64_bisil_epilogue_kernel, dim3((n_mem + 3) / 4), dim3(256), 0, st, (const double*)partial,
                         plan.chunks[sd][j], n_mem, k, j, mpos, umask, upts, dints + M.cnt[sd], L.active, n_pts, out);
      e = hipGetLastError();
    }
  }
  return e;
}
}  // namespace

extern "C" {

int resnmtf_fp64_bisil(int device_id, const resnmtf_fp64_bisil_job* job) {
  if (!job) return fp64_bad("job is NULL");
  if (job->struct_size != (int)sizeof(resnmtf_fp64_bisil_job)) return fp64_bad("resnmtf_fp64_bisil_job struct_size mismatch");
  const int n = job->n, m = job->m, k = job->k, metric = job->metric;
  if (k < 1 || k > RESNMTF_MAX_K) return fp64_bad("k must be in [1, 64]");
  if (n < 1 || m < 1) return fp64_bad("view dimensions must be positive");
  if (metric < F64_BISIL_EUCLIDEAN || metric > F64_BISIL_COSINE)
    return fp64_bad("metric must be 0 (euclidean), 1 (manhattan) or 2 (cosine)");
  const bool host_x = job->x != nullptr;
  if (host_x == (job->x_dev.ptr != nullptr))
    return fp64_bad(host_x ? "X is given in two places (job->x and job->x_dev)" : "X is given in no place (job->x or job->x_dev)");
  if (!job->row_clusters || !job->col_clusters || !job->row_sil || !job->col_sil)
    return fp64_bad("row_clusters / col_clusters / row_sil / col_sil are NULL");
  resnmtf_device_matrix x = job->x_dev;
  if (!host_x) {
    if (x.dtype < RESNMTF_DTYPE_F64 || x.dtype > RESNMTF_DTYPE_BF16) return fp64_bad("x_dev: unknown dtype");
    if (x.row_stride < 0 || x.col_stride < 0) return fp64_bad("x_dev: strides must be >= 0");
    const size_t last = (size_t)(n - 1) * (size_t)x.row_stride + (size_t)(m - 1) * (size_t)x.col_stride;
    bool beyond = false;
    if (!fp64_on_device(device_id, x.ptr, (last + 1) * fp64_dtype_bytes(x.dtype), beyond))
      return fp64_bad(beyond ? std::string("x_dev reaches beyond its allocation (too short for the shape and strides given)")
                             : "x_dev is not device memory of device " + std::to_string(device_id));
  }
  BisilHostLists L;
  if (const int which = bisil_build_lists(n, m, k, job->row_clusters, job->col_clusters, L))
    return fp64_bad(which == 1 ? "row_clusters entries must be 0 or 1" : "col_clusters entries must be 0 or 1");
  if (!L.active) {
    std::fill(job->row_sil, job->row_sil + (size_t)n * k, 0.0);
    std::fill(job->col_sil, job->col_sil + (size_t)m * k, 0.0);
    return RESNMTF_OK;
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) { resnmtf_set_create_error("no HIP device"); return RESNMTF_ERR_NO_DEVICE; }
  if (device_id < 0 || device_id >= ndev) return fp64_bad("device_id out of range");
  F64BisilRun run;
  hipError_t e = hipSetDevice(device_id);
  if (e != hipSuccess) return run.fail(e, "hipSetDevice: ");
  // the workspace, sized before anything is allocated
  F64BisilMeta M;
  f64_bisil_pack(k, L, M);
  const int n_u[2] = {(int)L.side[0].upts.size(), (int)L.side[1].upts.size()};
  const int* const cnt[2] = {L.side[0].cnt.data(), L.side[1].cnt.data()};
  F64BisilPlan plan;
  f64_bisil_plan(n, m, k, L.active, n_u, cnt, M.words.size(), host_x, plan);
  const size_t bytes = plan.total * sizeof(double);
  size_t free_b = 0, total_b = 0;
  if ((e = hipMemGetInfo(&free_b, &total_b)) != hipSuccess) return run.fail(e);
  if (bytes > free_b) {
    resnmtf_set_create_error("fp64_bisil workspace: " + std::to_string(bytes) + " bytes asked for (" + std::to_string(plan.g_dbl * sizeof(double)) +
                             " of them the restricted block, features x padded members" +
                             (host_x ? ", " + std::to_string((size_t)n * m * sizeof(double)) + " the fp64 copy of X" : std::string()) + "), " +
                             std::to_string(free_b) + " free on the device");
    return RESNMTF_ERR_ALLOC;
  }
  void* p = nullptr;
  if ((e = hipMalloc(&p, bytes)) != hipSuccess) {
    (void)hipGetLastError();
    resnmtf_set_create_error(std::string("fp64_bisil workspace: ") + hipGetErrorString(e) + " (" + std::to_string(bytes) + " bytes asked for)");
    return e == hipErrorOutOfMemory ? RESNMTF_ERR_ALLOC : RESNMTF_ERR_HIP;
  }
  run.buf = static_cast<double*>(p);
  if ((e = hipStreamCreateWithFlags(&run.st, hipStreamNonBlocking)) != hipSuccess) { run.st = nullptr; return run.fail(e, "hipStreamCreate: "); }
  if (host_x) {                               // one plain n x m fp64 copy; it then goes through the same gather
    e = hipMemcpyAsync(run.buf + plan.x, job->x, (size_t)n * m * sizeof(double), hipMemcpyHostToDevice, run.st);
    x.ptr = run.buf + plan.x; x.dtype = RESNMTF_DTYPE_F64; x.row_stride = 1; x.col_stride = n;
  } else {
    e = wait_for_caller(run.st, job->stream);
  }
  const size_t sil_dbl = (size_t)n * k + (size_t)m * k;
  if (e == hipSuccess) e = hipMemcpyAsync(run.buf + plan.meta, M.words.data(), M.words.size() * sizeof(unsigned long long), hipMemcpyHostToDevice, run.st);
  if (e == hipSuccess) e = hipMemsetAsync(run.buf + plan.sil, 0, sil_dbl * sizeof(double), run.st);
  auto gather = [&](int sd, const int* feat, int nf, const int* upts, int n_u, int upad, double* G) {
    fp64_bisil_gather(run.st, x, sd, feat, nf, upts, n_u, upad, G);
    return hipSuccess;
  };
  if (e == hipSuccess) e = fp64_bisil_enqueue(run.st, gather, n, m, k, metric, L, plan, M, run.buf);
  if (e == hipSuccess) e = hipMemcpyAsync(job->row_sil, run.buf + plan.sil, (size_t)n * k * sizeof(double), hipMemcpyDeviceToHost, run.st);
  if (e == hipSuccess) e = hipMemcpyAsync(job->col_sil, run.buf + plan.sil + (size_t)n * k, (size_t)m * k * sizeof(double), hipMemcpyDeviceToHost, run.st);
  if (e == hipSuccess) e = hipStreamSynchronize(run.st);
  return e == hipSuccess ? RESNMTF_OK : run.fail(e);
}

int resnmtf_fp64_bisil_plan(int n_u, int n_mem, int k, long long row_stride, long long col_stride, int* out) {
  if (!out) return fp64_bad("out is NULL");
  if (n_u < 1 || n_mem < 1) return fp64_bad("n_u and n_mem must be positive");
  if (k < 1 || k > RESNMTF_MAX_K) return fp64_bad("k must be in [1, 64]");
  if (row_stride < 0 || col_stride < 0) return fp64_bad("strides must be >= 0");
  const BisilChunks c = bisil_chunk_rule(n_u, n_mem);
  const int vals[RESNMTF_FP64_BISIL_PLAN_INTS] = {bisil_kq(k), c.chunk_tiles, c.chunks, f64_bisil_side_form(0, row_stride, col_stride),
                                                  f64_bisil_side_form(1, row_stride, col_stride)};
  std::memcpy(out, vals, sizeof(vals));
  return RESNMTF_OK;
}

// ---- resnmtf_fp64_bisil_sparse: the same silhouettes of a view stored sparse ----
int resnmtf_fp64_bisil_sparse(int device_id, const resnmtf_fp64_bisil_sparse_job* job) {
  static const char* const NAME = "fp64_bisil_sparse";
  if (!job) return fp64_bad("job is NULL");
  if (job->struct_size != (int)sizeof(resnmtf_fp64_bisil_sparse_job)) return fp64_bad("resnmtf_fp64_bisil_sparse_job struct_size mismatch");
  const int n = job->n, m = job->m, k = job->k, metric = job->metric;
  if (k < 1 || k > RESNMTF_MAX_K) return fp64_bad("k must be in [1, 64]");
  if (n < 1 || m < 1) return fp64_bad("view dimensions must be positive");
  if (metric < F64_BISIL_EUCLIDEAN || metric > F64_BISIL_COSINE)
    return fp64_bad("metric must be 0 (euclidean), 1 (manhattan) or 2 (cosine)");
  const bool host_x = job->x.col_ptr != nullptr;
  if (host_x == fp64_spd_given(job->x_dev))
    return fp64_bad(host_x ? "X is given in two places (job->x and job->x_dev)" : "X is given in no place (job->x or job->x_dev)");
  if (!job->row_clusters || !job->col_clusters || !job->row_sil || !job->col_sil)
    return fp64_bad("row_clusters / col_clusters / row_sil / col_sil are NULL");
  // the view's own refusals are those of view 0 of a one-view run, through the run's checks and with their texts
  F64SparseShape shape;
  resnmtf_fp64_sparse_device spd{};
  if (host_x) {
    if (!job->x.values) return fp64_bad("view 0: values is NULL");
    const std::string why = fp64_check_csc(n, m, job->x.col_ptr, job->x.row_idx, job->x.values, shape);
    if (!why.empty()) return fp64_bad("view 0: " + why);
  } else {
    resnmtf_group_job one{};
    one.struct_size = (int)sizeof(resnmtf_group_job);
    one.n_views = 1; one.k = k; one.n_rows[0] = n; one.n_cols[0] = m;
    spd.struct_size = (int)sizeof(resnmtf_fp64_sparse_device);
    spd.stream = job->stream;
    spd.view[0] = job->x_dev;
    F64Source src[RESNMTF_GROUP_MAX_VIEWS];
    fp64_resolve_sources(nullptr, nullptr, &spd, src);
    std::string why = fp64_check_sparse_device_struct(one, nullptr, nullptr, spd);
    if (why.empty()) why = fp64_check_sparse_device_pointers(device_id, one, spd, src);
    if (!why.empty()) return fp64_bad(why);
    shape.nnz = (size_t)job->x_dev.nnz;
  }
  BisilHostLists L;
  if (const int which = bisil_build_lists(n, m, k, job->row_clusters, job->col_clusters, L))
    return fp64_bad(which == 1 ? "row_clusters entries must be 0 or 1" : "col_clusters entries must be 0 or 1");
  if (!L.active) {
    std::fill(job->row_sil, job->row_sil + (size_t)n * k, 0.0);
    std::fill(job->col_sil, job->col_sil + (size_t)m * k, 0.0);
    return RESNMTF_OK;
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) { resnmtf_set_create_error("no HIP device"); return RESNMTF_ERR_NO_DEVICE; }
  if (device_id < 0 || device_id >= ndev) return fp64_bad("device_id out of range");
  // (declared before the run: what the stream may still read is released after the run has waited for it)
  F64BisilMeta M;
  std::vector<int> rank;
  F64Transient transient(NAME);
  F64BisilRun run;
  hipError_t e = hipSetDevice(device_id);
  if (e != hipSuccess) return run.fail(e, "hipSetDevice: ");
  // the workspace, sized before anything is allocated
  f64_bisil_pack(k, L, M);
  f64_bisil_ranks(L, rank);
  const int n_u[2] = {(int)L.side[0].upts.size(), (int)L.side[1].upts.size()};
  const int* const cnt[2] = {L.side[0].cnt.data(), L.side[1].cnt.data()};
  F64BisilSparsePlan plan;
  f64_bisil_sparse_plan(n, m, k, L.active, n_u, cnt, M.words.size(), shape.nnz, plan);
  const size_t nnz = shape.nnz, bytes = plan.total * sizeof(double);
  size_t free_b = 0, total_b = 0;
  if ((e = hipMemGetInfo(&free_b, &total_b)) != hipSuccess) return run.fail(e, "fp64_bisil_sparse: ");
  if (bytes > free_b) {
    resnmtf_set_create_error("fp64_bisil_sparse workspace: " + std::to_string(bytes) + " bytes asked for (" +
                             std::to_string(plan.dense.g_dbl * sizeof(double)) + " of them the restricted block, features x padded members, " +
                             std::to_string(plan.copies_dbl * sizeof(double)) + " the CSC and CSR copies of X), " +
                             std::to_string(free_b) + " free on the device");
    return RESNMTF_ERR_ALLOC;
  }
  if ((e = hipStreamCreateWithFlags(&run.st, hipStreamNonBlocking)) != hipSuccess) { run.st = nullptr; return run.fail(e, "hipStreamCreate: "); }
  // a device view: checked and sorted on the device before anything is scattered (the failure word is read back and
  // the stream synchronised inside); its canonical arrays wait in transient memory for the buffer
  F64SpdView dv;
  if (!host_x) {
    if ((e = wait_for_caller(run.st, job->stream)) != hipSuccess) return run.fail(e, "fp64_bisil_sparse: ");
    const int rc = fp64_build_sparse_device_view(run.st, transient, 0, job->x_dev, n, m, dv, shape, NAME);
    if (rc != RESNMTF_OK) return rc;
  }
  void* p = nullptr;
  if ((e = hipMalloc(&p, bytes)) != hipSuccess) {
    (void)hipGetLastError();
    resnmtf_set_create_error(std::string("fp64_bisil_sparse workspace: ") + hipGetErrorString(e) + " (" + std::to_string(bytes) + " bytes asked for)");
    return e == hipErrorOutOfMemory ? RESNMTF_ERR_ALLOC : RESNMTF_ERR_HIP;
  }
  run.buf = static_cast<double*>(p);
  double* buf = run.buf;
  hipStream_t st = run.st;
  // the two sparse copies into the buffer, as a run stores them (no stored entry: all pointers zero, nothing to scatter)
  const F64SparseAt at{plan.cptr, plan.cval, plan.cidx, plan.rptr, plan.rval, plan.ridx};
  if (nnz == 0) e = hipMemsetAsync(buf + plan.cptr, 0, plan.copies_dbl * sizeof(double), st);
  else if (host_x) e = fp64_upload_host_csc(buf, at, n, m, nnz, job->x);
  else e = fp64_copy_spd_view(st, buf, at, n, m, nnz, dv);
  const size_t sil_dbl = (size_t)n * k + (size_t)m * k;
  if (e == hipSuccess) e = hipMemcpyAsync(buf + plan.dense.meta, M.words.data(), M.words.size() * sizeof(unsigned long long), hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(buf + plan.rank, rank.data(), rank.size() * sizeof(int), hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemsetAsync(buf + plan.dense.sil, 0, sil_dbl * sizeof(double), st);
  // side 0 (points = rows): the features are columns, read from the CSC; side 1: rows of the CSR
  const int* drank = reinterpret_cast<const int*>(buf + plan.rank);
  auto scatter = [&](int sd, const int* feat, int nf, const int*, int, int upad, double* G) {
    return fp64_bisil_scatter(st, reinterpret_cast<const long long*>(buf + (sd == 0 ? plan.cptr : plan.rptr)),
                              reinterpret_cast<const int*>(buf + (sd == 0 ? plan.cidx : plan.ridx)),
                              buf + (sd == 0 ? plan.cval : plan.rval), feat, nf, drank + (sd == 0 ? 0 : n), upad, G);
  };
  if (e == hipSuccess) e = fp64_bisil_enqueue(st, scatter, n, m, k, metric, L, plan.dense, M, buf);
  if (e == hipSuccess) e = hipMemcpyAsync(job->row_sil, buf + plan.dense.sil, (size_t)n * k * sizeof(double), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipMemcpyAsync(job->col_sil, buf + plan.dense.sil + (size_t)n * k, (size_t)m * k * sizeof(double), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  return e == hipSuccess ? RESNMTF_OK : run.fail(e, "fp64_bisil_sparse: ");
}

}  // extern "C"

// ---- resnmtf_fp64_shuffle: shuffle_view of R/obtain_bicl.r:11-22 on the fp64 values of X ----
namespace {
// What a call of a handle-free entry (resnmtf_fp64_shuffle, and section 28's resnmtf_fp64_subsample and
// resnmtf_fp64_relevance) holds on the device: its stream, the small workspace and, for a host X, the staging copy.  On
// every way out the destructor waits for the stream and destroys it, then frees both buffers.  `name` heads its errors.
class F64CallRun {
 public:
  explicit F64CallRun(const char* name) : name_(name) {}
  F64CallRun(const F64CallRun&) = delete;
  F64CallRun& operator=(const F64CallRun&) = delete;
  ~F64CallRun() {
    if (st) { (void)hipStreamSynchronize(st); (void)hipStreamDestroy(st); }
    if (work) (void)hipFree(work);
    if (staging) (void)hipFree(staging);
  }
  // the HIP error as text, after `what` (the call that failed) or, without it, after the entry's name
  int fail(hipError_t e, const char* what = nullptr) {
    resnmtf_set_create_error((what ? std::string(what) : std::string(name_) + ": ") + hipGetErrorString(e));
    return RESNMTF_ERR_HIP;
  }
  // a buffer of `bytes`; a refusal names what it was for
  int alloc(void** p, size_t bytes, const char* what) {
    const hipError_t e = hipMalloc(p, bytes);
    if (e == hipSuccess) return RESNMTF_OK;
    (void)hipGetLastError();
    *p = nullptr;
    resnmtf_set_create_error(std::string(name_) + ": " + hipGetErrorString(e) + " (" + std::to_string(bytes) + " bytes asked for, " + what + ")");
    return e == hipErrorOutOfMemory ? RESNMTF_ERR_ALLOC : RESNMTF_ERR_HIP;
  }
  hipStream_t st = nullptr;
  char* work = nullptr;
  double* staging = nullptr;

 private:
  const char* name_;
};
}  // namespace

extern "C" {

int resnmtf_fp64_shuffle(int device_id, const resnmtf_fp64_shuffle_job* job) {
  if (const char* why = f64_shuffle_check_job(job)) return fp64_bad(why);
  const resnmtf_fp64_shuffle_job& j = *job;
  const int n = j.n, m = j.m;
  const bool host_x = j.x != nullptr;
  if (f64_shuffle_bytes_overflow(j)) {        // 8 n m does not fit 64 bits: no device holds the staging copy, or `out`
    if (!host_x) return fp64_bad("out reaches beyond its allocation (too short for n * m doubles)");
    resnmtf_set_create_error("fp64_shuffle: more than 9223372036854775808 bytes asked for (the fp64 staging copy of a host X)");
    return RESNMTF_ERR_ALLOC;
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) { resnmtf_set_create_error("no HIP device"); return RESNMTF_ERR_NO_DEVICE; }
  if (device_id < 0 || device_id >= ndev) return fp64_bad("device_id out of range");
  int host_ints[3] = {0, 0, 0};               // (declared before the run: its destructor waits for the copies into them)
  std::vector<unsigned char> host_mask;
  F64CallRun run("fp64_shuffle");
  hipError_t e = hipSetDevice(device_id);
  if (e != hipSuccess) return run.fail(e, "hipSetDevice: ");
  const size_t out_bytes = f64_shuffle_out_bytes(j);
  const F64ShufflePlan plan = f64_shuffle_plan(n, m);
  if (host_x) {                               // a shape the device cannot stage is refused on its byte count, x unread
    size_t free_b = 0, total_b = 0;
    if ((e = hipMemGetInfo(&free_b, &total_b)) != hipSuccess) return run.fail(e);
    if (out_bytes > free_b || plan.total > free_b - out_bytes) {
      resnmtf_set_create_error("fp64_shuffle: " + std::to_string(out_bytes) + " bytes asked for (the fp64 staging copy of a host X), " +
                               std::to_string(free_b) + " free on the device");
      return RESNMTF_ERR_ALLOC;
    }
  }
  bool beyond = false;
  if (!fp64_on_device(device_id, j.out, out_bytes, beyond))
    return fp64_bad(beyond ? std::string("out reaches beyond its allocation (too short for n * m doubles)")
                           : "out is not device memory of device " + std::to_string(device_id));
  resnmtf_device_matrix x = j.x_dev;
  if (!host_x) {
    const size_t src_bytes = f64_shuffle_source_bytes(j);
    if (!fp64_on_device(device_id, x.ptr, src_bytes, beyond))
      return fp64_bad(beyond ? std::string("x_dev reaches beyond its allocation (too short for the shape and strides given)")
                             : "x_dev is not device memory of device " + std::to_string(device_id));
    if (f64_shuffle_overlap(x.ptr, src_bytes, j.out, out_bytes)) return fp64_bad("out overlaps x_dev (the draw reads X while it writes out)");
  }
  void* p = nullptr;
  if ((e = hipMalloc(&p, plan.total)) != hipSuccess) {
    (void)hipGetLastError();
    resnmtf_set_create_error(std::string("fp64_shuffle workspace: ") + hipGetErrorString(e) + " (" + std::to_string(plan.total) + " bytes asked for)");
    return e == hipErrorOutOfMemory ? RESNMTF_ERR_ALLOC : RESNMTF_ERR_HIP;
  }
  run.work = static_cast<char*>(p);
  if (host_x) {
    if ((e = hipMalloc(&p, out_bytes)) != hipSuccess) {
      (void)hipGetLastError();
      resnmtf_set_create_error(std::string("fp64_shuffle: ") + hipGetErrorString(e) + " (" + std::to_string(out_bytes) +
                               " bytes asked for, the fp64 staging copy of a host X)");
      return e == hipErrorOutOfMemory ? RESNMTF_ERR_ALLOC : RESNMTF_ERR_HIP;
    }
    run.staging = static_cast<double*>(p);
  }
  if ((e = hipStreamCreateWithFlags(&run.st, hipStreamNonBlocking)) != hipSuccess) { run.st = nullptr; return run.fail(e, "hipStreamCreate: "); }
  e = wait_for_caller(run.st, j.stream);      // (a host X too: `out` may still be in use by what the caller enqueued)
  if (host_x) {                               // one plain n x m fp64 copy; it then goes through the same gather
    if (e == hipSuccess) e = hipMemcpyAsync(run.staging, j.x, out_bytes, hipMemcpyHostToDevice, run.st);
    x.ptr = run.staging; x.dtype = RESNMTF_DTYPE_F64; x.row_stride = 1; x.col_stride = n;
  }
  double* shift = reinterpret_cast<double*>(run.work + plan.shift);
  double* colsum = reinterpret_cast<double*>(run.work + plan.colsum);
  int* ints = reinterpret_cast<int*>(run.work + plan.ints);          // counts[0], counts[1], neg
  unsigned char* mask = reinterpret_cast<unsigned char*>(run.work + plan.mask);
  if (e == hipSuccess) e = hipMemsetAsync(ints, 0, 4 * sizeof(int), run.st);
  if (e == hipSuccess) {
    fp64_shuffle_gather(run.st, x, n, m, j.seed, j.out);
    fp64_shuffle_lines(run.st, j.out, n, m, mask, ints);
    if (j.normalise) fp64_shuffle_normalise(run.st, j.out, n, m, shift, colsum, ints + 2);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(host_ints, ints, sizeof(host_ints), hipMemcpyDeviceToHost, run.st);
  if (e == hipSuccess && (j.row_mask || j.col_mask)) {
    host_mask.resize((size_t)n + m);
    e = hipMemcpyAsync(host_mask.data(), mask, host_mask.size(), hipMemcpyDeviceToHost, run.st);
  }
  if (e == hipSuccess) e = hipStreamSynchronize(run.st);
  if (e != hipSuccess) return run.fail(e);
  *j.n_empty_rows = host_ints[0];
  *j.n_empty_cols = host_ints[1];
  if (j.was_negative) *j.was_negative = j.normalise ? host_ints[2] : 0;
  if (j.row_mask) std::memcpy(j.row_mask, host_mask.data(), (size_t)n);
  if (j.col_mask) std::memcpy(j.col_mask, host_mask.data() + n, (size_t)m);
  return RESNMTF_OK;
}

}  // extern "C"

// ---- resnmtf_fp64_subsample, resnmtf_fp64_relevance: a stability repeat's gather and scoring ----
// (the owner of a call's stream, workspace and staging copy is F64CallRun, above)
namespace {
// device_id names a device; RESNMTF_OK or the refusal
int fp64_check_device_id(int device_id) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) { resnmtf_set_create_error("no HIP device"); return RESNMTF_ERR_NO_DEVICE; }
  if (device_id < 0 || device_id >= ndev) return fp64_bad("device_id out of range");
  return RESNMTF_OK;
}
}  // namespace

extern "C" {

int resnmtf_fp64_subsample_plan(long long row_stride, long long col_stride, int* out) {
  if (!out) return fp64_bad("out is NULL");
  if (row_stride < 0 || col_stride < 0) return fp64_bad("strides must be >= 0");
  const int vals[RESNMTF_FP64_SUBSAMPLE_PLAN_INTS] = {f64_subsample_form(row_stride, col_stride), F64_SUB_BLOCK, F64_SUB_TILE,
                                                      F64_SUB_ROWSUM_BLOCK, F64_SUB_COLSUM_ROWS, F64_SUB_COLSUM_COLS};
  std::memcpy(out, vals, sizeof(vals));
  return RESNMTF_OK;
}

int resnmtf_fp64_subsample(int device_id, const resnmtf_fp64_subsample_job* job) {
  if (const char* why = f64_subsample_check_job(job)) return fp64_bad(why);
  const resnmtf_fp64_subsample_job& j = *job;
  const int n = j.n, m = j.m, ns = j.n_sub, ms = j.m_sub;
  const bool host_x = j.x != nullptr;
  {
    std::string why = f64_subsample_check_indices("rows", j.rows, ns, n);
    if (why.empty()) why = f64_subsample_check_indices("cols", j.cols, ms, m);
    if (!why.empty()) return fp64_bad(why);
  }
  if (host_x && f64_array_bytes_overflow(n, m)) {      // 8 n m does not fit 64 bits: no device holds the staging copy
    resnmtf_set_create_error("fp64_subsample: more than 9223372036854775808 bytes asked for (the fp64 staging copy of a host X)");
    return RESNMTF_ERR_ALLOC;
  }
  if (f64_array_bytes_overflow(ns, ms)) return fp64_bad("out reaches beyond its allocation (too short for n_sub * m_sub doubles)");
  if (int rc = fp64_check_device_id(device_id)) return rc;
  int host_ints[2] = {0, 0};                 // (declared before the run: its destructor waits for the copies into them)
  std::vector<unsigned char> host_mask;
  F64CallRun run("fp64_subsample");
  hipError_t e = hipSetDevice(device_id);
  if (e != hipSuccess) return run.fail(e, "hipSetDevice: ");
  const size_t out_bytes = f64_array_bytes(ns, ms), stage_bytes = f64_array_bytes(n, m);
  const F64SubsamplePlan plan = f64_subsample_plan(ns, ms);
  if (host_x) {                               // a shape the device cannot stage is refused on its byte count, x unread
    size_t free_b = 0, total_b = 0;
    if ((e = hipMemGetInfo(&free_b, &total_b)) != hipSuccess) return run.fail(e);
    if (stage_bytes > free_b || plan.total > free_b - stage_bytes) {
      resnmtf_set_create_error("fp64_subsample: " + std::to_string(stage_bytes) + " bytes asked for (the fp64 staging copy of a host X), " +
                               std::to_string(free_b) + " free on the device");
      return RESNMTF_ERR_ALLOC;
    }
  }
  bool beyond = false;
  if (!fp64_on_device(device_id, j.out, out_bytes, beyond))
    return fp64_bad(beyond ? std::string("out reaches beyond its allocation (too short for n_sub * m_sub doubles)")
                           : "out is not device memory of device " + std::to_string(device_id));
  resnmtf_device_matrix x = j.x_dev;
  if (!host_x) {
    const size_t src_bytes = f64_matrix_bytes(x, n, m);
    if (!fp64_on_device(device_id, x.ptr, src_bytes, beyond))
      return fp64_bad(beyond ? std::string("x_dev reaches beyond its allocation (too short for the shape and strides given)")
                             : "x_dev is not device memory of device " + std::to_string(device_id));
    if (f64_ranges_overlap(x.ptr, src_bytes, j.out, out_bytes)) return fp64_bad("out overlaps x_dev (the gather reads X while it writes out)");
  }
  void* p = nullptr;
  if (int rc = run.alloc(&p, plan.total, "the workspace")) return rc;
  run.work = static_cast<char*>(p);
  if (host_x) {
    if (int rc = run.alloc(&p, stage_bytes, "the fp64 staging copy of a host X")) return rc;
    run.staging = static_cast<double*>(p);
  }
  if ((e = hipStreamCreateWithFlags(&run.st, hipStreamNonBlocking)) != hipSuccess) { run.st = nullptr; return run.fail(e, "hipStreamCreate: "); }
  e = wait_for_caller(run.st, j.stream);      // (a host X too: `out` may still be in use by what the caller enqueued)
  if (host_x) {                               // one plain n x m fp64 copy; it then goes through the same gather
    if (e == hipSuccess) e = hipMemcpyAsync(run.staging, j.x, stage_bytes, hipMemcpyHostToDevice, run.st);
    x.ptr = run.staging; x.dtype = RESNMTF_DTYPE_F64; x.row_stride = 1; x.col_stride = n;
  }
  int* ints = reinterpret_cast<int*>(run.work + plan.ints);            // counts[0], counts[1]
  int* rows = reinterpret_cast<int*>(run.work + plan.rows);
  int* cols = reinterpret_cast<int*>(run.work + plan.cols);
  unsigned char* mask = reinterpret_cast<unsigned char*>(run.work + plan.mask);
  if (e == hipSuccess) e = hipMemsetAsync(ints, 0, 4 * sizeof(int), run.st);
  if (e == hipSuccess) e = hipMemcpyAsync(rows, j.rows, (size_t)ns * sizeof(int), hipMemcpyHostToDevice, run.st);
  if (e == hipSuccess) e = hipMemcpyAsync(cols, j.cols, (size_t)ms * sizeof(int), hipMemcpyHostToDevice, run.st);
  if (e == hipSuccess) {
    fp64_subsample_gather(run.st, x, rows, cols, ns, ms, j.out);
    fp64_subsample_lines(run.st, j.out, ns, ms, mask, ints);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(host_ints, ints, sizeof(host_ints), hipMemcpyDeviceToHost, run.st);
  if (e == hipSuccess && (j.row_mask || j.col_mask)) {
    host_mask.resize((size_t)ns + ms);
    e = hipMemcpyAsync(host_mask.data(), mask, host_mask.size(), hipMemcpyDeviceToHost, run.st);
  }
  if (e == hipSuccess) e = hipStreamSynchronize(run.st);
  if (e != hipSuccess) return run.fail(e);
  *j.n_empty_rows = host_ints[0];
  *j.n_empty_cols = host_ints[1];
  if (j.row_mask) std::memcpy(j.row_mask, host_mask.data(), (size_t)ns);
  if (j.col_mask) std::memcpy(j.col_mask, host_mask.data() + ns, (size_t)ms);
  return RESNMTF_OK;
}

int resnmtf_fp64_relevance(int device_id, const resnmtf_fp64_relevance_job* job) {
  if (const char* why = f64_relevance_check_job(job)) return fp64_bad(why);
  const resnmtf_fp64_relevance_job& j = *job;
  const int n = j.n, m = j.m, ns = j.n_sub, ms = j.m_sub, k = j.k, kr = j.k_ref;
  {
    std::string why = f64_subsample_check_indices("rows", j.rows, ns, n);
    if (why.empty()) why = f64_subsample_check_indices("cols", j.cols, ms, m);
    if (!why.empty()) return fp64_bad(why);
  }
  auto bad_entry = [](const char* name, unsigned long long pos, int len) {
    return fp64_bad(std::string(name) + " entries must be 0 or 1 (row " + std::to_string(pos % (unsigned long long)len) + ", column " +
                    std::to_string(pos / (unsigned long long)len) + ")");
  };
  if (j.true_r) { const long long at = f64_relevance_bad_entry(j.true_r, n, kr); if (at >= 0) return bad_entry("true_r", (unsigned long long)at, n); }
  if (j.true_c) { const long long at = f64_relevance_bad_entry(j.true_c, m, kr); if (at >= 0) return bad_entry("true_c", (unsigned long long)at, m); }
  if (int rc = fp64_check_device_id(device_id)) return rc;
  // the four matrices as the kernels read them; a host reference becomes its staged copy below
  struct Mat { const char* name; resnmtf_device_matrix a; int len, k; bool dev; };
  Mat mats[4] = {{"row_c", j.row_c, ns, k, true}, {"col_c", j.col_c, ms, k, true},
                 {"true_r_dev", j.true_r_dev, n, kr, j.true_r == nullptr}, {"true_c_dev", j.true_c_dev, m, kr, j.true_c == nullptr}};
  unsigned long long host_bad[4] = {F64_REL_NONE, F64_REL_NONE, F64_REL_NONE, F64_REL_NONE};   // (before the run: see above)
  std::vector<double> host_out((size_t)kr);
  F64CallRun run("fp64_relevance");
  hipError_t e = hipSetDevice(device_id);
  if (e != hipSuccess) return run.fail(e, "hipSetDevice: ");
  for (const Mat& t : mats) {
    if (!t.dev) continue;
    bool beyond = false;
    if (!fp64_on_device(device_id, t.a.ptr, f64_matrix_bytes(t.a, t.len, t.k), beyond))
      return fp64_bad(std::string(t.name) + (beyond ? " reaches beyond its allocation (too short for the shape and strides given)"
                                                    : " is not device memory of device " + std::to_string(device_id)));
  }
  const F64RelevancePlan plan = f64_relevance_plan(j);
  void* p = nullptr;
  if (int rc = run.alloc(&p, plan.total, "the workspace")) return rc;
  run.work = static_cast<char*>(p);
  if ((e = hipStreamCreateWithFlags(&run.st, hipStreamNonBlocking)) != hipSuccess) { run.st = nullptr; return run.fail(e, "hipStreamCreate: "); }
  e = wait_for_caller(run.st, j.stream);
  unsigned long long* bad = reinterpret_cast<unsigned long long*>(run.work + plan.bad);
  double* out = reinterpret_cast<double*>(run.work + plan.out);
  unsigned int* counts = reinterpret_cast<unsigned int*>(run.work + plan.counts);
  int* rows = reinterpret_cast<int*>(run.work + plan.rows);
  int* cols = reinterpret_cast<int*>(run.work + plan.cols);
  if (e == hipSuccess) e = hipMemsetAsync(bad, 0xFF, 4 * sizeof(unsigned long long), run.st);
  if (e == hipSuccess) e = hipMemsetAsync(counts, 0, 2 * plan.side_counts * sizeof(unsigned int), run.st);
  if (e == hipSuccess) e = hipMemcpyAsync(rows, j.rows, (size_t)ns * sizeof(int), hipMemcpyHostToDevice, run.st);
  if (e == hipSuccess) e = hipMemcpyAsync(cols, j.cols, (size_t)ms * sizeof(int), hipMemcpyHostToDevice, run.st);
  if (j.true_r) {
    if (e == hipSuccess) e = hipMemcpyAsync(run.work + plan.true_r, j.true_r, (size_t)n * kr * sizeof(double), hipMemcpyHostToDevice, run.st);
    mats[2].a = resnmtf_device_matrix{run.work + plan.true_r, RESNMTF_DTYPE_F64, 1, n};
  }
  if (j.true_c) {
    if (e == hipSuccess) e = hipMemcpyAsync(run.work + plan.true_c, j.true_c, (size_t)m * kr * sizeof(double), hipMemcpyHostToDevice, run.st);
    mats[3].a = resnmtf_device_matrix{run.work + plan.true_c, RESNMTF_DTYPE_F64, 1, m};
  }
  if (e == hipSuccess) {
    for (int t = 0; t < 4; ++t)
      if (mats[t].dev) fp64_relevance_check(run.st, mats[t].a, mats[t].len, mats[t].k, bad + t);
    fp64_relevance_count(run.st, mats[0].a, ns, k, mats[2].a, kr, rows, counts);
    fp64_relevance_count(run.st, mats[1].a, ms, k, mats[3].a, kr, cols, counts + plan.side_counts);
    hipLaunchKernelGGL(fp64_relevance_epilogue_kernel, dim3(1), dim3(64), 0, run.st, k, kr, (const unsigned int*)counts,
                       (const unsigned int*)(counts + plan.side_counts), out);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(host_bad, bad, sizeof(host_bad), hipMemcpyDeviceToHost, run.st);
  if (e == hipSuccess) e = hipMemcpyAsync(host_out.data(), out, (size_t)kr * sizeof(double), hipMemcpyDeviceToHost, run.st);
  if (e == hipSuccess) e = hipStreamSynchronize(run.st);
  if (e != hipSuccess) return run.fail(e);
  for (int t = 0; t < 4; ++t)
    if (host_bad[t] != F64_REL_NONE) return bad_entry(mats[t].name, host_bad[t], mats[t].len);
  std::memcpy(j.relevance, host_out.data(), (size_t)kr * sizeof(double));
  return RESNMTF_OK;
}

}  // extern "C"

// ---- resnmtf_fp64_shuffle_sparse: shuffle_view of R/obtain_bicl.r:11-22 on a view stored sparse ----
extern "C" {

int resnmtf_fp64_shuffle_sparse(int device_id, const resnmtf_fp64_shuffle_sparse_job* job) {
  static const char* const NAME = "fp64_shuffle_sparse";
  if (const char* why = f64_shuffle_sparse_check_job(job)) return fp64_bad(why);
  const resnmtf_fp64_shuffle_sparse_job& j = *job;
  const int n = j.n, m = j.m;
  const bool host_x = j.x.col_ptr != nullptr;
  // the view's own refusals are those of view 0 of a one-view run, through the run's checks and with their texts
  F64SparseShape shape;
  resnmtf_fp64_sparse_device spd{};
  resnmtf_group_job one{};
  F64Source src[RESNMTF_GROUP_MAX_VIEWS];
  if (host_x) {
    if (!j.x.values) return fp64_bad("view 0: values is NULL");
    const std::string why = fp64_check_csc(n, m, j.x.col_ptr, j.x.row_idx, j.x.values, shape);
    if (!why.empty()) return fp64_bad("view 0: " + why);
  } else {
    one.struct_size = (int)sizeof(resnmtf_group_job);
    one.n_views = 1; one.k = 1; one.n_rows[0] = n; one.n_cols[0] = m;
    spd.struct_size = (int)sizeof(resnmtf_fp64_sparse_device);
    spd.stream = j.stream;
    spd.view[0] = j.x_dev;
    fp64_resolve_sources(nullptr, nullptr, &spd, src);
    const std::string why = fp64_check_sparse_device_struct(one, nullptr, nullptr, spd);
    if (!why.empty()) return fp64_bad(why);
    shape.nnz = (size_t)j.x_dev.nnz;
  }
  const size_t nnz = shape.nnz;
  if (const char* why = f64_shuffle_sparse_check_nnz(j, nnz)) return fp64_bad(why);
  if (int rc = fp64_check_device_id(device_id)) return rc;
  int host_ints[2] = {0, 0};                 // (declared before the owners: the run's destructor waits for the copies into them)
  std::vector<unsigned char> host_mask;
  F64Transient tr(NAME);                     // (before the run: what the stream may still read is freed after the run has waited)
  F64CallRun run(NAME);
  hipError_t e = hipSetDevice(device_id);
  if (e != hipSuccess) return run.fail(e, "hipSetDevice: ");
  // whose memory the arrays are and how far they reach; then what shares a byte with what
  F64ShuffleSparseRange outs[3], ins[3];
  f64_shuffle_sparse_outputs(j, nnz, outs);
  static const char* const OUT_HOLDS[3] = {"m + 1 int64", "nnz int64", "nnz doubles"};
  for (int a = 0; a < 3; ++a) {
    if (!outs[a].bytes) continue;
    bool beyond = false;
    if (!fp64_on_device(device_id, outs[a].ptr, outs[a].bytes, beyond))
      return fp64_bad(std::string(outs[a].name) + (beyond ? std::string(" reaches beyond its allocation (too short for ") + OUT_HOLDS[a] + ")"
                                                          : " is not device memory of device " + std::to_string(device_id)));
  }
  if (!host_x) {
    const std::string why = fp64_check_sparse_device_pointers(device_id, one, spd, src);
    if (!why.empty()) return fp64_bad(why);
    f64_shuffle_sparse_sources(j, ins);
  }
  {
    const char *a = nullptr, *b = nullptr;
    if (f64_shuffle_sparse_overlap(outs, host_x ? nullptr : ins, a, b))
      return fp64_bad(std::string(a) + " overlaps " + b + (b[0] == 'o' ? " (each output is an array of its own)" : " (the draw reads X while it writes the outputs)"));
  }
  // the transient memory, sized per stored entry before anything is allocated
  const F64ShuffleSparsePlan plan = f64_shuffle_sparse_plan(n, m);
  {
    const size_t bytes = f64_shuffle_sparse_transient_bytes(n, m, nnz) + plan.total;
    size_t free_b = 0, total_b = 0;
    if ((e = hipMemGetInfo(&free_b, &total_b)) != hipSuccess) return run.fail(e);
    if (bytes > free_b) {
      resnmtf_set_create_error(std::string(NAME) + ": " + std::to_string(bytes) + " bytes asked for (" + std::to_string(F64_SHUFFLE_SPARSE_BYTES_PER_ENTRY) +
                               " per stored entry while the draw is sorted, the pointers and the masks), " + std::to_string(free_b) +
                               " free on the device");
      return RESNMTF_ERR_ALLOC;
    }
  }
  void* p = nullptr;
  if (int rc = run.alloc(&p, plan.total, "the workspace")) return rc;
  run.work = static_cast<char*>(p);
  if ((e = hipStreamCreateWithFlags(&run.st, hipStreamNonBlocking)) != hipSuccess) { run.st = nullptr; return run.fail(e, "hipStreamCreate: "); }
  hipStream_t st = run.st;
  if ((e = wait_for_caller(st, j.stream)) != hipSuccess) return run.fail(e);      // (a host X too: the outputs may still be in use)
  double* colsum = reinterpret_cast<double*>(run.work + plan.colsum);
  int* ints = reinterpret_cast<int*>(run.work + plan.ints);                      // counts[0], counts[1]
  unsigned char* mask = reinterpret_cast<unsigned char*>(run.work + plan.mask);
  if (nnz > 0) {
    // ---- the source as a canonical CSC in device memory, every index verified
    const long long* s_cptr = nullptr;
    const int* s_rows = nullptr;
    const double* s_val = nullptr;
    if (host_x) {
      long long* cp = tr.take_n<long long>((size_t)m + 1);
      int* ri = cp ? tr.take_n<int>(nnz) : nullptr;
      double* va = ri ? tr.take_n<double>(nnz) : nullptr;
      if (!va) return RESNMTF_ERR_ALLOC;
      e = hipMemcpyAsync(cp, j.x.col_ptr, ((size_t)m + 1) * sizeof(long long), hipMemcpyHostToDevice, st);
      if (e == hipSuccess) e = hipMemcpyAsync(ri, j.x.row_idx, nnz * sizeof(int), hipMemcpyHostToDevice, st);
      if (e == hipSuccess) e = hipMemcpyAsync(va, j.x.values, nnz * sizeof(double), hipMemcpyHostToDevice, st);
      if (e != hipSuccess) return run.fail(e);
      s_cptr = cp; s_rows = ri; s_val = va;
    } else {                                  // checked and sorted on the device; the stream is synchronised inside
      F64SpdView sv;
      F64SparseShape unused;
      if (int rc = fp64_build_sparse_device_view(st, tr, 0, j.x_dev, n, m, sv, unused, NAME)) return rc;
      tr.release(sv.rptr); tr.release(sv.ridx); tr.release(sv.perm);           // (the CSR half is not needed)
      s_cptr = sv.cptr; s_rows = sv.cidx; s_val = sv.cval;
    }
    // ---- where every stored entry lands, then the draw sorted into its canonical CSC by the same canonicaliser: a COO
    // in any order whose values are the source's, in place.  It verifies the coordinates again before it uses them.
    int* drow = tr.take_n<int>(nnz);
    int* dcol = drow ? tr.take_n<int>(nnz) : nullptr;
    if (!dcol) return RESNMTF_ERR_ALLOC;
    fp64_shuffle_sparse_dest(st, s_cptr, s_rows, (long long)nnz, n, m, j.seed, drow, dcol);
    if ((e = hipGetLastError()) != hipSuccess) return run.fail(e);
    resnmtf_fp64_sparse_device_view coo{};
    coo.layout = RESNMTF_SPARSE_COO; coo.index_type = RESNMTF_INDEX_I32; coo.dtype = RESNMTF_DTYPE_F64;
    coo.ptr_or_rows = drow; coo.idx_or_cols = dcol; coo.values = s_val; coo.nnz = (long long)nnz;
    F64SpdView dv;
    F64SparseShape unused;
    if (int rc = fp64_build_sparse_device_view(st, tr, 0, coo, n, m, dv, unused, NAME)) return rc;
    for (const void* q : {(const void*)s_cptr, (const void*)s_rows, (const void*)s_val, (const void*)drow, (const void*)dcol,
                          (const void*)dv.rptr, (const void*)dv.ridx, (const void*)dv.perm})
      tr.release(q);                          // (the build has synchronised the stream: nothing reads these any more)
    // ---- the outputs: pointers, rows widened, the redraw condition, the values
    e = hipMemcpyAsync(j.out_col_ptr, dv.cptr, ((size_t)m + 1) * sizeof(long long), hipMemcpyDeviceToDevice, st);
    if (e == hipSuccess) e = hipMemsetAsync(ints, 0, 4 * sizeof(int), st);
    if (e == hipSuccess) {
      fp64_shuffle_sparse_widen(st, dv.cidx, (long long)nnz, j.out_row_idx);
      e = fp64_shuffle_sparse_lines(st, dv.cptr, dv.cidx, dv.cval, (long long)nnz, n, m, mask, ints);
    }
    if (e == hipSuccess) {
      if (j.normalise) {
        fp64_shuffle_sparse_normalise(st, dv.cptr, dv.cidx, dv.cval, m, colsum, j.out_values);
        e = hipGetLastError();
      } else {
        e = hipMemcpyAsync(j.out_values, dv.cval, nnz * sizeof(double), hipMemcpyDeviceToDevice, st);
      }
    }
    if (e == hipSuccess) e = hipMemcpyAsync(host_ints, ints, sizeof(host_ints), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && (j.row_mask || j.col_mask)) {
      host_mask.resize((size_t)n + m);
      e = hipMemcpyAsync(host_mask.data(), mask, host_mask.size(), hipMemcpyDeviceToHost, st);
    }
  } else {                                    // no stored entry: zero pointers, every line empty, nothing of size zero launched
    if (!host_x) {                            // (the pointers of a CSC / CSR view are still judged on the device)
      F64SpdView sv;
      F64SparseShape unused;
      if (int rc = fp64_build_sparse_device_view(st, tr, 0, j.x_dev, n, m, sv, unused, NAME)) return rc;
    }
    e = hipMemsetAsync(j.out_col_ptr, 0, ((size_t)m + 1) * sizeof(long long), st);
    host_ints[0] = n; host_ints[1] = m;
    host_mask.assign((size_t)n + m, 1);
  }
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) return run.fail(e);
  *j.n_empty_rows = host_ints[0];
  *j.n_empty_cols = host_ints[1];
  if (j.row_mask) std::memcpy(j.row_mask, host_mask.data(), (size_t)n);
  if (j.col_mask) std::memcpy(j.col_mask, host_mask.data() + n, (size_t)m);
  return RESNMTF_OK;
}

}  // extern "C"

// ---- resnmtf_fp64_subsample_sparse: data[[i]][row_samples, col_samples] of
// R/stability_analysis.r:124 on a view stored sparse ----
extern "C" {

int resnmtf_fp64_subsample_sparse(int device_id, const resnmtf_fp64_subsample_sparse_job* job) {
  static const char* const NAME = "fp64_subsample_sparse";
  if (const char* why = f64_subsample_sparse_check_job(job)) return fp64_bad(why);
  const resnmtf_fp64_subsample_sparse_job& j = *job;
  const int n = j.n, m = j.m, ns = j.n_sub, ms = j.m_sub;
  const bool host_x = j.x.col_ptr != nullptr, fill = !f64_subsample_sparse_count_mode(j);
  {
    std::string why = f64_subsample_check_indices("rows", j.rows, ns, n);
    if (why.empty()) why = f64_subsample_check_indices("cols", j.cols, ms, m);
    if (!why.empty()) return fp64_bad(why);
  }
  // the view's own refusals are those of view 0 of a one-view run, through the run's checks and with their texts
  F64SparseShape shape;
  resnmtf_fp64_sparse_device spd{};
  resnmtf_group_job one{};
  F64Source src[RESNMTF_GROUP_MAX_VIEWS];
  if (host_x) {
    if (!j.x.values) return fp64_bad("view 0: values is NULL");
    const std::string why = fp64_check_csc(n, m, j.x.col_ptr, j.x.row_idx, j.x.values, shape);
    if (!why.empty()) return fp64_bad("view 0: " + why);
  } else {
    one.struct_size = (int)sizeof(resnmtf_group_job);
    one.n_views = 1; one.k = 1; one.n_rows[0] = n; one.n_cols[0] = m;
    spd.struct_size = (int)sizeof(resnmtf_fp64_sparse_device);
    spd.stream = j.stream;
    spd.view[0] = j.x_dev;
    fp64_resolve_sources(nullptr, nullptr, &spd, src);
    const std::string why = fp64_check_sparse_device_struct(one, nullptr, nullptr, spd);
    if (!why.empty()) return fp64_bad(why);
    shape.nnz = (size_t)j.x_dev.nnz;
  }
  const size_t nnz = shape.nnz;
  if (int rc = fp64_check_device_id(device_id)) return rc;
  long long host_nnz_sub = 0;                // (declared before the owners: the run's destructor waits for the copies into them)
  int host_ints[2] = {0, 0};
  std::vector<unsigned char> host_mask;
  F64Transient tr(NAME);                     // (before the run: what the stream may still read is freed after the run has waited)
  F64CallRun run(NAME);
  hipError_t e = hipSetDevice(device_id);
  if (e != hipSuccess) return run.fail(e, "hipSetDevice: ");
  // whose memory the arrays are and how far they reach; then what shares a byte with what
  F64ShuffleSparseRange outs[3], ins[3];
  f64_subsample_sparse_outputs(j, outs);
  static const char* const OUT_HOLDS[3] = {"m_sub + 1 int64", "out_capacity int64", "out_capacity doubles"};
  for (int a = 0; a < 3; ++a) {
    if (!outs[a].bytes) continue;
    bool beyond = false;
    if (!fp64_on_device(device_id, outs[a].ptr, outs[a].bytes, beyond))
      return fp64_bad(std::string(outs[a].name) + (beyond ? std::string(" reaches beyond its allocation (too short for ") + OUT_HOLDS[a] + ")"
                                                          : " is not device memory of device " + std::to_string(device_id)));
  }
  if (!host_x) {
    const std::string why = fp64_check_sparse_device_pointers(device_id, one, spd, src);
    if (!why.empty()) return fp64_bad(why);
    f64_subsample_sparse_sources(j, ins);
  }
  {
    const char *a = nullptr, *b = nullptr;
    if (f64_shuffle_sparse_overlap(outs, host_x ? nullptr : ins, a, b))
      return fp64_bad(std::string(a) + " overlaps " + b + (b[0] == 'o' ? " (each output is an array of its own)" : " (the gather reads X while it writes the outputs)"));
  }
  // the transient memory, sized on the most entries the sub-sample can keep before anything is allocated
  const F64SubsampleSparsePlan plan = f64_subsample_sparse_plan(n, ns, ms);
  {
    const unsigned long long bound = fill ? f64_subsample_sparse_bound(ns, ms, nnz) : 0;
    const size_t bytes = f64_subsample_sparse_transient_bytes(n, m, ns, ms, nnz, bound, !host_x) + plan.total;
    size_t free_b = 0, total_b = 0;
    if ((e = hipMemGetInfo(&free_b, &total_b)) != hipSuccess) return run.fail(e);
    if (bytes > free_b) {
      resnmtf_set_create_error(std::string(NAME) + ": " + std::to_string(bytes) + " bytes asked for (" +
                               std::to_string(F64_SUBSAMPLE_SPARSE_BYTES_PER_STORED) + " per stored entry, " +
                               std::to_string(F64_SUBSAMPLE_SPARSE_BYTES_PER_STORED_BUILD) + " while a view in device memory is sorted, " +
                               std::to_string(F64_SUBSAMPLE_SPARSE_BYTES_PER_KEPT) +
                               " per kept entry while the sub-sample is sorted, the pointers, the lists and the masks), " +
                               std::to_string(free_b) + " free on the device");
      return RESNMTF_ERR_ALLOC;
    }
  }
  void* p = nullptr;
  if (int rc = run.alloc(&p, plan.total, "the workspace")) return rc;
  run.work = static_cast<char*>(p);
  if ((e = hipStreamCreateWithFlags(&run.st, hipStreamNonBlocking)) != hipSuccess) { run.st = nullptr; return run.fail(e, "hipStreamCreate: "); }
  hipStream_t st = run.st;
  if ((e = wait_for_caller(st, j.stream)) != hipSuccess) return run.fail(e);      // (a host X too: the outputs may still be in use)
  long long* counts = reinterpret_cast<long long*>(run.work + plan.counts);
  long long* scan = reinterpret_cast<long long*>(run.work + plan.scan);
  int* inv_row = reinterpret_cast<int*>(run.work + plan.inv_row);
  int* rows = reinterpret_cast<int*>(run.work + plan.rows);
  int* cols = reinterpret_cast<int*>(run.work + plan.cols);
  int* ints = reinterpret_cast<int*>(run.work + plan.ints);                      // counts[0], counts[1]
  unsigned char* mask = reinterpret_cast<unsigned char*>(run.work + plan.mask);
  bool lines_on_device = false;              // the counts and the masks come from the device (else: every line is empty)
  if (nnz > 0) {
    // ---- the source as a canonical CSC in device memory, every index verified
    const long long* s_cptr = nullptr;
    const int* s_rows = nullptr;
    const double* s_val = nullptr;
    if (host_x) {
      long long* cp = tr.take_n<long long>((size_t)m + 1);
      int* ri = cp ? tr.take_n<int>(nnz) : nullptr;
      double* va = ri ? tr.take_n<double>(nnz) : nullptr;
      if (!va) return RESNMTF_ERR_ALLOC;
      e = hipMemcpyAsync(cp, j.x.col_ptr, ((size_t)m + 1) * sizeof(long long), hipMemcpyHostToDevice, st);
      if (e == hipSuccess) e = hipMemcpyAsync(ri, j.x.row_idx, nnz * sizeof(int), hipMemcpyHostToDevice, st);
      if (e == hipSuccess) e = hipMemcpyAsync(va, j.x.values, nnz * sizeof(double), hipMemcpyHostToDevice, st);
      if (e != hipSuccess) return run.fail(e);
      s_cptr = cp; s_rows = ri; s_val = va;
    } else {                                  // checked and sorted on the device; the stream is synchronised inside
      F64SpdView sv;
      F64SparseShape unused;
      if (int rc = fp64_build_sparse_device_view(st, tr, 0, j.x_dev, n, m, sv, unused, NAME)) return rc;
      tr.release(sv.rptr); tr.release(sv.ridx); tr.release(sv.perm);           // (the CSR half is not needed)
      s_cptr = sv.cptr; s_rows = sv.cidx; s_val = sv.cval;
    }
    // ---- the kept entries of every destination column, their scan, the empty lines; nnz_sub comes to the host
    e = hipMemcpyAsync(rows, j.rows, (size_t)ns * sizeof(int), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(cols, j.cols, (size_t)ms * sizeof(int), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemsetAsync(ints, 0, 4 * sizeof(int), st);
    if (e == hipSuccess) e = fp64_subsample_sparse_count(st, s_cptr, s_rows, s_val, rows, cols, n, ns, ms, inv_row, counts, scan, mask);
    if (e == hipSuccess) {
      hipLaunchKernelGGL(fp64_shuffle_sparse_count_kernel, dim3(f64_shuffle_sparse_grid((long long)ns + ms)), dim3(256), 0, st,
                         (const unsigned char*)mask, ns, ms, ints);
      e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(&host_nnz_sub, scan + ms, sizeof(long long), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(host_ints, ints, sizeof(host_ints), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && (j.row_mask || j.col_mask)) {
      host_mask.resize((size_t)ns + ms);
      e = hipMemcpyAsync(host_mask.data(), mask, host_mask.size(), hipMemcpyDeviceToHost, st);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return run.fail(e);
    lines_on_device = true;
    if (fill && host_nnz_sub > j.out_capacity) {             // known only now; nothing but *nnz_sub is written
      *j.nnz_sub = host_nnz_sub;
      return fp64_bad("out_capacity = " + std::to_string(j.out_capacity) + " is below nnz_sub = " + std::to_string(host_nnz_sub) +
                      " (the stored entries of the sub-sample; *nnz_sub is set)");
    }
    if (fill && host_nnz_sub > 0) {
      // ---- the kept entries as a COO, sorted into the canonical CSC by the same canonicaliser (the rows of a destination
      // column arrive in SOURCE row order).  It verifies the coordinates again before it uses them.
      const size_t kept = (size_t)host_nnz_sub;
      int* drow = tr.take_n<int>(kept);
      int* dcol = drow ? tr.take_n<int>(kept) : nullptr;
      double* dval = dcol ? tr.take_n<double>(kept) : nullptr;
      if (!dval) return RESNMTF_ERR_ALLOC;
      if ((e = fp64_subsample_sparse_emit(st, s_cptr, s_rows, s_val, cols, inv_row, ms, scan, drow, dcol, dval)) != hipSuccess)
        return run.fail(e);
      resnmtf_fp64_sparse_device_view coo{};
      coo.layout = RESNMTF_SPARSE_COO; coo.index_type = RESNMTF_INDEX_I32; coo.dtype = RESNMTF_DTYPE_F64;
      coo.ptr_or_rows = drow; coo.idx_or_cols = dcol; coo.values = dval; coo.nnz = host_nnz_sub;
      F64SpdView dv;
      F64SparseShape unused;
      if (int rc = fp64_build_sparse_device_view(st, tr, 0, coo, ns, ms, dv, unused, NAME)) return rc;
      for (const void* q : {(const void*)s_cptr, (const void*)s_rows, (const void*)s_val, (const void*)drow, (const void*)dcol,
                            (const void*)dval, (const void*)dv.rptr, (const void*)dv.ridx, (const void*)dv.perm})
        tr.release(q);                        // (the build has synchronised the stream: nothing reads these any more)
      // ---- the outputs: pointers, rows widened, values
      e = hipMemcpyAsync(j.out_col_ptr, dv.cptr, ((size_t)ms + 1) * sizeof(long long), hipMemcpyDeviceToDevice, st);
      if (e == hipSuccess) {
        fp64_shuffle_sparse_widen(st, dv.cidx, host_nnz_sub, j.out_row_idx);
        e = hipGetLastError();
      }
      if (e == hipSuccess) e = hipMemcpyAsync(j.out_values, dv.cval, kept * sizeof(double), hipMemcpyDeviceToDevice, st);
    } else if (fill) {                        // nothing kept: zero pointers (the scan's own), nothing of size zero launched
      e = hipMemcpyAsync(j.out_col_ptr, scan, ((size_t)ms + 1) * sizeof(long long), hipMemcpyDeviceToDevice, st);
    }
  } else {                                    // no stored entry: zero pointers, every line empty, nothing of size zero launched
    if (!host_x) {                            // (the pointers of a CSC / CSR view are still judged on the device)
      F64SpdView sv;
      F64SparseShape unused;
      if (int rc = fp64_build_sparse_device_view(st, tr, 0, j.x_dev, n, m, sv, unused, NAME)) return rc;
    }
    if (fill) e = hipMemsetAsync(j.out_col_ptr, 0, ((size_t)ms + 1) * sizeof(long long), st);
  }
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) return run.fail(e);
  if (!lines_on_device) {
    host_ints[0] = ns; host_ints[1] = ms;
    host_mask.assign((size_t)ns + ms, 1);
  }
  *j.nnz_sub = host_nnz_sub;
  *j.n_empty_rows = host_ints[0];
  *j.n_empty_cols = host_ints[1];
  if (j.row_mask) std::memcpy(j.row_mask, host_mask.data(), (size_t)ns);
  if (j.col_mask) std::memcpy(j.col_mask, host_mask.data() + ns, (size_t)ms);
  return RESNMTF_OK;
}

}  // extern "C"

// ---- resnmtf_fp64_init_svd: init_mats_inner (R/update_steps.r:78-125) in double precision ----
// The algorithm and its constants are resnmtf_init_svd's (resnmtf_hip.hip); tests/init_ref.py describes both.  A view's
// data come in through the run's own checks and uploads (fp64_checks, fp64_upload_view); its buffer is the run's layout
// of a one-view job whose k is the sketch width, so the products, the SpMM and the Gram find what they find in a run.
namespace {
const char* const F64_INIT_NAME = "fp64_init_svd";
constexpr double kF64InitRidge = 1e-14;     // times trace(C), round 0 of CholeskyQR2 (orthonormalise of resnmtf_init_svd)
constexpr double kF64InitRankCut = 2e-14;   // times trace(C): kRankCut of resnmtf_init_svd

inline int f64_init_width(int k) { return std::min(64, 16 * ((k + 8 + 15) / 16)); }

// device memory that goes with its scope
struct F64Block {
  F64Block() = default;
  F64Block(const F64Block&) = delete;
  F64Block& operator=(const F64Block&) = delete;
  ~F64Block() { if (p) (void)hipFree(p); }
  double* p = nullptr;
};

// where the results of one view lie in the results block, in doubles; the block holds them until every view is done
struct F64InitOut { size_t f = 0, s = 0, g = 0, lam = 0, mu = 0, cf = 0, cg = 0; };
// what waits on the host for the same reason
struct F64InitHost { std::vector<double> d, u, v; };

int f64_init_fail(F64Run& run, hipError_t e) { return run.fail(e, "fp64_init_svd: "); }

// C = Y^T Y (width x width) on the host: the run's Gram partials, reduced in workgroup order
int f64_init_gram(F64Run& run, const F64Layout& L1, const double* Y, int len, int width, std::vector<double>& C) {
  const int nblk = (len + F64_GRAM_ROWS - 1) / F64_GRAM_ROWS;
  F64GramArgs ga{};
  ga.A[0] = Y; ga.B[0] = Y; ga.part[0] = run.buf + L1.part0; ga.len = len; ga.k = width;
  hipLaunchKernelGGL(fp64_gram_kernel, dim3(nblk, 1), dim3(F64_THREADS), 0, run.st, ga);
  fp64_init_reduce(run.st, run.buf + L1.part0, nblk, width * width, run.buf + L1.kk);
  C.resize((size_t)width * width);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpyAsync(C.data(), run.buf + L1.kk, C.size() * sizeof(double), hipMemcpyDeviceToHost, run.st);
  if (e == hipSuccess) e = hipStreamSynchronize(run.st);
  return e == hipSuccess ? RESNMTF_OK : f64_init_fail(run, e);
}

// Q = Y M (M width x width, row-major, from the host)
int f64_init_apply_host(F64Run& run, const F64Layout& L1, const double* Y, int len, int width, const std::vector<double>& M, double* Q) {
  double* dM = run.buf + L1.kk + (size_t)width * width;
  hipError_t e = hipMemcpyAsync(dM, M.data(), M.size() * sizeof(double), hipMemcpyHostToDevice, run.st);
  if (e == hipSuccess) {
    fp64_init_apply(run.st, Y, len, width, dM, Q);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipStreamSynchronize(run.st);     // (M may go out of scope)
  return e == hipSuccess ? RESNMTF_OK : f64_init_fail(run, e);
}

// CholeskyQR2 with the ridge in round 0 and the rank cut in both: Y (in `a`) -> orthonormal columns (back in `a`, `b` is scratch)
int f64_init_orthonormalise(F64Run& run, const F64Layout& L1, int v, double* a, double* b, int len, int width) {
  std::vector<double> C, R, Ri;
  for (int round = 0; round < 2; ++round) {
    double* src = round == 0 ? a : b;
    double* dst = round == 0 ? b : a;
    if (int rc = f64_init_gram(run, L1, src, len, width, C)) return rc;
    double tr = 0.0;
    for (int i = 0; i < width; ++i) tr += C[(size_t)i * width + i];
    if (round == 0)
      for (int i = 0; i < width; ++i) C[(size_t)i * width + i] += kF64InitRidge * tr;
    const int kept = cholesky_upper(C, width, kF64InitRankCut * tr, R);
    if (kept < 0) return fp64_bad("fp64_init_svd: view " + std::to_string(v) + " holds entries that are not finite");
    if (kept == 0) return fp64_bad("fp64_init_svd: view " + std::to_string(v) + " is all zero");
    invert_upper(R, width, Ri);
    if (int rc = f64_init_apply_host(run, L1, src, len, width, Ri, dst)) return rc;
  }
  return RESNMTF_OK;
}

// the eigenpairs of the Gram C in descending order: d = sqrt of the eigenvalues, Ms the vectors, Mn the vectors over d
void f64_init_eigen(std::vector<double>& C, int width, std::vector<double>& d, std::vector<double>& Ms, std::vector<double>& Mn) {
  std::vector<double> W;
  jacobi_eigen(C, width, W);
  std::vector<int> order(width);
  for (int i = 0; i < width; ++i) order[i] = i;
  std::sort(order.begin(), order.end(), [&](int a, int b) { return C[(size_t)a * width + a] > C[(size_t)b * width + b]; });
  d.assign(width, 0.0); Ms.assign((size_t)width * width, 0.0); Mn.assign((size_t)width * width, 0.0);
  for (int j = 0; j < width; ++j) {
    const int src = order[j];
    d[j] = std::sqrt(std::max(C[(size_t)src * width + src], 0.0));
    for (int i = 0; i < width; ++i) {
      Ms[(size_t)i * width + j] = W[(size_t)i * width + src];
      Mn[(size_t)i * width + j] = d[j] > 0.0 ? W[(size_t)i * width + src] / d[j] : 0.0;
    }
  }
}

// one view: its data into a buffer of its own, the iteration (or the thin route), the finish into the results block
int f64_init_view(F64Job& J, F64Run& run, int v, const resnmtf_fp64_init& in, double* res, const F64InitOut& at, F64InitHost& hs) {
  const int n = J.j.n_rows[v], m = J.j.n_cols[v], k = J.j.k;
  const int L = f64_init_width(k);
  const bool thin = std::min(n, m) < L, tall = m <= n;
  const int width = thin ? std::min(n, m) : L;
  hipStream_t st = run.st;
  if (J.src[v] == F64Source::DeviceSparse)
    if (int rc = fp64_build_sparse_device_view(st, run.transient, v, J.spd->view[v], n, m, run.spdv[v], J.shapes[v], F64_INIT_NAME)) return rc;
  resnmtf_group_job one{};
  one.struct_size = (int)sizeof(resnmtf_group_job);
  one.n_views = 1; one.k = width; one.n_rows[0] = n; one.n_cols[0] = m;
  F64Source src1[RESNMTF_GROUP_MAX_VIEWS] = {};
  F64SparseShape sh1[RESNMTF_GROUP_MAX_VIEWS];
  src1[0] = J.src[v]; sh1[0] = J.shapes[v];
  F64Layout L1;
  fp64_layout(one, 1, L1, src1, sh1);
  J.L.vw[v] = L1.vw[0];                      // (what fp64_upload_view reads)
  const F64View& w = J.L.vw[v];
  const size_t bytes = L1.total * sizeof(double);
  size_t free_b = 0, total_b = 0;
  hipError_t e = hipMemGetInfo(&free_b, &total_b);
  if (e != hipSuccess) return f64_init_fail(run, e);
  if (bytes > free_b) {
    resnmtf_set_create_error("fp64_init_svd: " + std::to_string(bytes) + " bytes asked for (view " + std::to_string(v) +
                             ": its fp64 images or sparse copies, four sketch matrices, a product slab), " + std::to_string(free_b) +
                             " free on the device");
    return RESNMTF_ERR_ALLOC;
  }
  void* p = nullptr;
  if ((e = hipMalloc(&p, std::max<size_t>(bytes, 8))) != hipSuccess) {
    (void)hipGetLastError();
    resnmtf_set_create_error(std::string("fp64_init_svd: ") + hipGetErrorString(e) + " (" + std::to_string(bytes) + " bytes asked for)");
    return e == hipErrorOutOfMemory ? RESNMTF_ERR_ALLOC : RESNMTF_ERR_HIP;
  }
  double* buf = run.buf = static_cast<double*>(p);
  e = hipMemsetAsync(buf, 0, bytes, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  std::vector<double> img;
  if (e == hipSuccess) e = fp64_upload_view(J, run, v, img);
  if (e == hipSuccess && J.src[v] == F64Source::DeviceSparse) {
    e = hipStreamSynchronize(st);
    run.transient.release_all();
  }
  if (e != hipSuccess) return f64_init_fail(run, e);
  img = std::vector<double>();

  std::mt19937_64 gen(in.seed[v]);
  std::vector<double> d, Ms, Mn, C;
  const double *U = nullptr, *V = nullptr;     // n x width and m x width, column-major
  if (thin) {
    // the exact SVD through the Gram of the short side: Y = X (m <= n) or X^T, len x width, no sketch and no iteration
    const int len = tall ? n : m;
    double* Y = buf + L1.scratch;
    double* Yl = buf + L1.scratch2;
    if (w.sparse()) {
      fp64_init_densify(st, reinterpret_cast<const long long*>(buf + (tall ? w.cptr : w.rptr)),
                        reinterpret_cast<const int*>(buf + (tall ? w.cidx : w.ridx)), buf + (tall ? w.cval : w.rval), width, len, Y);
      e = hipGetLastError();
    } else {
      e = hipMemcpy2DAsync(Y, (size_t)len * sizeof(double), buf + (tall ? w.x : w.xt), (tall ? w.ldn : w.ldm) * sizeof(double),
                           (size_t)len * sizeof(double), (size_t)width, hipMemcpyDeviceToDevice, st);
    }
    if (e != hipSuccess) return f64_init_fail(run, e);
    if (int rc = f64_init_gram(run, L1, Y, len, width, C)) return rc;
    for (double x : C)
      if (x != x) return fp64_bad("fp64_init_svd: view " + std::to_string(v) + " holds entries that are not finite");
    f64_init_eigen(C, width, d, Ms, Mn);
    if (int rc = f64_init_apply_host(run, L1, Y, len, width, Mn, Yl)) return rc;            // the long-side vectors
    std::vector<double> short_cm((size_t)width * width);                                    // the short side's, column-major
    for (int i = 0; i < width; ++i)
      for (int j = 0; j < width; ++j) short_cm[(size_t)i + (size_t)j * width] = Ms[(size_t)i * width + j];
    double* Ws = buf + w.f;
    e = hipMemcpyAsync(Ws, short_cm.data(), short_cm.size() * sizeof(double), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return f64_init_fail(run, e);
    U = tall ? Yl : Ws;
    V = tall ? Ws : Yl;
  } else {
    double* Yn = buf + w.f;
    double* Zm = buf + w.g;
    double* Yn2 = buf + L1.scratch;
    double* Zm2 = buf + L1.scratch2;
    {  // Omega: m x L standard normal, drawn row by row as resnmtf_init_svd draws it
      std::normal_distribution<double> normal(0.0, 1.0);
      std::vector<double> omega((size_t)m * L);
      for (size_t j = 0; j < (size_t)m; ++j)
        for (int c = 0; c < L; ++c) omega[j + (size_t)c * m] = normal(gen);
      e = hipMemcpyAsync(Zm, omega.data(), omega.size() * sizeof(double), hipMemcpyHostToDevice, st);
      if (e == hipSuccess) e = hipStreamSynchronize(st);
      if (e != hipSuccess) return f64_init_fail(run, e);
    }
    auto product = [&](bool is_xg) {             // Y = X Z into Yn, or Z = X^T Q into Zm
      const double* O = is_xg ? Zm : Yn;
      const int contr = is_xg ? m : n, lines = is_xg ? n : m;
      const size_t ld = is_xg ? w.ldn : w.ldm;
      int splits;
      if (w.sparse()) {
        const F64SparsePlan& sp = is_xg ? w.sxg : w.sxtf;
        fp64_spmm(st, L, sp, reinterpret_cast<const long long*>(buf + (is_xg ? w.rptr : w.cptr)),
                  reinterpret_cast<const int*>(buf + (is_xg ? w.ridx : w.cidx)), buf + (is_xg ? w.rval : w.cval), O, contr, L,
                  buf + L1.ot, lines, ld, buf + L1.slab);
        splits = sp.splits;
      } else {
        const F64ProductPlan& pp = is_xg ? w.xg : w.xtf;
        fp64_product(st, L, pp, buf + (is_xg ? w.x : w.xt), ld, O, contr, L, is_xg ? w.mpad : w.npad, buf + L1.slab);
        splits = pp.splits;
      }
      fp64_init_slab_sum(st, L, buf + L1.slab, splits, ld, lines, is_xg ? Yn : Zm);
      return hipGetLastError();
    };
    const int n_power = in.n_power < 1 ? 3 : in.n_power;
    for (int it = 0; it < n_power; ++it) {
      if ((e = product(true)) != hipSuccess) return f64_init_fail(run, e);
      if (int rc = f64_init_orthonormalise(run, L1, v, Yn, Yn2, n, L)) return rc;
      if ((e = product(false)) != hipSuccess) return f64_init_fail(run, e);
      if (it + 1 < n_power)
        if (int rc = f64_init_orthonormalise(run, L1, v, Zm, Zm2, m, L)) return rc;
    }
    // Z = X^T Q = V Sigma Ut^T  ->  Z^T Z = Ut Sigma^2 Ut^T;  U = Q Ut,  V = Z Ut Sigma^-1
    if (int rc = f64_init_gram(run, L1, Zm, m, L, C)) return rc;
    f64_init_eigen(C, L, d, Ms, Mn);
    if (int rc = f64_init_apply_host(run, L1, Yn, n, L, Ms, Yn2)) return rc;
    if (int rc = f64_init_apply_host(run, L1, Zm, m, L, Mn, Zm2)) return rc;
    U = Yn2; V = Zm2;
  }

  // R/update_steps.r:93-115 on the k leading triplets; the noise in resnmtf_init_svd's draw order (column by column)
  std::vector<double> base((size_t)k * k);
  std::normal_distribution<double> noise(0.0, std::sqrt(in.sigma));                 // mvrnorm(k, 0, sigma I), :96-99
  for (int j = 0; j < k; ++j)
    for (int i = 0; i < k; ++i) {
      double sv = (i == j ? std::fabs(d[j]) : 0.0);                                 // :95
      if (in.sigma > 0.0) sv += std::fabs(noise(gen));
      base[(size_t)j * k + i] = sv;
    }
  double* dbase = buf + L1.kk + 2 * (size_t)width * width;
  e = hipMemcpyAsync(dbase, base.data(), base.size() * sizeof(double), hipMemcpyHostToDevice, st);
  if (e == hipSuccess) {
    F64InitFinishArgs fa{};
    fa.U = U; fa.V = V; fa.n = n; fa.m = m;
    fa.F0 = res + at.f; fa.G0 = res + at.g; fa.cf = res + at.cf; fa.cg = res + at.cg; fa.lam = res + at.lam; fa.mu = res + at.mu;
    fp64_init_finish(st, fa, k, dbase, res + at.s);
    e = hipGetLastError();
  }
  hs.d = d;
  if (in.basis_u[v]) {                       // the signed basis, asked for: the k leading columns
    hs.u.resize((size_t)n * k); hs.v.resize((size_t)m * k);
    if (e == hipSuccess) e = hipMemcpyAsync(hs.u.data(), U, hs.u.size() * sizeof(double), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(hs.v.data(), V, hs.v.size() * sizeof(double), hipMemcpyDeviceToHost, st);
  }
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) return f64_init_fail(run, e);
  (void)hipFree(run.buf);                    // the next view's buffer takes its place
  run.buf = nullptr;
  return RESNMTF_OK;
}

// the refusals of the outputs that need no device: all five of every view, none beyond; a basis whole or not at all
std::string f64_init_check_outputs(const resnmtf_group_job& j, const resnmtf_fp64_init& in) {
  auto view = [](int v) { return "view " + std::to_string(v) + ": "; };
  for (int v = 0; v < RESNMTF_GROUP_MAX_VIEWS; ++v) {
    const int five = (in.f0[v] ? 1 : 0) + (in.s0[v] ? 1 : 0) + (in.g0[v] ? 1 : 0) + (in.lambda0[v] ? 1 : 0) + (in.mu0[v] ? 1 : 0);
    const int four = (in.basis_u[v] ? 1 : 0) + (in.basis_v[v] ? 1 : 0) + (in.basis_d[v] ? 1 : 0) + (in.basis_n_d[v] ? 1 : 0);
    if (v >= j.n_views) {
      if (five || four || in.singular_values[v]) return view(v) + "an output is given beyond n_views";
      continue;
    }
    if (five != 5) return view(v) + "an output is NULL: f0, s0, g0, lambda0 and mu0 of every view";
    if (four != 0 && four != 4) return view(v) + "the basis is given in part: basis_u, basis_v, basis_d and basis_n_d, or none of them";
  }
  return "";
}
// ... and the one that asks the runtime: device outputs are device memory of device_id and hold their element counts
std::string f64_init_check_output_pointers(int device_id, const resnmtf_group_job& j, const resnmtf_fp64_init& in) {
  auto view = [](int v) { return "view " + std::to_string(v) + ": "; };
  if (!in.outputs_on_device) return "";
  for (int v = 0; v < j.n_views; ++v) {
    const size_t n = (size_t)j.n_rows[v], m = (size_t)j.n_cols[v], k = (size_t)j.k;
    struct Out { const char* name; const double* p; size_t count; };
    const Out outs[5] = {{"f0", in.f0[v], n * k}, {"s0", in.s0[v], k * k}, {"g0", in.g0[v], m * k}, {"lambda0", in.lambda0[v], k}, {"mu0", in.mu0[v], k}};
    for (const Out& o : outs) {
      bool beyond = false;
      if (!fp64_on_device(device_id, o.p, o.count * sizeof(double), beyond))
        return view(v) + "init->" + o.name + (beyond ? " reaches beyond its allocation" : " is not device memory of device " + std::to_string(device_id));
    }
  }
  return "";
}
}  // namespace

extern "C" {

int resnmtf_fp64_init_svd(int device_id, const resnmtf_group_job* job, const resnmtf_fp64_sparse* sp, const resnmtf_fp64_device* dev,
                          const resnmtf_fp64_sparse_device* spd, const resnmtf_fp64_init* init) {
  if (sp && sp->struct_size != (int)sizeof(resnmtf_fp64_sparse)) return fp64_bad("resnmtf_fp64_sparse struct_size mismatch");
  if (spd && spd->struct_size != (int)sizeof(resnmtf_fp64_sparse_device)) return fp64_bad("resnmtf_fp64_sparse_device struct_size mismatch");
  if (dev && dev->struct_size != (int)sizeof(resnmtf_fp64_device)) return fp64_bad("resnmtf_fp64_device struct_size mismatch");
  if (!job) return fp64_bad("job is NULL");
  if (!init) return fp64_bad("init is NULL");
  if (init->struct_size != (int)sizeof(resnmtf_fp64_init)) return fp64_bad("resnmtf_fp64_init struct_size mismatch");
  if (job->struct_size != (int)sizeof(resnmtf_group_job)) return fp64_bad("resnmtf_group_job struct_size mismatch");
  if (!std::isfinite(init->sigma) || init->sigma < 0.0) return fp64_bad("sigma must be finite and >= 0");
  // what is read of the job and of dev, and nothing else: the shapes, k and where the views are
  resnmtf_group_job jj{};
  double unused_err = 0.0;
  int unused_iters = 0;
  jj.struct_size = (int)sizeof(resnmtf_group_job);
  jj.n_views = job->n_views; jj.k = job->k; jj.n_iters = 1;
  std::memcpy(jj.n_rows, job->n_rows, sizeof(jj.n_rows));
  std::memcpy(jj.n_cols, job->n_cols, sizeof(jj.n_cols));
  std::memcpy(jj.x, job->x, sizeof(jj.x));
  jj.all_error = &unused_err; jj.err_capacity = 1; jj.iters_done = &unused_iters;
  resnmtf_fp64_device dd{};
  if (dev) {
    dd.struct_size = (int)sizeof(resnmtf_fp64_device);
    dd.stream = dev->stream;
    std::memcpy(dd.x, dev->x, sizeof(dd.x));
  }
  F64Job J{device_id, jj, sp, dev ? &dd : nullptr, spd, 0.0, 1, {}, {}, {}, {}};
  J.start_only = true;
  F64Block results;                         // (before the run: freed after the run's stream has been waited for)
  F64Run run;
  if (fp64_shapes_ok(jj)) {                 // (else the job's own checks refuse it below)
    const std::string why = f64_init_check_outputs(jj, *init);
    if (!why.empty()) return fp64_bad(why);
  }
  int rc = fp64_checks(J);
  if (rc != RESNMTF_OK) return rc;
  const std::string why = f64_init_check_output_pointers(device_id, jj, *init);
  if (!why.empty()) return fp64_bad(why);
  if ((rc = fp64_open_stream(J, run)) != RESNMTF_OK) return rc;

  const int V = jj.n_views, k = jj.k;
  F64InitOut at[RESNMTF_GROUP_MAX_VIEWS];
  size_t total = 0;
  for (int v = 0; v < V; ++v) {
    const size_t n = (size_t)jj.n_rows[v], m = (size_t)jj.n_cols[v], sk = (size_t)k;
    at[v].f = total; total += n * sk;
    at[v].s = total; total += sk * sk;
    at[v].g = total; total += m * sk;
    at[v].lam = total; total += sk;
    at[v].mu = total; total += sk;
    at[v].cf = total; total += sk;
    at[v].cg = total; total += sk;
  }
  size_t free_b = 0, total_b = 0;
  hipError_t e = hipMemGetInfo(&free_b, &total_b);
  if (e != hipSuccess) return f64_init_fail(run, e);
  if (total * sizeof(double) > free_b) {
    resnmtf_set_create_error("fp64_init_svd: " + std::to_string(total * sizeof(double)) + " bytes asked for (the initial factors of every view), " +
                             std::to_string(free_b) + " free on the device");
    return RESNMTF_ERR_ALLOC;
  }
  void* p = nullptr;
  if ((e = hipMalloc(&p, total * sizeof(double))) != hipSuccess) {
    (void)hipGetLastError();
    resnmtf_set_create_error(std::string("fp64_init_svd: ") + hipGetErrorString(e) + " (" + std::to_string(total * sizeof(double)) + " bytes asked for)");
    return e == hipErrorOutOfMemory ? RESNMTF_ERR_ALLOC : RESNMTF_ERR_HIP;
  }
  results.p = static_cast<double*>(p);

  std::vector<F64InitHost> hs((size_t)V);
  for (int v = 0; v < V; ++v)
    if ((rc = f64_init_view(J, run, v, *init, results.p, at[v], hs[(size_t)v])) != RESNMTF_OK) return rc;

  // every view is done: the outputs, device to device or through one host copy
  const resnmtf_fp64_init& in = *init;
  std::vector<double> host;
  if (in.outputs_on_device) {
    for (int v = 0; v < V && e == hipSuccess; ++v) {
      const size_t n = (size_t)jj.n_rows[v], m = (size_t)jj.n_cols[v], sk = (size_t)k;
      struct Piece { double* to; size_t from, count; };
      const Piece pieces[5] = {{in.f0[v], at[v].f, n * sk}, {in.s0[v], at[v].s, sk * sk}, {in.g0[v], at[v].g, m * sk},
                               {in.lambda0[v], at[v].lam, sk}, {in.mu0[v], at[v].mu, sk}};
      for (int q = 0; q < 5 && e == hipSuccess; ++q)
        e = hipMemcpyAsync(pieces[q].to, results.p + pieces[q].from, pieces[q].count * sizeof(double), hipMemcpyDeviceToDevice, run.st);
    }
  } else {
    host.resize(total);
    e = hipMemcpyAsync(host.data(), results.p, total * sizeof(double), hipMemcpyDeviceToHost, run.st);
  }
  if (e == hipSuccess) e = hipStreamSynchronize(run.st);
  if (e != hipSuccess) return f64_init_fail(run, e);
  for (int v = 0; v < V; ++v) {
    const size_t n = (size_t)jj.n_rows[v], m = (size_t)jj.n_cols[v], sk = (size_t)k;
    if (!in.outputs_on_device) {
      std::memcpy(in.f0[v], &host[at[v].f], n * sk * sizeof(double));
      std::memcpy(in.s0[v], &host[at[v].s], sk * sk * sizeof(double));
      std::memcpy(in.g0[v], &host[at[v].g], m * sk * sizeof(double));
      std::memcpy(in.lambda0[v], &host[at[v].lam], sk * sizeof(double));
      std::memcpy(in.mu0[v], &host[at[v].mu], sk * sizeof(double));
    }
    const F64InitHost& h = hs[(size_t)v];
    if (in.singular_values[v]) std::memcpy(in.singular_values[v], h.d.data(), sk * sizeof(double));
    if (in.basis_u[v]) {
      std::memcpy(in.basis_u[v], h.u.data(), h.u.size() * sizeof(double));
      std::memcpy(in.basis_v[v], h.v.data(), h.v.size() * sizeof(double));
      std::memcpy(in.basis_d[v], h.d.data(), h.d.size() * sizeof(double));
      *in.basis_n_d[v] = (int)h.d.size();
    }
  }
  return RESNMTF_OK;
}

}  // extern "C"
