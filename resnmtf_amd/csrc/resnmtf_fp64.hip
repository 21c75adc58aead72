// Device-wide fp64 factorisation (DESIGN.md sections 21 to 24): the host side of resnmtf_fp64_run, resnmtf_fp64_run_sparse,
// resnmtf_fp64_run_device, resnmtf_fp64_run_sparse_device and the two plan queries, and -- through resnmtf_fp64.hip.inc,
// resnmtf_fp64_sparse.hip.inc (sparse views), resnmtf_fp64_device.hip.inc (views and factors from device memory) and
// resnmtf_fp64_sparse_device.hip.inc (sparse views from device memory) -- their kernels.  A translation unit of its own: the kernels get a code object of their
// own and leave the main unit's device code as it was.  The job checks and the error text are the main unit's
// (resnmtf_internal.h): this entry and resnmtf_group_run refuse the same things with the same texts.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "resnmtf_hip.h"
#include "resnmtf_internal.h"
#include "resnmtf_fp64.hip.inc"
#include "resnmtf_fp64_sparse.hip.inc"
#include "resnmtf_fp64_device.hip.inc"
#include "resnmtf_fp64_sparse_device.hip.inc"

namespace {
struct DeviceBuffer {
  void* p = nullptr;
  ~DeviceBuffer() { if (p) (void)hipFree(p); }
};

inline size_t rup(size_t x, size_t a) { return (x + a - 1) / a * a; }

struct F64View {
  int n = 0, m = 0;
  size_t ldn = 0, mpad = 0;                // X: ldn x mpad, column-major (ldn = f64_ld(n), mpad = m to 64), zero-filled
  size_t ldm = 0, npad = 0;                // X^T: ldm x npad
  size_t x = 0, xt = 0, f = 0, g = 0;      // offsets in doubles
  F64ProductPlan xg, xtf, res;
  // a sparse view (section 22) keeps no images: CSC (columns of X, for X^T F) and CSR (rows, for X G), offsets in doubles
  bool sparse = false;
  size_t nnz = 0;
  size_t cptr = 0, cval = 0, cidx = 0, rptr = 0, rval = 0, ridx = 0;
  F64SparsePlan sxg, sxtf;                 // how X G cuts its rows, X^T F its columns
};

// what the layout needs to know of a sparse view: its stored entries and its longest row and column
struct F64SparseShape {
  bool sparse = false;
  size_t nnz = 0;
  long long longest_row = 0, longest_col = 0;
};

// the job's one device buffer, in doubles: [X, X^T per dense view, CSC and CSR per sparse view | F, G per view | S |
// lambda | mu] (uploaded) | the k x k work area | column sums, norms, errors | two scratch matrices | product slab |
// partials | error history | with a sparse view: the k x k slots of every view, the row-major operand | maps (ints)
struct F64Layout {
  int V = 0, k = 0, KP = 0, cap = 0;
  F64View vw[RESNMTF_GROUP_MAX_VIEWS];
  size_t out_begin = 0, out_end = 0;       // F, G, S, lambda, mu: one contiguous region, read back at the end
  size_t s = 0, lam = 0, mu = 0, kk = 0, cf = 0, cg = 0, norms = 0, errs = 0, scratch = 0, scratch2 = 0, slab = 0;
  size_t part0 = 0, part1 = 0, colf = 0, colg = 0, spart = 0, err = 0, slots = 0, ot = 0, maps = 0, total = 0;
  long long rmap[RESNMTF_GROUP_MAX_VIEWS][RESNMTF_GROUP_MAX_VIEWS];     // int offsets from the buffer base, -1 = NA
  long long cmap[RESNMTF_GROUP_MAX_VIEWS][RESNMTF_GROUP_MAX_VIEWS];
};

// the shapes alone pass (what fp64_layout may be called on); everything else is check_group_job's to say
bool fp64_shapes_ok(const resnmtf_group_job& j) {
  if (j.struct_size != (int)sizeof(resnmtf_group_job)) return false;
  if (j.n_views < 1 || j.n_views > RESNMTF_GROUP_MAX_VIEWS || j.k < 1 || j.k > RESNMTF_MAX_K || j.n_iters < 0) return false;
  for (int v = 0; v < j.n_views; ++v)
    if (j.n_rows[v] < 1 || j.n_cols[v] < 1 || j.k > j.n_rows[v] || j.k > j.n_cols[v]) return false;
  return true;
}

// bytes of the two images of every dense view, the bulk of the buffer, without overflow
long double fp64_image_bytes(const resnmtf_group_job& j, unsigned sparse_views) {
  long double b = 0;
  for (int v = 0; v < j.n_views; ++v) {
    if ((sparse_views >> v) & 1u) continue;
    const long double n = j.n_rows[v], m = j.n_cols[v];
    b += ((n + 63) * (m + 63) + (m + 63) * (n + 63)) * sizeof(double);
  }
  return b;
}

void fp64_layout(const resnmtf_group_job& j, int cap, F64Layout& L, const F64SparseShape* shapes = nullptr) {
  L.V = j.n_views; L.k = j.k; L.KP = f64_kp(j.k); L.cap = cap;
  const size_t k = (size_t)L.k, V = (size_t)L.V;
  size_t off = 0, big = 1, slab = 1, gram_blk = 1, col_blk = 1, spart = 1;
  bool any_sparse = false;
  for (int v = 0; v < L.V; ++v) {
    F64View& w = L.vw[v];
    w.n = j.n_rows[v]; w.m = j.n_cols[v];
    w.ldn = f64_ld(w.n); w.mpad = rup(w.m, F64_JC); w.ldm = f64_ld(w.m); w.npad = rup(w.n, F64_JC);
    if (shapes && shapes[v].sparse) {          // 24 bytes per stored entry plus the pointers; no image, no residual
      any_sparse = true;
      w.sparse = true; w.nnz = shapes[v].nnz;
      const size_t idx_doubles = (w.nnz + 1) / 2;
      w.cptr = off; off += (size_t)w.m + 1;
      w.cval = off; off += w.nnz;
      w.cidx = off; off += idx_doubles;
      w.rptr = off; off += (size_t)w.n + 1;
      w.rval = off; off += w.nnz;
      w.ridx = off; off += idx_doubles;
      w.sxg = f64_plan_sparse(shapes[v].longest_row);
      w.sxtf = f64_plan_sparse(shapes[v].longest_col);
      big = std::max(big, (size_t)std::max(w.n, w.m));
      slab = std::max(slab, std::max((size_t)w.sxg.splits * w.ldn, (size_t)w.sxtf.splits * w.ldm) * (size_t)L.KP);
      spart = std::max(spart, (w.nnz + F64_NORM_CHUNK - 1) / F64_NORM_CHUNK);
      continue;
    }
    w.x = off; off += w.ldn * w.mpad;
    w.xt = off; off += w.ldm * w.npad;
    w.xg = f64_plan_product(w.n, w.m);
    w.xtf = f64_plan_product(w.m, w.n);
    w.res = f64_plan_resid(w.n, w.m);
    big = std::max(big, (size_t)std::max(w.n, w.m));
    slab = std::max(slab, std::max((size_t)w.xg.splits * w.ldn, (size_t)w.xtf.splits * w.ldm) * (size_t)L.KP);
    spart = std::max(spart, (size_t)w.res.tiles * w.res.splits);
    spart = std::max(spart, (std::max(w.ldn * w.mpad, w.ldm * w.npad) + F64_NORM_CHUNK - 1) / F64_NORM_CHUNK);
  }
  gram_blk = (big + F64_GRAM_ROWS - 1) / F64_GRAM_ROWS;
  col_blk = (big + F64_UPD_ROWS - 1) / F64_UPD_ROWS;
  L.out_begin = off;
  for (int v = 0; v < L.V; ++v) {
    L.vw[v].f = off; off += (size_t)L.vw[v].n * k;
    L.vw[v].g = off; off += (size_t)L.vw[v].m * k;
  }
  L.s = off; off += V * k * k;
  L.lam = off; off += V * k;
  L.mu = off; off += V * k;
  L.out_end = off;
  L.kk = off; off += 4 * k * k;
  L.cf = off; off += V * k;
  L.cg = off; off += V * k;
  L.norms = off; off += RESNMTF_GROUP_MAX_VIEWS;
  L.errs = off; off += RESNMTF_GROUP_MAX_VIEWS;
  L.scratch = off; off += big * k;
  L.scratch2 = off; off += big * k;
  L.slab = off; off += slab;
  L.part0 = off; off += gram_blk * k * k;
  L.part1 = off; off += gram_blk * k * k;
  L.colf = off; off += col_blk * k;
  L.colg = off; off += col_blk * k;
  L.spart = off; off += spart;
  L.err = off; off += (size_t)cap;
  if (any_sparse) {
    L.slots = off; off += V * 3 * k * k;
    L.ot = off; off += big * (size_t)L.KP;
  }
  L.maps = off;
  size_t ioff = off * 2;
  for (int v = 0; v < RESNMTF_GROUP_MAX_VIEWS; ++v)
    for (int w = 0; w < RESNMTF_GROUP_MAX_VIEWS; ++w) {
      const bool pair = v < L.V && w < L.V && v != w;
      L.rmap[v][w] = pair && j.row_count[v][w] > 0 ? (long long)ioff : -1;
      if (L.rmap[v][w] >= 0) ioff += (size_t)L.vw[v].n;
      L.cmap[v][w] = pair && j.col_count[v][w] > 0 ? (long long)ioff : -1;
      if (L.cmap[v][w] >= 0) ioff += (size_t)L.vw[v].m;
    }
  L.total = (ioff + 1) / 2;
}

// numpy's pairwise sum of a column of a V x V restriction (as grp_vec_sum)
double fp64_col_sum(const double* r, int V, int v) {
  if (!r) return 0.0;
  const double* a = r + (size_t)v * V;       // column v of the column-major matrix: entries [w + v V] = r[w, v]
  if (V < 8) {
    double s = 0.0;
    for (int w = 0; w < V; ++w) s += a[w];
    return s;
  }
  return ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]));
}
bool fp64_all_zero(const double* r, int V) {
  if (!r) return true;
  for (int e = 0; e < V * V; ++e)
    if (r[e] != 0.0) return false;
  return true;
}

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
      if (w.sparse) {                        // the operand row-major, then the SpMM over the lines of this side
        fp64_spmm(st, KP, g_form ? w.sxtf : w.sxg, reinterpret_cast<const long long*>(buf + (g_form ? w.cptr : w.rptr)),
                  reinterpret_cast<const int*>(buf + (g_form ? w.cidx : w.ridx)), buf + (g_form ? w.cval : w.rval), O, m, k,
                  buf + L.ot, n, g_form ? w.ldm : w.ldn, buf + L.slab);
      } else {
        fp64_product(st, KP, g_form ? w.xtf : w.xg, buf + (g_form ? w.xt : w.x), g_form ? w.ldm : w.ldn, O, m, k,
                     g_form ? w.npad : w.mpad, buf + L.slab);
      }
      F64UpdArgs u{};
      u.n = n; u.k = k; u.KP = KP; u.V = V;
      u.nsplit = w.sparse ? (g_form ? w.sxtf.splits : w.sxg.splits) : (g_form ? w.xtf.splits : w.xg.splits);
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
    if (w.sparse) {                          // the three k x k matrices of the trace-form error, before update_s reuses kkA
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
    if (w.sparse) {                          // the trace form, all k x k (section 22): no pass over X
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
// what resnmtf_set_view_csc refuses on the host, for one n x m CSC structure (values NULL: the structure alone); the
// text of the refusal or "" when it is fine, and then the view's stored entries, longest row and longest column
std::string fp64_check_csc(int n, int m, const long long* col_ptr, const int* row_idx, const double* values,
                           F64SparseShape& sh) {
  if (!col_ptr || !row_idx) return "col_ptr / row_idx is NULL";
  if (col_ptr[0] != 0) return "col_ptr[0] must be 0 (0-based CSC)";
  for (int c = 0; c < m; ++c)
    if (col_ptr[c + 1] < col_ptr[c]) return "col_ptr is not monotone (column " + std::to_string(c) + ")";
  std::vector<long long> per_row((size_t)n, 0);
  long long longest_col = 0;
  for (int c = 0; c < m; ++c) {
    longest_col = std::max(longest_col, col_ptr[c + 1] - col_ptr[c]);
    for (long long e = col_ptr[c]; e < col_ptr[c + 1]; ++e) {
      const int i = row_idx[e];
      if (i < 0 || i >= n) return "row index out of range in column " + std::to_string(c);
      if (e > col_ptr[c] && i <= row_idx[e - 1])
        return "row indices must be strictly increasing within a column (column " + std::to_string(c) + ")";
      if (values) {
        if (!std::isfinite(values[e])) return "non-finite entry in column " + std::to_string(c);
        if (values[e] < 0.0) return "negative entry in column " + std::to_string(c);
      }
      ++per_row[(size_t)i];
    }
  }
  sh.sparse = true;
  sh.nnz = (size_t)col_ptr[m];
  sh.longest_col = longest_col;
  sh.longest_row = n > 0 ? *std::max_element(per_row.begin(), per_row.end()) : 0;
  return "";
}

// the CSR copy of a checked CSC structure by a counting sort: a row's entries in ascending column order
void fp64_csr_from_csc(int n, int m, const long long* col_ptr, const int* row_idx, const double* values,
                       std::vector<long long>& rp, std::vector<int>& ci, std::vector<double>& rv) {
  const size_t nnz = (size_t)col_ptr[m];
  rp.assign((size_t)n + 1, 0); ci.resize(nnz); rv.resize(nnz);
  for (size_t e = 0; e < nnz; ++e) ++rp[(size_t)row_idx[e] + 1];
  for (int i = 0; i < n; ++i) rp[(size_t)i + 1] += rp[(size_t)i];
  std::vector<long long> next(rp.begin(), rp.end() - 1);
  for (int c = 0; c < m; ++c)
    for (long long e = col_ptr[c]; e < col_ptr[c + 1]; ++e) {
      const size_t p = (size_t)next[(size_t)row_idx[e]]++;
      ci[p] = c; rv[p] = values[e];
    }
}

// ---- resnmtf_fp64_run_device: what it refuses before any allocation or launch ----
// what of a job comes from, and goes to, device memory
struct F64DeviceUse {
  unsigned views = 0, factors = 0;          // bit v: view v's data / its initial factors are device matrices
  bool out = false, state = false;          // the results / the raw state are written to device memory
};

inline size_t fp64_dtype_bytes(int dtype) { return dtype == RESNMTF_DTYPE_F64 ? 8 : dtype == RESNMTF_DTYPE_F32 ? 4 : 2; }

// the refusals that need no device: the text, or "" when the struct is fine (and then `use`)
std::string fp64_check_device_struct(const resnmtf_group_job& j, const resnmtf_fp64_device& d, unsigned sparse_views, F64DeviceUse& use) {
  if (d.struct_size != (int)sizeof(resnmtf_fp64_device)) return "resnmtf_fp64_device struct_size mismatch";
  if (j.struct_size != (int)sizeof(resnmtf_group_job) || j.n_views < 1 || j.n_views > RESNMTF_GROUP_MAX_VIEWS) return "";   // (the job check says it)
  const int V = j.n_views;
  auto view = [](int v) { return "view " + std::to_string(v) + ": "; };
  struct Field { const char* name; const resnmtf_device_matrix* m; };
  for (int v = 0; v < RESNMTF_GROUP_MAX_VIEWS; ++v) {
    const Field in[6] = {{"x", &d.x[v]}, {"f0", &d.f0[v]}, {"s0", &d.s0[v]}, {"g0", &d.g0[v]}, {"lambda0", &d.lambda0[v]}, {"mu0", &d.mu0[v]}};
    double* const out[10] = {d.f_out[v], d.s_out[v], d.g_out[v], d.lambda_out[v], d.mu_out[v],
                             d.state_f[v], d.state_s[v], d.state_g[v], d.state_lambda[v], d.state_mu[v]};
    if (v >= V) {
      for (const Field& f : in)
        if (f.m->ptr) return view(v) + "dev->" + f.name + " is given beyond n_views";
      for (double* p : out)
        if (p) return view(v) + "a device output is given beyond n_views";
      continue;
    }
    for (const Field& f : in) {
      if (!f.m->ptr) continue;
      if (f.m->dtype < RESNMTF_DTYPE_F64 || f.m->dtype > RESNMTF_DTYPE_BF16)
        return view(v) + "dev->" + f.name + " has an unknown dtype (" + std::to_string(f.m->dtype) + ")";
      if (f.m->row_stride < 0 || f.m->col_stride < 0) return view(v) + "dev->" + f.name + " has a negative stride";
    }
    const bool sparse = (sparse_views >> v) & 1u;
    if (d.x[v].ptr && j.x[v]) return view(v) + "x is given both in the job (job->x) and in device memory (dev->x): one of them must be NULL";
    if (d.x[v].ptr && sparse) return view(v) + "x is given both sparse (col_ptr) and in device memory (dev->x): one of them must be NULL";
    if (!d.x[v].ptr && !j.x[v] && !sparse) return view(v) + "x is given neither in the job (job->x) nor in device memory (dev->x)";
    if (d.x[v].ptr) use.views |= 1u << v;
    const int n_there = (d.f0[v].ptr ? 1 : 0) + (d.s0[v].ptr ? 1 : 0) + (d.g0[v].ptr ? 1 : 0);
    if (n_there != 0 && n_there != 3)
      return view(v) + "f0 / s0 / g0 are given partly in device memory (" + (d.f0[v].ptr ? "" : "dev->f0 ") + (d.s0[v].ptr ? "" : "dev->s0 ") +
             (d.g0[v].ptr ? "" : "dev->g0 ") + "NULL): all three of a view in one place";
    if (n_there == 3 && (j.f0[v] || j.s0[v] || j.g0[v] || j.lambda0[v] || j.mu0[v]))
      return view(v) + "f0 / s0 / g0 are given in device memory: job->f0 / s0 / g0 / lambda0 / mu0 must be NULL";
    if (n_there == 0 && (d.lambda0[v].ptr || d.mu0[v].ptr))
      return view(v) + "dev->lambda0 / dev->mu0 need f0 / s0 / g0 in device memory (dev->f0, dev->s0, dev->g0)";
    if (n_there == 3) use.factors |= 1u << v;
  }
  static const char* const names[10] = {"f_out", "s_out", "g_out", "lambda_out", "mu_out",
                                        "state_f", "state_s", "state_g", "state_lambda", "state_mu"};
  for (int set = 0; set < 2; ++set) {                  // each set of five: for every view of the job, or for none
    int given = 0, missing_v = -1, missing_f = -1;
    for (int v = 0; v < V; ++v) {
      double* const out[10] = {d.f_out[v], d.s_out[v], d.g_out[v], d.lambda_out[v], d.mu_out[v],
                               d.state_f[v], d.state_s[v], d.state_g[v], d.state_lambda[v], d.state_mu[v]};
      for (int f = 0; f < 5; ++f) {
        if (out[set * 5 + f]) ++given;
        else if (missing_v < 0) { missing_v = v; missing_f = set * 5 + f; }
      }
    }
    if (given != 0 && given != 5 * V)
      return view(missing_v) + "dev->" + names[missing_f] + " is NULL while other device " + (set ? "state outputs" : "outputs") +
             " are given: all five of every view, or none";
    (set ? use.state : use.out) = given != 0;
  }
  return "";
}

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
    struct Out { const char* name; const double* p; size_t count; };
    const Out out[10] = {{"f_out", d.f_out[v], n * kk}, {"s_out", d.s_out[v], kk * kk}, {"g_out", d.g_out[v], m * kk},
                         {"lambda_out", d.lambda_out[v], kk}, {"mu_out", d.mu_out[v], kk},
                         {"state_f", d.state_f[v], n * kk}, {"state_s", d.state_s[v], kk * kk}, {"state_g", d.state_g[v], m * kk},
                         {"state_lambda", d.state_lambda[v], kk}, {"state_mu", d.state_mu[v], kk}};
    for (int f = 0; f < 10; ++f) {
      if (!(f < 5 ? use.out : use.state)) continue;
      bool beyond = false;
      if (!fp64_on_device(device_id, out[f].p, out[f].count * sizeof(double), beyond)) return refusal(v, out[f].name, beyond);
    }
  }
  return "";
}

// ---- resnmtf_fp64_run_sparse_device (section 24): sparse views from device memory ----
inline bool fp64_spd_given(const resnmtf_fp64_sparse_device_view& c) {
  return c.layout || c.index_type || c.dtype || c.ptr_or_rows || c.idx_or_cols || c.values || c.nnz;
}

// the refusals that need no device: the text, or "" when every view of the job has its data in exactly one place and
// every sparse device view is well formed
std::string fp64_check_sparse_device_struct(const resnmtf_group_job& j, const resnmtf_fp64_sparse* sp, const resnmtf_fp64_device* dev,
                                            const resnmtf_fp64_sparse_device& d) {
  if (dev && dev->struct_size == (int)sizeof(resnmtf_fp64_device) && dev->stream != d.stream)
    return "dev->stream and spd->stream differ: both structs name the one stream the caller's work was enqueued on";
  if (j.struct_size != (int)sizeof(resnmtf_group_job) || j.n_views < 1 || j.n_views > RESNMTF_GROUP_MAX_VIEWS) return "";   // (the job check says it)
  auto view = [](int v) { return "view " + std::to_string(v) + ": "; };
  for (int v = 0; v < RESNMTF_GROUP_MAX_VIEWS; ++v) {
    const resnmtf_fp64_sparse_device_view& c = d.view[v];
    const bool given = fp64_spd_given(c);
    if (v >= j.n_views) {
      if (given) return view(v) + "spd->view is given beyond n_views";
      continue;
    }
    const bool in_job = j.x[v] != nullptr, in_sp = sp && sp->view[v].col_ptr, in_dev = dev && dev->x[v].ptr;
    const int places = (in_job ? 1 : 0) + (in_sp ? 1 : 0) + (in_dev ? 1 : 0) + (given ? 1 : 0);
    if (places > 1 && given)
      return view(v) + "x is given in two places, in sparse device arrays (spd->view) and " +
             (in_job ? "in the job (job->x)" : in_sp ? "as host CSC arrays (sp->view)" : "as a device matrix (dev->x)") +
             ": exactly one of job->x, sp, dev->x and spd";
    if (places == 0) return view(v) + "x is given in none of job->x, sp, dev->x and spd";
    if (!given) continue;
    const std::string w = view(v) + "spd->view: ";
    if (c.layout != RESNMTF_SPARSE_CSC && c.layout != RESNMTF_SPARSE_CSR && c.layout != RESNMTF_SPARSE_COO)
      return w + "unknown layout: one of RESNMTF_SPARSE_CSC / _CSR / _COO";
    if (c.index_type != RESNMTF_INDEX_I32 && c.index_type != RESNMTF_INDEX_I64) return w + "unknown index type: RESNMTF_INDEX_I32 or _I64";
    if (c.dtype != RESNMTF_DTYPE_F64 && c.dtype != RESNMTF_DTYPE_F32 && c.dtype != RESNMTF_DTYPE_F16 && c.dtype != RESNMTF_DTYPE_BF16)
      return w + "unknown dtype: one of RESNMTF_DTYPE_F64 / _F32 / _F16 / _BF16";
    if (c.nnz < 0) return w + "nnz is negative";
    const bool coo = c.layout == RESNMTF_SPARSE_COO;
    if ((!c.ptr_or_rows && !(coo && c.nnz == 0)) || ((!c.idx_or_cols || !c.values) && c.nnz > 0))
      return w + "ptr_or_rows / idx_or_cols / values is NULL";
  }
  return "";
}

// the refusals that ask the runtime: every array is device memory of device_id and holds its element count
std::string fp64_check_sparse_device_pointers(int device_id, const resnmtf_group_job& j, const resnmtf_fp64_sparse_device& d, unsigned spd_views) {
  for (int v = 0; v < j.n_views; ++v) {
    if (!((spd_views >> v) & 1u)) continue;
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
  F64Transient() = default;
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
      resnmtf_set_create_error("fp64_run: " + std::to_string(bytes) + " bytes asked for (the canonical arrays of a sparse view in device memory), " +
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
// error text set.
int fp64_build_sparse_device_view(hipStream_t st, F64Transient& tr, int v, const resnmtf_fp64_sparse_device_view& c, int n, int m,
                                  F64SpdView& out, F64SparseShape& sh) {
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
  if (rc == RESNMTF_ERR_HIP) resnmtf_set_create_error("fp64_run: view " + std::to_string(v) + ": " + why);
  if (rc != RESNMTF_OK) return rc;
  sh.sparse = true; sh.nnz = nnz; sh.longest_row = sh.longest_col = 0;
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
    resnmtf_set_create_error(std::string("fp64_run: view ") + std::to_string(v) + ": " + hipGetErrorString(e));
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
  if (sp && sp->struct_size != (int)sizeof(resnmtf_fp64_sparse)) {
    resnmtf_set_create_error("resnmtf_fp64_sparse struct_size mismatch");
    return RESNMTF_ERR_INVALID;
  }
  return fp64_run_impl(device_id, job, sp, nullptr, nullptr, tol, max_iters);
}

int resnmtf_fp64_run_device(int device_id, const resnmtf_group_job* job, const resnmtf_fp64_sparse* sp,
                            const resnmtf_fp64_device* dev, double tol, int max_iters) {
  if (sp && sp->struct_size != (int)sizeof(resnmtf_fp64_sparse)) {
    resnmtf_set_create_error("resnmtf_fp64_sparse struct_size mismatch");
    return RESNMTF_ERR_INVALID;
  }
  return fp64_run_impl(device_id, job, sp, dev, nullptr, tol, max_iters);
}

// res_nmtf_inner (R/main.r:32-140) with sparse views that are already in device memory (R/utils.r:416-419 densifies a sparse
// Matrix; these arrays stand for that matrix): resnmtf_fp64_run_device's body, the views of spd checked and sorted on the
// device first
int resnmtf_fp64_run_sparse_device(int device_id, const resnmtf_group_job* job, const resnmtf_fp64_sparse* sp,
                                   const resnmtf_fp64_device* dev, const resnmtf_fp64_sparse_device* spd, double tol, int max_iters) {
  if (sp && sp->struct_size != (int)sizeof(resnmtf_fp64_sparse)) {
    resnmtf_set_create_error("resnmtf_fp64_sparse struct_size mismatch");
    return RESNMTF_ERR_INVALID;
  }
  if (spd && spd->struct_size != (int)sizeof(resnmtf_fp64_sparse_device)) {
    resnmtf_set_create_error("resnmtf_fp64_sparse_device struct_size mismatch");
    return RESNMTF_ERR_INVALID;
  }
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
// step is resnmtf_fp64_run_device's.
int fp64_run_impl(int device_id, const resnmtf_group_job* job, const resnmtf_fp64_sparse* sp, const resnmtf_fp64_device* dev,
                  const resnmtf_fp64_sparse_device* spd, double tol, int max_iters) {
  auto bad = [](const std::string& msg) { resnmtf_set_create_error(msg); return RESNMTF_ERR_INVALID; };
  if (!job) return bad("job is NULL");
  if (max_iters < 1) return bad("max_iters must be >= 1");
  if (!std::isfinite(tol)) return bad("tol must be finite");
  const resnmtf_group_job& j = *job;
  unsigned sparse_views = 0;                // bit v: view v comes as CSC arrays
  if (sp)
    for (int v = 0; v < RESNMTF_GROUP_MAX_VIEWS; ++v)
      if (sp->view[v].col_ptr) sparse_views |= 1u << v;
  unsigned spd_views = 0;                   // bit v: view v comes as sparse arrays in device memory (section 24)
  if (spd)
    for (int v = 0; v < RESNMTF_GROUP_MAX_VIEWS; ++v)
      if (fp64_spd_given(spd->view[v])) spd_views |= 1u << v;
  // a shape no device holds is refused on its byte count before the data behind it is read
  if (fp64_shapes_ok(j)) {
    const long double img = fp64_image_bytes(j, sparse_views | spd_views);
    if (img >= 0x1p58L) {
      char text[160];
      std::snprintf(text, sizeof(text), "fp64_run: more than %.0Lf bytes asked for (the fp64 images of the views alone)", img);
      resnmtf_set_create_error(text);
      return RESNMTF_ERR_ALLOC;
    }
  }
  if (spd) {                                // (first: a view in two places or in none is named with all four of them)
    const std::string why = fp64_check_sparse_device_struct(j, sp, dev, *spd);
    if (!why.empty()) return bad(why);
  }
  F64DeviceUse use;                         // what comes from, and goes to, device memory (resnmtf_fp64_run_device)
  if (dev) {
    const std::string why = fp64_check_device_struct(j, *dev, sparse_views | spd_views, use);
    if (!why.empty()) return bad(why);
  }
  if (const char* why = resnmtf_check_fp64_job(j, max_iters, sparse_views | use.views | spd_views, use.factors, use.out)) return bad(why);
  if (sparse_views >> j.n_views) return bad("a sparse view is given beyond n_views");
  if (dev) {
    const std::string why = fp64_check_device_pointers(device_id, j, *dev, use);
    if (!why.empty()) return bad(why);
  }
  if (spd_views) {
    const std::string why = fp64_check_sparse_device_pointers(device_id, j, *spd, spd_views);
    if (!why.empty()) return bad(why);
  }
  F64SparseShape shapes[RESNMTF_GROUP_MAX_VIEWS];
  for (int v = 0; v < j.n_views; ++v) {
    if (!((sparse_views >> v) & 1u)) continue;
    const resnmtf_fp64_sparse_view& c = sp->view[v];
    if (!c.values) return bad("view " + std::to_string(v) + ": values is NULL");
    const std::string why = fp64_check_csc(j.n_rows[v], j.n_cols[v], c.col_ptr, c.row_idx, c.values, shapes[v]);
    if (!why.empty()) return bad("view " + std::to_string(v) + ": " + why);
  }

  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) { resnmtf_set_create_error("no HIP device"); return RESNMTF_ERR_NO_DEVICE; }
  if (device_id < 0 || device_id >= ndev) return bad("device_id out of range");
  hipError_t e = hipSetDevice(device_id);
  if (e != hipSuccess) { resnmtf_set_create_error(std::string("hipSetDevice: ") + hipGetErrorString(e)); return RESNMTF_ERR_HIP; }
  hipStream_t st = nullptr;
  // the sparse views in device memory (section 24): the layout needs their longest lines, so their canonical arrays are
  // built first, in transient memory, on the run's own stream, and copied into the job's buffer once that exists
  F64Transient transient;
  F64SpdView spdv[RESNMTF_GROUP_MAX_VIEWS];
  if (spd_views) {
    e = hipStreamCreateWithFlags(&st, hipStreamNonBlocking);
    if (e != hipSuccess) { resnmtf_set_create_error(std::string("hipStreamCreate: ") + hipGetErrorString(e)); return RESNMTF_ERR_HIP; }
    hipEvent_t ev = nullptr;
    e = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
    if (e == hipSuccess) {
      e = hipEventRecord(ev, static_cast<hipStream_t>(spd->stream));
      if (e == hipSuccess) e = hipStreamWaitEvent(st, ev, 0);
      (void)hipEventDestroy(ev);
    }
    int rc = RESNMTF_OK;
    if (e != hipSuccess) { resnmtf_set_create_error(std::string("fp64_run: ") + hipGetErrorString(e)); rc = RESNMTF_ERR_HIP; }
    for (int v = 0; v < j.n_views && rc == RESNMTF_OK; ++v)
      if ((spd_views >> v) & 1u) rc = fp64_build_sparse_device_view(st, transient, v, spd->view[v], j.n_rows[v], j.n_cols[v], spdv[v], shapes[v]);
    if (rc != RESNMTF_OK) {
      (void)hipStreamSynchronize(st);
      (void)hipStreamDestroy(st);
      return rc;
    }
  }

  const int cap = j.n_iters > 0 ? std::min(j.n_iters, max_iters) : max_iters;
  F64Layout L;
  fp64_layout(j, cap, L, (sparse_views | spd_views) ? shapes : nullptr);
  const size_t bytes = L.total * sizeof(double);
  auto drop_stream = [&]() { if (st) { (void)hipStreamSynchronize(st); (void)hipStreamDestroy(st); } };
  size_t free_b = 0, total_b = 0;
  e = hipMemGetInfo(&free_b, &total_b);
  if (e != hipSuccess) { drop_stream(); resnmtf_set_create_error(std::string("fp64_run: ") + hipGetErrorString(e)); return RESNMTF_ERR_HIP; }
  if (bytes > free_b) {
    drop_stream();
    resnmtf_set_create_error("fp64_run: " + std::to_string(bytes) + " bytes asked for (two fp64 images of every view, factors, slabs), " +
                     std::to_string(free_b) + " free on the device");
    return RESNMTF_ERR_ALLOC;
  }
  if (!st) e = hipStreamCreateWithFlags(&st, hipStreamNonBlocking);
  if (e != hipSuccess) { resnmtf_set_create_error(std::string("hipStreamCreate: ") + hipGetErrorString(e)); return RESNMTF_ERR_HIP; }
  DeviceBuffer owner;                      // (freed on every path out; hipFree waits for the stream's work)
  e = hipMalloc(&owner.p, std::max<size_t>(bytes, 8));
  double* buf = static_cast<double*>(owner.p);
  if (e != hipSuccess) {
    (void)hipStreamDestroy(st);
    resnmtf_set_create_error(std::string("fp64_run: ") + hipGetErrorString(e) + " (" + std::to_string(bytes) + " bytes asked for)");
    return e == hipErrorOutOfMemory ? RESNMTF_ERR_ALLOC : RESNMTF_ERR_HIP;
  }
  auto fail = [&](hipError_t err) {
    (void)hipStreamSynchronize(st);
    (void)hipStreamDestroy(st);
    resnmtf_set_create_error(std::string("fp64_run: ") + hipGetErrorString(err));
    return RESNMTF_ERR_HIP;
  };
  const int V = L.V, k = L.k;
  if (dev) {                                // the run's stream waits for what the caller's stream holds so far
    hipEvent_t ev = nullptr;
    e = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
    if (e == hipSuccess) {
      e = hipEventRecord(ev, static_cast<hipStream_t>(dev->stream));
      if (e == hipSuccess) e = hipStreamWaitEvent(st, ev, 0);
      (void)hipEventDestroy(ev);            // (released once the recorded work completes)
    }
    if (e != hipSuccess) return fail(e);
  }
  e = hipMemsetAsync(buf, 0, bytes, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) return fail(e);

  // upload: the padded images view by view (one staging vector), then the initial state and the maps
  {
    std::vector<double> img;
    for (int v = 0; v < V && e == hipSuccess; ++v) {
      const F64View& w = L.vw[v];
      if ((spd_views >> v) & 1u) {           // from device memory (section 24): the canonical arrays device to device, the
        const F64SpdView& c = spdv[v];       // CSR values gathered in fp64; nnz = 0: the zeros of the memset are the view
        if (w.nnz == 0) continue;
        e = hipMemcpyAsync(buf + w.cptr, c.cptr, ((size_t)w.m + 1) * sizeof(long long), hipMemcpyDeviceToDevice, st);
        if (e == hipSuccess) e = hipMemcpyAsync(buf + w.rptr, c.rptr, ((size_t)w.n + 1) * sizeof(long long), hipMemcpyDeviceToDevice, st);
        if (e == hipSuccess) e = hipMemcpyAsync(buf + w.cval, c.cval, w.nnz * sizeof(double), hipMemcpyDeviceToDevice, st);
        if (e == hipSuccess) e = hipMemcpyAsync(buf + w.cidx, c.cidx, w.nnz * sizeof(int), hipMemcpyDeviceToDevice, st);
        if (e == hipSuccess) e = hipMemcpyAsync(buf + w.ridx, c.ridx, w.nnz * sizeof(int), hipMemcpyDeviceToDevice, st);
        if (e == hipSuccess) {
          fp64_spd_gather(st, c.perm, c.cval, (long long)w.nnz, buf + w.rval);
          e = hipGetLastError();
        }
        continue;
      }
      if (w.sparse) {                        // the CSC arrays as given, and the CSR copy built here
        const resnmtf_fp64_sparse_view& c = sp->view[v];
        std::vector<long long> rp;
        std::vector<int> ci;
        std::vector<double> rv;
        fp64_csr_from_csc(w.n, w.m, c.col_ptr, c.row_idx, c.values, rp, ci, rv);
        e = hipMemcpy(buf + w.cptr, c.col_ptr, ((size_t)w.m + 1) * sizeof(long long), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(buf + w.rptr, rp.data(), rp.size() * sizeof(long long), hipMemcpyHostToDevice);
        if (w.nnz > 0) {
          if (e == hipSuccess) e = hipMemcpy(buf + w.cval, c.values, w.nnz * sizeof(double), hipMemcpyHostToDevice);
          if (e == hipSuccess) e = hipMemcpy(buf + w.cidx, c.row_idx, w.nnz * sizeof(int), hipMemcpyHostToDevice);
          if (e == hipSuccess) e = hipMemcpy(buf + w.rval, rv.data(), w.nnz * sizeof(double), hipMemcpyHostToDevice);
          if (e == hipSuccess) e = hipMemcpy(buf + w.ridx, ci.data(), w.nnz * sizeof(int), hipMemcpyHostToDevice);
        }
        continue;
      }
      if ((use.views >> v) & 1u) {           // from device memory: one read, both images, no staging (section 23)
        fp64_images(st, dev->x[v], w.n, w.m, buf + w.x, w.ldn, buf + w.xt, w.ldm);
        e = hipGetLastError();
        continue;
      }
      const double* x = j.x[v];
      const size_t n = (size_t)w.n, m = (size_t)w.m;
      img.assign(w.ldn * w.mpad, 0.0);
      for (size_t c = 0; c < m; ++c) std::memcpy(&img[c * w.ldn], x + c * n, n * sizeof(double));
      e = hipMemcpy(buf + w.x, img.data(), img.size() * sizeof(double), hipMemcpyHostToDevice);
      if (e != hipSuccess) break;
      img.assign(w.ldm * w.npad, 0.0);
      for (size_t c = 0; c < m; ++c)
        for (size_t i = 0; i < n; ++i) img[c + i * w.ldm] = x[i + c * n];
      e = hipMemcpy(buf + w.xt, img.data(), img.size() * sizeof(double), hipMemcpyHostToDevice);
    }
  }
  if (e == hipSuccess && spd_views) {       // the job's buffer holds the views: their transient arrays go
    e = hipStreamSynchronize(st);
    transient.release_all();
  }
  if (e != hipSuccess) return fail(e);
  std::vector<double> host(L.out_end - L.out_begin, 0.0);
  auto at = [&](size_t off) { return host.data() + (off - L.out_begin); };
  for (int v = 0; v < V; ++v) {
    if ((use.factors >> v) & 1u) continue;  // (from device memory, below)
    const size_t n = (size_t)L.vw[v].n, m = (size_t)L.vw[v].m;
    std::memcpy(at(L.vw[v].f), j.f0[v], n * k * sizeof(double));
    std::memcpy(at(L.vw[v].g), j.g0[v], m * k * sizeof(double));
    std::memcpy(at(L.s + (size_t)v * k * k), j.s0[v], (size_t)k * k * sizeof(double));
    for (int c = 0; c < k; ++c) {                                         // explicit init: colSums (R/update_steps.r:55-56)
      double cf = 0.0, cg = 0.0;
      if (!j.lambda0[v]) for (size_t i = 0; i < n; ++i) cf += j.f0[v][i + (size_t)c * n];
      if (!j.mu0[v]) for (size_t i = 0; i < m; ++i) cg += j.g0[v][i + (size_t)c * m];
      *at(L.lam + (size_t)v * k + c) = j.lambda0[v] ? j.lambda0[v][c] : cf;
      *at(L.mu + (size_t)v * k + c) = j.mu0[v] ? j.mu0[v][c] : cg;
    }
  }
  if (!use.factors) {
    e = hipMemcpy(buf + L.out_begin, host.data(), host.size() * sizeof(double), hipMemcpyHostToDevice);
  } else {                                  // the host views' pieces alone; the others are written by kernels on the stream
    for (int v = 0; v < V && e == hipSuccess; ++v) {
      if ((use.factors >> v) & 1u) continue;
      const size_t fg = ((size_t)L.vw[v].n + L.vw[v].m) * k;               // F and G of a view are neighbours
      const size_t pieces[4][2] = {{L.vw[v].f, fg}, {L.s + (size_t)v * k * k, (size_t)k * k}, {L.lam + (size_t)v * k, (size_t)k},
                                   {L.mu + (size_t)v * k, (size_t)k}};
      for (int p = 0; p < 4 && e == hipSuccess; ++p)
        e = hipMemcpy(buf + pieces[p][0], at(pieces[p][0]), pieces[p][1] * sizeof(double), hipMemcpyHostToDevice);
    }
    for (int v = 0; v < V && e == hipSuccess; ++v) {
      if (!((use.factors >> v) & 1u)) continue;
      const F64View& w = L.vw[v];
      double* lam = buf + L.lam + (size_t)v * k;
      double* mu = buf + L.mu + (size_t)v * k;
      fp64_factors_in(st, dev->f0[v], w.n, k, buf + w.f);
      fp64_factors_in(st, dev->s0[v], k, k, buf + L.s + (size_t)v * k * k);
      fp64_factors_in(st, dev->g0[v], w.m, k, buf + w.g);
      for (int side = 0; side < 2; ++side) {                               // given: a k x 1 matrix (col_stride is not read)
        resnmtf_device_matrix vec = side ? dev->mu0[v] : dev->lambda0[v];
        vec.col_stride = vec.row_stride;
        if (vec.ptr) fp64_factors_in(st, vec, k, 1, side ? mu : lam);
      }
      if (!dev->lambda0[v].ptr || !dev->mu0[v].ptr)                        // not given: colSums (R/update_steps.r:55-56)
        hipLaunchKernelGGL(fp64_colsum_seq_kernel, dim3(2), dim3(64), 0, st, (const double*)(buf + w.f), w.n,
                           dev->lambda0[v].ptr ? nullptr : lam, (const double*)(buf + w.g), w.m, dev->mu0[v].ptr ? nullptr : mu, k);
      e = hipGetLastError();
    }
  }
  if (e != hipSuccess) return fail(e);
  if (L.total > L.maps) {
    std::vector<int> maps((L.total - L.maps) * 2, -1);
    const size_t ibase = L.maps * 2;
    for (int v = 0; v < V; ++v)
      for (int w = 0; w < V; ++w) {
        if (L.rmap[v][w] >= 0)
          for (int p = 0; p < j.row_count[v][w]; ++p) maps[(size_t)L.rmap[v][w] - ibase + j.row_idx_v[v][w][p]] = j.row_idx_w[v][w][p];
        if (L.cmap[v][w] >= 0)
          for (int p = 0; p < j.col_count[v][w]; ++p) maps[(size_t)L.cmap[v][w] - ibase + j.col_idx_v[v][w][p]] = j.col_idx_w[v][w][p];
      }
    e = hipMemcpy(buf + L.maps, maps.data(), maps.size() * sizeof(int), hipMemcpyHostToDevice);
    if (e != hipSuccess) return fail(e);
  }

  // ||X_v||_F^2 as norm()^2 (R/main.r:48)
  for (int v = 0; v < V; ++v) {
    const F64View& w = L.vw[v];
    // (a sparse view: over the CSC values, the image's non-zeros in entry order)
    const size_t total = w.sparse ? w.nnz : w.ldn * w.mpad;
    const int nb = (int)((total + F64_NORM_CHUNK - 1) / F64_NORM_CHUNK);
    if (nb > 0)
      hipLaunchKernelGGL(fp64_norm_kernel, dim3(nb), dim3(F64_THREADS), 0, st, (const double*)(buf + (w.sparse ? w.cval : w.x)),
                         total, buf + L.spart);
    F64KKArgs kk{};
    kk.mode = F64_KK_NORM; kk.k = k; kk.V = V; kk.v = v; kk.part_a = buf + L.spart; kk.nblk_a = nb;
    kk.S = buf + L.s; kk.norms = buf + L.norms; kk.errs = buf + L.errs; kk.err_out = buf + L.err;
    hipLaunchKernelGGL(fp64_kk_kernel, dim3(1), dim3(F64_THREADS), 0, st, kk);
  }
  e = hipGetLastError();
  if (e != hipSuccess) return fail(e);

  // the loop of R/main.r:53-80.  A fixed count is enqueued whole; in convergence mode the 8-byte mean error comes back
  // after every sweep and the host applies the stop rule, so the state on the device is the stop sweep's own
  int it = 0;
  double err_temp = 0.0;
  while (it < cap) {
    fp64_enqueue_sweep(st, j, L, buf, it);
    e = hipGetLastError();
    if (e != hipSuccess) return fail(e);
    ++it;
    if (j.n_iters == 0) {
      double mean = 0.0;
      e = hipMemcpyAsync(&mean, buf + L.err + (it - 1), sizeof(double), hipMemcpyDeviceToHost, st);
      if (e == hipSuccess) e = hipStreamSynchronize(st);
      if (e != hipSuccess) return fail(e);
      const double diff = std::fabs(mean - err_temp);
      err_temp = mean;
      if (!(diff > tol)) break;
    }
  }
  // the raw state, as a later call resumes from it, and the normalised results: device to device, on the run's stream
  auto copy_out = [&](int v, double* f, double* s, double* g, double* lam, double* mu) {
    const F64View& w = L.vw[v];
    const size_t kk = (size_t)k;
    hipError_t c = hipMemcpyAsync(f, buf + w.f, (size_t)w.n * kk * sizeof(double), hipMemcpyDeviceToDevice, st);
    if (c == hipSuccess) c = hipMemcpyAsync(s, buf + L.s + (size_t)v * kk * kk, kk * kk * sizeof(double), hipMemcpyDeviceToDevice, st);
    if (c == hipSuccess) c = hipMemcpyAsync(g, buf + w.g, (size_t)w.m * kk * sizeof(double), hipMemcpyDeviceToDevice, st);
    if (c == hipSuccess) c = hipMemcpyAsync(lam, buf + L.lam + (size_t)v * kk, kk * sizeof(double), hipMemcpyDeviceToDevice, st);
    if (c == hipSuccess) c = hipMemcpyAsync(mu, buf + L.mu + (size_t)v * kk, kk * sizeof(double), hipMemcpyDeviceToDevice, st);
    return c;
  };
  if (use.state)
    for (int v = 0; v < V; ++v) {
      e = copy_out(v, dev->state_f[v], dev->state_s[v], dev->state_g[v], dev->state_lambda[v], dev->state_mu[v]);
      if (e != hipSuccess) return fail(e);
    }
  for (int v = 0; v < V; ++v) {            // normalisation_check (R/utils.r:176-195)
    const F64View& w = L.vw[v];
    const size_t total = ((size_t)w.n + w.m + k) * k;
    const int nb = (int)std::min<size_t>((total + F64_THREADS - 1) / F64_THREADS, 4096);
    hipLaunchKernelGGL(fp64_normalise_kernel, dim3(nb), dim3(F64_THREADS), 0, st, buf + w.f, buf + w.g,
                       buf + L.s + (size_t)v * k * k, (const double*)(buf + L.cf + (size_t)v * k),
                       (const double*)(buf + L.cg + (size_t)v * k), w.n, w.m, k);
  }
  e = hipGetLastError();
  std::vector<double> errs((size_t)it);
  bool to_host = !use.out;                  // with device outputs the host copy is made only for a host pointer that is set
  for (int v = 0; v < V; ++v) {
    if (use.out && e == hipSuccess) e = copy_out(v, dev->f_out[v], dev->s_out[v], dev->g_out[v], dev->lambda_out[v], dev->mu_out[v]);
    to_host = to_host || j.f_out[v] || j.s_out[v] || j.g_out[v] || j.lambda_out[v] || j.mu_out[v];
  }
  if (e == hipSuccess && to_host)
    e = hipMemcpyAsync(host.data(), buf + L.out_begin, host.size() * sizeof(double), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess && it > 0) e = hipMemcpyAsync(errs.data(), buf + L.err, errs.size() * sizeof(double), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) return fail(e);
  (void)hipStreamDestroy(st);
  for (int v = 0; v < V; ++v) {            // (a host pointer may be NULL only beside device outputs)
    if (j.f_out[v]) std::memcpy(j.f_out[v], at(L.vw[v].f), (size_t)L.vw[v].n * k * sizeof(double));
    if (j.g_out[v]) std::memcpy(j.g_out[v], at(L.vw[v].g), (size_t)L.vw[v].m * k * sizeof(double));
    if (j.s_out[v]) std::memcpy(j.s_out[v], at(L.s + (size_t)v * k * k), (size_t)k * k * sizeof(double));
    if (j.lambda_out[v]) std::memcpy(j.lambda_out[v], at(L.lam + (size_t)v * k), (size_t)k * sizeof(double));
    if (j.mu_out[v]) std::memcpy(j.mu_out[v], at(L.mu + (size_t)v * k), (size_t)k * sizeof(double));
  }
  for (int t = 0; t < it; ++t) j.all_error[t] = errs[(size_t)t];
  *j.iters_done = it;
  return RESNMTF_OK;
}
}  // namespace
