// The host-only description of a device-wide fp64 job: the shape constants and shape-only plans of
// the fp64 kernels, where each view's data come from, the layout of the job's one device buffer, the CSC check and the
// CSR build, and the struct checks that need no device.  No HIP: it compiles with a plain C++17 compiler against
// include/resnmtf_hip.h alone, which is how tests/host/fp64_job_check.cpp runs it.  The kernel files include it for the
// constants and plans; resnmtf_fp64.hip for everything.
#ifndef RESNMTF_FP64_JOB_H
#define RESNMTF_FP64_JOB_H

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <string>
#include <vector>

#include "resnmtf_hip.h"

#ifdef __HIPCC__
#define F64_HD __host__ __device__
#else
#define F64_HD
#endif

#define F64_THREADS 256
#define F64_ROWS 128          // rows of a product workgroup: 4 waves x two 16-row MFMA tiles
#define F64_JC 64             // contraction indices per LDS stage of the product (X's columns are padded to this)
#define F64_TARGET_WGS 512    // workgroups a product or residual launch aims for (a constant: the split count must
                              // depend on (n, m, k) alone, never on the device)
#define F64_GRAM_ROWS 256     // rows per workgroup of the Gram partials
#define F64_UPD_ROWS 64       // rows (= threads) per workgroup of the row-local kernels
#define F64_RES_ROWS 64       // rows per workgroup of the residual
#define F64_NORM_CHUNK (F64_THREADS * 64)
#define F64_SP_PIECE 256       // stored entries a line piece aims for: a line longer than this is cut
#define F64_SP_MAX_SPLITS 16    // at most this many pieces (= slab splits) per line

F64_HD inline int f64_kp(int k) { return (k + 15) / 16 * 16; }

// leading dimension of an image with `rows` rows: a multiple of 32 (two 16-row MFMA tiles per wave, 16-byte row pairs),
// kept off the multiples of 1024 -- with a power-of-two column stride the columns a launch reads together fall on the
// same memory channels (a precaution: its effect is within the noise of the measurements)
inline size_t f64_ld(size_t rows) {
  const size_t ld = (rows + 31) / 32 * 32;
  return ld % 1024 == 0 ? ld + 32 : ld;
}

// launch geometry of one tall-skinny product (rows x contr) . (contr x k): row tiles, contraction splits, indices per
// split.  A function of the shapes alone.
struct F64ProductPlan { int tiles, splits, chunk; };
inline F64ProductPlan f64_plan_product(int rows, int contr) {
  F64ProductPlan p;
  p.tiles = (rows + F64_ROWS - 1) / F64_ROWS;
  const int stages = (contr + F64_JC - 1) / F64_JC;
  int splits = std::min(stages, std::max(1, F64_TARGET_WGS / p.tiles));
  const int per = (stages + splits - 1) / splits;
  p.splits = (stages + per - 1) / per;
  p.chunk = per * F64_JC;
  return p;
}
// the residual: 64-row tiles, the columns of X split in whole 16-column MFMA tiles (at least 4 per split: one per wave)
inline F64ProductPlan f64_plan_resid(int n, int m) {
  F64ProductPlan p;
  p.tiles = (n + F64_RES_ROWS - 1) / F64_RES_ROWS;
  const int jt = (m + 15) / 16;
  int splits = std::min((jt + 3) / 4, std::max(1, F64_TARGET_WGS / p.tiles));
  const int per = (jt + splits - 1) / splits;
  p.splits = (jt + per - 1) / per;
  p.chunk = per * 16;
  return p;
}

// lanes that own one line piece: KP of them where KP divides the wave (16, 32), else the whole wave (48, 64)
F64_HD constexpr int f64_sp_group(int KP) { return KP == 16 ? 16 : (KP == 32 ? 32 : 64); }

// how one SpMM cuts its lines: `splits` pieces of `piece` entries each.  Piece s of a line of len entries holds its
// entries [s piece, min((s + 1) piece, len)): a line of at most `piece` entries is whole in split 0 and zero in the
// others.  A function of the longest line alone (so of the pointer array), never of the device.
struct F64SparsePlan { int splits; long long piece, longest; };
inline F64SparsePlan f64_plan_sparse(long long longest) {
  F64SparsePlan p;
  p.longest = longest;
  const long long want = (longest + F64_SP_PIECE - 1) / F64_SP_PIECE;
  p.splits = (int)std::max<long long>(1, std::min<long long>(F64_SP_MAX_SPLITS, want));
  p.piece = std::max<long long>(1, (longest + p.splits - 1) / p.splits);
  return p;
}

// ---- where the data of a view are: exactly one of four places, resolved once per view (fp64_resolve_sources) ----
enum class F64Source {
  HostDense,      // job->x[v]
  HostCsc,        // sp->view[v] (section 22)
  DeviceDense,    // dev->x[v] (section 23)
  DeviceSparse    // spd->view[v] (section 24)
};
inline bool f64_is_sparse(F64Source s) { return s == F64Source::HostCsc || s == F64Source::DeviceSparse; }

inline bool fp64_spd_given(const resnmtf_fp64_sparse_device_view& c) {
  return c.layout || c.index_type || c.dtype || c.ptr_or_rows || c.idx_or_cols || c.values || c.nnz;
}

// The source of every view slot, those beyond n_views included (a view given there is refused by the checks).  sp and
// spd have passed their struct-size checks; dev is read only when its size is right (the struct check refuses it
// otherwise).  A view given in two places resolves to the sparser one, and the struct checks refuse it before anything
// is read through the answer.
inline void fp64_resolve_sources(const resnmtf_fp64_sparse* sp, const resnmtf_fp64_device* dev,
                                 const resnmtf_fp64_sparse_device* spd, F64Source* src) {
  const bool dev_ok = dev && dev->struct_size == (int)sizeof(resnmtf_fp64_device);
  for (int v = 0; v < RESNMTF_GROUP_MAX_VIEWS; ++v)
    src[v] = spd && fp64_spd_given(spd->view[v]) ? F64Source::DeviceSparse
             : sp && sp->view[v].col_ptr         ? F64Source::HostCsc
             : dev_ok && dev->x[v].ptr           ? F64Source::DeviceDense
                                                 : F64Source::HostDense;
}
// bit v: job->x[v] must be NULL, the view comes from elsewhere (what resnmtf_check_fp64_job takes as x_elsewhere)
inline unsigned fp64_x_elsewhere(const F64Source* src) {
  unsigned mask = 0;
  for (int v = 0; v < RESNMTF_GROUP_MAX_VIEWS; ++v)
    if (src[v] != F64Source::HostDense) mask |= 1u << v;
  return mask;
}

inline size_t rup(size_t x, size_t a) { return (x + a - 1) / a * a; }

struct F64View {
  int n = 0, m = 0;
  size_t ldn = 0, mpad = 0;                // X: ldn x mpad, column-major (ldn = f64_ld(n), mpad = m to 64), zero-filled
  size_t ldm = 0, npad = 0;                // X^T: ldm x npad
  size_t x = 0, xt = 0, f = 0, g = 0;      // offsets in doubles
  F64ProductPlan xg, xtf, res;
  // a sparse view (section 22) keeps no images: CSC (columns of X, for X^T F) and CSR (rows, for X G), offsets in doubles
  F64Source src = F64Source::HostDense;
  bool sparse() const { return f64_is_sparse(src); }
  size_t nnz = 0;
  size_t cptr = 0, cval = 0, cidx = 0, rptr = 0, rval = 0, ridx = 0;
  F64SparsePlan sxg, sxtf;                 // how X G cuts its rows, X^T F its columns
};

// what the layout needs to know of a sparse view: its stored entries and its longest row and column
struct F64SparseShape {
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
inline bool fp64_shapes_ok(const resnmtf_group_job& j) {
  if (j.struct_size != (int)sizeof(resnmtf_group_job)) return false;
  if (j.n_views < 1 || j.n_views > RESNMTF_GROUP_MAX_VIEWS || j.k < 1 || j.k > RESNMTF_MAX_K || j.n_iters < 0) return false;
  for (int v = 0; v < j.n_views; ++v)
    if (j.n_rows[v] < 1 || j.n_cols[v] < 1 || j.k > j.n_rows[v] || j.k > j.n_cols[v]) return false;
  return true;
}

// bytes of the two images of every dense view, the bulk of the buffer, without overflow
inline long double fp64_image_bytes(const resnmtf_group_job& j, const F64Source* src) {
  long double b = 0;
  for (int v = 0; v < j.n_views; ++v) {
    if (f64_is_sparse(src[v])) continue;
    const long double n = j.n_rows[v], m = j.n_cols[v];
    b += ((n + 63) * (m + 63) + (m + 63) * (n + 63)) * sizeof(double);
  }
  return b;
}

// src == nullptr: every view dense in host memory; else shapes[v] is read for every sparse view
inline void fp64_layout(const resnmtf_group_job& j, int cap, F64Layout& L, const F64Source* src = nullptr,
                        const F64SparseShape* shapes = nullptr) {
  L.V = j.n_views; L.k = j.k; L.KP = f64_kp(j.k); L.cap = cap;
  const size_t k = (size_t)L.k, V = (size_t)L.V;
  size_t off = 0, big = 1, slab = 1, gram_blk = 1, col_blk = 1, spart = 1;
  bool any_sparse = false;
  for (int v = 0; v < L.V; ++v) {
    F64View& w = L.vw[v];
    w.n = j.n_rows[v]; w.m = j.n_cols[v];
    w.ldn = f64_ld(w.n); w.mpad = rup(w.m, F64_JC); w.ldm = f64_ld(w.m); w.npad = rup(w.n, F64_JC);
    w.src = src ? src[v] : F64Source::HostDense;
    if (w.sparse()) {                          // 24 bytes per stored entry plus the pointers; no image, no residual
      any_sparse = true;
      w.nnz = shapes[v].nnz;
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
inline double fp64_col_sum(const double* r, int V, int v) {
  if (!r) return 0.0;
  const double* a = r + (size_t)v * V;       // column v of the column-major matrix: entries [w + v V] = r[w, v]
  if (V < 8) {
    double s = 0.0;
    for (int w = 0; w < V; ++w) s += a[w];
    return s;
  }
  return ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]));
}
inline bool fp64_all_zero(const double* r, int V) {
  if (!r) return true;
  for (int e = 0; e < V * V; ++e)
    if (r[e] != 0.0) return false;
  return true;
}

// what resnmtf_set_view_csc refuses on the host, for one n x m CSC structure (values NULL: the structure alone); the
// text of the refusal or "" when it is fine, and then the view's stored entries, longest row and longest column
inline std::string fp64_check_csc(int n, int m, const long long* col_ptr, const int* row_idx, const double* values,
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
  sh.nnz = (size_t)col_ptr[m];
  sh.longest_col = longest_col;
  sh.longest_row = n > 0 ? *std::max_element(per_row.begin(), per_row.end()) : 0;
  return "";
}

// the CSR copy of a checked CSC structure by a counting sort: a row's entries in ascending column order
inline void fp64_csr_from_csc(int n, int m, const long long* col_ptr, const int* row_idx, const double* values,
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
// The five results and the five raw-state arrays of a view in resnmtf_fp64_device: the name, the member, and which piece
// of the state it receives (so its element count and its place in the job's buffer).  The struct check, the pointer check
// and the copies out all walk this one table.
enum F64Piece { F64_PIECE_F, F64_PIECE_S, F64_PIECE_G, F64_PIECE_LAMBDA, F64_PIECE_MU };
struct F64OutField {
  const char* name;
  double* (resnmtf_fp64_device::*member)[RESNMTF_GROUP_MAX_VIEWS];
  F64Piece piece;
  double* ptr(const resnmtf_fp64_device& d, int v) const { return (d.*member)[v]; }
  size_t count(size_t n, size_t m, size_t k) const {
    return piece == F64_PIECE_F ? n * k : piece == F64_PIECE_S ? k * k : piece == F64_PIECE_G ? m * k : k;
  }
};
constexpr int F64_OUT_SET = 5;              // fields [0, 5): the results; [5, 10): the raw state
static const F64OutField F64_OUT_FIELDS[2 * F64_OUT_SET] = {
    {"f_out", &resnmtf_fp64_device::f_out, F64_PIECE_F},       {"s_out", &resnmtf_fp64_device::s_out, F64_PIECE_S},
    {"g_out", &resnmtf_fp64_device::g_out, F64_PIECE_G},       {"lambda_out", &resnmtf_fp64_device::lambda_out, F64_PIECE_LAMBDA},
    {"mu_out", &resnmtf_fp64_device::mu_out, F64_PIECE_MU},    {"state_f", &resnmtf_fp64_device::state_f, F64_PIECE_F},
    {"state_s", &resnmtf_fp64_device::state_s, F64_PIECE_S},   {"state_g", &resnmtf_fp64_device::state_g, F64_PIECE_G},
    {"state_lambda", &resnmtf_fp64_device::state_lambda, F64_PIECE_LAMBDA}, {"state_mu", &resnmtf_fp64_device::state_mu, F64_PIECE_MU}};

// where a piece of view v's state lies in the job's buffer
inline size_t fp64_piece_offset(const F64Layout& L, int v, F64Piece piece) {
  const size_t k = (size_t)L.k;
  return piece == F64_PIECE_F ? L.vw[v].f : piece == F64_PIECE_S ? L.s + (size_t)v * k * k : piece == F64_PIECE_G ? L.vw[v].g
         : piece == F64_PIECE_LAMBDA ? L.lam + (size_t)v * k : L.mu + (size_t)v * k;
}

// what of a job's factors and results comes from, and goes to, device memory (the views' data: F64Source)
struct F64DeviceUse {
  unsigned factors = 0;                     // bit v: view v's initial factors are device matrices
  bool out = false, state = false;          // the results / the raw state are written to device memory
};

// the refusals that need no device: the text, or "" when the struct is fine (and then `use`)
inline std::string fp64_check_device_struct(const resnmtf_group_job& j, const resnmtf_fp64_device& d, const F64Source* src,
                                            F64DeviceUse& use) {
  if (d.struct_size != (int)sizeof(resnmtf_fp64_device)) return "resnmtf_fp64_device struct_size mismatch";
  if (j.struct_size != (int)sizeof(resnmtf_group_job) || j.n_views < 1 || j.n_views > RESNMTF_GROUP_MAX_VIEWS) return "";   // (the job check says it)
  const int V = j.n_views;
  auto view = [](int v) { return "view " + std::to_string(v) + ": "; };
  struct Field { const char* name; const resnmtf_device_matrix* m; };
  for (int v = 0; v < RESNMTF_GROUP_MAX_VIEWS; ++v) {
    const Field in[6] = {{"x", &d.x[v]}, {"f0", &d.f0[v]}, {"s0", &d.s0[v]}, {"g0", &d.g0[v]}, {"lambda0", &d.lambda0[v]}, {"mu0", &d.mu0[v]}};
    if (v >= V) {
      for (const Field& f : in)
        if (f.m->ptr) return view(v) + "dev->" + f.name + " is given beyond n_views";
      for (const F64OutField& f : F64_OUT_FIELDS)
        if (f.ptr(d, v)) return view(v) + "a device output is given beyond n_views";
      continue;
    }
    for (const Field& f : in) {
      if (!f.m->ptr) continue;
      if (f.m->dtype < RESNMTF_DTYPE_F64 || f.m->dtype > RESNMTF_DTYPE_BF16)
        return view(v) + "dev->" + f.name + " has an unknown dtype (" + std::to_string(f.m->dtype) + ")";
      if (f.m->row_stride < 0 || f.m->col_stride < 0) return view(v) + "dev->" + f.name + " has a negative stride";
    }
    const bool sparse = f64_is_sparse(src[v]);
    if (d.x[v].ptr && j.x[v]) return view(v) + "x is given both in the job (job->x) and in device memory (dev->x): one of them must be NULL";
    if (d.x[v].ptr && sparse) return view(v) + "x is given both sparse (col_ptr) and in device memory (dev->x): one of them must be NULL";
    if (!d.x[v].ptr && !j.x[v] && !sparse) return view(v) + "x is given neither in the job (job->x) nor in device memory (dev->x)";
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
  for (int set = 0; set < 2; ++set) {                  // each set of five: for every view of the job, or for none
    int given = 0, missing_v = -1, missing_f = -1;
    for (int v = 0; v < V; ++v)
      for (int f = set * F64_OUT_SET; f < (set + 1) * F64_OUT_SET; ++f) {
        if (F64_OUT_FIELDS[f].ptr(d, v)) ++given;
        else if (missing_v < 0) { missing_v = v; missing_f = f; }
      }
    if (given != 0 && given != F64_OUT_SET * V)
      return view(missing_v) + "dev->" + F64_OUT_FIELDS[missing_f].name + " is NULL while other device " +
             (set ? "state outputs" : "outputs") + " are given: all five of every view, or none";
    (set ? use.state : use.out) = given != 0;
  }
  return "";
}

// ---- resnmtf_fp64_run_sparse_device (section 24): sparse views from device memory ----
// the refusals that need no device: the text, or "" when every view of the job has its data in exactly one place and
// every sparse device view is well formed
inline std::string fp64_check_sparse_device_struct(const resnmtf_group_job& j, const resnmtf_fp64_sparse* sp,
                                                   const resnmtf_fp64_device* dev, const resnmtf_fp64_sparse_device& d) {
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

#endif  // RESNMTF_FP64_JOB_H
