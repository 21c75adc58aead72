// The host-only half of resnmtf_fp64_subsample and resnmtf_fp64_relevance: what depends on
// nothing but the job structs.  No HIP: it compiles with a plain C++17 compiler against include/resnmtf_hip.h alone, which
// is how tests/host/fp64_subsample_check.cpp runs it.  resnmtf_fp64.hip adds the checks that ask the runtime (whose memory
// a pointer is, how far its allocation reaches) and the launches.
#ifndef RESNMTF_FP64_SUBSAMPLE_JOB_H
#define RESNMTF_FP64_SUBSAMPLE_JOB_H

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "resnmtf_hip.h"
#include "resnmtf_fp64_extent.h"

// ---- the tile edges of resnmtf_fp64_subsample.hip.inc (resnmtf_fp64_subsample_plan reports them) ----
constexpr int F64_SUB_BLOCK = 256;        // threads of the gather kernels; the row form takes that many destination rows
constexpr int F64_SUB_TILE = 32;          // the LDS transpose form: a 32 x 32 tile of the destination
constexpr int F64_SUB_ROWSUM_BLOCK = 64;  // rows (lanes) per workgroup of the row sums
constexpr int F64_SUB_COLSUM_ROWS = 64;   // the column sums: a tile of 64 rows x 32 columns staged through LDS
constexpr int F64_SUB_COLSUM_COLS = 32;

// The gather form, from the source's strides alone: 0 = lanes along the destination rows (the source's row stride is the
// smaller: a column-major source, a host X), 1 = the padded LDS tile transpose (the column stride is the smaller: a
// row-major tensor is read along its rows).  Equal strides (an expanded tensor, a single line) take form 0.
inline int f64_subsample_form(long long row_stride, long long col_stride) { return col_stride < row_stride ? 1 : 0; }

// every refusal that needs no device and no look at the index lists, in the order the header documents; nullptr: sound
inline const char* f64_subsample_check_job(const resnmtf_fp64_subsample_job* job) {
  if (!job) return "job is NULL";
  if (job->struct_size != (int)sizeof(resnmtf_fp64_subsample_job)) return "resnmtf_fp64_subsample_job struct_size mismatch";
  if (job->n < 1 || job->m < 1) return "view dimensions must be positive";
  if (job->n_sub < 1 || job->n_sub > job->n) return "n_sub must be in [1, n]";
  if (job->m_sub < 1 || job->m_sub > job->m) return "m_sub must be in [1, m]";
  if (!job->rows || !job->cols) return "rows / cols are NULL";
  const bool host_x = job->x != nullptr;
  if (host_x == (job->x_dev.ptr != nullptr))
    return host_x ? "X is given in two places (job->x and job->x_dev)" : "X is given in no place (job->x or job->x_dev)";
  if (!job->out) return "out is NULL";
  if (!job->n_empty_rows || !job->n_empty_cols) return "n_empty_rows / n_empty_cols are NULL";
  if (!host_x) {
    if (job->x_dev.dtype < RESNMTF_DTYPE_F64 || job->x_dev.dtype > RESNMTF_DTYPE_BF16) return "x_dev: unknown dtype";
    if (job->x_dev.row_stride < 0 || job->x_dev.col_stride < 0) return "x_dev: strides must be >= 0";
  }
  return nullptr;
}

// An index list of a sub-sample: `count` indices into [0, extent), each at most once (the reference samples without
// replacement, R/stability_analysis.r:114-123).  Empty: sound; else the refusal, the lowest offending position named.
inline std::string f64_subsample_check_indices(const char* name, const int* idx, int count, int extent) {
  std::vector<unsigned char> seen((size_t)extent, 0);
  for (int i = 0; i < count; ++i) {
    const int t = idx[i];
    if (t < 0 || t >= extent)
      return std::string(name) + "[" + std::to_string(i) + "] = " + std::to_string(t) + " is out of range [0, " + std::to_string(extent) + ")";
    if (seen[(size_t)t]) return std::string(name) + "[" + std::to_string(i) + "] = " + std::to_string(t) + " occurs twice";
    seen[(size_t)t] = 1;
  }
  return std::string();
}

// (the extents of the matrices, of `out` and of the staging copy, and the overlap test: resnmtf_fp64_extent.h)

// The small workspace of a call, in bytes from its start (the staging copy of a host X, n m doubles, is a buffer of its
// own): the two counts (and two spare ints: the lists start 8-byte aligned), rows[n_sub], cols[m_sub] as ints, then the
// masks, rows first.
struct F64SubsamplePlan { size_t ints, rows, cols, mask, total; };
inline F64SubsamplePlan f64_subsample_plan(int n_sub, int m_sub) {
  F64SubsamplePlan p;
  p.ints = 0;
  p.rows = p.ints + 4 * sizeof(int);
  p.cols = p.rows + (size_t)n_sub * sizeof(int);
  p.mask = p.cols + (size_t)m_sub * sizeof(int);
  p.total = (p.mask + (size_t)n_sub + (size_t)m_sub + 7) / 8 * 8;
  return p;
}

// ---- resnmtf_fp64_relevance ----
inline const char* f64_relevance_check_matrix(const resnmtf_device_matrix& a, const char* unknown, const char* negative) {
  if (a.dtype < RESNMTF_DTYPE_F64 || a.dtype > RESNMTF_DTYPE_BF16) return unknown;
  if (a.row_stride < 0 || a.col_stride < 0) return negative;
  return nullptr;
}

inline const char* f64_relevance_check_job(const resnmtf_fp64_relevance_job* job) {
  if (!job) return "job is NULL";
  if (job->struct_size != (int)sizeof(resnmtf_fp64_relevance_job)) return "resnmtf_fp64_relevance_job struct_size mismatch";
  if (job->n < 1 || job->m < 1) return "view dimensions must be positive";
  if (job->n_sub < 1 || job->n_sub > job->n) return "n_sub must be in [1, n]";
  if (job->m_sub < 1 || job->m_sub > job->m) return "m_sub must be in [1, m]";
  if (job->k < 1 || job->k > RESNMTF_MAX_K) return "k must be in [1, 64]";
  if (job->k_ref < 1 || job->k_ref > RESNMTF_MAX_K) return "k_ref must be in [1, 64]";
  if (!job->rows || !job->cols) return "rows / cols are NULL";
  if (!job->relevance) return "relevance is NULL";
  if (!job->row_c.ptr || !job->col_c.ptr) return "row_c / col_c are NULL";
  if ((job->true_r != nullptr) == (job->true_r_dev.ptr != nullptr))
    return job->true_r ? "true_r is given in two places (job->true_r and job->true_r_dev)" : "true_r is given in no place (job->true_r or job->true_r_dev)";
  if ((job->true_c != nullptr) == (job->true_c_dev.ptr != nullptr))
    return job->true_c ? "true_c is given in two places (job->true_c and job->true_c_dev)" : "true_c is given in no place (job->true_c or job->true_c_dev)";
  if (const char* why = f64_relevance_check_matrix(job->row_c, "row_c: unknown dtype", "row_c: strides must be >= 0")) return why;
  if (const char* why = f64_relevance_check_matrix(job->col_c, "col_c: unknown dtype", "col_c: strides must be >= 0")) return why;
  if (!job->true_r)
    if (const char* why = f64_relevance_check_matrix(job->true_r_dev, "true_r_dev: unknown dtype", "true_r_dev: strides must be >= 0")) return why;
  if (!job->true_c)
    if (const char* why = f64_relevance_check_matrix(job->true_c_dev, "true_c_dev: unknown dtype", "true_c_dev: strides must be >= 0")) return why;
  return nullptr;
}

// a host reference matrix (len x k doubles, column-major): the lowest column-major position of an entry other than 0 / 1,
// or -1
inline long long f64_relevance_bad_entry(const double* a, int len, int k) {
  for (long long i = 0; i < (long long)len * k; ++i)
    if (a[i] != 0.0 && a[i] != 1.0) return i;
  return -1;
}

// The workspace of a relevance call, in bytes from its start: the four lowest-offender words, the result, the staged host
// references (len x k_ref doubles each, or none), the counts of both sides ([k k_ref] [k] [k_ref] unsigned each), the
// index lists.
struct F64RelevancePlan { size_t bad, out, true_r, true_c, counts, rows, cols, total; size_t side_counts; };
inline F64RelevancePlan f64_relevance_plan(const resnmtf_fp64_relevance_job& j) {
  F64RelevancePlan p;
  p.side_counts = (size_t)j.k * j.k_ref + (size_t)j.k + (size_t)j.k_ref;
  p.bad = 0;
  p.out = p.bad + 4 * sizeof(unsigned long long);
  p.true_r = p.out + (size_t)j.k_ref * sizeof(double);
  p.true_c = p.true_r + (j.true_r ? (size_t)j.n * j.k_ref * sizeof(double) : 0);
  p.counts = p.true_c + (j.true_c ? (size_t)j.m * j.k_ref * sizeof(double) : 0);
  p.rows = p.counts + 2 * p.side_counts * sizeof(unsigned int);
  p.cols = p.rows + (size_t)j.n_sub * sizeof(int);
  p.total = (p.cols + (size_t)j.m_sub * sizeof(int) + 7) / 8 * 8;
  return p;
}

#endif  // RESNMTF_FP64_SUBSAMPLE_JOB_H
