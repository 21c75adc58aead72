// The host-only half of resnmtf_fp64_subsample_sparse: what depends on nothing but the job struct.
// No HIP: it compiles with a plain C++17 compiler against include/resnmtf_hip.h alone, which is how
// tests/host/fp64_subsample_sparse_check.cpp runs it.  resnmtf_fp64.hip adds the view's own checks (resnmtf_fp64_job.h),
// the checks that ask the runtime (whose memory a pointer is, how far its allocation reaches) and the launches.  The
// index-list check is section 28's (f64_subsample_check_indices), the byte ranges and their overlap test section 30's.
#ifndef RESNMTF_FP64_SUBSAMPLE_SPARSE_JOB_H
#define RESNMTF_FP64_SUBSAMPLE_SPARSE_JOB_H

#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "resnmtf_hip.h"
#include "resnmtf_fp64_extent.h"
#include "resnmtf_fp64_job.h"
#include "resnmtf_fp64_shuffle_sparse_job.h"
#include "resnmtf_fp64_subsample_job.h"

// ---- the edges of resnmtf_fp64_subsample_sparse.hip.inc ----
constexpr int F64_SUBSAMPLE_SPARSE_TRIP = 64;          // entries of a source column one wave takes per trip
constexpr int F64_SUBSAMPLE_SPARSE_WAVES = 4;          // destination columns (waves) per workgroup of the two walks
constexpr int F64_SUBSAMPLE_SPARSE_SCAN_BLOCK = 256;   // counts the single workgroup of the scan takes per block

// count mode: nothing of the sub-sample is written to the caller's device memory, only nnz_sub, the counts and the masks
inline bool f64_subsample_sparse_count_mode(const resnmtf_fp64_subsample_sparse_job& j) {
  return !j.out_col_ptr && !j.out_row_idx && !j.out_values && j.out_capacity == 0;
}

// every refusal that needs no device, no look at the index lists and none at the view's arrays, in the order the header
// documents; nullptr: the struct is sound
inline const char* f64_subsample_sparse_check_job(const resnmtf_fp64_subsample_sparse_job* job) {
  if (!job) return "job is NULL";
  if (job->struct_size != (int)sizeof(resnmtf_fp64_subsample_sparse_job)) return "resnmtf_fp64_subsample_sparse_job struct_size mismatch";
  if (job->n < 1 || job->m < 1) return "view dimensions must be positive";
  if (job->n_sub < 1 || job->n_sub > job->n) return "n_sub must be in [1, n]";
  if (job->m_sub < 1 || job->m_sub > job->m) return "m_sub must be in [1, m]";
  if (!job->rows || !job->cols) return "rows / cols are NULL";
  const bool host_x = job->x.col_ptr != nullptr;
  if (host_x == fp64_spd_given(job->x_dev))
    return host_x ? "X is given in two places (job->x and job->x_dev)" : "X is given in no place (job->x or job->x_dev)";
  if (job->out_capacity < 0) return "out_capacity is negative";
  if (!f64_subsample_sparse_count_mode(*job)) {          // fill mode
    if (!job->out_col_ptr) return "out_col_ptr is NULL";
    if (job->out_capacity > 0 && (!job->out_row_idx || !job->out_values)) return "out_row_idx / out_values are NULL";
  }
  if (!job->nnz_sub) return "nnz_sub is NULL";
  if (!job->n_empty_rows || !job->n_empty_cols) return "n_empty_rows / n_empty_cols are NULL";
  return nullptr;
}

// the most entries a sub-sample can keep: every stored entry, or every position
inline unsigned long long f64_subsample_sparse_bound(int n_sub, int m_sub, unsigned long long nnz) {
  return std::min<unsigned long long>(nnz, (unsigned long long)n_sub * (unsigned long long)m_sub);
}

// ---- extents: the byte ranges the call writes (the three outputs, by their capacity) and reads (a device view) ----
// out_col_ptr, out_row_idx, out_values; bytes 0 = nothing is written there (count mode, out_capacity = 0)
inline void f64_subsample_sparse_outputs(const resnmtf_fp64_subsample_sparse_job& j, F64ShuffleSparseRange out[3]) {
  out[0] = {"out_col_ptr", j.out_col_ptr, j.out_col_ptr ? ((size_t)j.m_sub + 1) * sizeof(long long) : 0};
  out[1] = {"out_row_idx", j.out_row_idx, (size_t)j.out_capacity * sizeof(long long)};
  out[2] = {"out_values", j.out_values, (size_t)j.out_capacity * sizeof(double)};
}
// ptr_or_rows, idx_or_cols, values of a device view whose struct has passed its checks: section 30's, for the n x m source
inline void f64_subsample_sparse_sources(const resnmtf_fp64_subsample_sparse_job& j, F64ShuffleSparseRange in[3]) {
  resnmtf_fp64_shuffle_sparse_job as{};
  as.n = j.n; as.m = j.m; as.x_dev = j.x_dev;
  f64_shuffle_sparse_sources(as, in);
}
// (the overlap test: f64_shuffle_sparse_overlap)

// ---- the workspace of a call, in bytes from its start: the kept entries per destination column and their exclusive scan
// (m_sub and m_sub + 1 int64), inv_row[n], rows[n_sub], cols[m_sub] and the two counts (and two spare) as ints, then the
// masks, rows first ----
struct F64SubsampleSparsePlan { size_t counts, scan, inv_row, rows, cols, ints, mask, total; };
inline F64SubsampleSparsePlan f64_subsample_sparse_plan(int n, int n_sub, int m_sub) {
  F64SubsampleSparsePlan p;
  p.counts = 0;
  p.scan = p.counts + (size_t)m_sub * sizeof(long long);
  p.inv_row = p.scan + ((size_t)m_sub + 1) * sizeof(long long);
  p.rows = p.inv_row + (size_t)n * sizeof(int);
  p.cols = p.rows + (size_t)n_sub * sizeof(int);
  p.ints = p.cols + (size_t)m_sub * sizeof(int);
  p.mask = p.ints + 4 * sizeof(int);
  p.total = (p.mask + (size_t)n_sub + (size_t)m_sub + 7) / 8 * 8;
  return p;
}

// ---- the transient device memory of a call, at its peak, beside the workspace above ----
// Per STORED entry the call holds the source's canonical CSC, rows and fp64 values (4 + 8 = 12); while a source that lies
// in device memory is built, the canonicaliser's arrays instead (5 x 8 + 2 x 4 = 48, section 30).  Per KEPT entry it
// holds the emitted COO (4 + 4 + 8 = 16) and, while that is sorted, the canonicaliser's arrays for it (48): 64.  The kept
// entries are known only after the counting pass, so the call sizes itself on their bound (f64_subsample_sparse_bound).
// Beside them the source's m + 1 (and, during its build, n + 1) pointers, the sub-sample's m_sub + 1 and n_sub + 1 and
// the flag words.  Count mode stops before anything per kept entry exists.
constexpr size_t F64_SUBSAMPLE_SPARSE_BYTES_PER_STORED = 12;
constexpr size_t F64_SUBSAMPLE_SPARSE_BYTES_PER_STORED_BUILD = 48;
constexpr size_t F64_SUBSAMPLE_SPARSE_BYTES_PER_KEPT = 64;
inline size_t f64_subsample_sparse_transient_bytes(int n, int m, int n_sub, int m_sub, unsigned long long nnz,
                                                   unsigned long long nnz_sub_bound, bool device_source = false) {
  const size_t source_ptrs = ((size_t)m + 1) * sizeof(long long), flags = 24;
  const size_t build = device_source ? (size_t)nnz * F64_SUBSAMPLE_SPARSE_BYTES_PER_STORED_BUILD + source_ptrs +
                                           ((size_t)n + 1) * sizeof(long long) + flags
                                     : 0;
  const size_t sorted = (size_t)nnz * F64_SUBSAMPLE_SPARSE_BYTES_PER_STORED + source_ptrs + (device_source ? flags : 0) +
                        (size_t)nnz_sub_bound * F64_SUBSAMPLE_SPARSE_BYTES_PER_KEPT +
                        (nnz_sub_bound ? ((size_t)m_sub + 1 + (size_t)n_sub + 1) * sizeof(long long) + flags : 0);
  return std::max(build, sorted);
}

#endif  // RESNMTF_FP64_SUBSAMPLE_SPARSE_JOB_H
