// The host-only half of resnmtf_fp64_shuffle_sparse: what depends on nothing but the job struct.
// No HIP: it compiles with a plain C++17 compiler against include/resnmtf_hip.h alone, which is how
// tests/host/fp64_shuffle_sparse_check.cpp runs it.  resnmtf_fp64.hip adds the view's own checks (resnmtf_fp64_job.h),
// the checks that ask the runtime (whose memory a pointer is, how far its allocation reaches) and the launches.
#ifndef RESNMTF_FP64_SHUFFLE_SPARSE_JOB_H
#define RESNMTF_FP64_SHUFFLE_SPARSE_JOB_H

#include <cstddef>
#include <cstdint>

#include "resnmtf_hip.h"
#include "resnmtf_fp64_extent.h"
#include "resnmtf_fp64_job.h"
#include "resnmtf_fp64_shuffle_job.h"

// every refusal that needs neither the device nor the view's arrays, in the order the header documents; nullptr: the
// struct is sound.  (out_row_idx / out_values may be NULL for a view without a stored entry: f64_shuffle_sparse_check_nnz.)
inline const char* f64_shuffle_sparse_check_job(const resnmtf_fp64_shuffle_sparse_job* job) {
  if (!job) return "job is NULL";
  if (job->struct_size != (int)sizeof(resnmtf_fp64_shuffle_sparse_job)) return "resnmtf_fp64_shuffle_sparse_job struct_size mismatch";
  if (job->n < 1 || job->m < 1) return "view dimensions must be positive";
  if ((unsigned long long)job->n * (unsigned long long)job->m > F64_SHUFFLE_MAX_COUNT)
    return "n * m exceeds 2^62 (the domain of the Feistel permutation)";
  const bool host_x = job->x.col_ptr != nullptr;
  if (host_x == fp64_spd_given(job->x_dev))
    return host_x ? "X is given in two places (job->x and job->x_dev)" : "X is given in no place (job->x or job->x_dev)";
  if (!job->out_col_ptr) return "out_col_ptr is NULL";
  if (!job->n_empty_rows || !job->n_empty_cols) return "n_empty_rows / n_empty_cols are NULL";
  return nullptr;
}
// once the stored entries are counted: the two arrays of nnz
inline const char* f64_shuffle_sparse_check_nnz(const resnmtf_fp64_shuffle_sparse_job& j, unsigned long long nnz) {
  if (nnz > 0 && (!j.out_row_idx || !j.out_values)) return "out_row_idx / out_values are NULL";
  return nullptr;
}

// ---- extents: the byte ranges the call writes (the three outputs) and reads (the arrays of a device view) ----
struct F64ShuffleSparseRange { const char* name; const void* ptr; size_t bytes; };
// out_col_ptr, out_row_idx, out_values; bytes 0 = nothing is written there (nnz = 0)
inline void f64_shuffle_sparse_outputs(const resnmtf_fp64_shuffle_sparse_job& j, unsigned long long nnz, F64ShuffleSparseRange out[3]) {
  out[0] = {"out_col_ptr", j.out_col_ptr, ((size_t)j.m + 1) * sizeof(long long)};
  out[1] = {"out_row_idx", j.out_row_idx, (size_t)nnz * sizeof(long long)};
  out[2] = {"out_values", j.out_values, (size_t)nnz * sizeof(double)};
}
// ptr_or_rows, idx_or_cols, values of a device view whose struct has passed its checks
inline void f64_shuffle_sparse_sources(const resnmtf_fp64_shuffle_sparse_job& j, F64ShuffleSparseRange in[3]) {
  const resnmtf_fp64_sparse_device_view& c = j.x_dev;
  const size_t ib = c.index_type == RESNMTF_INDEX_I64 ? 8 : 4, nnz = (size_t)c.nnz;
  const size_t lines = (size_t)(c.layout == RESNMTF_SPARSE_CSC ? j.m : j.n);
  in[0] = {"x_dev.ptr_or_rows", c.ptr_or_rows, (c.layout == RESNMTF_SPARSE_COO ? nnz : lines + 1) * ib};
  in[1] = {"x_dev.idx_or_cols", c.idx_or_cols, nnz * ib};
  in[2] = {"x_dev.values", c.values, nnz * f64_dtype_bytes(c.dtype)};
}
// the first pair that shares a byte: outputs with each other (a = b = names of outputs), then outputs with sources;
// false when none does.  Empty ranges and NULL pointers overlap nothing.
inline bool f64_shuffle_sparse_overlap(const F64ShuffleSparseRange out[3], const F64ShuffleSparseRange* in, const char*& a, const char*& b) {
  auto hit = [](const F64ShuffleSparseRange& p, const F64ShuffleSparseRange& q) {
    return p.ptr && q.ptr && p.bytes && q.bytes && f64_ranges_overlap(p.ptr, p.bytes, q.ptr, q.bytes);
  };
  for (int x = 0; x < 3; ++x)
    for (int y = x + 1; y < 3; ++y)
      if (hit(out[x], out[y])) { a = out[x].name; b = out[y].name; return true; }
  if (in)
    for (int x = 0; x < 3; ++x)
      for (int y = 0; y < 3; ++y)
        if (hit(out[x], in[y])) { a = out[x].name; b = in[y].name; return true; }
  return false;
}

// ---- the small workspace of a call, in bytes from its start: colsum[m] doubles, the two counts as ints (and two
// spare: the masks start 8-byte aligned), then the masks, rows first ----
struct F64ShuffleSparsePlan { size_t colsum, ints, mask, total; };
inline F64ShuffleSparsePlan f64_shuffle_sparse_plan(int n, int m) {
  F64ShuffleSparsePlan p;
  p.colsum = 0;
  p.ints = p.colsum + (size_t)m * sizeof(double);
  p.mask = p.ints + 4 * sizeof(int);
  p.total = (p.mask + (size_t)n + (size_t)m + 7) / 8 * 8;
  return p;
}

// ---- the transient device memory of a call, at its peak ----
// While the destination is sorted the call holds, per stored entry: the source's values in fp64 and its rows (8 + 4),
// the destination coordinates (4 + 4), and the canonicaliser's arrays for the destination -- two keys, three payloads
// (5 x 8) and the two index arrays (2 x 4): 68 bytes.  Beside them the source's m + 1 pointers, the destination's m + 1
// and n + 1 pointers and the flag words.  (Building a source that lies in device memory peaks lower, at 48 per entry,
// before the destination exists; the sort's own temporary storage does not grow with nnz.)
constexpr size_t F64_SHUFFLE_SPARSE_BYTES_PER_ENTRY = 68;
inline size_t f64_shuffle_sparse_transient_bytes(int n, int m, unsigned long long nnz) {
  return (size_t)nnz * F64_SHUFFLE_SPARSE_BYTES_PER_ENTRY + (2 * ((size_t)m + 1) + (size_t)n + 1) * sizeof(long long) + 2 * 24;
}

// ---- the ordered column sum, restated for the host: what fp64_shuffle_sparse_colsum_kernel computes for one column
// whose stored rows ascend.  Trip by trip the entries of one block of 256 rows go to acc[row % 256]; then the 256-wide
// tree.  Equal, bit for bit, to fp64_shuffle_stats_kernel's sum of the densified non-negative column.
inline double f64_shuffle_sparse_colsum_host(const int* rows, const double* vals, long long len) {
  double acc[256];
  for (double& a : acc) a = 0.0;
  long long pos = 0;
  while (pos < len) {
    const int b = rows[pos] >> 8;
    long long e = pos;
    for (; e < len && e < pos + 256 && (rows[e] >> 8) == b; ++e) acc[rows[e] & 255] += vals[e] + 0.0;
    pos = e;
  }
  for (int s = 128; s > 0; s >>= 1)
    for (int t = 0; t < s; ++t) acc[t] += acc[t + s];
  return acc[0];
}

#endif  // RESNMTF_FP64_SHUFFLE_SPARSE_JOB_H
