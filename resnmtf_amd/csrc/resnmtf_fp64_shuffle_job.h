// The host-only half of resnmtf_fp64_shuffle: what depends on nothing but the job struct.  No HIP:
// it compiles with a plain C++17 compiler against include/resnmtf_hip.h alone, which is how
// tests/host/fp64_shuffle_check.cpp runs it.  resnmtf_fp64.hip adds the checks that ask the runtime (whose memory a
// pointer is, how far its allocation reaches) and the launches.
#ifndef RESNMTF_FP64_SHUFFLE_JOB_H
#define RESNMTF_FP64_SHUFFLE_JOB_H

#include <cstddef>
#include <cstdint>

#include "resnmtf_hip.h"
#include "resnmtf_fp64_extent.h"

constexpr unsigned long long F64_SHUFFLE_MAX_COUNT = 1ull << 62;      // the Feistel domain: 2^(2 half_bits), half_bits <= 31

// every refusal that needs no device, in the order the header documents; nullptr: the struct is sound
inline const char* f64_shuffle_check_job(const resnmtf_fp64_shuffle_job* job) {
  if (!job) return "job is NULL";
  if (job->struct_size != (int)sizeof(resnmtf_fp64_shuffle_job)) return "resnmtf_fp64_shuffle_job struct_size mismatch";
  if (job->n < 1 || job->m < 1) return "view dimensions must be positive";
  if ((unsigned long long)job->n * (unsigned long long)job->m > F64_SHUFFLE_MAX_COUNT)
    return "n * m exceeds 2^62 (the domain of the Feistel permutation)";
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

// the extents of the checked job, from the helpers the handle-free fp64 entries share (resnmtf_fp64_extent.h)
inline size_t f64_shuffle_dtype_bytes(int dtype) { return f64_dtype_bytes(dtype); }
// the bytes [ptr, ptr + bytes) a device source of the checked job spans: up to its last element
inline size_t f64_shuffle_source_bytes(const resnmtf_fp64_shuffle_job& j) { return f64_matrix_bytes(j.x_dev, j.n, j.m); }
// n m doubles beyond what 64 bits count in bytes (n m > 2^60): no device holds them; asked before f64_shuffle_out_bytes
inline bool f64_shuffle_bytes_overflow(const resnmtf_fp64_shuffle_job& j) { return f64_array_bytes_overflow(j.n, j.m); }
inline size_t f64_shuffle_out_bytes(const resnmtf_fp64_shuffle_job& j) { return f64_array_bytes(j.n, j.m); }
// two byte ranges share a byte
inline bool f64_shuffle_overlap(const void* a, size_t a_bytes, const void* b, size_t b_bytes) {
  return f64_ranges_overlap(a, a_bytes, b, b_bytes);
}

// The small workspace of a call, in bytes from its start (the staging copy of a host X, n m doubles, is a buffer of its
// own): shift[m], colsum[m] doubles, then the two counts and the negative flag as ints, then the masks, rows first.
struct F64ShufflePlan { size_t shift, colsum, ints, mask, total; };
inline F64ShufflePlan f64_shuffle_plan(int n, int m) {
  F64ShufflePlan p;
  p.shift = 0;
  p.colsum = p.shift + (size_t)m * sizeof(double);
  p.ints = p.colsum + (size_t)m * sizeof(double);
  p.mask = p.ints + 4 * sizeof(int);              // counts[0], counts[1], neg, one spare: the masks start 8-byte aligned
  p.total = (p.mask + (size_t)n + (size_t)m + 7) / 8 * 8;
  return p;
}

#endif  // RESNMTF_FP64_SHUFFLE_JOB_H
