// Pointer and extent helpers of the handle-free fp64 entries (resnmtf_fp64_shuffle, resnmtf_fp64_subsample,
// resnmtf_fp64_relevance; DESIGN.md sections 27 and 28), stated once: how many bytes a strided device matrix spans, how
// many an n x m fp64 array takes and when that no longer fits 64 bits, and whether two byte ranges share a byte.  No HIP:
// plain C++17 against include/resnmtf_hip.h, included by resnmtf_fp64_shuffle_job.h and resnmtf_fp64_subsample_job.h.
#ifndef RESNMTF_FP64_EXTENT_H
#define RESNMTF_FP64_EXTENT_H

#include <cstddef>
#include <cstdint>

#include "resnmtf_hip.h"

inline size_t f64_dtype_bytes(int dtype) { return dtype == RESNMTF_DTYPE_F64 ? 8 : dtype == RESNMTF_DTYPE_F32 ? 4 : 2; }

// the bytes [ptr, ptr + bytes) an n x m device matrix spans: up to its last element
inline size_t f64_matrix_bytes(const resnmtf_device_matrix& a, int n, int m) {
  const size_t last = (size_t)(n - 1) * (size_t)a.row_stride + (size_t)(m - 1) * (size_t)a.col_stride;
  return (last + 1) * f64_dtype_bytes(a.dtype);
}
// n m doubles beyond what 64 bits count in bytes (n m > 2^60): no device holds them; asked before f64_array_bytes
inline bool f64_array_bytes_overflow(int n, int m) { return (unsigned long long)n * (unsigned long long)m > (1ull << 60); }
inline size_t f64_array_bytes(int n, int m) { return (size_t)n * (size_t)m * sizeof(double); }

// two byte ranges share a byte
inline bool f64_ranges_overlap(const void* a, size_t a_bytes, const void* b, size_t b_bytes) {
  const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
  return a0 < b0 + b_bytes && b0 < a0 + a_bytes;
}

#endif  // RESNMTF_FP64_EXTENT_H
