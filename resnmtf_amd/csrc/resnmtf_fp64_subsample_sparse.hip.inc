// resnmtf_fp64_subsample_sparse.hip.inc -- the sub-sample X[rows, cols] of stability_repeat (R/stability_analysis.r:124)
// of a SPARSE view in double precision (resnmtf_fp64_subsample_sparse, DESIGN.md section 31): resnmtf_fp64_subsample's
// gather made of the stored entries alone.  Included by resnmtf_fp64.hip only, after resnmtf_fp64_subsample_sparse_job.h.
//
// The source arrives as a canonical CSC in device memory (cptr int64, rows int32, values fp64), every index verified
// (fp64_check_csc on the host route, the main unit's canonicaliser on the device route); the lists have passed
// f64_subsample_check_indices.  The kept entries are sorted by the same canonicaliser, handed to it as a COO; the widening
// of the rows and the two line counts are section 30's kernels.  What is new here, wave64:
//   fp64_subsample_sparse_inverse_kernel  inv_row[rows[i]] = i, one thread per destination row (inv_row preset to -1: a
//                                         source row that is not sampled stays negative).
//   fp64_subsample_sparse_count_kernel    one wave per destination column j walks source column cols[j], 64 entries per
//                                         trip: the entries with inv_row[r] >= 0 are counted by ballot + popcount into
//                                         counts[j] (int64); a kept entry with a value > 0 clears the "empty" byte of its
//                                         destination row, and column j's byte is cleared when any did.  Plain byte stores
//                                         of one value: no order matters.
//   fp64_subsample_sparse_scan_kernel     the exclusive scan of the m_sub counts into m_sub + 1 int64, by ONE workgroup:
//                                         blocks of 256 counts through an LDS scan, the running total carried from block
//                                         to block in a register.  Its last element is nnz_sub.
//   fp64_subsample_sparse_emit_kernel     the same walk: a kept entry goes to slot scan[j] + (kept in earlier trips) + (its
//                                         rank in the trip's ballot) as a COO triple -- int32 destination row, int32
//                                         destination column, the fp64 value as it is.  Every slot is written once.
// No floating-point arithmetic at all, no atomics, no waits between workgroups; entry offsets are 64-bit throughout.

static __global__ void __launch_bounds__(256)
fp64_subsample_sparse_inverse_kernel(const int* __restrict__ rows, int n_sub, int* __restrict__ inv_row) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i < n_sub) inv_row[rows[i]] = (int)i;
}

// mask[0 .. n_sub) rows, mask[n_sub .. n_sub + m_sub) columns, all 1 on entry
static __global__ void __launch_bounds__(64 * F64_SUBSAMPLE_SPARSE_WAVES)
fp64_subsample_sparse_count_kernel(const long long* __restrict__ cptr, const int* __restrict__ srows, const double* __restrict__ val,
                                   const int* __restrict__ cols, const int* __restrict__ inv_row, int n_sub, int m_sub,
                                   long long* __restrict__ counts, unsigned char* __restrict__ mask) {
  const int lane = threadIdx.x & 63;
  const long long j = (long long)blockIdx.x * F64_SUBSAMPLE_SPARSE_WAVES + (threadIdx.x >> 6);
  if (j >= m_sub) return;                              // (the whole wave)
  const int c = cols[j];
  const long long end = cptr[c + 1];
  long long kept = 0;
  bool positive = false;
  for (long long base = cptr[c]; base < end; base += F64_SUBSAMPLE_SPARSE_TRIP) {      // (the same trips in every lane)
    const long long e = base + lane;
    const int i = e < end ? inv_row[srows[e]] : -1;
    kept += __popcll(__ballot(i >= 0));
    if (i >= 0 && val[e] > 0.0) {
      mask[i] = 0;
      positive = true;
    }
  }
  const bool any_positive = __ballot(positive) != 0ull;
  if (lane == 0) {
    counts[j] = kept;
    if (any_positive) mask[(size_t)n_sub + (size_t)j] = 0;
  }
}

static __global__ void __launch_bounds__(F64_SUBSAMPLE_SPARSE_SCAN_BLOCK)
fp64_subsample_sparse_scan_kernel(const long long* __restrict__ counts, int m_sub, long long* __restrict__ scan) {
  constexpr int B = F64_SUBSAMPLE_SPARSE_SCAN_BLOCK;
  __shared__ long long s[B];
  const int t = threadIdx.x;
  long long carry = 0;                                 // (the same in every thread)
  for (long long base = 0; base < m_sub; base += B) {
    const long long j = base + t;
    const long long own = j < m_sub ? counts[j] : 0;
    s[t] = own;
    __syncthreads();
    for (int d = 1; d < B; d <<= 1) {
      const long long add = t >= d ? s[t - d] : 0;
      __syncthreads();
      s[t] += add;
      __syncthreads();
    }
    if (j < m_sub) scan[j] = carry + s[t] - own;
    carry += s[B - 1];
    __syncthreads();                                   // (s is written again in the next block)
  }
  if (t == 0) scan[m_sub] = carry;
}

static __global__ void __launch_bounds__(64 * F64_SUBSAMPLE_SPARSE_WAVES)
fp64_subsample_sparse_emit_kernel(const long long* __restrict__ cptr, const int* __restrict__ srows, const double* __restrict__ val,
                                  const int* __restrict__ cols, const int* __restrict__ inv_row, int m_sub,
                                  const long long* __restrict__ scan, int* __restrict__ drow, int* __restrict__ dcol,
                                  double* __restrict__ dval) {
  const int lane = threadIdx.x & 63;
  const long long j = (long long)blockIdx.x * F64_SUBSAMPLE_SPARSE_WAVES + (threadIdx.x >> 6);
  if (j >= m_sub) return;
  const int c = cols[j];
  const long long end = cptr[c + 1];
  long long slot = scan[j];                            // where this trip's first kept entry goes; at most scan[j + 1] at the end
  for (long long base = cptr[c]; base < end; base += F64_SUBSAMPLE_SPARSE_TRIP) {
    const long long e = base + lane;
    const int i = e < end ? inv_row[srows[e]] : -1;
    const unsigned long long keep = __ballot(i >= 0);
    if (i >= 0) {
      const long long at = slot + __popcll(keep & ((1ull << lane) - 1ull));
      drow[at] = i;
      dcol[at] = (int)j;
      dval[at] = val[e];
    }
    slot += __popcll(keep);
  }
}

// ---- launches ----
inline unsigned f64_subsample_sparse_waves_grid(int m_sub) {
  return (unsigned)(((long long)m_sub + F64_SUBSAMPLE_SPARSE_WAVES - 1) / F64_SUBSAMPLE_SPARSE_WAVES);
}
// inv_row[n] (preset here), then the kept entries per destination column, their scan and the masks (all lines empty on
// entry: set here)
inline hipError_t fp64_subsample_sparse_count(hipStream_t st, const long long* cptr, const int* srows, const double* val, const int* rows,
                                              const int* cols, int n, int n_sub, int m_sub, int* inv_row, long long* counts,
                                              long long* scan, unsigned char* mask) {
  hipError_t e = hipMemsetAsync(inv_row, 0xFF, (size_t)n * sizeof(int), st);                       // -1 everywhere
  if (e == hipSuccess) e = hipMemsetAsync(mask, 1, (size_t)n_sub + (size_t)m_sub, st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(fp64_subsample_sparse_inverse_kernel, dim3((unsigned)(((long long)n_sub + 255) / 256)), dim3(256), 0, st, rows,
                     n_sub, inv_row);
  hipLaunchKernelGGL(fp64_subsample_sparse_count_kernel, dim3(f64_subsample_sparse_waves_grid(m_sub)),
                     dim3(64 * F64_SUBSAMPLE_SPARSE_WAVES), 0, st, cptr, srows, val, cols, (const int*)inv_row, n_sub, m_sub, counts, mask);
  hipLaunchKernelGGL(fp64_subsample_sparse_scan_kernel, dim3(1), dim3(F64_SUBSAMPLE_SPARSE_SCAN_BLOCK), 0, st,
                     (const long long*)counts, m_sub, scan);
  return hipGetLastError();
}
// the kept entries as a COO of scan[m_sub] >= 1 triples
inline hipError_t fp64_subsample_sparse_emit(hipStream_t st, const long long* cptr, const int* srows, const double* val, const int* cols,
                                             const int* inv_row, int m_sub, const long long* scan, int* drow, int* dcol, double* dval) {
  hipLaunchKernelGGL(fp64_subsample_sparse_emit_kernel, dim3(f64_subsample_sparse_waves_grid(m_sub)),
                     dim3(64 * F64_SUBSAMPLE_SPARSE_WAVES), 0, st, cptr, srows, val, cols, inv_row, m_sub, scan, drow, dcol, dval);
  return hipGetLastError();
}
