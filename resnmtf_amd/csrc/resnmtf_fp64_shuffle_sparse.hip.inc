// resnmtf_fp64_shuffle_sparse.hip.inc -- shuffle_view (R/obtain_bicl.r:11-22) of a SPARSE view in double precision
// (resnmtf_fp64_shuffle_sparse, DESIGN.md section 30): resnmtf_fp64_shuffle's draw made of the stored entries alone.
// Included by resnmtf_fp64.hip only, after resnmtf_feistel.h.
//
// The source arrives as a canonical CSC in device memory (cptr int64, rows int32 ascending within a column, values
// fp64), every index verified (fp64_check_csc on the host route, the main unit's canonicaliser on the device route).
// The destination entries are sorted by the same canonicaliser, handed to it as a COO in any order; its kernels stay the
// main unit's.  What is new here:
//   fp64_shuffle_sparse_dest_kernel     one thread per stored entry e: its column c by bisection of the pointers, its row
//                                       r, then i = feistel_perm_inverse(r m + c, n m, seed) in 64 bits (n m may exceed
//                                       2^32) -> destination row i % n, column i / n.  The values stay where they are: the
//                                       COO's value array is the source's.
//   fp64_shuffle_sparse_mark_kernel     the redraw condition (:14-18): one thread per entry of the sorted draw clears the
//                                       "empty" byte of its row and of its column (bisection) when its value is > 0.  Plain
//                                       byte stores of one value: no order matters.
//   fp64_shuffle_sparse_count_kernel    one thread per line: the two counts, integer atomics.
//   fp64_shuffle_sparse_colsum_kernel   one workgroup per column: sum(x + 0.0) in fp64_shuffle_stats_kernel's order over
//                                       the stored entries -- lane t of 256 owns the rows = t (mod 256), ascending, from
//                                       0.0; then the 256-wide LDS tree.  The column is walked one block of 256 rows per
//                                       trip: the at most 256 entries of a block have distinct residues and go to
//                                       acc[row % 256], a barrier between trips keeps a residue's additions in row order.
//                                       Absent entries would add +0.0 to a non-negative sum: no bit changes.
//   fp64_shuffle_sparse_divide_kernel   out[e] = (x + 0.0) / colsum[c], one workgroup per column; 0 / 0 = NaN stays.
//   fp64_shuffle_sparse_widen_kernel    the int32 row indices as int64 into the caller's array.
// No floating-point atomics, no waits between workgroups; entry offsets are 64-bit throughout.

// the column of entry e: the c with cptr[c] <= e < cptr[c + 1] (cptr[0] = 0 <= e < nnz = cptr[m]; empty columns skipped)
static __device__ __forceinline__ int f64_shuffle_sparse_column(const long long* __restrict__ cptr, int m, long long e) {
  int lo = 0, hi = m;
  while (hi - lo > 1) {
    const int mid = lo + (hi - lo) / 2;
    if (cptr[mid] <= e) lo = mid; else hi = mid;
  }
  return lo;
}

static __global__ void __launch_bounds__(256)
fp64_shuffle_sparse_dest_kernel(const long long* __restrict__ cptr, const int* __restrict__ rows, long long nnz, unsigned long long n,
                                int m, unsigned long long count, int half_bits, unsigned long long seed, int* __restrict__ drow,
                                int* __restrict__ dcol) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= nnz) return;
  const unsigned long long c = (unsigned long long)f64_shuffle_sparse_column(cptr, m, e);
  const unsigned long long j = (unsigned long long)rows[e] * (unsigned long long)m + c;
  const unsigned long long i = feistel_perm_inverse(j, count, half_bits, seed);
  drow[e] = (int)(i % n);
  dcol[e] = (int)(i / n);
}

// mask[0 .. n) rows, mask[n .. n + m) columns, all 1 on entry
static __global__ void __launch_bounds__(256)
fp64_shuffle_sparse_mark_kernel(const long long* __restrict__ cptr, const int* __restrict__ rows, const double* __restrict__ val,
                                long long nnz, int n, int m, unsigned char* __restrict__ mask) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= nnz || !(val[e] > 0.0)) return;
  mask[rows[e]] = 0;
  mask[(size_t)n + (size_t)f64_shuffle_sparse_column(cptr, m, e)] = 0;
}

static __global__ void __launch_bounds__(256)
fp64_shuffle_sparse_count_kernel(const unsigned char* __restrict__ mask, int n, int m, int* __restrict__ counts) {
  const long long line = (long long)blockIdx.x * 256 + threadIdx.x;
  if (line >= (long long)n + m) return;
  if (mask[line]) atomicAdd(&counts[line < n ? 0 : 1], 1);
}

static __global__ void __launch_bounds__(256)
fp64_shuffle_sparse_colsum_kernel(const long long* __restrict__ cptr, const int* __restrict__ rows, const double* __restrict__ val,
                                  double* __restrict__ colsum) {
  __shared__ double acc[256];
  __shared__ long long next[2];                    // where the next trip starts, by the parity of the trip
  const int t = threadIdx.x;
  const long long end = cptr[blockIdx.x + 1];
  long long pos = cptr[blockIdx.x];
  acc[t] = 0.0;
  __syncthreads();
  for (int trip = 0; pos < end; ++trip) {          // (pos is the same in every lane)
    const int block = rows[pos] >> 8;
    const long long e = pos + t;
    if (e < end && (rows[e] >> 8) == block) {      // the lanes that hold an entry of this block are 0 .. count - 1
      acc[rows[e] & 255] += val[e] + 0.0;
      if (t == 255 || e + 1 >= end || (rows[e + 1] >> 8) != block) next[trip & 1] = e + 1;       // exactly one lane
    }
    __syncthreads();
    pos = next[trip & 1];
  }
  for (int s = 128; s > 0; s >>= 1) {
    if (t < s) acc[t] += acc[t + s];
    __syncthreads();
  }
  if (t == 0) colsum[blockIdx.x] = acc[0];
}

static __global__ void __launch_bounds__(64)
fp64_shuffle_sparse_divide_kernel(const long long* __restrict__ cptr, const double* __restrict__ val, const double* __restrict__ colsum,
                                  double* __restrict__ out) {
  const double cs = colsum[blockIdx.x];
  const long long end = cptr[blockIdx.x + 1];
  for (long long e = cptr[blockIdx.x] + threadIdx.x; e < end; e += 64) out[e] = (val[e] + 0.0) / cs;
}

static __global__ void __launch_bounds__(256)
fp64_shuffle_sparse_widen_kernel(const int* __restrict__ src, long long nnz, long long* __restrict__ dst) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e < nnz) dst[e] = (long long)src[e];
}

// ---- launches (nnz >= 1) ----
inline unsigned f64_shuffle_sparse_grid(long long count) { return (unsigned)((count + 255) / 256); }

inline void fp64_shuffle_sparse_dest(hipStream_t st, const long long* cptr, const int* rows, long long nnz, int n, int m,
                                     unsigned long long seed, int* drow, int* dcol) {
  const unsigned long long count = (unsigned long long)n * (unsigned long long)m;
  hipLaunchKernelGGL(fp64_shuffle_sparse_dest_kernel, dim3(f64_shuffle_sparse_grid(nnz)), dim3(256), 0, st, cptr, rows, nnz,
                     (unsigned long long)n, m, count, feistel_half_bits(count), seed, drow, dcol);
}
// the masks (all lines empty on entry: set here) and the two counts (zero on entry)
inline hipError_t fp64_shuffle_sparse_lines(hipStream_t st, const long long* cptr, const int* rows, const double* val, long long nnz,
                                            int n, int m, unsigned char* mask, int* counts) {
  const hipError_t e = hipMemsetAsync(mask, 1, (size_t)n + (size_t)m, st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(fp64_shuffle_sparse_mark_kernel, dim3(f64_shuffle_sparse_grid(nnz)), dim3(256), 0, st, cptr, rows, val, nnz, n, m, mask);
  hipLaunchKernelGGL(fp64_shuffle_sparse_count_kernel, dim3(f64_shuffle_sparse_grid((long long)n + m)), dim3(256), 0, st,
                     (const unsigned char*)mask, n, m, counts);
  return hipGetLastError();
}
inline void fp64_shuffle_sparse_normalise(hipStream_t st, const long long* cptr, const int* rows, const double* val, int m, double* colsum,
                                          double* out) {
  hipLaunchKernelGGL(fp64_shuffle_sparse_colsum_kernel, dim3((unsigned)m), dim3(256), 0, st, cptr, rows, val, colsum);
  hipLaunchKernelGGL(fp64_shuffle_sparse_divide_kernel, dim3((unsigned)m), dim3(64), 0, st, cptr, val, (const double*)colsum, out);
}
inline void fp64_shuffle_sparse_widen(hipStream_t st, const int* src, long long nnz, long long* dst) {
  hipLaunchKernelGGL(fp64_shuffle_sparse_widen_kernel, dim3(f64_shuffle_sparse_grid(nnz)), dim3(256), 0, st, src, nnz, dst);
}
