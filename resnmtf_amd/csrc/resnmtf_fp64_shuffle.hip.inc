// resnmtf_fp64_shuffle.hip.inc -- shuffle_view (R/obtain_bicl.r:11-22) of a view in double precision
// (resnmtf_fp64_shuffle, DESIGN.md section 27): the draw obtain_shuffled_f (:31-42) factorises, made of the numbers that
// precision="fp64" factorised.  Included by resnmtf_fp64.hip only, after resnmtf_fp64_device.hip.inc (f64_load_wide).
//
// Four kernels, the gather form of the main unit's staged route (shuffle_gather_kernel -> empty_lines_kernel ->
// column_stats_kernel -> the division convert_x_kernel fuses), with two differences: the source is read where it lies -- a
// resnmtf_device_matrix of fp64 / fp32 / fp16 / bf16 with any strides >= 0, pi(i) -> (row, col) -> strides, no image in
// between -- and the destination is the caller's n x m fp64 column-major array, normalised in place.
//   fp64_shuffle_gather_kernel<DT>  out[i] = X[pi(i)]: i column-major in out, pi(i) row-major in X, pi = feistel_perm of
//                                   csrc/resnmtf_feistel.h (the text shuffle_gather_kernel runs).  Writes coalesced
//                                   along i; reads one element per random line, F64_SHUFFLE_ILP of them in flight per lane.
//   fp64_shuffle_lines_kernel       the redraw condition (:14-18) on the draw before any shift: a line is empty when its
//                                   sum is exactly 0.0; empty_lines_kernel's sums in its order (a row: columns ascending;
//                                   a column: rows ascending).  The two counts are integer atomics.
//   fp64_shuffle_stats_kernel       column_stats_kernel, statement by statement: lane t of 256 takes rows t, t + 256,
//                                   ..., then the 256-wide tree, for the minimum and then for sum(x + shift).
//   fp64_shuffle_divide_kernel      out[r, c] = (out[r, c] + shift[c]) / colsum[c], in fp64 (R/utils.r:22, :87); a column
//                                   that shifted to all zero divides 0 / 0 = NaN as sweep(..., "/") does.
// No floating-point atomics, no waits between workgroups; offsets are size_t / 64-bit throughout.

constexpr int F64_SHUFFLE_ILP = 4;             // elements per lane and trip of the gather: that many loads in flight

template <int DT>
static __global__ void __launch_bounds__(256)
fp64_shuffle_gather_kernel(const void* __restrict__ src, size_t rs, size_t cs, unsigned long long m, unsigned long long count,
                           int half_bits, unsigned long long seed, double* __restrict__ out) {
  const unsigned long long step = (unsigned long long)gridDim.x * (256 * F64_SHUFFLE_ILP);
  for (unsigned long long base = (unsigned long long)blockIdx.x * (256 * F64_SHUFFLE_ILP) + threadIdx.x; base < count; base += step) {
    double val[F64_SHUFFLE_ILP];
#pragma unroll
    for (int u = 0; u < F64_SHUFFLE_ILP; ++u) {
      const unsigned long long i = base + (unsigned long long)u * 256;
      if (i < count) {
        const unsigned long long j = feistel_perm(i, count, half_bits, seed);
        val[u] = f64_load_wide<DT>(src, (size_t)(j / m) * rs + (size_t)(j % m) * cs);
      }
    }
#pragma unroll
    for (int u = 0; u < F64_SHUFFLE_ILP; ++u) {
      const unsigned long long i = base + (unsigned long long)u * 256;
      if (i < count) out[i] = val[u];
    }
  }
}

// mask[0 .. n) rows, mask[n .. n + m) columns; counts[0 / 1]
static __global__ void __launch_bounds__(256)
fp64_shuffle_lines_kernel(const double* __restrict__ src, int n, int m, unsigned char* __restrict__ mask, int* __restrict__ counts) {
  const long long line = (long long)blockIdx.x * 256 + threadIdx.x;
  if (line >= (long long)n + m) return;
  double s = 0.0;
  if (line < n) { for (int c = 0; c < m; ++c) s += src[(size_t)c * n + (size_t)line]; }     // row sum (coalesced across lanes)
  else { const double* col = src + (size_t)(line - n) * n; for (int r = 0; r < n; ++r) s += col[r]; }
  const bool empty = s == 0.0;
  mask[line] = empty ? 1 : 0;
  if (empty) atomicAdd(&counts[line < n ? 0 : 1], 1);
}

// one workgroup per column c: shift[c] = |min(0, min(x[, c]))|, colsum[c] = sum(x[, c] + shift[c]), *neg |= shift > 0
static __global__ void __launch_bounds__(256)
fp64_shuffle_stats_kernel(const double* __restrict__ src, int n, double* __restrict__ shift, double* __restrict__ colsum,
                          int* __restrict__ neg) {
  __shared__ double red[256];
  const int c = blockIdx.x;
  const double* col = src + (size_t)c * n;
  double mn = 0.0;                                     // min(0, min(x))
  for (long long r = threadIdx.x; r < n; r += 256) mn = fmin(mn, col[r]);
  red[threadIdx.x] = mn;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] = fmin(red[threadIdx.x], red[threadIdx.x + s]);
    __syncthreads();
  }
  const double sh = fabs(red[0]);
  __syncthreads();
  double sum = 0.0;
  for (long long r = threadIdx.x; r < n; r += 256) sum += col[r] + sh;
  red[threadIdx.x] = sum;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    shift[c] = sh;
    colsum[c] = red[0];
    if (sh > 0.0) atomicOr(neg, 1);
  }
}

// blockIdx.y = the column, lanes along its rows
static __global__ void __launch_bounds__(256)
fp64_shuffle_divide_kernel(double* __restrict__ x, int n, const double* __restrict__ shift, const double* __restrict__ colsum) {
  const int c = blockIdx.y;
  const double sh = shift[c], cs = colsum[c];
  double* col = x + (size_t)c * n;
  for (long long r = (long long)blockIdx.x * 256 + threadIdx.x; r < n; r += (long long)gridDim.x * 256) col[r] = (col[r] + sh) / cs;
}

// ---- launches ----
template <int DT>
void f64_shuffle_launch_gather(hipStream_t st, const resnmtf_device_matrix& x, int n, int m, unsigned long long seed, double* out) {
  const unsigned long long count = (unsigned long long)n * (unsigned long long)m;
  const unsigned long long per_block = 256ull * F64_SHUFFLE_ILP;
  const unsigned blocks = (unsigned)std::min<unsigned long long>((count + per_block - 1) / per_block, 1u << 20);
  hipLaunchKernelGGL((fp64_shuffle_gather_kernel<DT>), dim3(blocks), dim3(256), 0, st, x.ptr, (size_t)x.row_stride, (size_t)x.col_stride,
                     (unsigned long long)m, count, feistel_half_bits(count), seed, out);
}
inline void fp64_shuffle_gather(hipStream_t st, const resnmtf_device_matrix& x, int n, int m, unsigned long long seed, double* out) {
  switch (x.dtype) {
    case RESNMTF_DTYPE_F64: f64_shuffle_launch_gather<RESNMTF_DTYPE_F64>(st, x, n, m, seed, out); break;
    case RESNMTF_DTYPE_F32: f64_shuffle_launch_gather<RESNMTF_DTYPE_F32>(st, x, n, m, seed, out); break;
    case RESNMTF_DTYPE_F16: f64_shuffle_launch_gather<RESNMTF_DTYPE_F16>(st, x, n, m, seed, out); break;
    default: f64_shuffle_launch_gather<RESNMTF_DTYPE_BF16>(st, x, n, m, seed, out); break;
  }
}
inline void fp64_shuffle_lines(hipStream_t st, const double* out, int n, int m, unsigned char* mask, int* counts) {
  const unsigned blocks = (unsigned)(((long long)n + m + 255) / 256);
  hipLaunchKernelGGL(fp64_shuffle_lines_kernel, dim3(blocks), dim3(256), 0, st, out, n, m, mask, counts);
}
inline void fp64_shuffle_normalise(hipStream_t st, double* out, int n, int m, double* shift, double* colsum, int* neg) {
  // (a grid's y extent ends at 65535: the columns go in slices of that many)
  for (long long c0 = 0; c0 < m; c0 += 65535) {
    const int mc = (int)std::min<long long>(65535, m - c0);
    double* x = out + (size_t)c0 * n;
    hipLaunchKernelGGL(fp64_shuffle_stats_kernel, dim3(mc), dim3(256), 0, st, (const double*)x, n, shift + c0, colsum + c0, neg);
    hipLaunchKernelGGL(fp64_shuffle_divide_kernel, dim3((unsigned)std::min<long long>(((long long)n + 255) / 256, 64), mc), dim3(256), 0, st, x, n,
                       (const double*)(shift + c0), (const double*)(colsum + c0));
  }
}
