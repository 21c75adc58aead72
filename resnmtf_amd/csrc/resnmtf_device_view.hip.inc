// resnmtf_device_view.hip.inc -- a dense view taken straight from device memory (resnmtf_set_view_device, DESIGN.md
// section 15).  Included by resnmtf_hip.hip after resnmtf_kernels.hip.inc.
//
// The source is (pointer, dtype, row stride, column stride) in ELEMENTS: element (r, c) of the n x m view is
// src[r * rs + c * cs].  Column-major (R), row-major (torch), transposed views and slices are all strides.  These kernels
// replace the fp64 staging image of upload_view: they read the source where column_stats_kernel / convert_x_kernel read
// the staging buffer, widen it to fp64 (exact for fp64 / fp32 / fp16 / bf16) and keep EVERY sum order of those two kernels,
// so the images, data_norms and the negative flag are bit for bit those of resnmtf_set_view / resnmtf_set_view_raw of the
// widened matrix:
//   column statistics   256 partials per column, partial p = the ascending sequential sum over the rows r = p (mod 256) of
//                       x + shift, then the 256 -> 1 tree red[p] += red[p + s], s = 128 .. 1; the fmin of the shift is
//                       order-free (fabs() of the result: a -0 gives the same shift as +0);
//   squares             thread (tx, ty) of a 32 x 32 block owns elements (r0 + tx, c0 + ty + 8 i), i = 0 .. 3, in that
//                       order, then the 256 -> 1 tree; reduce_sum_kernel over the blocks as before;
//   value               (x + shift[c]) / colsum[c] in fp64, one rounding to f32.
// Which thread LOADS an element is free.  Two access patterns:
//   generic (any strides; coalesced when rs == 1)   the patterns of the two host-route kernels, threads along r;
//   rows    (cs == 1: a row-major source)           threads along c.  Statistics: a workgroup takes 32 adjacent columns,
//                       thread (cx = tid & 31, py = tid >> 5) keeps the 32 partials py * 32 + q of column cx in registers
//                       and walks the rows base + py * 32 + q, base += 256 (every load = 32 adjacent elements of one row),
//                       then the 256-partial tree of all 32 columns in LDS, laid out [partial][column] (64 KB; lanes on
//                       adjacent 8-byte words, conflict-free).  Conversion: the 32 x 32 block is read along c, X32 is
//                       written straight from the loading thread, and the fp64 value crosses to its owning thread through
//                       a [32][33] fp64 LDS tile (ds_read_b64 at a pitch of 66 dwords: the 32 lanes of a half wave fall on
//                       32 distinct bank pairs), which adds the square and writes Xt32 along r.

template <int DT>
__device__ __forceinline__ double load_wide(const void* __restrict__ src, long long i) {
  if constexpr (DT == RESNMTF_DTYPE_F64) return static_cast<const double*>(src)[i];
  else if constexpr (DT == RESNMTF_DTYPE_F32) return (double)static_cast<const float*>(src)[i];
  else if constexpr (DT == RESNMTF_DTYPE_F16) return (double)static_cast<const _Float16*>(src)[i];
  else return (double)__uint_as_float((unsigned int)static_cast<const unsigned short*>(src)[i] << 16);      // bf16 = the top half of an f32
}

// column_stats_kernel on a strided source: one workgroup per column
template <int DT>
static __global__ __launch_bounds__(256) void device_column_stats_kernel(const void* __restrict__ src, long long rs, long long cs, int n,
                                                                         int m, double* __restrict__ shift,
                                                                         double* __restrict__ colsum, int* __restrict__ neg) {
  __shared__ double red[256];
  const int c = blockIdx.x;
  const long long col = (long long)c * cs;
  double mn = 0.0;                                     // min(0, min(x))
  for (int r = threadIdx.x; r < n; r += 256) mn = fmin(mn, load_wide<DT>(src, col + (long long)r * rs));
  red[threadIdx.x] = mn;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] = fmin(red[threadIdx.x], red[threadIdx.x + s]);
    __syncthreads();
  }
  const double sh = fabs(red[0]);
  __syncthreads();
  double sum = 0.0;
  for (int r = threadIdx.x; r < n; r += 256) sum += load_wide<DT>(src, col + (long long)r * rs) + sh;
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

// the same statistics of a row-major source (cs == 1): 32 adjacent columns per workgroup, see the head of this file
template <int DT>
static __global__ __launch_bounds__(256) void device_column_stats_rows_kernel(const void* __restrict__ src, long long rs, int n, int m,
                                                                              double* __restrict__ shift,
                                                                              double* __restrict__ colsum, int* __restrict__ neg) {
  __shared__ double red[256 * 32];                     // [partial][column]
  const int cx = threadIdx.x & 31, py = threadIdx.x >> 5;
  const int c = blockIdx.x * 32 + cx;
  const bool live = c < m;
  double mn = 0.0;
  if (live) {
    int base = py * 32;
    for (; base + 32 <= n; base += 256) {
#pragma unroll
      for (int q = 0; q < 32; ++q) mn = fmin(mn, load_wide<DT>(src, (long long)(base + q) * rs + c));
    }
    if (base < n)
      for (int r = base; r < n; ++r) mn = fmin(mn, load_wide<DT>(src, (long long)r * rs + c));
  }
  red[py * 32 + cx] = mn;
  __syncthreads();
  if (threadIdx.x < 32) {
    double v = red[threadIdx.x];
    for (int j = 1; j < 8; ++j) v = fmin(v, red[j * 32 + threadIdx.x]);
    red[threadIdx.x] = v;
  }
  __syncthreads();
  const double sh = fabs(red[cx]);
  __syncthreads();
  double acc[32];                                      // partials py * 32 + q of column cx
#pragma unroll
  for (int q = 0; q < 32; ++q) acc[q] = 0.0;
  if (live) {
    int base = py * 32;
    for (; base + 32 <= n; base += 256) {
#pragma unroll
      for (int q = 0; q < 32; ++q) acc[q] += load_wide<DT>(src, (long long)(base + q) * rs + c) + sh;
    }
    if (base < n) {                                    // the ragged last trip: rows base .. n - 1
#pragma unroll
      for (int q = 0; q < 32; ++q)
        if (base + q < n) acc[q] += load_wide<DT>(src, (long long)(base + q) * rs + c) + sh;
    }
  }
#pragma unroll
  for (int q = 0; q < 32; ++q) red[(py * 32 + q) * 32 + cx] = acc[q];
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {                  // red[p][.] += red[p + s][.], p < s, for the 32 columns at once
    for (int i = threadIdx.x; i < s * 32; i += 256) red[i] += red[i + s * 32];
    __syncthreads();
  }
  if (threadIdx.x < 32 && live) {
    shift[c] = sh;
    colsum[c] = red[threadIdx.x];
    if (sh > 0.0) atomicOr(neg, 1);
  }
}

// convert_x_kernel on a strided source.  ROWS: cs == 1, the block is read along c
template <int DT, bool ROWS>
static __global__ __launch_bounds__(256) void device_convert_x_kernel(const void* __restrict__ src, long long rs, long long cs, int n, int m,
                                                                      float* __restrict__ X32, size_t tsx,
                                                                      float* __restrict__ Xt32, size_t tsxt,
                                                                      double* __restrict__ sq_partial,
                                                                      const double* __restrict__ shift,
                                                                      const double* __restrict__ colsum) {
  __shared__ double red[256];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
  const int r0 = blockIdx.x * 32, c0 = blockIdx.y * 32;
  double sq = 0.0;
  if constexpr (ROWS) {
    __shared__ double wide[32][33];                    // wide[r_local][c_local]: the fp64 value on its way to the owning thread
    for (int j = ty; j < 32; j += 8) {
      const int r = r0 + j, c = c0 + tx;
      double d = 0.0;
      if (r < n && c < m) {
        d = load_wide<DT>(src, (long long)r * rs + c);
        if (shift) d = (d + shift[c]) / colsum[c];
        X32[xidx(r, c, tsx)] = (float)d;
      }
      wide[j][tx] = d;
    }
    __syncthreads();
    for (int j = ty; j < 32; j += 8) {
      const int r = r0 + tx, c = c0 + j;
      if (r < n && c < m) {
        const double d = wide[tx][j];
        sq += d * d;
        Xt32[xidx(c, r, tsxt)] = (float)d;
      }
    }
  } else {
    __shared__ float tile[32][33];
    for (int j = ty; j < 32; j += 8) {
      const int r = r0 + tx, c = c0 + j;
      float v = 0.f;
      if (r < n && c < m) {
        double d = load_wide<DT>(src, (long long)r * rs + (long long)c * cs);
        if (shift) d = (d + shift[c]) / colsum[c];
        sq += d * d;
        v = (float)d;
        Xt32[xidx(c, r, tsxt)] = v;
      }
      tile[j][tx] = v;  // tile[c_local][r_local]
    }
    __syncthreads();
    for (int j = ty; j < 32; j += 8) {
      const int r = r0 + j, c = c0 + tx;
      if (r < n && c < m) X32[xidx(r, c, tsx)] = tile[tx][j];
    }
  }
  red[threadIdx.x] = sq;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) sq_partial[blockIdx.y * gridDim.x + blockIdx.x] = red[0];
}
