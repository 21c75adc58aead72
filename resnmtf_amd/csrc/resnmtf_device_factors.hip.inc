// resnmtf_device_factors.hip.inc -- the factors of a view taken from, and handed back to, device memory
// (resnmtf_set_factors_device / resnmtf_get_factors_device, DESIGN.md section 17).  Included by resnmtf_hip.hip after
// resnmtf_device_view.hip.inc (it uses that file's load_wide).
//
// A source matrix is (pointer, dtype, row stride, column stride) in ELEMENTS, as a view is in resnmtf_device_view.hip.inc.
// The handle keeps a factor as row-major fp64 W[len][k] (S as [k][k]); the raw state leaves it as column-major fp64.
// Widening is exact for fp64 / fp32 / fp16 / bf16 and nothing else is computed on the way in or out, so W and S hold the
// bits the host route uploads.  Three kernels:
//   device_factor_copy_kernel       threads along the columns of the row-major destination: a widening copy of a
//                                   row-major source (torch's default), correct for any strides;
//   device_factor_transpose_kernel  a 32 x 32 tile through LDS: read with threads along the rows (a column-major source,
//                                   row stride 1), written with threads along the columns (column stride 1).  tile[33]
//                                   fp64: the read tile[tx][j] has a pitch of 66 dwords, so the 32 lanes of a half wave
//                                   fall on 32 distinct bank pairs; the write tile[j][tx] is contiguous.  The get direction
//                                   is the same kernel on the transposed problem (W as a k x len matrix of row stride 1);
//   device_factor_colsum_kernel     lambda = colSums(F), mu = colSums(G) (R/update_steps.r:55-56) in the order of
//                                   resnmtf_set_factors' host loop: per column ONE accumulator that starts at 0.0 and takes
//                                   the rows in ascending order.  The additions are sequential; only the loads are shared:
//                                   the workgroup stages kFactorSumChunk contiguous doubles of W (whole rows) in LDS while
//                                   the next chunk is already on its way in registers, and thread j < k then walks
//                                   column j of the staged rows (adjacent lanes on adjacent 8-byte words: conflict-free).

constexpr int kFactorSumChunk = 4096;      // doubles staged per trip (32 KB of LDS): 4096 / k whole rows, 64 at k = 64

template <int DT>
static __global__ __launch_bounds__(256) void device_factor_copy_kernel(const void* __restrict__ src, long long rs, long long cs, int rows,
                                                                        int cols, double* __restrict__ dst /* [rows][cols] */) {
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (size_t)rows * cols) return;
  const long long r = (long long)(idx / cols), c = (long long)(idx % cols);
  dst[idx] = load_wide<DT>(src, r * rs + c * cs);
}

// dst[r * drs + c * dcs] = src[r * rs + c * cs]; one 32 x 32 tile per workgroup, tiles numbered along r first
template <int DT>
static __global__ __launch_bounds__(256) void device_factor_transpose_kernel(const void* __restrict__ src, long long rs, long long cs, int rows,
                                                                             int cols, double* __restrict__ dst, long long drs,
                                                                             long long dcs) {
  __shared__ double tile[32][33];                      // tile[c_local][r_local]
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
  const unsigned tiles_r = (unsigned)((rows + 31) / 32);
  const int r0 = (int)(blockIdx.x % tiles_r) * 32, c0 = (int)(blockIdx.x / tiles_r) * 32;
  for (int j = ty; j < 32; j += 8) {
    const int r = r0 + tx, c = c0 + j;
    if (r < rows && c < cols) tile[j][tx] = load_wide<DT>(src, (long long)r * rs + (long long)c * cs);
  }
  __syncthreads();
  for (int j = ty; j < 32; j += 8) {
    const int r = r0 + j, c = c0 + tx;
    if (r < rows && c < cols) dst[(long long)r * drs + (long long)c * dcs] = tile[tx][j];
  }
}

// block 0: lam[j] = sum over r of WF[r][j]; block 1: mu[j] of WG -- a side whose output is NULL is skipped
static __global__ __launch_bounds__(256) void device_factor_colsum_kernel(const double* __restrict__ WF, int n, double* __restrict__ lam,
                                                                          const double* __restrict__ WG, int m, double* __restrict__ mu,
                                                                          int k) {
  __shared__ double stage[kFactorSumChunk];
  constexpr int PER_THREAD = kFactorSumChunk / 256;
  const double* __restrict__ W = blockIdx.x ? WG : WF;
  double* __restrict__ out = blockIdx.x ? mu : lam;
  if (!out) return;
  const int tid = threadIdx.x;
  const int chunk_rows = kFactorSumChunk / k;
  const int per = chunk_rows * k;                      // doubles per trip
  const long long total = (long long)(blockIdx.x ? m : n) * k;
  double pre[PER_THREAD];
#pragma unroll
  for (int i = 0; i < PER_THREAD; ++i) {
    const int e = tid + 256 * i;
    pre[i] = (e < per && e < total) ? W[e] : 0.0;
  }
  double t = 0.0;
  for (long long base = 0; base < total; base += per) {
#pragma unroll
    for (int i = 0; i < PER_THREAD; ++i) {
      const int e = tid + 256 * i;
      if (e < per) stage[e] = pre[i];
    }
    __syncthreads();
    const long long next = base + per;
#pragma unroll
    for (int i = 0; i < PER_THREAD; ++i) {
      const int e = tid + 256 * i;
      pre[i] = (e < per && next + e < total) ? W[next + e] : 0.0;
    }
    if (tid < k) {
      const long long left = (total - base) / k;       // rows not yet summed
      const int nrows = left < chunk_rows ? (int)left : chunk_rows;
#pragma unroll 8
      for (int r = 0; r < nrows; ++r) t += stage[r * k + tid];
    }
    __syncthreads();
  }
  if (tid < k) out[tid] = t;
}
