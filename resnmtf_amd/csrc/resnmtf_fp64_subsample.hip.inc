// resnmtf_fp64_subsample.hip.inc -- the sub-sample of stability_repeat (R/stability_analysis.r:124, :184, :232, :238:
// data[[i]][row_samples, col_samples]) of a view in double precision (resnmtf_fp64_subsample, DESIGN.md section 28).
// Included by resnmtf_fp64.hip only, after resnmtf_fp64_device.hip.inc (f64_load_wide) and resnmtf_fp64_subsample_job.h
// (the tile edges and the form chooser).
//
// The source is read where it lies -- a resnmtf_device_matrix of fp64 / fp32 / fp16 / bf16 with any strides >= 0 -- and
// the destination is the caller's n_sub x m_sub fp64 column-major array.  Values are carried over, not re-normalised.
//   fp64_subsample_gather_rows_kernel<DT>  form 0: lanes along the destination rows, one destination column per trip of
//                                   blockIdx.y; reads rows[i] * rs apart (neighbours when the source's row stride is
//                                   the smaller), writes coalesced.
//   fp64_subsample_gather_tile_kernel<DT>  form 1: a 32 x 32 destination tile through a padded LDS tile; read with lanes
//                                   along the destination COLUMNS (a row-major source is read along its rows), written
//                                   with lanes along the destination rows: coalesced.
//   fp64_subsample_row_sums_kernel  lane = destination row, columns ascending: coalesced, one running sum per row.
//   fp64_subsample_col_sums_kernel  32 columns per workgroup; tiles of 64 rows x 32 columns are read with lanes along the
//                                   rows (coalesced) into LDS, lane c < 32 then adds its column's 64 rows in ascending
//                                   order into its running sum, carried from tile to tile; the next tile's loads are in
//                                   flight while the lanes add.
// A line is empty when its sum is exactly 0.0 (empty_lines_kernel's sums in its order); the two counts are integer
// atomics.  No floating-point atomics, no waits between workgroups; offsets are size_t / 64-bit throughout.

template <int DT>
static __global__ void __launch_bounds__(F64_SUB_BLOCK)
fp64_subsample_gather_rows_kernel(const void* __restrict__ src, size_t rs, size_t cs, const int* __restrict__ rows,
                                  const int* __restrict__ cols, int n_sub, int m_sub, double* __restrict__ out) {
  const long long i = (long long)blockIdx.x * F64_SUB_BLOCK + threadIdx.x;
  if (i >= n_sub) return;
  const size_t ro = (size_t)rows[i] * rs;
  for (int c = blockIdx.y; c < m_sub; c += gridDim.y)
    out[(size_t)c * (size_t)n_sub + (size_t)i] = f64_load_wide<DT>(src, ro + (size_t)cols[c] * cs);
}

// blockIdx.x = the row tile, blockIdx.y strides over the column tiles; 256 threads as 32 x 8
template <int DT>
static __global__ void __launch_bounds__(F64_SUB_BLOCK)
fp64_subsample_gather_tile_kernel(const void* __restrict__ src, size_t rs, size_t cs, const int* __restrict__ rows,
                                  const int* __restrict__ cols, int n_sub, int m_sub, double* __restrict__ out) {
  __shared__ double tile[F64_SUB_TILE][F64_SUB_TILE + 1];              // [destination row][destination column]
  const int tx = threadIdx.x & (F64_SUB_TILE - 1), ty = threadIdx.x / F64_SUB_TILE;
  const long long r0 = (long long)blockIdx.x * F64_SUB_TILE;
  const int col_tiles = (m_sub + F64_SUB_TILE - 1) / F64_SUB_TILE;
  for (int ct = blockIdx.y; ct < col_tiles; ct += gridDim.y) {
    const long long c0 = (long long)ct * F64_SUB_TILE;
    const long long c = c0 + tx;
    const size_t co = c < m_sub ? (size_t)cols[c] * cs : 0;
    for (int j = ty; j < F64_SUB_TILE; j += F64_SUB_BLOCK / F64_SUB_TILE) {
      const long long r = r0 + j;
      if (r < n_sub && c < m_sub) tile[j][tx] = f64_load_wide<DT>(src, (size_t)rows[r] * rs + co);
    }
    __syncthreads();
    const long long rw = r0 + tx;
    for (int j = ty; j < F64_SUB_TILE; j += F64_SUB_BLOCK / F64_SUB_TILE) {
      const long long cw = c0 + j;
      if (rw < n_sub && cw < m_sub) out[(size_t)cw * (size_t)n_sub + (size_t)rw] = tile[tx][j];
    }
    __syncthreads();
  }
}

static __global__ void __launch_bounds__(F64_SUB_ROWSUM_BLOCK)
fp64_subsample_row_sums_kernel(const double* __restrict__ src, int n_sub, int m_sub, unsigned char* __restrict__ mask,
                               int* __restrict__ count) {
  const long long i = (long long)blockIdx.x * F64_SUB_ROWSUM_BLOCK + threadIdx.x;
  if (i >= n_sub) return;
  const double* p = src + (size_t)i;
  double s = 0.0;
  int c = 0;
  for (; c + 8 <= m_sub; c += 8) {                   // eight loads in flight, added in column order
    double v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = p[(size_t)(c + u) * (size_t)n_sub];
#pragma unroll
    for (int u = 0; u < 8; ++u) s += v[u];
  }
  for (; c < m_sub; ++c) s += p[(size_t)c * (size_t)n_sub];
  const bool empty = s == 0.0;
  mask[i] = empty ? 1 : 0;
  if (empty) atomicAdd(count, 1);
}

static __global__ void __launch_bounds__(F64_SUB_BLOCK)
fp64_subsample_col_sums_kernel(const double* __restrict__ src, int n_sub, int m_sub, unsigned char* __restrict__ mask,
                               int* __restrict__ count) {
  constexpr int TR = F64_SUB_COLSUM_ROWS, TC = F64_SUB_COLSUM_COLS, PER = TR * TC / F64_SUB_BLOCK;      // 8 elements per thread
  __shared__ double tile[TC][TR + 1];                                  // [column][row]
  const int rl = threadIdx.x % TR, cg = threadIdx.x / TR;              // the row of the tile, the first of its columns
  const long long c0 = (long long)blockIdx.x * TC;
  double v[PER];
  auto load = [&](long long r0) {
    const long long r = r0 + rl;
#pragma unroll
    for (int u = 0; u < PER; ++u) {
      const long long c = c0 + cg + u * (F64_SUB_BLOCK / TR);
      v[u] = (r < n_sub && c < m_sub) ? src[(size_t)c * (size_t)n_sub + (size_t)r] : 0.0;
    }
  };
  double s = 0.0;
  load(0);
  for (long long r0 = 0; r0 < n_sub; r0 += TR) {
#pragma unroll
    for (int u = 0; u < PER; ++u) tile[cg + u * (F64_SUB_BLOCK / TR)][rl] = v[u];
    __syncthreads();
    if (r0 + TR < n_sub) load(r0 + TR);
    if (threadIdx.x < TC) {
      const int len = (int)(n_sub - r0 < TR ? n_sub - r0 : TR);        // (rows past the end are not added: -0.0 + 0.0)
      for (int r = 0; r < len; ++r) s += tile[threadIdx.x][r];
    }
    __syncthreads();
  }
  const long long c = c0 + threadIdx.x;
  if (threadIdx.x < TC && c < m_sub) {
    const bool empty = s == 0.0;
    mask[c] = empty ? 1 : 0;
    if (empty) atomicAdd(count, 1);
  }
}

// ---- launches ----
template <int DT>
void f64_subsample_launch_gather(hipStream_t st, const resnmtf_device_matrix& x, const int* rows, const int* cols, int n_sub, int m_sub,
                                 double* out) {
  const size_t rs = (size_t)x.row_stride, cs = (size_t)x.col_stride;
  if (f64_subsample_form(x.row_stride, x.col_stride) == 0) {
    const dim3 grid((unsigned)(((long long)n_sub + F64_SUB_BLOCK - 1) / F64_SUB_BLOCK), (unsigned)std::min(m_sub, 65535));
    hipLaunchKernelGGL((fp64_subsample_gather_rows_kernel<DT>), grid, dim3(F64_SUB_BLOCK), 0, st, x.ptr, rs, cs, rows, cols, n_sub, m_sub, out);
  } else {
    const int col_tiles = (m_sub + F64_SUB_TILE - 1) / F64_SUB_TILE;
    const dim3 grid((unsigned)(((long long)n_sub + F64_SUB_TILE - 1) / F64_SUB_TILE), (unsigned)std::min(col_tiles, 65535));
    hipLaunchKernelGGL((fp64_subsample_gather_tile_kernel<DT>), grid, dim3(F64_SUB_BLOCK), 0, st, x.ptr, rs, cs, rows, cols, n_sub, m_sub, out);
  }
}
inline void fp64_subsample_gather(hipStream_t st, const resnmtf_device_matrix& x, const int* rows, const int* cols, int n_sub, int m_sub,
                                  double* out) {
  switch (x.dtype) {
    case RESNMTF_DTYPE_F64: f64_subsample_launch_gather<RESNMTF_DTYPE_F64>(st, x, rows, cols, n_sub, m_sub, out); break;
    case RESNMTF_DTYPE_F32: f64_subsample_launch_gather<RESNMTF_DTYPE_F32>(st, x, rows, cols, n_sub, m_sub, out); break;
    case RESNMTF_DTYPE_F16: f64_subsample_launch_gather<RESNMTF_DTYPE_F16>(st, x, rows, cols, n_sub, m_sub, out); break;
    default: f64_subsample_launch_gather<RESNMTF_DTYPE_BF16>(st, x, rows, cols, n_sub, m_sub, out); break;
  }
}
// mask[0 .. n_sub) rows, mask[n_sub .. n_sub + m_sub) columns; counts[0 / 1]
inline void fp64_subsample_lines(hipStream_t st, const double* out, int n_sub, int m_sub, unsigned char* mask, int* counts) {
  hipLaunchKernelGGL(fp64_subsample_row_sums_kernel, dim3((unsigned)(((long long)n_sub + F64_SUB_ROWSUM_BLOCK - 1) / F64_SUB_ROWSUM_BLOCK)),
                     dim3(F64_SUB_ROWSUM_BLOCK), 0, st, out, n_sub, m_sub, mask, counts);
  hipLaunchKernelGGL(fp64_subsample_col_sums_kernel, dim3((unsigned)(((long long)m_sub + F64_SUB_COLSUM_COLS - 1) / F64_SUB_COLSUM_COLS)),
                     dim3(F64_SUB_BLOCK), 0, st, out, n_sub, m_sub, mask + n_sub, counts + 1);
}
