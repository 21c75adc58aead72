// resnmtf_fp64_device.hip.inc -- views and initial factors of the device-wide fp64 path taken from device memory
// (resnmtf_fp64_run_device, DESIGN.md section 23).  Included by resnmtf_fp64.hip only.
//
// A source matrix is (pointer, dtype, row stride, column stride) in ELEMENTS, strides >= 0, as resnmtf_device_matrix
// describes it.  Widening fp32 / fp16 / bf16 to fp64 is exact and nothing else is computed, so what these kernels write
// is byte for byte what the host route uploads.  Three kernels:
//   fp64_images_kernel<DT, ROWS_FAST>   one read of the n x m source, both images of section 21 written: X column-major
//                                       with leading dimension ldn, X^T column-major with leading dimension ldm.  A
//                                       32 x 32 tile per workgroup goes through LDS; the padding of the images stays the
//                                       zeros of the buffer's memset (nothing outside n x m is written).
//   fp64_factors_in_kernel<DT, ROWS_FAST>  the same tile, one destination: rows x cols column-major, contiguous (an
//                                       initial F, S or G in its slot; lambda0 / mu0 as a k x 1 matrix).
//   fp64_colsum_seq_kernel              lambda = colSums(F0), mu = colSums(G0) when they are not given: one lane per
//                                       column, one accumulator from 0.0 over ascending rows -- the host loop's order.
//
// The tile.  256 threads are 32 lanes (tx) x 8 (ty).  ROWS_FAST says along which axis the source has the smaller
// stride, and neighbouring lanes read along it: ROWS_FAST (a column-major source) lane tx reads row r0 + tx, else (a
// row-major one, torch's default) column c0 + tx.  Either way the staging store is tile[j][tx], 32 lanes on 32
// consecutive doubles.  tile[32][33] doubles: a pitch of 66 dwords.  A destination whose unit stride runs along the
// axis the lanes read along takes tile[j][tx] back (contiguous); the other one takes tile[tx][j], whose 32 lanes of a
// half wave sit at dwords 66 tx + 2 j, i.e. on bank pairs (2 tx + 2 j) mod 64: 32 distinct pairs, no conflict
// (ds_read_b64 banks per 32-lane half over 64 dwords).  Every global store has neighbouring lanes on neighbouring
// doubles of its image.  Offsets are size_t throughout: an image of 50000 x 8000 has 4e8 entries, a strided source can
// reach further.

constexpr int F64_DEV_TILE = 32;

template <int DT>
__device__ __forceinline__ double f64_load_wide(const void* __restrict__ src, size_t i) {
  if constexpr (DT == RESNMTF_DTYPE_F64) return static_cast<const double*>(src)[i];
  else if constexpr (DT == RESNMTF_DTYPE_F32) return (double)static_cast<const float*>(src)[i];
  else if constexpr (DT == RESNMTF_DTYPE_F16) return (double)static_cast<const _Float16*>(src)[i];
  else return (double)__uint_as_float((unsigned int)static_cast<const unsigned short*>(src)[i] << 16);   // bf16 = the top half of an f32
}

// the tile at (r0, c0) of the rows x cols source into LDS; ROWS_FAST: tile[c_local][r_local], else tile[r_local][c_local]
template <int DT, bool ROWS_FAST>
__device__ __forceinline__ void f64_tile_in(double (&tile)[F64_DEV_TILE][F64_DEV_TILE + 1], const void* __restrict__ src, size_t rs,
                                            size_t cs, int rows, int cols, int r0, int c0, int tx, int ty) {
  for (int j = ty; j < F64_DEV_TILE; j += 8) {
    const int r = ROWS_FAST ? r0 + tx : r0 + j, c = ROWS_FAST ? c0 + j : c0 + tx;
    if (r < rows && c < cols) tile[j][tx] = f64_load_wide<DT>(src, (size_t)r * rs + (size_t)c * cs);
  }
}

// the staged tile into a column-major destination dst[r + c * ld] (lanes along r)
template <bool ROWS_FAST>
__device__ __forceinline__ void f64_tile_out_rows(const double (&tile)[F64_DEV_TILE][F64_DEV_TILE + 1], double* __restrict__ dst, size_t ld,
                                                  int rows, int cols, int r0, int c0, int tx, int ty) {
  for (int j = ty; j < F64_DEV_TILE; j += 8) {
    const int r = r0 + tx, c = c0 + j;
    if (r < rows && c < cols) dst[(size_t)r + (size_t)c * ld] = ROWS_FAST ? tile[j][tx] : tile[tx][j];
  }
}

// one workgroup per tile, tiles numbered along the rows first
template <int DT, bool ROWS_FAST>
static __global__ __launch_bounds__(256) void fp64_images_kernel(const void* __restrict__ src, size_t rs, size_t cs, int n, int m,
                                                                 double* __restrict__ X, size_t ldn, double* __restrict__ XT,
                                                                 size_t ldm) {
  __shared__ double tile[F64_DEV_TILE][F64_DEV_TILE + 1];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const unsigned tiles_r = (unsigned)((n + F64_DEV_TILE - 1) / F64_DEV_TILE);
  const int r0 = (int)(blockIdx.x % tiles_r) * F64_DEV_TILE, c0 = (int)(blockIdx.x / tiles_r) * F64_DEV_TILE;
  f64_tile_in<DT, ROWS_FAST>(tile, src, rs, cs, n, m, r0, c0, tx, ty);
  __syncthreads();
  f64_tile_out_rows<ROWS_FAST>(tile, X, ldn, n, m, r0, c0, tx, ty);
  for (int j = ty; j < F64_DEV_TILE; j += 8) {             // X^T[c + r * ldm]: lanes along c
    const int r = r0 + j, c = c0 + tx;
    if (r < n && c < m) XT[(size_t)c + (size_t)r * ldm] = ROWS_FAST ? tile[tx][j] : tile[j][tx];
  }
}

template <int DT, bool ROWS_FAST>
static __global__ __launch_bounds__(256) void fp64_factors_in_kernel(const void* __restrict__ src, size_t rs, size_t cs, int rows,
                                                                     int cols, double* __restrict__ dst /* rows x cols column-major */) {
  __shared__ double tile[F64_DEV_TILE][F64_DEV_TILE + 1];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const unsigned tiles_r = (unsigned)((rows + F64_DEV_TILE - 1) / F64_DEV_TILE);
  const int r0 = (int)(blockIdx.x % tiles_r) * F64_DEV_TILE, c0 = (int)(blockIdx.x / tiles_r) * F64_DEV_TILE;
  f64_tile_in<DT, ROWS_FAST>(tile, src, rs, cs, rows, cols, r0, c0, tx, ty);
  __syncthreads();
  f64_tile_out_rows<ROWS_FAST>(tile, dst, (size_t)rows, rows, cols, r0, c0, tx, ty);
}

// block 0: lam[c] = sum over i of F[i + c n]; block 1: mu[c] of G (column-major) -- a side whose output is NULL is skipped.
// Lane c owns column c: the additions of a column are sequential (the host loop's order, from 0.0); eight loads are
// issued ahead of the eight additions that use them.
static __global__ __launch_bounds__(64) void fp64_colsum_seq_kernel(const double* __restrict__ F, int n, double* __restrict__ lam,
                                                                    const double* __restrict__ G, int m, double* __restrict__ mu, int k) {
  const double* __restrict__ P = blockIdx.x ? G : F;
  double* __restrict__ out = blockIdx.x ? mu : lam;
  const int len = blockIdx.x ? m : n;
  const int c = threadIdx.x;
  if (!out || c >= k) return;
  const double* __restrict__ col = P + (size_t)c * len;
  double t = 0.0;
  int i = 0;
  for (; i + 8 <= len; i += 8) {
    double x[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) x[q] = col[i + q];
#pragma unroll
    for (int q = 0; q < 8; ++q) t += x[q];
  }
  for (; i < len; ++i) t += col[i];
  out[c] = t;
}

// ---- launches ----
// neighbouring lanes read along the source's smaller stride (a tie: along the rows)
template <int DT>
void f64_launch_images(hipStream_t st, const resnmtf_device_matrix& x, int n, int m, double* X, size_t ldn, double* XT, size_t ldm) {
  const unsigned tiles = (unsigned)((n + F64_DEV_TILE - 1) / F64_DEV_TILE) * (unsigned)((m + F64_DEV_TILE - 1) / F64_DEV_TILE);
  const size_t rs = (size_t)x.row_stride, cs = (size_t)x.col_stride;
  if (rs <= cs) hipLaunchKernelGGL((fp64_images_kernel<DT, true>), dim3(tiles), dim3(256), 0, st, x.ptr, rs, cs, n, m, X, ldn, XT, ldm);
  else hipLaunchKernelGGL((fp64_images_kernel<DT, false>), dim3(tiles), dim3(256), 0, st, x.ptr, rs, cs, n, m, X, ldn, XT, ldm);
}
inline void fp64_images(hipStream_t st, const resnmtf_device_matrix& x, int n, int m, double* X, size_t ldn, double* XT, size_t ldm) {
  switch (x.dtype) {
    case RESNMTF_DTYPE_F64: f64_launch_images<RESNMTF_DTYPE_F64>(st, x, n, m, X, ldn, XT, ldm); break;
    case RESNMTF_DTYPE_F32: f64_launch_images<RESNMTF_DTYPE_F32>(st, x, n, m, X, ldn, XT, ldm); break;
    case RESNMTF_DTYPE_F16: f64_launch_images<RESNMTF_DTYPE_F16>(st, x, n, m, X, ldn, XT, ldm); break;
    default: f64_launch_images<RESNMTF_DTYPE_BF16>(st, x, n, m, X, ldn, XT, ldm); break;
  }
}

template <int DT>
void f64_launch_factors_in(hipStream_t st, const resnmtf_device_matrix& a, int rows, int cols, double* dst) {
  const unsigned tiles = (unsigned)((rows + F64_DEV_TILE - 1) / F64_DEV_TILE) * (unsigned)((cols + F64_DEV_TILE - 1) / F64_DEV_TILE);
  const size_t rs = (size_t)a.row_stride, cs = (size_t)a.col_stride;
  if (rs <= cs) hipLaunchKernelGGL((fp64_factors_in_kernel<DT, true>), dim3(tiles), dim3(256), 0, st, a.ptr, rs, cs, rows, cols, dst);
  else hipLaunchKernelGGL((fp64_factors_in_kernel<DT, false>), dim3(tiles), dim3(256), 0, st, a.ptr, rs, cs, rows, cols, dst);
}
inline void fp64_factors_in(hipStream_t st, const resnmtf_device_matrix& a, int rows, int cols, double* dst) {
  switch (a.dtype) {
    case RESNMTF_DTYPE_F64: f64_launch_factors_in<RESNMTF_DTYPE_F64>(st, a, rows, cols, dst); break;
    case RESNMTF_DTYPE_F32: f64_launch_factors_in<RESNMTF_DTYPE_F32>(st, a, rows, cols, dst); break;
    case RESNMTF_DTYPE_F16: f64_launch_factors_in<RESNMTF_DTYPE_F16>(st, a, rows, cols, dst); break;
    default: f64_launch_factors_in<RESNMTF_DTYPE_BF16>(st, a, rows, cols, dst); break;
  }
}
