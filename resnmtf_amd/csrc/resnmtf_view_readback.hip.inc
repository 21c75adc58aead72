// resnmtf_view_readback.hip.inc -- what a handle holds, handed to the caller in device memory, and the one result it takes
// back from there (resnmtf_get_view_device / resnmtf_get_view_sparse_device / resnmtf_set_reference_clusters_device,
// DESIGN.md section 18).  Included by resnmtf_hip.hip after resnmtf_device_view.hip.inc (it uses that file's load_wide).
//
// Nothing is computed: a stored f32 is kept or widened (exact), a stored index is kept or widened, a 0 / 1 entry becomes
// a byte.  No kernel uses an atomic and none depends on its grid beyond covering its elements.  Four kernels:
//   view_readback_kernel        a 32 x 32 tile of the dense view through LDS.  Read from Xt32, the tile-major image
//                               resnmtf_get_view reads (xidx(c, r, ts): 64 consecutive rows of one column are contiguous),
//                               with threads along the rows, so a half wave reads 128 contiguous bytes whatever the pitch
//                               padding of ts; written with threads along the rows (ALONG_C = false: a column-major
//                               output, row stride the smaller) or along the columns (true: row-major).  tile[32][33]
//                               f32: the transposed read tile[tx][j] has a pitch of 33 dwords, 32 distinct banks;
//   readback_convert_kernel     dst[i] = (DST)src[i]: the int64 pointers as int32, the int32 indices as int64, the f32
//                               values as fp64 (a kept type is a device-to-device copy, no kernel);
//   readback_expand_rows_kernel COO: the row of stored entry e of the CSR copy, rows[e] = the r with ptr[r] <= e <
//                               ptr[r + 1], by a binary search per entry over the n + 1 pointers (empty rows are passed
//                               over: the LAST r with ptr[r] <= e).  A pure function of e and ptr: a fixed order;
//   reference_clusters_pack_kernel  a 32 x 32 tile of a strided 0 / 1 matrix of any of the four types into the row-major
//                               byte block [len][k] that resnmtf_set_reference_clusters uploads; read with threads along
//                               the rows (ALONG_R = true: a column-major source, as resnmtf_finalise_device emits it)
//                               through LDS, or along the columns (false: row-major, no LDS needed); written with
//                               threads along the columns.  An entry other than 0 or 1 (NaN included; -0.0 is 0, as on
//                               the host route: x != 0.0 && x != 1.0) sets *bad = 1 with a plain store (every writer
//                               stores the same value).

template <class OUT, bool ALONG_C>
static __global__ __launch_bounds__(256) void view_readback_kernel(const float* __restrict__ Xt32, size_t tsxt, int n, int m,
                                                                   OUT* __restrict__ out, long long rs, long long cs) {
  __shared__ float tile[32][33];                       // tile[c_local][r_local]
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
  const unsigned tiles_r = (unsigned)((n + 31) / 32);
  const int r0 = (int)(blockIdx.x % tiles_r) * 32, c0 = (int)(blockIdx.x / tiles_r) * 32;
  for (int j = ty; j < 32; j += 8) {
    const int r = r0 + tx, c = c0 + j;
    if (r < n && c < m) tile[j][tx] = Xt32[xidx(c, r, tsxt)];
  }
  __syncthreads();
  for (int j = ty; j < 32; j += 8) {
    const int r = ALONG_C ? r0 + j : r0 + tx, c = ALONG_C ? c0 + tx : c0 + j;
    if (r < n && c < m) out[(long long)r * rs + (long long)c * cs] = (OUT)(ALONG_C ? tile[tx][j] : tile[j][tx]);
  }
}

template <class SRC, class DST>
static __global__ __launch_bounds__(256) void readback_convert_kernel(const SRC* __restrict__ src, long long count, DST* __restrict__ dst) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i < count) dst[i] = (DST)src[i];
}

template <class DST>
static __global__ __launch_bounds__(256) void readback_expand_rows_kernel(const long long* __restrict__ ptr /* [n + 1] */, int n, long long nnz,
                                                                          DST* __restrict__ rows) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= nnz) return;
  int lo = 0, hi = n;                                  // ptr[lo] <= e (ptr[0] = 0) and ptr[hi] > e (ptr[n] = nnz)
  while (hi - lo > 1) {
    const int mid = lo + (hi - lo) / 2;
    if (ptr[mid] <= e) lo = mid; else hi = mid;
  }
  rows[e] = (DST)lo;
}

// dst[r * k + j] = src[r * rs + j * cs] != 0; one 32 x 32 tile per workgroup, tiles numbered along r first
template <int DT, bool ALONG_R>
static __global__ __launch_bounds__(256) void reference_clusters_pack_kernel(const void* __restrict__ src, long long rs, long long cs, int len,
                                                                             int k, unsigned char* __restrict__ dst, int* __restrict__ bad) {
  __shared__ unsigned char tile[32][33];               // tile[j_local][r_local]
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
  const unsigned tiles_r = (unsigned)((len + 31) / 32);
  const int r0 = (int)(blockIdx.x % tiles_r) * 32, j0 = (int)(blockIdx.x / tiles_r) * 32;
  if constexpr (ALONG_R) {
    for (int q = ty; q < 32; q += 8) {
      const int r = r0 + tx, j = j0 + q;
      if (r < len && j < k) {
        const double x = load_wide<DT>(src, (long long)r * rs + (long long)j * cs);
        if (x != 0.0 && x != 1.0) *bad = 1;
        tile[q][tx] = x != 0.0;
      }
    }
    __syncthreads();
    for (int q = ty; q < 32; q += 8) {
      const int r = r0 + q, j = j0 + tx;
      if (r < len && j < k) dst[(size_t)r * k + j] = tile[tx][q];
    }
  } else {
    for (int q = ty; q < 32; q += 8) {
      const int r = r0 + q, j = j0 + tx;
      if (r < len && j < k) {
        const double x = load_wide<DT>(src, (long long)r * rs + (long long)j * cs);
        if (x != 0.0 && x != 1.0) *bad = 1;
        dst[(size_t)r * k + j] = x != 0.0;
      }
    }
  }
}
