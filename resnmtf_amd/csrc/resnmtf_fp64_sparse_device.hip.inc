// resnmtf_fp64_sparse_device.hip.inc -- sparse views of the device-wide fp64 path taken from device memory
// (resnmtf_fp64_run_sparse_device, DESIGN.md section 24).  Included by resnmtf_fp64.hip only.
//
// The caller's CSC / CSR / COO arrays are checked and sorted by the main unit's kernels (resnmtf_sparse_device_canonical,
// resnmtf_internal.h): this unit holds no copy of them.  What that leaves in transient memory is the canonical structure
// in the fp64 path's own types -- int64 line pointers and int32 indices of the CSC and of the CSR --, the values in CSC
// order as fp64 and the CSC position of every CSR entry.  Two kernels finish the view:
//   fp64_spd_longest_kernel   the longest row and the longest column: one thread per line, its length from two
//                             neighbouring pointers (coalesced), a wave maximum by shuffles, the wave maxima through
//                             LDS, one integer atomicMax per workgroup and side.  An integer maximum has no order, so
//                             the two ints are the host's (fp64_check_csc) whatever the arrival order.  They size the
//                             slab (f64_plan_sparse) and, with the failure word, are all the host reads back;
//   fp64_spd_gather_kernel    the CSR values: rval[p] = cval[perm[p]], fp64 (csr_gather_kernel of the f32 engine stores
//                             floats), one thread per entry, the permutation and the store coalesced.  perm is the
//                             payload of the second sort of the positions 0 .. nnz - 1, a permutation of them.
// Pointers, indices and the CSC values go into the job's buffer as they are, device to device.  No floating-point
// atomics, no flags, nothing waits on another workgroup.
//
// Both kernels are templates (resnmtf_fp64_sparse.hip.inc says why: a template lands between the other kernels of the
// code object and displaces no section's last symbol).

constexpr int F64_SPD_THREADS = 256;

// out[0] = max over rows of rptr[i + 1] - rptr[i], out[1] = max over columns of cptr[c + 1] - cptr[c]; out zeroed by the
// caller.  Line l < n is row l, line n + c is column c.  A line holds distinct positions, so its length fits an int.
template <int THREADS>
__global__ __launch_bounds__(THREADS) void fp64_spd_longest_kernel(const long long* __restrict__ rptr, int n,
                                                                   const long long* __restrict__ cptr, int m,
                                                                   int* __restrict__ out) {
  __shared__ int red[2][THREADS / 64];
  const long long line = (long long)blockIdx.x * THREADS + threadIdx.x;
  int r = 0, c = 0;
  if (line < n) r = (int)(rptr[line + 1] - rptr[line]);
  else if (line < (long long)n + m) c = (int)(cptr[line - n + 1] - cptr[line - n]);
  for (int off = 32; off > 0; off >>= 1) {
    r = max(r, __shfl_down(r, off, 64));
    c = max(c, __shfl_down(c, off, 64));
  }
  if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = r; red[1][threadIdx.x >> 6] = c; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < THREADS / 64; ++w) { r = max(r, red[0][w]); c = max(c, red[1][w]); }
    if (r > 0) atomicMax(&out[0], r);
    if (c > 0) atomicMax(&out[1], c);
  }
}

template <int THREADS>
__global__ __launch_bounds__(THREADS) void fp64_spd_gather_kernel(const long long* __restrict__ perm, const double* __restrict__ cval,
                                                                  long long nnz, double* __restrict__ rval) {
  const long long p = (long long)blockIdx.x * THREADS + threadIdx.x;
  if (p < nnz) rval[p] = cval[perm[p]];
}

// ---- launches ----
static void fp64_spd_longest(hipStream_t st, const long long* rptr, int n, const long long* cptr, int m, int* out) {
  const unsigned grid = (unsigned)(((long long)n + m + F64_SPD_THREADS - 1) / F64_SPD_THREADS);
  hipLaunchKernelGGL(fp64_spd_longest_kernel<F64_SPD_THREADS>, dim3(grid), dim3(F64_SPD_THREADS), 0, st, rptr, n, cptr, m, out);
}
// nnz >= 1
static void fp64_spd_gather(hipStream_t st, const long long* perm, const double* cval, long long nnz, double* rval) {
  const unsigned grid = (unsigned)((nnz + F64_SPD_THREADS - 1) / F64_SPD_THREADS);
  hipLaunchKernelGGL(fp64_spd_gather_kernel<F64_SPD_THREADS>, dim3(grid), dim3(F64_SPD_THREADS), 0, st, perm, cval, nnz, rval);
}
