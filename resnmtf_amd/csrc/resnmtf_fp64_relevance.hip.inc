// resnmtf_fp64_relevance.hip.inc -- relevance_results (R/stability_analysis.r:45-67) with jaccard_main (:16-33) of cluster
// matrices that are in device memory (resnmtf_fp64_relevance, DESIGN.md section 28).  Included by resnmtf_fp64.hip only,
// after resnmtf_fp64_device.hip.inc (f64_load_wide).
//
// Bicluster i is the pair set R_i x C_i, so the Jaccard index of two biclusters is a function of integer counts per side
// (DESIGN.md section 9b).  The arithmetic is the main unit's relevance_count_kernel / relevance_epilogue_kernel; what
// differs is where the memberships come from: 0 / 1 matrices of any of the four dtypes with any strides, for the
// sub-sample (len x k) and for the reference (len_ref x k_ref, gathered through idx), and k != k_ref.
//   fp64_relevance_check_kernel   an entry other than 0 / 1: the lowest column-major position, by an integer atomicMin
//   fp64_relevance_count_kernel   ONE side per launch: a wave takes 64 lines at a time, forms the membership masks with
//                                 __ballot and adds popcounts of the ANDed masks into LDS counters, then into `counts` --
//                                 integer atomics only.  counts: [k k_ref: |A_i ^ B_j| at i k_ref + j] [k: |A_i|]
//                                 [k_ref: |B_j|] (A = sub-sample, B = reference)
//   fp64_relevance_epilogue_kernel  relevance[j] = max_i I / U after the row-clusters-only edge cases

// a load of any of the four dtypes, widened (the dtype is uniform over the launch)
__device__ __forceinline__ double f64_load_any(const void* __restrict__ src, int dtype, size_t i) {
  switch (dtype) {
    case RESNMTF_DTYPE_F64: return f64_load_wide<RESNMTF_DTYPE_F64>(src, i);
    case RESNMTF_DTYPE_F32: return f64_load_wide<RESNMTF_DTYPE_F32>(src, i);
    case RESNMTF_DTYPE_F16: return f64_load_wide<RESNMTF_DTYPE_F16>(src, i);
    default: return f64_load_wide<RESNMTF_DTYPE_BF16>(src, i);
  }
}

constexpr unsigned long long F64_REL_NONE = ~0ull;        // no offender

static __global__ void __launch_bounds__(256)
fp64_relevance_check_kernel(const void* __restrict__ a, int dtype, size_t rs, size_t cs, int len, int k, unsigned long long* __restrict__ bad) {
  const unsigned long long total = (unsigned long long)len * (unsigned long long)k;
  unsigned long long worst = F64_REL_NONE;
  for (unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (unsigned long long)gridDim.x * 256) {
    const double x = f64_load_any(a, dtype, (size_t)(i % (unsigned long long)len) * rs + (size_t)(i / (unsigned long long)len) * cs);
    if (x != 0.0 && x != 1.0 && i < worst) worst = i;             // (NaN is an offender too)
  }
  if (worst != F64_REL_NONE) atomicMin(bad, worst);
}

static __global__ void __launch_bounds__(256)
fp64_relevance_count_kernel(const void* __restrict__ A, int a_dtype, size_t a_rs, size_t a_cs, int len, int k,
                            const void* __restrict__ B, int b_dtype, size_t b_rs, size_t b_cs, int k_ref,
                            const int* __restrict__ idx, unsigned int* __restrict__ counts) {
  __shared__ unsigned int cnt[RESNMTF_MAX_K * RESNMTF_MAX_K + 2 * RESNMTF_MAX_K];
  const int total = k * k_ref + k + k_ref;
  for (int t = threadIdx.x; t < total; t += 256) cnt[t] = 0u;
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long chunks = ((long long)len + 63) / 64;
  for (long long ch = (long long)blockIdx.x * 4 + wave; ch < chunks; ch += (long long)gridDim.x * 4) {
    const long long r = ch * 64 + lane;
    const bool valid = r < len;
    const size_t rr = (size_t)(valid ? r : len - 1);      // lanes past the end address the last line and vote 0
    const size_t bo = (size_t)idx[rr] * b_rs;
    unsigned long long mine = 0ull;                       // lane j < k_ref: the reference's cluster j over these 64 lines
    for (int j = 0; j < k_ref; ++j) {
      const unsigned long long b = __ballot(valid && f64_load_any(B, b_dtype, bo + (size_t)j * b_cs) != 0.0);
      if (lane == j) mine = b;
    }
    if (lane < k_ref && mine) atomicAdd(&cnt[k * k_ref + k + lane], (unsigned int)__popcll(mine));
    for (int i = 0; i < k; ++i) {
      const unsigned long long a = __ballot(valid && f64_load_any(A, a_dtype, rr * a_rs + (size_t)i * a_cs) != 0.0);
      if (a == 0ull) continue;                            // (wave-uniform)
      if (lane == 0) atomicAdd(&cnt[k * k_ref + i], (unsigned int)__popcll(a));
      if (lane < k_ref) {
        const unsigned int p = (unsigned int)__popcll(a & mine);
        if (p) atomicAdd(&cnt[i * k_ref + lane], p);
      }
    }
  }
  __syncthreads();
  for (int t = threadIdx.x; t < total; t += 256)
    if (cnt[t]) atomicAdd(&counts[t], cnt[t]);
}

// one thread per reference cluster j; m_0 / n_0 = the non-empty columns of row_c / of the gathered true_r
static __global__ void fp64_relevance_epilogue_kernel(int k, int k_ref, const unsigned int* __restrict__ rows_cnt,
                                                      const unsigned int* __restrict__ cols_cnt, double* __restrict__ out) {
  const int j = threadIdx.x;
  if (j >= k_ref) return;
  const unsigned int *rI = rows_cnt, *rA = rows_cnt + k * k_ref, *rB = rA + k;
  const unsigned int *cI = cols_cnt, *cA = cols_cnt + k * k_ref, *cB = cA + k;
  int m0 = 0, n0 = 0;
  for (int t = 0; t < k; ++t) m0 += rA[t] != 0u;
  for (int t = 0; t < k_ref; ++t) n0 += rB[t] != 0u;
  if ((m0 == 0) != (n0 == 0)) { out[j] = 0.0; return; }     // R/stability_analysis.r:57-59
  if (m0 == 0) { out[j] = 1.0; return; }                     // :62-64
  double best = 0.0;
  for (int i = 0; i < k; ++i) {
    const long long inter = (long long)rI[i * k_ref + j] * (long long)cI[i * k_ref + j];
    const long long uni = (long long)rA[i] * (long long)cA[i] + (long long)rB[j] * (long long)cB[j] - inter;
    const double jac = uni == 0 ? 0.0 : (double)inter / (double)uni;      // jaccard_func, R/utils.r:117-126
    if (i == 0 || jac > best) best = jac;
  }
  out[j] = best;
}

// ---- launches ----
inline void fp64_relevance_check(hipStream_t st, const resnmtf_device_matrix& a, int len, int k, unsigned long long* bad) {
  const unsigned long long total = (unsigned long long)len * (unsigned long long)k;
  const unsigned blocks = (unsigned)std::min<unsigned long long>((total + 255) / 256, 1024);
  hipLaunchKernelGGL(fp64_relevance_check_kernel, dim3(blocks), dim3(256), 0, st, a.ptr, a.dtype, (size_t)a.row_stride, (size_t)a.col_stride, len, k, bad);
}
inline void fp64_relevance_count(hipStream_t st, const resnmtf_device_matrix& a, int len, int k, const resnmtf_device_matrix& b, int k_ref,
                                 const int* idx, unsigned int* counts) {
  const unsigned blocks = (unsigned)std::min<long long>(((long long)len + 255) / 256, 256);
  hipLaunchKernelGGL(fp64_relevance_count_kernel, dim3(blocks), dim3(256), 0, st, a.ptr, a.dtype, (size_t)a.row_stride, (size_t)a.col_stride, len, k,
                     b.ptr, b.dtype, (size_t)b.row_stride, (size_t)b.col_stride, k_ref, idx, counts);
}
