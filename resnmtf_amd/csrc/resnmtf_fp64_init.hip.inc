// The SVD initialisation in double precision (resnmtf_fp64_init_svd, DESIGN.md section 32): init_mats_inner
// (R/update_steps.r:78-125) as the randomized subspace iteration of resnmtf_init_svd, on the fp64 values of a view.  The
// two big products per half step are the run's own -- fp64_product_kernel over the padded images of a dense view, the
// fp64 SpMM over the CSR / CSC copies of a sparse one -- and so are the Gram partials (fp64_gram_kernel); the L x L
// factorisations stay on the host (resnmtf_small_linalg.h).  What is new is here: the sum of a product's slab into a
// column-major sketch matrix (the layout the products and the Gram read), the tall-skinny apply Q = Y M on the fp64
// MFMA, the reduction of the Gram partials, the dense copy of the short side of a thin sparse view, and the finish
// (R/update_steps.r:93-115) on the device.
//
// Every sketch matrix is column-major with its row count as leading dimension.  Determinism as in resnmtf_fp64.hip.inc:
// no atomics, nothing waits on another workgroup, every sum order is a function of the shapes (and of a sparse view's
// structure) alone.  Every kernel is a template, instantiated by a launcher in this file (see resnmtf_fp64_sparse.hip.inc
// for why).

#define F64_INIT_ROWS 64        // rows per workgroup of the slab sum and of the apply (four waves x one 16-row MFMA tile)

// ---- Y[i, c] = sum over the splits s, in split order, of slab[s][i][c]: the product as a column-major len x KP matrix ----
// 64 rows per workgroup through LDS: the slab rows are read whole, the columns of Y written whole.  The order of the
// sum is fp64_update_kernel's.
template <int KP>
__global__ __launch_bounds__(F64_THREADS) void fp64_init_slab_sum_kernel(const double* __restrict__ slab, int nsplit, size_t ldx,
                                                                         int len, double* __restrict__ Y) {
  constexpr int LD = KP + 1;
  __shared__ double tile[F64_INIT_ROWS * LD];
  const size_t i0 = (size_t)blockIdx.x * F64_INIT_ROWS, slen = (size_t)len;
  for (int e = threadIdx.x; e < F64_INIT_ROWS * KP; e += F64_THREADS) {
    const int jj = e / KP, c = e % KP;
    double acc = 0.0;
    if (i0 + jj < slen)
      for (int s = 0; s < nsplit; ++s) acc += slab[((size_t)s * ldx + i0 + jj) * KP + c];
    tile[jj * LD + c] = acc;
  }
  __syncthreads();
  for (int e = threadIdx.x; e < F64_INIT_ROWS * KP; e += F64_THREADS) {
    const int jj = e % F64_INIT_ROWS, c = e / F64_INIT_ROWS;
    if (i0 + jj < slen) Y[i0 + jj + (size_t)c * slen] = tile[jj * LD + c];
  }
}

// ---- the tall-skinny apply Q = Y M: Y (len x L) and Q column-major, M (L x L) row-major, L <= KP ----
// M lies in LDS, padded with zeros to KP x KP.  Wave w of workgroup b owns rows 64 b + 16 w .. + 15 as one MFMA tile per
// 16 columns of Q (v_mfma_f64_16x16x4_f64: lane (p, q) supplies A[p][q] = Y[i0 + p, e + q] and B[q][p] = M[e + q, c0 + p],
// register t of the result is Q[i0 + 4 t + q, c0 + p]); the contraction runs over e in ascending steps of 4.  Rows from
// len on and columns from L on are read as zero and not written.
template <int KP>
__global__ __launch_bounds__(F64_THREADS) void fp64_init_apply_kernel(const double* __restrict__ Y, int len, int L,
                                                                      const double* __restrict__ M, double* __restrict__ Q) {
  constexpr int LD = KP + 1, NTC = KP / 16;
  __shared__ double Ml[KP * LD];
  for (int e = threadIdx.x; e < KP * KP; e += F64_THREADS) {
    const int r = e / KP, c = e % KP;
    Ml[r * LD + c] = (r < L && c < L) ? M[r * L + c] : 0.0;
  }
  __syncthreads();
  const int wv = threadIdx.x >> 6, ln = threadIdx.x & 63, p = ln & 15, q = ln >> 4;
  const size_t i0 = (size_t)blockIdx.x * F64_INIT_ROWS + (size_t)wv * 16, slen = (size_t)len;
  if (i0 >= slen) return;                         // (the whole wave)
  const bool row_ok = i0 + p < slen;
  f64x4 acc[NTC];
#pragma unroll
  for (int tc = 0; tc < NTC; ++tc) acc[tc] = f64x4{0.0, 0.0, 0.0, 0.0};
#pragma unroll 4
  for (int e0 = 0; e0 < KP; e0 += 4) {
    const int e = e0 + q;
    const double a = (row_ok && e < L) ? Y[i0 + p + (size_t)e * slen] : 0.0;
#pragma unroll
    for (int tc = 0; tc < NTC; ++tc) acc[tc] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, Ml[e * LD + 16 * tc + p], acc[tc], 0, 0, 0);
  }
#pragma unroll
  for (int tc = 0; tc < NTC; ++tc)
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const size_t row = i0 + 4 * t + q;
      const int col = 16 * tc + p;
      if (row < slen && col < L) Q[row + (size_t)col * slen] = acc[tc][t];
    }
}

// ---- out[q] = sum over the workgroups b of a Gram launch, in workgroup order, of part[b][q] (as f64_kk_reduce sums) ----
template <int UNUSED>
__global__ __launch_bounds__(F64_THREADS) void fp64_init_reduce_kernel(const double* __restrict__ part, int nblk, int Q,
                                                                       double* __restrict__ out) {
  const int q = blockIdx.x * F64_THREADS + threadIdx.x;
  if (q >= Q) return;
  double acc = 0.0;
  for (int b = 0; b < nblk; ++b) acc += part[(size_t)b * Q + q];
  out[q] = acc;
}

// ---- the short side of a thin sparse view as a dense column-major len x lines matrix (zero-filled by the caller): line
// l of the CSC (a tall view) or of the CSR (a wide one) becomes column l.  Stored positions are distinct: plain stores. ----
template <int UNUSED>
__global__ __launch_bounds__(F64_THREADS) void fp64_init_densify_kernel(const long long* __restrict__ ptr, const int* __restrict__ idx,
                                                                        const double* __restrict__ val, int len,
                                                                        double* __restrict__ Y) {
  const size_t l = blockIdx.x;
  for (long long e = ptr[l] + threadIdx.x; e < ptr[l + 1]; e += F64_THREADS) Y[(size_t)idx[e] + l * (size_t)len] = val[e];
}

// ---- the finish, R/update_steps.r:93-115: workgroup (j, side) owns column j of F0 (side 0, from U) or of G0 (side 1, from
// V).  |.| (:93-94) and the column sum (:100-101): thread t sums its rows t, t + 256, ... in order, then the fixed tree; a
// column that sums to zero (a triplet past the rank of X) becomes the constant unit vector; then the division
// (:106-113) and the sum of the divided column (:114-115) in the same order.  No workgroup reads what another wrote. ----
struct F64InitFinishArgs {
  const double *U, *V;                    // n x k and m x k, column-major, leading dimensions n and m
  int n, m;
  double *F0, *G0;                        // n x k, m x k
  double *cf, *cg, *lam, *mu;             // k each
};
template <int UNUSED>
__global__ __launch_bounds__(F64_THREADS) void fp64_init_finish_kernel(F64InitFinishArgs a) {
  __shared__ double red[F64_THREADS];
  const int j = blockIdx.x, side = blockIdx.y, t = threadIdx.x;
  const size_t len = (size_t)(side ? a.m : a.n);
  const double* src = (side ? a.V : a.U) + (size_t)j * len;
  double* dst = (side ? a.G0 : a.F0) + (size_t)j * len;
  double acc = 0.0;
  for (size_t i = t; i < len; i += F64_THREADS) {
    const double x = fabs(src[i]);
    dst[i] = x;
    acc += x;
  }
  double c = f64_block_sum(acc, red);
  if (c == 0.0) {
    const double root = sqrt((double)len), fill = 1.0 / root;
    for (size_t i = t; i < len; i += F64_THREADS) dst[i] = fill;
    c = root;
  }
  acc = 0.0;
  for (size_t i = t; i < len; i += F64_THREADS) {   // (every thread reads back its own stores alone)
    const double x = dst[i] / c;
    dst[i] = x;
    acc += x;
  }
  const double lm = f64_block_sum(acc, red);
  if (t == 0) {
    (side ? a.cg : a.cf)[j] = c;
    (side ? a.mu : a.lam)[j] = lm;
  }
}

// S0[i, j] = base[i, j] cF[j] cG[j] (:102-105, the column sweep); base = |diag(d)| + |noise| comes from the host
template <int UNUSED>
__global__ __launch_bounds__(F64_THREADS) void fp64_init_s0_kernel(const double* __restrict__ base, const double* __restrict__ cf,
                                                                   const double* __restrict__ cg, int k, double* __restrict__ S0) {
  for (int q = threadIdx.x; q < k * k; q += F64_THREADS) S0[q] = base[q] * cf[q / k] * cg[q / k];
}

// ---- launchers: one instance of the templated kernels per padded width (16 / 32 / 48 / 64) ----
static void fp64_init_slab_sum(hipStream_t st, int KP, const double* slab, int nsplit, size_t ldx, int len, double* Y) {
  const dim3 grid((len + F64_INIT_ROWS - 1) / F64_INIT_ROWS), block(F64_THREADS);
  switch (KP) {
    case 16: hipLaunchKernelGGL(fp64_init_slab_sum_kernel<16>, grid, block, 0, st, slab, nsplit, ldx, len, Y); break;
    case 32: hipLaunchKernelGGL(fp64_init_slab_sum_kernel<32>, grid, block, 0, st, slab, nsplit, ldx, len, Y); break;
    case 48: hipLaunchKernelGGL(fp64_init_slab_sum_kernel<48>, grid, block, 0, st, slab, nsplit, ldx, len, Y); break;
    default: hipLaunchKernelGGL(fp64_init_slab_sum_kernel<64>, grid, block, 0, st, slab, nsplit, ldx, len, Y); break;
  }
}
static void fp64_init_apply(hipStream_t st, const double* Y, int len, int L, const double* M, double* Q) {
  const dim3 grid((len + F64_INIT_ROWS - 1) / F64_INIT_ROWS), block(F64_THREADS);
  switch (f64_kp(L)) {
    case 16: hipLaunchKernelGGL(fp64_init_apply_kernel<16>, grid, block, 0, st, Y, len, L, M, Q); break;
    case 32: hipLaunchKernelGGL(fp64_init_apply_kernel<32>, grid, block, 0, st, Y, len, L, M, Q); break;
    case 48: hipLaunchKernelGGL(fp64_init_apply_kernel<48>, grid, block, 0, st, Y, len, L, M, Q); break;
    default: hipLaunchKernelGGL(fp64_init_apply_kernel<64>, grid, block, 0, st, Y, len, L, M, Q); break;
  }
}
static void fp64_init_reduce(hipStream_t st, const double* part, int nblk, int Q, double* out) {
  hipLaunchKernelGGL(fp64_init_reduce_kernel<0>, dim3((Q + F64_THREADS - 1) / F64_THREADS), dim3(F64_THREADS), 0, st, part, nblk, Q, out);
}
static void fp64_init_densify(hipStream_t st, const long long* ptr, const int* idx, const double* val, int lines, int len, double* Y) {
  hipLaunchKernelGGL(fp64_init_densify_kernel<0>, dim3(lines), dim3(F64_THREADS), 0, st, ptr, idx, val, len, Y);
}
static void fp64_init_finish(hipStream_t st, const F64InitFinishArgs& a, int k, const double* base, double* S0) {
  hipLaunchKernelGGL(fp64_init_finish_kernel<0>, dim3(k, 2), dim3(F64_THREADS), 0, st, a);
  hipLaunchKernelGGL(fp64_init_s0_kernel<0>, dim3(1), dim3(F64_THREADS), 0, st, base, (const double*)a.cf, (const double*)a.cg, k, S0);
}
