// resnmtf_sparse.hip.inc -- sparse data views (resnmtf_create_sparse / resnmtf_set_view_csc): the two big contractions
// X.G and Xt.F' from CSR / CSC copies of X, and the upload-time kernels that build those copies.  Included by
// resnmtf_hip.hip after resnmtf_kernels.hip.inc (it uses f32x4, SweepCtl and the k x k job bodies).
//
// Storage of a sparse view (DESIGN.md section 10): CSC (column pointers int64 [m + 1], row indices int32, values f32) for
// Xt.F', CSR (row pointers int64 [n + 1], column indices int32, values f32) for X.G; no dense image.  Entries of a row of
// the CSR come in ascending column order, entries of a column of the CSC in ascending row order.
//
// spmm_kernel writes exactly the partial slabs the dense passes write -- [nsplit][cols_pad][KP] f32, natural column
// order, rows >= the view's extent untouched (zero) -- so every consumer (factor updates, EMIT partials, the F / G chains,
// the S rule, the trace-form error, the stop test) reads them unchanged.  Determinism: output line r of slab s is the
// sum over the s-th of nsplit equal pieces of line r's entry range, accumulated in ascending entry order with f32 FMAs --
// by ONE group of lanes (narrow blocks), or by every group of the wave on a fixed stride followed by a fixed xor butterfly
// (wide blocks: long lines); no atomics.  The bits therefore depend only on the data, nsplit and the form (both fixed
// at upload), not on the grid, the work blocks or the timing: two runs, and graph replay against eager launches, give
// the same bits.

// one wave = one (work block, split) unit; a work block is a range of output lines balanced by nnz on the host
struct SpmmArgs {
  const long long* ptr;       // [lines + 1] line pointers (X.G: CSR rows; Xt.F: CSC columns)
  const int* idx;             // contraction index of every entry
  const float* val;           // value of every entry
  const int* blk;             // [nblk + 1] first line of every work block, then [nblk] form flags: 1 = wide (every group
                              // of the wave works on the SAME line, then a fixed butterfly sums them), 0 = narrow
  int nblk;
  int nsplit;                 // pieces of every line's entry range = slabs
  const float* B; int ldb;    // operand [rows][ldb], its KP columns interleaved (fperm)
  float* P; int cols_pad;     // slabs [nsplit][cols_pad][KP]
  int kk_block0;              // 1: workgroup 0 runs the k x k job (hand-off mode A), the units start at workgroup 1
  int no_kk;                  // (with kk_block0: workgroup 0 idles)
  const SweepCtl* ctl; int check_done;
};

constexpr int spmm_lanes_per_line(int KP) { return KP <= 16 ? 4 : (KP <= 32 ? 8 : 16); }   // one float4 of the row per lane
constexpr int spmm_groups(int KP) { return 64 / spmm_lanes_per_line(KP); }                   // lines a wave works at once

template <int KP, bool IS_XG>
__global__ __launch_bounds__(512) void spmm_kernel(SpmmArgs a, KKFArgs kf, KKSArgs ks) {
  if (a.check_done && a.ctl->done) return;
  extern __shared__ __attribute__((aligned(16))) double smem_d[];
  if (a.kk_block0 && blockIdx.x == 0) {
    // mode A: the k x k job's inputs (fp64 partials of the preceding update kernel) are complete before this launch starts
    if (a.no_kk) return;
    if (IS_XG) { KKSPre<KP, 512> pre; kk_s_prefetch<KP, 512>(ks, pre); kk_s_body<KP, 512, true>(ks, pre, nullptr, 0, smem_d); }
    else { KKFPre<KP, 512> pre; kk_f_prefetch<KP, 512>(kf, pre); kk_f_body<KP, 512, true>(kf, pre, nullptr, 0, smem_d); }
    return;
  }
  constexpr int LPE = spmm_lanes_per_line(KP), NG = spmm_groups(KP), NT = KP / 16;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int unit = ((int)blockIdx.x - (a.kk_block0 ? 1 : 0)) * 8 + wave;
  if (unit >= a.nblk * a.nsplit) return;
  const int b = unit % a.nblk, s = unit / a.nblk;
  const int g = lane / LPE, l = lane % LPE;
  if (4 * l >= KP) return;                                // KP = 48: four idle lanes per group
  const int r0 = a.blk[b], r1 = a.blk[b + 1];
  const float* __restrict__ bcol = a.B + 4 * l;
  float* __restrict__ out = a.P + (size_t)s * a.cols_pad * KP;
  if (a.blk[a.nblk + 1 + b]) {
    // group g takes entries g, g + NG, ... of the piece in ascending order; the NG partial sums are then combined by an
    // xor butterfly over the groups (offsets 32 ... LPE: the lane's column position l is kept), the same tree on every lane
    for (int r = r0; r < r1; ++r) {
      const long long p0 = a.ptr[r], len = a.ptr[r + 1] - p0;
      const long long e0 = p0 + len * s / a.nsplit, e1 = p0 + len * (s + 1) / a.nsplit;
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      long long e = e0 + g;
      for (; e + NG < e1; e += 2 * NG) {
        const int c0 = a.idx[e], c1 = a.idx[e + NG];
        const float x0 = a.val[e], x1 = a.val[e + NG];
        const f32x4 b0 = *reinterpret_cast<const f32x4*>(bcol + (size_t)c0 * a.ldb);
        const f32x4 b1 = *reinterpret_cast<const f32x4*>(bcol + (size_t)c1 * a.ldb);
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[t] = __builtin_fmaf(x1, b1[t], __builtin_fmaf(x0, b0[t], acc[t]));
      }
      if (e < e1) {
        const int c = a.idx[e];
        const float x = a.val[e];
        const f32x4 bv = *reinterpret_cast<const f32x4*>(bcol + (size_t)c * a.ldb);
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[t] = __builtin_fmaf(x, bv[t], acc[t]);
      }
#pragma unroll
      for (int off = 32; off >= LPE; off >>= 1)
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[t] += __shfl_xor(acc[t], off);
      if (g == 0) {
        float* o = out + (size_t)r * KP;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const int p = 4 * l + t;
          o[16 * (p % NT) + p / NT] = acc[t];
        }
      }
    }
    return;
  }
  for (int r = r0 + g; r < r1; r += NG) {
    const long long p0 = a.ptr[r], len = a.ptr[r + 1] - p0;
    const long long e0 = p0 + len * s / a.nsplit, e1 = p0 + len * (s + 1) / a.nsplit;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    long long e = e0;
    // four entries per trip: their index / value loads and factor-row gathers are all in flight before the FMAs
    for (; e + 4 <= e1; e += 4) {
      int c[4]; float x[4]; f32x4 bv[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) { c[u] = a.idx[e + u]; x[u] = a.val[e + u]; }
#pragma unroll
      for (int u = 0; u < 4; ++u) bv[u] = *reinterpret_cast<const f32x4*>(bcol + (size_t)c[u] * a.ldb);
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[t] = __builtin_fmaf(x[u], bv[u][t], acc[t]);
    }
    for (; e < e1; ++e) {
      const int c = a.idx[e];
      const float x = a.val[e];
      const f32x4 bv = *reinterpret_cast<const f32x4*>(bcol + (size_t)c * a.ldb);
#pragma unroll
      for (int t = 0; t < 4; ++t) acc[t] = __builtin_fmaf(x, bv[t], acc[t]);
    }
    // operand position p = 4 l + t holds column 16 (p % NT) + p / NT (fperm); the slab is in natural column order
    float* o = out + (size_t)r * KP;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int p = 4 * l + t;
      o[16 * (p % NT) + p / NT] = acc[t];
    }
  }
}

// ---- upload (resnmtf_set_view_csc)
// one thread per column: matrix_normalisation (R/utils.r:86-88: x / colSums(x), fp64) when `normalise`, the f32 copy of
// the CSC values and the column's share of ||X||_F^2 (data_norms, R/main.r:48), summed in fp64 in entry order
static __global__ __launch_bounds__(256) void csc_normalise_kernel(const long long* __restrict__ cp, const double* __restrict__ v64,
                                                                   int m, int normalise, float* __restrict__ v32,
                                                                   double* __restrict__ sq_col) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= m) return;
  const long long p0 = cp[j], p1 = cp[j + 1];
  double cs = 1.0;
  if (normalise) {
    cs = 0.0;
    for (long long e = p0; e < p1; ++e) cs += v64[e];
  }
  double sq = 0.0;
  for (long long e = p0; e < p1; ++e) {
    const double d = normalise ? v64[e] / cs : v64[e];
    sq += d * d;
    v32[e] = (float)d;
  }
  sq_col[j] = sq;
}
// CSR values from the CSC ones: perm[p] = CSC position of the p-th CSR entry (built on the host)
static __global__ __launch_bounds__(256) void csr_gather_kernel(const long long* __restrict__ perm, const float* __restrict__ vcsc,
                                                                long long nnz, float* __restrict__ vcsr) {
  const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
  if (p < nnz) vcsr[p] = vcsc[perm[p]];
}
// thin SVD route: the short side as a dense fp64 [lines][width] matrix (Y[line][idx] = value) from CSR or CSC
static __global__ __launch_bounds__(256) void sparse_widen_kernel(const long long* __restrict__ ptr, const int* __restrict__ idx,
                                                                  const float* __restrict__ val, int lines, int width,
                                                                  double* __restrict__ Y) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= lines) return;
  for (long long e = ptr[t]; e < ptr[t + 1]; ++e) Y[(size_t)t * width + idx[e]] = (double)val[e];
}
