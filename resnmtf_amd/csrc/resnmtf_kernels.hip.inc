// resnmtf_kernels.hip.inc -- device kernels of the ResNMTF multiplicative-update sweep (gfx950).
// Included by resnmtf_hip.hip.  See DESIGN.md for the data layout and the per-kernel roofline.
//
// Notation (one view): X is n x m, F n x k, G m x k, S k x k; KP = 16*NT >= k (NT = #MFMA N-tiles).
//   device layouts:  X32 = X and Xt32 = X^T in f32, zero padded to multiples of 64, stored TILE-MAJOR: the
//   64-column tile t of a [rows_pad][cols_pad] image is a contiguous [rows_pad][64] block at t * tile_stride
//   (xidx), so that the rows one workgroup of a streaming pass reads are contiguous in memory;  factors fp64 row-major [len][k];  f32 operand copies F32/G32/T32
//   [len_pad][64] zero padded (mode A uses the buffer compactly, pitch KP), columns interleaved (fperm).
//
// Kernels of one sweep of one view (R/update_steps.r:282-314), one stream, four launches:
//   factor_update<F>   update_f, reads U = X G and the F coefficients
//   pass Xt.F          main workgroups: T = X^T F'      + the k x k job kk_f
//   factor_update<G>   update_g, reads T and the G coefficients
//   pass X.G'          main workgroups: U = X G'        + the k x k job kk_s
// Every k x k chain (Gram sums, S rule, lambda/mu, error, coefficient matrices) depends only on the
// factor update that precedes the pass, so it runs ONCE, inside the pass launch, while the main
// workgroups stream X; the update kernels only read its results.  Two hand-off modes (per view):
//   mode A (k <= 16): the update kernel emits fp64 partial Gram / cross / column sums per workgroup,
//          the job is workgroup 0 of the pass launch (inputs complete before the launch starts);
//   mode B (k > 16):  the products are extra 64-column MFMA tiles of the same pass body (A operand =
//          the f32 copy of a factor, or the constant 1) at the front of the grid; the LAST of them to
//          arrive (ticket counter, agent-scope release / acquire) runs the job.

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef double f64x4 __attribute__((ext_vector_type(4)));
// element (r, c) of a tile-major f32 image (tile stride ts floats)
__host__ __device__ __forceinline__ size_t xidx(int r, int c, size_t ts) { return (size_t)(c >> 6) * ts + (size_t)r * 64 + (c & 63); }

// Diagnostic build only (-DRESNMTF_STAMPS, tools/stamps.py): per-block wall-clock stamps (100 MHz
// s_memrealtime) written to a buffer nothing else reads.  No stamp executes in the product build.
#ifdef RESNMTF_STAMPS
__device__ unsigned long long* g_stamp_buf = nullptr;     // [blocks][16]
__device__ int g_stamp_sel = 3;                           // bit 0: the pass launches stamp, bit 1: the update kernels
#define STAMP_IF(bit, idx)                                                              \
  do {                                                                                  \
    if (g_stamp_buf && (g_stamp_sel & (bit)) && threadIdx.x == 0) g_stamp_buf[(size_t)blockIdx.x * 16 + (idx)] = wall_clock64(); \
  } while (0)
#define STAMP(idx) STAMP_IF(1, idx)
#define STAMP_U(idx) STAMP_IF(2, idx)
#else
#define STAMP(idx) do { } while (0)
#define STAMP_U(idx) do { } while (0)
#endif

struct SweepCtl {            // device-resident loop control (one per handle)
  int sweep;                 // sweeps whose F and G updates have completed in this run
  int done;                  // set by end_sweep_kernel when the convergence test fires
  int stop_sweep;            // sweep count at which it fired
  int pad;
  double prev_mean;          // err_temp of R/main.r:54,80
};

// The kernels that are not templates are `static __global__`: every translation unit that includes them emits its own copy.
// resnmtf_pass_k16.hip needs the templates alone and defines RESNMTF_TEMPLATES_ONLY: the three stretches of such kernels
// (upload and pre-processing here, the operand copy below, everything after the passes at the end) are left out there.
#ifndef RESNMTF_TEMPLATES_ONLY
// --------------------------------------------------------------------------------------
// Pre-processing of a raw view on upload (SURVEY 8(f2)): per column c of the column-major source
//   shift[c]  = |min(0, min(x[, c]))|                 make_non_neg_inner, R/utils.r:22
//   colsum[c] = sum(x[, c] + shift[c])                colSums of matrix_normalisation, R/utils.r:87
// and *neg = 1 if any entry is negative (the reference's warning, R/utils.r:23-25).  One workgroup
// per column (contiguous in the source).  The division itself is fused into convert_x_kernel.
// A zero column divides 0 / 0 = NaN exactly as sweep(..., "/") does.
// --------------------------------------------------------------------------------------
static __global__ __launch_bounds__(256) void column_stats_kernel(const double* __restrict__ src, int n, int m,
                                                           double* __restrict__ shift, double* __restrict__ colsum,
                                                           int* __restrict__ neg) {
  __shared__ double red[256];
  const int c = blockIdx.x;
  const double* col = src + (size_t)c * n;
  double mn = 0.0;                                     // min(0, min(x))
  for (int r = threadIdx.x; r < n; r += 256) mn = fmin(mn, col[r]);
  red[threadIdx.x] = mn;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] = fmin(red[threadIdx.x], red[threadIdx.x + s]);
    __syncthreads();
  }
  const double sh = fabs(red[0]);
  __syncthreads();
  double sum = 0.0;
  for (int r = threadIdx.x; r < n; r += 256) sum += col[r] + sh;
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

// --------------------------------------------------------------------------------------
// shuffle_view (R/obtain_bicl.r:11-22) on the device: staging[i] = X[pi(i)] for a pseudo-random
// permutation pi of the n m entries -- a 4-round Feistel network on the next even power of two with
// cycle walking (a bijection on [0, n m), evaluated independently per element: no sort, no atomics).
// R draws the permutation from its Mersenne Twister (sample()); neither is reproducible by the other.
// feistel_perm itself is csrc/resnmtf_feistel.h: one text for this unit, the fp64 unit and the host check.
// --------------------------------------------------------------------------------------
#include "resnmtf_feistel.h"
static __global__ __launch_bounds__(256) void shuffle_gather_kernel(const float* __restrict__ X32, size_t tsx, int n, int m,
                                                             unsigned long long seed, double* __restrict__ staging) {
  const unsigned long long count = (unsigned long long)n * m;
  const unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= count) return;
  int half_bits = 1;
  while ((1ull << (2 * half_bits)) < count) ++half_bits;
  const unsigned long long j = feistel_perm(i, count, half_bits, seed);
  staging[i] = (double)X32[xidx((int)(j / m), (int)(j % m), tsx)];
}

// sub-sample of a view (stability_repeat, R/stability_analysis.r:230-249): staging = X[rows, cols], column-major
static __global__ __launch_bounds__(256) void subsample_gather_kernel(const float* __restrict__ X32, size_t tsx, const int* __restrict__ rows,
                                                               int n_sub, const int* __restrict__ cols, int m_sub,
                                                               double* __restrict__ staging) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)n_sub * m_sub) return;
  const int r = (int)(i % n_sub), c = (int)(i / n_sub);
  staging[i] = (double)X32[xidx(rows[r], cols[c], tsx)];
}

// rows / columns of the staged view (fp64 column-major, BEFORE shift and normalisation) that sum to exactly zero:
// the condition of shuffle_view's redraw loop (R/obtain_bicl.r:14-18) and of the trimming of sub-samples
// (check_empty, R/stability_analysis.r:165-190, :233-240).  mask[0 .. n) rows, mask[n .. n + m) columns; counts[0/1].
static __global__ __launch_bounds__(256) void empty_lines_kernel(const double* __restrict__ src, int n, int m,
                                                          unsigned char* __restrict__ mask, int* __restrict__ counts) {
  const int line = blockIdx.x * 256 + threadIdx.x;
  if (line >= n + m) return;
  double s = 0.0;
  if (line < n) { for (int c = 0; c < m; ++c) s += src[(size_t)c * n + line]; }            // row sum (coalesced across threads)
  else { const double* col = src + (size_t)(line - n) * n; for (int r = 0; r < n; ++r) s += col[r]; }
  const bool empty = s == 0.0;
  mask[line] = empty ? 1 : 0;
  if (empty) atomicAdd(&counts[line < n ? 0 : 1], 1);
}

// --------------------------------------------------------------------------------------
// Upload: fp64 column-major (R layout) -> X32 (X, tile-major) + Xt32 (X^T, tile-major) and
// block partials of sum(x^2) (data_norms, R/main.r:48).  With shift / colsum (raw upload) the value
// converted is (x + shift[c]) / colsum[c], evaluated in fp64 like the reference.
// --------------------------------------------------------------------------------------
static __global__ __launch_bounds__(256) void convert_x_kernel(const double* __restrict__ src, int n, int m,
                                                        float* __restrict__ X32, size_t tsx,
                                                        float* __restrict__ Xt32, size_t tsxt,
                                                        double* __restrict__ sq_partial,
                                                        const double* __restrict__ shift,
                                                        const double* __restrict__ colsum) {
  __shared__ float tile[32][33];
  __shared__ double red[256];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
  const int r0 = blockIdx.x * 32, c0 = blockIdx.y * 32;
  double sq = 0.0;
  // read: threads contiguous along r (the contiguous direction of the column-major source)
  for (int j = ty; j < 32; j += 8) {
    const int r = r0 + tx, c = c0 + j;
    float v = 0.f;
    if (r < n && c < m) {
      double d = src[(size_t)c * n + r];
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
  red[threadIdx.x] = sq;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) sq_partial[blockIdx.y * gridDim.x + blockIdx.x] = red[0];
}

static __global__ __launch_bounds__(256) void reduce_sum_kernel(const double* __restrict__ part, int count,
                                                         double* __restrict__ out) {
  __shared__ double red[256];
  double s = 0.0;
  for (int i = threadIdx.x; i < count; i += 256) s += part[i];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int st = 128; st > 0; st >>= 1) {
    if ((int)threadIdx.x < st) red[threadIdx.x] += red[threadIdx.x + st];
    __syncthreads();
  }
  if (threadIdx.x == 0) *out = red[0];
}
#endif      // RESNMTF_TEMPLATES_ONLY

// f32 factor operand copies keep their KP columns INTERLEAVED: column i = 16 nt + p lives at position
// p NT + nt (NT = KP / 16), so that a lane's NT B-operand values B[row][16 nt + p], nt = 0..NT-1, are
// one contiguous dwordx{NT} load instead of NT dword loads (identity for k <= 16).  An aux tile that
// uses such a copy as its A operand therefore delivers row i of its product at slab row fperm(i).
__device__ __forceinline__ constexpr int fperm(int i, int NT) { return (i & 15) * NT + (i >> 4); }
template <int NT>
__device__ __forceinline__ void load_b(const float* __restrict__ p, float (&out)[NT]) {
  struct __attribute__((packed, aligned(4))) Pack { float v[NT]; };
  const Pack t = *reinterpret_cast<const Pack*>(p);
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) out[nt] = t.v[nt];
}
template <>
__device__ __forceinline__ void load_b<2>(const float* __restrict__ p, float (&out)[2]) {
  typedef float f32x2 __attribute__((ext_vector_type(2)));
  const f32x2 t = *reinterpret_cast<const f32x2*>(p);
  out[0] = t[0]; out[1] = t[1];
}
template <>
__device__ __forceinline__ void load_b<4>(const float* __restrict__ p, float (&out)[4]) {
  const f32x4 t = *reinterpret_cast<const f32x4*>(p);
  out[0] = t[0]; out[1] = t[1]; out[2] = t[2]; out[3] = t[3];
}

// K-packed f32 operand copy (fp16 passes, k <= 16): element (r, i) at ((r / 4) * 16 + i) * 4 + r % 4, so that the
// four contraction rows 4 g .. 4 g + 3 of a column are one 16-B vector (the K = 4 q + u slots of a lane's B operand)
__device__ __forceinline__ size_t kpack16(int r, int i) { return ((size_t)(r >> 2) * 16 + i) * 4 + (r & 3); }
// fp64 factor [len][k] -> f32 operand copy [len_pad][ld] (columns >= k and rows >= len stay zero)
__host__ __device__ __forceinline__ size_t bk_index(int r, int i, int NT, int piece);
__device__ __forceinline__ void bk_store(unsigned short* __restrict__ Bk, int r, int i, int NT, float x);
#ifndef RESNMTF_TEMPLATES_ONLY
static __global__ __launch_bounds__(256) void factor_to_f32_kernel(const double* __restrict__ W, int len, int k,
                                                            float* __restrict__ W32, int ld, int nt, int kpack,
                                                            unsigned short* __restrict__ Wk /* bf16 pieces (k > 16) or nullptr */) {
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (size_t)len * k) return;
  const int r = (int)(idx / k), i = (int)(idx % k);
  W32[kpack ? kpack16(r, i) : (size_t)r * ld + fperm(i, nt)] = (float)W[idx];
  if (Wk) bk_store(Wk, r, i, nt, (float)W[idx]);
}
// ---- fp16 images of X for the bandwidth-bound passes (k <= 16): max entry (X >= 0), then the K-packed, scaled image
static __global__ __launch_bounds__(256) void max_entry_kernel(const float* __restrict__ X, size_t count, unsigned int* __restrict__ out) {
  float m = 0.f;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < count; i += (size_t)gridDim.x * 256) m = fmaxf(m, X[i]);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off));
  if ((threadIdx.x & 63) == 0) atomicMax(out, __float_as_uint(m));     // non-negative floats order like their bit patterns
}
// tile-major f32 image [rows_pad][64] per tile  ->  tile-major K-packed fp16 image [rows_pad / 4][64][4] per tile, x scale
// u16 != 0: uniform 16-bit quantisation instead (round(x * scale), scale = 1 / step, step a power of two with
// max / step < 2^16): the absolute error is 2^-17 of the largest entry on EVERY entry, where fp16's is 2^-12 of each
// entry -- on block-structured data an order of magnitude less in Frobenius norm (tools/quant_study.py)
static __global__ __launch_bounds__(256) void pack_half_kernel(const float* __restrict__ X32, size_t ts32, int rows_pad, int ntiles,
                                                        float scale, _Float16* __restrict__ X16, size_t ts16, int u16,
                                                        double* __restrict__ sq_err /* [gridDim.x]: the block's sum (x~ - x)^2, or nullptr */) {
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;       // (tile, row group, column)
  const size_t per_tile = (size_t)(rows_pad / 4) * 64;
  __shared__ double red[4];
  double e2 = 0.0;
  const bool active = idx < per_tile * ntiles;
  if (active) {
  const int tile = (int)(idx / per_tile);
  const size_t rem = idx % per_tile;
  const int g = (int)(rem / 64), c = (int)(rem % 64);
  const float* src = X32 + (size_t)tile * ts32 + (size_t)(4 * g) * 64 + c;
  typedef _Float16 h4 __attribute__((ext_vector_type(4)));
  typedef unsigned short us4 __attribute__((ext_vector_type(4)));
  _Float16* dst = X16 + (size_t)tile * ts16 + ((size_t)g * 64 + c) * 4;
  if (u16) {
    us4 v;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const float x = src[(size_t)u * 64];
      v[u] = (unsigned short)fminf(rintf(x * scale), 65535.f);
      const double d = (double)v[u] / (double)scale - (double)x;
      e2 += d * d;
    }
    *reinterpret_cast<us4*>(dst) = v;
  } else {
    h4 v;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const float x = src[(size_t)u * 64];
      v[u] = (_Float16)(x * scale);
      const double d = (double)(float)v[u] / (double)scale - (double)x;
      e2 += d * d;
    }
    *reinterpret_cast<h4*>(dst) = v;
  }
  }
  if (sq_err) {                                         // one partial per block, summed in a fixed order by reduce_sum_kernel: the same bits on every run
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) e2 += __shfl_xor(e2, off);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = e2;
    __syncthreads();
    if (threadIdx.x == 0) sq_err[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
  }
}
#endif      // RESNMTF_TEMPLATES_ONLY

// --------------------------------------------------------------------------------------
// Streaming pass  P[s] = A[rows of split s]^T * B[rows of split s]   (the two big contractions)
//   X.G   : A = Xt32 [m_pad][n_pad],  B = G32  ->  U = X G      (R/update_steps.r:146  x %*% input_g)
//   Xt.F  : A = X32  [n_pad][m_pad],  B = F32  ->  T = X^T F    (R/update_steps.r:185  crossprod(x, input_f))
// (crossprod(input_f, x) %*% input_g of :223 needs no third pass: (F^T X) G = (X^T F)^T G = T^T G.)
// Aux tiles reuse the body with A = a factor's f32 copy ([rows_pad][64]) or the constant 1:
//   X.G launch : G32 -> G^T G (:148,:224),  T32 -> T^T G (:223),  1 -> colSums(G) (:250)
//   Xt.F launch: F32 -> F^T F (:187,:224),  1 -> colSums(F)
//
// One workgroup = NW waves = one 64-column tile of A x one row split.  Wave w takes rows
// r0 + 4 NW i + 4 w + q (q = lane>>4), each lane loads 16 B = A[row][c0 + 4p .. 4p+3] (p = lane&15)
// -> 4 rows x 256 contiguous bytes per wave-instruction, the workgroup as a whole streams 4 NW
// consecutive rows per step.  Element jj of that float4 is the A operand of MFMA jj
// (v_mfma_f32_16x16x4_f32: A[i=p][k=q]), so MFMA jj produces the output rows c0 + 4 i + jj; the
// B operand B[k=q][j=p] = B32[row][16 nt + p] is shared by the four.  No LDS and no barrier in
// the main loop; the waves' accumulators are tree-summed through LDS at the end.
// --------------------------------------------------------------------------------------
#define RESNMTF_MAX_AUX 3
struct PassArgs {
  const float* A; int lda; int ntiles;      // main operand, ntiles = cols_pad / 64
  size_t tile_stride;                       // floats between the 64-column tiles of A (tile-major image: lda = 64)
  const _Float16* A16; size_t tile_stride16;  // fp16 passes: K-packed image and its tile stride (halves)
  float out_scale;                          // fp16 passes: 1 / (scale of A16 x scale of the B pieces)
  const float* B; int ldb;                  // [rows_pad][ldb]: ldb = KP (mode A, compact) or 64 (mode B: also an aux tile)
  const unsigned short* Bk;                 // k > 16: the K-packed bf16 pieces of B (pass_body_wide), written by the update kernels
  int tw, ntg;                              // k > 16: tiles per workgroup (8 or 4) and tile groups = ceil(ntiles / tw); main grid = ntg * nsplit
  float* P;                                 // main partials [nsplit][cols_pad][KP]
  int cols_pad;
  int rows_pad;                             // contraction extent (multiple of 64)
  int rows_per_split; int nsplit;           // main: rows per split (multiple of 64)
  const float* aux[RESNMTF_MAX_AUX];        // aux operands ([rows_pad][64], mode B); nullptr = constant 1
  int naux;
  float* Paux;                              // aux partials [naux][nsplit_aux][64][KP]
  int rows_per_split_aux; int nsplit_aux;
  int* aux_cnt;                             // arrival counter of the aux workgroups (0 between launches)
  int kk_block0;                            // mode A: no aux workgroups, the k x k job is workgroup 0
  int no_kk;                                // mode A launch without a k x k job (SVD initialisation passes)
  const SweepCtl* ctl; int check_done;      // convergence mode only: leave when ctl->done
  int* fuse_zero;                           // mode A: arrival counter of the SIBLING launch's fused update blocks (pass_fused_kernel),
                                            // zeroed here by workgroup 0 -- the two launches of a pair never overlap in stream order
  // k > 16 (wide form), XCD-aware order of the main workgroups: the dispatcher deals workgroups round-robin to the 8 XCDs
  // (workgroup i -> XCD i % 8), each with its own L2, and every workgroup of a row split re-reads that split's B block (the
  // factor's bf16 pieces) from L2 -- in split-major grid order all 8 L2s fetch every split (c5 Xt.F: +154 MB = 8 x the 19 MB
  // of F per launch, profiles/r02_pmc_c5v1_summary.txt).  The first xcd_n main workgroups are therefore renumbered so that
  // XCD x works through a CONTIGUOUS range of the split-major list (one or two splits per L2): workgroup i of the grid becomes
  // number xcd_off[i % 8] + (i - xcd_first[i % 8]) / 8.  (A short last split keeps its place at the end of the grid: its
  // workgroups are the late starters of the launch model.)
  int xcd_n; int xcd_first[8]; int xcd_off[8];
};
__device__ __forceinline__ int xcd_order(const PassArgs& a, int b /* main-workgroup number in grid order */, int gi /* blockIdx.x */) {
  if (b >= a.xcd_n) return b;
  const int x = gi & 7;
  return a.xcd_off[x] + ((gi - a.xcd_first[x]) >> 3);
}

// Shared end of a pass workgroup: tree-sum of the NW waves' accumulators through LDS (lane-major slots: conflict-free,
// no index math), then the [64][KP] f32 slab of this (tile, split).
template <int NT, int NW>
__device__ __forceinline__ void pass_epilogue(f32x4 (&acc)[4][NT], float* red /*[max(NW/2,1)][64*KP]*/, float* __restrict__ out /*[64][KP]*/) {
  constexpr int KP = 16 * NT;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int p = lane & 15, q = lane >> 4;
#pragma unroll
  for (int s = NW / 2; s >= 1; s >>= 1) {
    if (wave >= s && wave < 2 * s) {
      float* slot = red + (size_t)(wave - s) * 64 * KP;
#pragma unroll
      for (int jj = 0; jj < 4; ++jj)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
          for (int t = 0; t < 4; ++t) slot[((jj * NT + nt) * 4 + t) * 64 + lane] = acc[jj][nt][t];
    }
    __syncthreads();
    if (wave < s) {
      const float* slot = red + (size_t)wave * 64 * KP;
#pragma unroll
      for (int jj = 0; jj < 4; ++jj)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
          for (int t = 0; t < 4; ++t) acc[jj][nt][t] += slot[((jj * NT + nt) * 4 + t) * 64 + lane];
    }
    __syncthreads();
  }
  // D layout of 16x16x4 (and of every bf16 16x16 form): reg t of lane (p,q) = D[i = 4q + t][j = p]; MFMA jj's row i is
  // output row 4 i + jj of the tile  ->  tile row 16 q + 4 t + jj, column 16 nt + p.
  if (wave == 0) {
#pragma unroll
    for (int jj = 0; jj < 4; ++jj)
#pragma unroll
      for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int t = 0; t < 4; ++t)
          red[(16 * q + 4 * t + jj) * KP + 16 * nt + p] = acc[jj][nt][t];
  }
  __syncthreads();
  for (int e = threadIdx.x * 4; e < 64 * KP; e += 256 * NW)
    *reinterpret_cast<f32x4*>(out + e) = *reinterpret_cast<const f32x4*>(&red[e]);
}

// PRE (pass_fused_kernel): the A rows of the FIRST trip were requested by pass_prefetch_a before the workgroup waited for
// its B operand to be published; the first trip only loads B
template <int NW, int UNROLL>
__device__ __forceinline__ bool pass_prefetch_a(const float* __restrict__ A, int lda, int r_begin, int r_end, f32x4 (&av)[UNROLL]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nsteps = (r_end - r_begin) / (4 * NW);
  const bool usable = UNROLL == 4 ? nsteps >= 2 * UNROLL : nsteps >= UNROLL;       // (the trip forms of pass_body)
  const float* a_ptr = A + (size_t)(r_begin + 4 * wave + (lane >> 4)) * lda + 4 * (lane & 15);
  const size_t a_step = (size_t)4 * NW * lda;
#pragma unroll
  for (int u = 0; u < UNROLL; ++u) av[u] = *reinterpret_cast<const f32x4*>(a_ptr + (size_t)(usable ? u : 0) * a_step);
  return usable;
}
template <int NT, int NW, int UNROLL, bool PRE = false>
__device__ __forceinline__ void pass_body(const float* __restrict__ A, int lda, const float* __restrict__ B, int ldb,
                                          int r_begin, int r_end, float* red /*[max(NW/2,1)][64*KP]*/,
                                          float* __restrict__ out /*[64][KP]*/, const f32x4* pre_av = nullptr) {
  constexpr int KP = 16 * NT;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int p = lane & 15, q = lane >> 4;
  const int nsteps = (r_end - r_begin) / (4 * NW);

  f32x4 acc[4][NT];
#pragma unroll
  for (int jj = 0; jj < 4; ++jj)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) acc[jj][nt] = (f32x4){0.f, 0.f, 0.f, 0.f};

  const int row0 = r_begin + 4 * wave + q;
  const float* b_ptr = B + (size_t)row0 * ldb + p * NT;
  const size_t b_step = (size_t)4 * NW * ldb;
  if (A != nullptr) {
    const float* a_ptr = A + (size_t)row0 * lda + 4 * p;
    const size_t a_step = (size_t)4 * NW * lda;
    // UNROLL steps per trip, all loads of a trip in flight together.  Full trips carry no predicate at
    // all; the ragged last trip loads from clamped (valid) addresses and zeroes what lies beyond the
    // split -- branch-free, so the compiler never parks an s_waitcnt vmcnt(0) between loads.
    auto load_full = [&](int i, f32x4 (&av)[UNROLL], float (&bv)[UNROLL][NT]) {
#pragma unroll
      for (int u = 0; u < UNROLL; ++u) {
        // k >= 32: the stream is marked non-temporal (keeps the B operand and the partial slabs in L2;
        // +2.5 % at c4 / c5, -5 % at c2, tools/bench_configs.py)
        if (NT >= 2) av[u] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(a_ptr + (size_t)(i + u) * a_step));
        else av[u] = *reinterpret_cast<const f32x4*>(a_ptr + (size_t)(i + u) * a_step);
        load_b<NT>(b_ptr + (size_t)(i + u) * b_step, bv[u]);
      }
    };
    auto load_masked = [&](int i, f32x4 (&av)[UNROLL], float (&bv)[UNROLL][NT]) {
#pragma unroll
      for (int u = 0; u < UNROLL; ++u) {
        const bool in = i + u < nsteps;
        const int st = in ? i + u : nsteps - 1;
        const f32x4 a = *reinterpret_cast<const f32x4*>(a_ptr + (size_t)st * a_step);
        av[u] = in ? a : (f32x4){0.f, 0.f, 0.f, 0.f};
        float b[NT];
        load_b<NT>(b_ptr + (size_t)st * b_step, b);
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) bv[u][nt] = in ? b[nt] : 0.f;
      }
    };
    auto load_first = [&](f32x4 (&av)[UNROLL], float (&bv)[UNROLL][NT]) {      // trip 0: A from the prefetch (PRE), B now
      if (PRE) {
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) { av[u] = pre_av[u]; load_b<NT>(b_ptr + (size_t)u * b_step, bv[u]); }
      } else {
        load_full(0, av, bv);
      }
    };
    auto mma_trip = [&](const f32x4 (&av)[UNROLL], const float (&bv)[UNROLL][NT]) {
#pragma unroll
      for (int u = 0; u < UNROLL; ++u)
#pragma unroll
        for (int jj = 0; jj < 4; ++jj)
#pragma unroll
          for (int nt = 0; nt < NT; ++nt)
            acc[jj][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[u][jj], bv[u][nt], acc[jj][nt], 0, 0, 0);
    };
    int done = 0;
    if (NT >= 2 || UNROLL == 4) {
      // (k <= 16 takes this form in its UNROLL = 4 instantiation: streamed geometry, see resnmtf_hip.hip)
      // k >= 32 is bound by the f32 MFMA pipe (4 NT MFMAs of 32 cycles per 1 KB load): a wave keeps its
      // next trip's loads in flight while it multiplies -- two register buffers, ping-pong (prefetching
      // two trips ahead -- ring or explicit rotation of three buffers -- measured slower at k = 64: 656 / 710
      // vs 783 view-updates/s on c5v1: the limit there is the MFMA pipe itself, not load latency)
      const int ndouble = nsteps / (2 * UNROLL);
      if (ndouble > 0) {
        f32x4 a0[UNROLL], a1[UNROLL];
        float b0[UNROLL][NT], b1[UNROLL][NT];
        load_first(a0, b0);
        for (int d = 0; d < ndouble; ++d) {
          const int i = d * 2 * UNROLL;
          load_full(i + UNROLL, a1, b1);
          mma_trip(a0, b0);
          if (d + 1 < ndouble) load_full(i + 2 * UNROLL, a0, b0);
          mma_trip(a1, b1);
        }
      }
      done = ndouble * 2 * UNROLL;
    } else {
      const int nfull = nsteps / UNROLL;
      if (PRE && nfull > 0) {
        f32x4 av[UNROLL];
        float bv[UNROLL][NT];
        load_first(av, bv);
        mma_trip(av, bv);
      }
      for (int t = (PRE && nfull > 0) ? 1 : 0; t < nfull; ++t) {
        f32x4 av[UNROLL];
        float bv[UNROLL][NT];
        load_full(t * UNROLL, av, bv);
        mma_trip(av, bv);
      }
      done = nfull * UNROLL;
    }
    for (int i = done; i < nsteps; i += UNROLL) {
      f32x4 av[UNROLL];
      float bv[UNROLL][NT];
      load_masked(i, av, bv);
      mma_trip(av, bv);
    }
  } else {
    // constant-ones operand: every output row is the column sum of B; rows 4i+jj are identical
    for (int i = 0; i < nsteps; ++i) {
      float b[NT];
      load_b<NT>(b_ptr + (size_t)i * b_step, b);
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) acc[0][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(1.0f, b[nt], acc[0][nt], 0, 0, 0);
    }
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) { acc[1][nt] = acc[0][nt]; acc[2][nt] = acc[0][nt]; acc[3][nt] = acc[0][nt]; }
  }

  pass_epilogue<NT, NW>(acc, red, out);
}


// --------------------------------------------------------------------------------------
// k > 16: bf16-piece form of the streaming pass on v_mfma_f32_16x16x32_bf16 (f32-grade), "wide" workgroups.
// The f32 MFMA (32 cycles per 16x16x4) limits the pass once k > 32, and the K = 16 bf16 MFMA of gfx950 takes the same 16
// cycles as the K = 32 one (PMC, profiles/r02_pmc_c5v1_k16_*: 16.2 busy cycles per v_mfma_f32_16x16x16_bf16), so EIGHT
// steps become one K = 32 group.  Each operand is split into three bf16 pieces, each rounded to nearest even,
//     x = h + m + l + O(2^-26 |x|)   (h = bf16(x), m = bf16(x - h), l = bf16(x - h - m); |m| <= 2^-9 |x|, |l| <= 2^-18 |x|),
// and the products  mm + hl + lh + hm + mh + hh  are accumulated in f32, smallest first (dropped: ml, lm, ll <= 2^-26
// relative): f32-grade.  (Pieces cut by TRUNCATION -- an exact sum, but |m| up to 2^-7, |l| up to 2^-14 -- drop
// terms of 2^-21: F / G then sat 1e-5 ... 1e-4 from the fp64 restatement where the plain f32 MFMA sits at 1e-6; tools/k_parity.py.)
//   A (the X image): split in registers, 11 VALU operations per pair of values (v_cvt_pk_bf16_f32 / shift / v_sub).
//   B (the factor): its pieces are written ONCE by the kernel that updates the factor (bk_store), K-packed.
// Workgroup = 8 waves = TW adjacent 64-column tiles x RW = 8 / TW row groups over the same row split.  A trip is 32 RW
// rows; its B block (the pieces of 32 RW rows: 1.5 KB per N-tile and row group... NT 3 64 fragments of 16 B per group)
// is loaded ONCE per workgroup into LDS (double-buffered, one barrier per trip) and read by every wave from there: with
// one tile per workgroup -- the k <= 16 form -- every 64-column tile re-reads the whole B operand from L2, which at
// k = 64 is 1.5 x the bytes of the X stream itself (tools/micro/pass_k32_lab.hip: c5 passes 439 / 369 us -> 343 / 321).
// Each wave owns the [64][KP] outputs of its tile: no cross-wave reduction for RW = 1, one pairwise sum for RW = 2.
// K-slot 8 q + u of lane (p, q) = row 4 u + q of the wave's 32-row block: step u of a wave is 4 consecutive rows = 1 KB
// contiguous of the tile-major image, a wave's trip its own contiguous 8 KB, double-buffered in registers.
// Bk layout (bf16): [block = row / 32][nt = column / 16][piece 0..2][q = row % 4][p = column % 16][u = (row % 32) / 4]:
// the 64 lanes of a wave read 64 consecutive 16-byte fragments.
// --------------------------------------------------------------------------------------
typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef unsigned int u32x4_t __attribute__((ext_vector_type(4)));
__host__ __device__ __forceinline__ size_t bk_index(int r, int i, int NT, int piece) {
  return ((((size_t)(r >> 5) * NT + (i >> 4)) * 3 + piece) * 64 + (r & 3) * 16 + (i & 15)) * 8 + ((r & 31) >> 2);
}
// two f32 -> packed bf16 pair (v_cvt_pk_bf16_f32, round to nearest even); element 0 in the low half
typedef float f32x2_t __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ unsigned int pk_bf16(float a, float b) {
  const f32x2_t v = {a, b};
  return __builtin_bit_cast(unsigned int, __builtin_convertvector(v, bf16x2_t));
}
// the three pieces of one value (each rounded to nearest even), stored at its K-packed place
__device__ __forceinline__ void bk_store(unsigned short* __restrict__ Bk, int r, int i, int NT, float x) {
  const unsigned int h = pk_bf16(x, 0.f) & 0xFFFFu;
  const float r1 = x - __uint_as_float(h << 16);
  const unsigned int m = pk_bf16(r1, 0.f) & 0xFFFFu;
  const float r2 = r1 - __uint_as_float(m << 16);
  const size_t at = bk_index(r, i, NT, 0);
  Bk[at] = (unsigned short)h;
  Bk[at + 512] = (unsigned short)m;                          // (a piece = 64 fragments of 8 values)
  Bk[at + 1024] = (unsigned short)(pk_bf16(r2, 0.f) & 0xFFFFu);
}
// LDS of the wide form: two B buffers of up to two row groups (whole multiples of 512 fragments: every thread stores
// the same number, no predicate); reused at the end (RW = 2) for the partner sums of four tiles
__host__ __device__ constexpr int wide_buf_frags(int NT, int RW) { return (NT * 3 * 64 * RW + 511) / 512 * 512; }
__host__ __device__ constexpr size_t wide_smem_bytes(int NT) {
  return (size_t)2 * wide_buf_frags(NT, 2) * 16 > (size_t)4 * 64 * 16 * NT * 4 ? (size_t)2 * wide_buf_frags(NT, 2) * 16 : (size_t)4 * 64 * 16 * NT * 4;
}

// (no predicate inside the trip loop: a lane-predicated or wave-predicated load makes the compiler park an
// s_waitcnt vmcnt(0) in front of the NEXT trip's loads -- measured 443 instead of 343 us on the c5 X.G pass.  Waves of
// the last tile group that have no tile of their own redo the last tile and do not store; fragments beyond the B block
// are loaded from a clamped address into LDS padding.)
template <int NT, int RW>
__device__ __forceinline__ void pass_body_wide(const float* __restrict__ A, size_t tile_stride, int ntiles, int tile0,
                                               const unsigned short* __restrict__ Bk, int r_begin, int r_end,
                                               u32x4_t* __restrict__ lds, float* __restrict__ out_split /* P + split * cols_pad * KP */) {
  constexpr int KP = 16 * NT, NQ = NT * 3 * 64;         // 16-byte fragments of one 32-row B block
  constexpr int TW = 8 / RW, BUF = wide_buf_frags(NT, RW), NB = BUF / 512, nq = NQ * RW;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), p = lane & 15, q = lane >> 4;
  const int tl = wave % TW, rg = wave / TW;
  const int tile = tile0 + tl;
  const bool valid = tile < ntiles;
  constexpr int trip_rows = 32 * RW;
  const int ntrip = (r_end - r_begin) / trip_rows;      // (the host sizes splits in whole trips)
  f32x4 acc[4][NT];
#pragma unroll
  for (int jj = 0; jj < 4; ++jj)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) acc[jj][nt] = (f32x4){0.f, 0.f, 0.f, 0.f};
  const float* a_ptr = A + (size_t)(valid ? tile : ntiles - 1) * tile_stride + (size_t)(r_begin + 32 * rg + q) * 64 + 4 * p;
  constexpr size_t a_trip = (size_t)trip_rows * 64;
  const u32x4_t* bg = reinterpret_cast<const u32x4_t*>(Bk) + (size_t)(r_begin >> 5) * NQ;
  u32x4_t* ldsB = lds;                                  // [2][BUF]
  int bidx[NB];
#pragma unroll
  for (int e = 0; e < NB; ++e) bidx[e] = min((int)threadIdx.x + 512 * e, nq - 1);
  auto load_a = [&](int t, f32x4 (&av)[8]) {
#pragma unroll
    for (int u = 0; u < 8; ++u) av[u] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(a_ptr + (size_t)t * a_trip + (size_t)u * 256));
  };
  auto load_bg = [&](int t, u32x4_t (&g)[NB]) {
#pragma unroll
    for (int e = 0; e < NB; ++e) g[e] = bg[(size_t)t * nq + bidx[e]];
  };
  auto store_b = [&](int buf, const u32x4_t (&g)[NB]) {
#pragma unroll
    for (int e = 0; e < NB; ++e) ldsB[buf * BUF + threadIdx.x + 512 * e] = g[e];
  };
  auto compute = [&](const f32x4 (&av)[8], int buf) {
    u32x4_t bq[NT][3];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
      for (int pc = 0; pc < 3; ++pc) bq[nt][pc] = ldsB[buf * BUF + rg * NQ + (nt * 3 + pc) * 64 + lane];
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) {
      u32x4_t ah, am, al;
#pragma unroll
      for (int d = 0; d < 4; ++d) {                     // K-slots 2 d (low half) and 2 d + 1 (high half)
        const float x0 = av[2 * d][jj], x1 = av[2 * d + 1][jj];
        const unsigned int ph = pk_bf16(x0, x1);
        const float r0 = x0 - __uint_as_float(ph << 16), r1 = x1 - __uint_as_float(ph & 0xFFFF0000u);
        const unsigned int pm = pk_bf16(r0, r1);
        const float s0 = r0 - __uint_as_float(pm << 16), s1 = r1 - __uint_as_float(pm & 0xFFFF0000u);
        ah[d] = ph; am[d] = pm; al[d] = pk_bf16(s0, s1);
      }
      const bf16x8_t fh = __builtin_bit_cast(bf16x8_t, ah), fm = __builtin_bit_cast(bf16x8_t, am), fl = __builtin_bit_cast(bf16x8_t, al);
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {                 // smallest terms first
        const bf16x8_t gh = __builtin_bit_cast(bf16x8_t, bq[nt][0]), gm = __builtin_bit_cast(bf16x8_t, bq[nt][1]),
                       gl = __builtin_bit_cast(bf16x8_t, bq[nt][2]);
        acc[jj][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fm, gm, acc[jj][nt], 0, 0, 0);
        acc[jj][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fh, gl, acc[jj][nt], 0, 0, 0);
        acc[jj][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fl, gh, acc[jj][nt], 0, 0, 0);
        acc[jj][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fh, gm, acc[jj][nt], 0, 0, 0);
        acc[jj][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fm, gh, acc[jj][nt], 0, 0, 0);
        acc[jj][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fh, gh, acc[jj][nt], 0, 0, 0);
      }
    }
  };
#ifdef WIDE_DEPTH3
  // (experiment, tools/micro/pass_k32_lab.hip -DWIDE_DEPTH3: the A rows TWO trips ahead -- three register buffers -- so that a
  //  trip's loads have two compute phases to land; the B block stays one trip ahead)
  if (ntrip > 0) {
    f32x4 a0[8], a1[8], a2[8];
    u32x4_t g[NB];
    load_bg(0, g); load_a(0, a0);
    if (ntrip > 1) load_a(1, a1);
    store_b(0, g);
    __syncthreads();
#define WIDE_STAGE(T, ACUR, ANEXT2, BUFCUR)                                  \
    if ((T) < ntrip) {                                                       \
      if ((T) + 1 < ntrip) load_bg((T) + 1, g);                              \
      if ((T) + 2 < ntrip) load_a((T) + 2, ANEXT2);                          \
      compute(ACUR, BUFCUR);                                                 \
      if ((T) + 1 < ntrip) store_b((BUFCUR) ^ 1, g);                         \
      __syncthreads();                                                       \
    }
    for (int t = 0; t < ntrip; t += 6) {
      WIDE_STAGE(t, a0, a2, 0) WIDE_STAGE(t + 1, a1, a0, 1) WIDE_STAGE(t + 2, a2, a1, 0)
      WIDE_STAGE(t + 3, a0, a2, 1) WIDE_STAGE(t + 4, a1, a0, 0) WIDE_STAGE(t + 5, a2, a1, 1)
    }
#undef WIDE_STAGE
  }
#else
  if (ntrip > 0) {
    f32x4 a0[8], a1[8];
    u32x4_t g[NB];
    // (the B fragments are requested BEFORE the A rows of the same trip: loads complete in order, so waiting for the B
    // block -- it has to be in LDS one trip ahead -- then leaves the eight A loads behind it in flight)
#ifdef WIDE_A_FIRST
#define WIDE_LOADS(T, AV) load_a(T, AV); load_bg(T, g)
#else
#define WIDE_LOADS(T, AV) load_bg(T, g); load_a(T, AV)
#endif
    WIDE_LOADS(0, a0);
    store_b(0, g);
    __syncthreads();
    for (int t = 0; t < ntrip; t += 2) {
      if (t + 1 < ntrip) { WIDE_LOADS(t + 1, a1); }
      compute(a0, 0);
      if (t + 1 < ntrip) store_b(1, g);
      __syncthreads();
      if (t + 1 < ntrip) {
        if (t + 2 < ntrip) { WIDE_LOADS(t + 2, a0); }
        compute(a1, 1);
        if (t + 2 < ntrip) store_b(0, g);
        __syncthreads();
      }
    }
  }
#endif
  // D layout: reg t of lane (p, q) = D[i = 4 q + t][j = p]; MFMA jj's row i is output row 4 i + jj of the tile
  if (RW == 2) {                                         // the two row groups of a tile: one pairwise sum through LDS
    float* red = reinterpret_cast<float*>(lds);          // (the trip loop ended with a barrier: nobody reads the B buffers any more)
    if (rg == 1) {
#pragma unroll
      for (int jj = 0; jj < 4; ++jj)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
          for (int t = 0; t < 4; ++t) red[(size_t)tl * 64 * KP + ((jj * NT + nt) * 4 + t) * 64 + lane] = acc[jj][nt][t];
    }
    __syncthreads();
    if (rg == 0) {
#pragma unroll
      for (int jj = 0; jj < 4; ++jj)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
          for (int t = 0; t < 4; ++t) acc[jj][nt][t] += red[(size_t)tl * 64 * KP + ((jj * NT + nt) * 4 + t) * 64 + lane];
    }
  }
  if (!valid || rg != 0) return;
  float* out = out_split + (size_t)tile * 64 * KP;
#pragma unroll
  for (int jj = 0; jj < 4; ++jj)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
      for (int t = 0; t < 4; ++t) out[(16 * q + 4 * t + jj) * KP + 16 * nt + p] = acc[jj][nt][t];
}

// --------------------------------------------------------------------------------------
// helpers
// --------------------------------------------------------------------------------------
// sum_{t < count} p[t * stride] in index order, fp64 accumulation, up to 8 loads in flight (a plain
// loop with a runtime bound is compiled to one load -> wait -> add per iteration)
template <typename T>
__device__ __forceinline__ double sum_strided(const T* __restrict__ p, size_t stride, int count) {
  double s = 0.0;
  for (int sp = 0; sp < count; sp += 8) {
    T t[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) t[q] = (sp + q < count) ? p[(size_t)(sp + q) * stride] : (T)0;
#pragma unroll
    for (int q = 0; q < 8; ++q) s += (double)t[q];
  }
  return s;
}

// k x k matrices live in LDS as fp64 [KP][KP], exactly zero outside the k x k corner, so every
// product can run over the padded extent with compile-time loop bounds.
// C = A * B   (optionally A^T or B^T) by a workgroup of NTHR threads
template <int KP, int NTHR, bool TA, bool TB>
__device__ __forceinline__ void kk_mm(double* __restrict__ C, const double* __restrict__ A,
                                      const double* __restrict__ B) {
  // thread t owns the outputs e = t + NTHR ii.  With K K >= NTHR they share their column j, so B[l][j] is read once
  // per l for all of them (9 LDS reads per 8 FMAs instead of 16; the A reads of a wave are broadcasts); every output
  // still accumulates in the order l = 0 .. KP - 1.  (TB -- B read along a column of a row-major matrix, all lanes on
  // one bank -- is kept for completeness; the callers transpose in LDS first, kk_transpose.)
  constexpr int NE = (KP * KP + NTHR - 1) / NTHR;
  if (KP >= 32 && KP % 16 == 0) {
    // k > 16: 16 x 16 output tiles on the fp64 MFMA (v_mfma_f64_16x16x4_f64: lane (p, q) supplies A[i = p][l = q] and
    // B[l = q][j = p], register t of the result is C[4 t + q][p]), tiles dealt round-robin to the waves.  Two LDS reads per
    // 16 x 16 x 4 block instead of nine per eight FMAs: the scalar form below is LDS-bound at k = 64 (8 us per product on
    // 1024 threads, 15 on 512 -- the k x k job of a c5-sized view 53-63 us, s_chain_kernel 280).  The A read of the
    // untransposed form walks a column of a row-major matrix (16-way bank conflict, 32 cycles) -- still under the 64
    // cycles the instruction itself takes on this part.
    constexpr int NTL = KP / 16, NWV = NTHR / 64;
    const int wv = threadIdx.x >> 6, ln = threadIdx.x & 63, p = ln & 15, q = ln >> 4;
    for (int tile = wv; tile < NTL * NTL; tile += NWV) {
      const int ti = tile / NTL, tj = tile % NTL;
      f64x4 d = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int s4 = 0; s4 < KP / 4; ++s4) {
        const int l = 4 * s4 + q;
        const double av = TA ? A[l * KP + 16 * ti + p] : A[(16 * ti + p) * KP + l];
        const double bv = TB ? B[(16 * tj + p) * KP + l] : B[l * KP + 16 * tj + p];
        d = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, d, 0, 0, 0);
      }
#pragma unroll
      for (int t = 0; t < 4; ++t) C[(16 * ti + 4 * t + q) * KP + 16 * tj + p] = d[t];
    }
    return;
  }
  if (KP * KP >= NTHR && NTHR % KP == 0) {
    const int j = threadIdx.x % KP, i0 = threadIdx.x / KP;
    constexpr int ISTEP = NTHR / KP;
    double acc[NE];
#pragma unroll
    for (int ii = 0; ii < NE; ++ii) acc[ii] = 0.0;
#pragma unroll 8
    for (int l = 0; l < KP; ++l) {
      const double bv = TB ? B[j * KP + l] : B[l * KP + j];
#pragma unroll
      for (int ii = 0; ii < NE; ++ii) {
        const int i = i0 + ISTEP * ii;
        acc[ii] += (TA ? A[l * KP + i] : A[i * KP + l]) * bv;
      }
    }
#pragma unroll
    for (int ii = 0; ii < NE; ++ii) C[(i0 + ISTEP * ii) * KP + j] = acc[ii];
    return;
  }
#pragma unroll
  for (int ii = 0; ii < NE; ++ii) {
    const int e = threadIdx.x + NTHR * ii, i = e / KP, j = e % KP;
    if (e < KP * KP) {
      double s = 0.0;
#pragma unroll 16
      for (int l = 0; l < KP; ++l) {
        const double av = TA ? A[l * KP + i] : A[i * KP + l];
        const double bv = TB ? B[j * KP + l] : B[l * KP + j];
        s += av * bv;
      }
      C[e] = s;
    }
  }
}
// dst = src^T  (LDS to LDS)
template <int KP, int NTHR>
__device__ __forceinline__ void kk_transpose(double* __restrict__ dst, const double* __restrict__ src) {
#pragma unroll
  for (int ii = 0; ii < (KP * KP + NTHR - 1) / NTHR; ++ii) {
    const int e = threadIdx.x + NTHR * ii, i = e / KP, j = e % KP;
    if (e < KP * KP) dst[j * KP + i] = src[e];
  }
}
// LDS [KP][KP] <- global [k][k] (zero padded)
template <int KP, int NTHR>
__device__ __forceinline__ void kk_load(double* __restrict__ M, const double* __restrict__ src, int k) {
#pragma unroll
  for (int ii = 0; ii < (KP * KP + NTHR - 1) / NTHR; ++ii) {
    const int e = threadIdx.x + NTHR * ii, i = e / KP, j = e % KP;
    if (e < KP * KP) M[e] = (i < k && j < k) ? src[i * k + j] : 0.0;
  }
}
// global [k][k] <- LDS [KP][KP]
template <int KP, int NTHR>
__device__ __forceinline__ void kk_store(double* __restrict__ dst, const double* __restrict__ M, int k) {
#pragma unroll
  for (int ii = 0; ii < (KP * KP + NTHR - 1) / NTHR; ++ii) {
    const int e = threadIdx.x + NTHR * ii, i = e / KP, j = e % KP;
    if (e < KP * KP && i < k && j < k) dst[i * k + j] = M[e];
  }
}
// Sums the aux tiles' partial slabs over the aux splits (split order, fp64 accumulation):
//   M0 [KP][KP] (LDS)      <- rows a < k of kind 0                       (a Gram product)
//   X1 (registers, e = tid + NTHR ii) <- rows a < k of kind 1            (the cross product; NMAT == 2)
//   returns to thread j < k the column sum  = row 0 of the constant-ones kind `ones_kind`
// Every load of a batch (all matrices, up to BATCH splits) is issued before the first add, and
// with KP*KP < NTHR the splits are divided over NTHR / (KP*KP) thread groups that are combined
// through `tmp` (>= NMAT * NTHR + NTHR doubles): one or two memory round trips in total.
// Ends with a barrier.
template <int KP, int NTHR, int NMAT>
__device__ __forceinline__ double kk_sum_slabs(double* __restrict__ M0, double (&X1)[(KP * KP + NTHR - 1) / NTHR],
                                               const float* __restrict__ Paux, int nsplit, int ones_kind, int k,
                                               double* __restrict__ tmp) {
  constexpr int KK = KP * KP;
  constexpr int NE = (KK + NTHR - 1) / NTHR;
  constexpr int BATCH = (NE * NMAT <= 2) ? 16 : 4;      // (up to 2 x 8 x 4 loads in flight per thread at k = 64)
  const size_t sstride = (size_t)64 * KP;                 // one slab
  const size_t kstride = (size_t)nsplit * sstride;        // one kind
  double csum = 0.0;
  if (KK >= NTHR) {
    // column sum first (its loads overlap the first matrix batch)
    // (every load of a batch is issued without a test in between and nothing touches a loaded value before the adds: a
    // load behind `if (b + q < nsplit)` is a memory round trip of its own -- the k = 64 job spent most of its 40-65 us in
    // them.  Slots beyond nsplit and lanes outside the k x k corner re-read a valid address and are left out of the sum.)
    float ct[16];
    const bool cj = threadIdx.x < (unsigned)k;
    const unsigned cjx = cj ? threadIdx.x : 0u;
    for (int b = 0; b < nsplit; b += 16) {
#pragma unroll
      for (int q = 0; q < 16; ++q) ct[q] = Paux[ones_kind * kstride + (size_t)min(b + q, nsplit - 1) * sstride + cjx];
#pragma unroll
      for (int q = 0; q < 16; ++q) csum += (cj && b + q < nsplit) ? (double)ct[q] : 0.0;
    }
    double s0[NE], s1[NE];
#pragma unroll
    for (int ii = 0; ii < NE; ++ii) { s0[ii] = 0.0; s1[ii] = 0.0; }
    for (int b = 0; b < nsplit; b += BATCH) {
      float t0[NE][BATCH], t1[NE][BATCH];
#pragma unroll
      for (int ii = 0; ii < NE; ++ii) {
        const int e = threadIdx.x + NTHR * ii, i = e / KP, j = e % KP;
        const int ep = fperm(i, KP / 16) * KP + j;          // slab row of product row i (interleaved A operand)
        const bool on = e < KK && i < k && j < k;
        const int epc = on ? ep : 0;
#pragma unroll
        for (int q = 0; q < BATCH; ++q) {
          const size_t at = (size_t)min(b + q, nsplit - 1) * sstride + epc;
          t0[ii][q] = Paux[at];
          t1[ii][q] = NMAT == 2 ? Paux[kstride + at] : 0.f;
        }
      }
#pragma unroll
      for (int ii = 0; ii < NE; ++ii) {
        const int e = threadIdx.x + NTHR * ii, i = e / KP, j = e % KP;
        const bool on = e < KK && i < k && j < k;
#pragma unroll
        for (int q = 0; q < BATCH; ++q) {
          const bool in = on && b + q < nsplit;
          s0[ii] += in ? (double)t0[ii][q] : 0.0; s1[ii] += (NMAT == 2 && in) ? (double)t1[ii][q] : 0.0;
        }
      }
    }
#pragma unroll
    for (int ii = 0; ii < NE; ++ii) {
      const int e = threadIdx.x + NTHR * ii;
      if (e < KK) M0[e] = s0[ii];
      X1[ii] = s1[ii];
    }
    __syncthreads();
  } else {
    constexpr int NG = NTHR / KK;                          // thread groups over the splits
    const int g = threadIdx.x / KK, e = threadIdx.x % KK, i = e / KP, j = e % KP;
    const int ep = fperm(i, KP / 16) * KP + j;            // (identity here: this branch is k <= 16)
    const int per = (nsplit + NG - 1) / NG;
    const int b0 = min(g * per, nsplit), b1 = min(b0 + per, nsplit);
    const bool on = g < NG && i < k && j < k;
    // column sum: group g, column j = e (threads e < k of every group)
    const bool cj = g < NG && e < k;
    double s0 = 0.0, s1 = 0.0, sc = 0.0;
    for (int b = b0; b < b1; b += BATCH) {
      float t0[BATCH], t1[BATCH], tc[BATCH];
#pragma unroll
      for (int q = 0; q < BATCH; ++q) {
        const bool in = b + q < b1;
        t0[q] = (on && in) ? Paux[(size_t)(b + q) * sstride + ep] : 0.f;
        t1[q] = (NMAT == 2 && on && in) ? Paux[kstride + (size_t)(b + q) * sstride + ep] : 0.f;
        tc[q] = (cj && in) ? Paux[ones_kind * kstride + (size_t)(b + q) * sstride + e] : 0.f;
      }
#pragma unroll
      for (int q = 0; q < BATCH; ++q) { s0 += (double)t0[q]; s1 += (double)t1[q]; sc += (double)tc[q]; }
    }
    tmp[threadIdx.x] = s0;
    tmp[NTHR + threadIdx.x] = (NMAT == 2) ? s1 : sc;
    if (NMAT == 2) tmp[2 * NTHR + threadIdx.x] = sc;
    __syncthreads();
    X1[0] = 0.0;
    if (threadIdx.x < KK) {
      double r0 = 0.0, r1 = 0.0;
#pragma unroll
      for (int gg = 0; gg < NG; ++gg) { r0 += tmp[gg * KK + threadIdx.x]; if (NMAT == 2) r1 += tmp[NTHR + gg * KK + threadIdx.x]; }
      M0[threadIdx.x] = r0;
      X1[0] = r1;
    }
    if (threadIdx.x < (unsigned)k) {
#pragma unroll
      for (int gg = 0; gg < NG; ++gg) csum += tmp[(NMAT == 2 ? 2 : 1) * NTHR + gg * KK + threadIdx.x];
    }
    __syncthreads();
  }
  return csum;
}
// Mode A source: the update kernel's fp64 partials [nblk][stride] = Gram [KP*KP], (cross [KP*KP]),
// colsum [KP].  Same outputs as kk_sum_slabs.  Ends with a barrier.
template <int KP, int NTHR, int NMAT>
__device__ __forceinline__ double kk_sum_partials(double* __restrict__ M0, double (&X1)[(KP * KP + NTHR - 1) / NTHR],
                                                  const double* __restrict__ part, int nblk, double* __restrict__ tmp) {
  constexpr int KK = KP * KP;
  constexpr int NE = (KK + NTHR - 1) / NTHR;
  // loads in flight per thread: the job's length is the number of dependent batches (each a memory
  // round trip under the pass's load, tools/stamps.py), so the batch is as deep as registers allow
  constexpr int BATCH = (NE * NMAT == 1) ? 16 : (NE * NMAT == 2) ? 6 : 2;
  const size_t stride = (size_t)NMAT * KK + KP;
  double csum = 0.0;
  if (KK >= NTHR) {
    if (threadIdx.x < KP) csum = sum_strided(part + (size_t)NMAT * KK + threadIdx.x, stride, nblk);
    double s0[NE], s1[NE];
#pragma unroll
    for (int ii = 0; ii < NE; ++ii) { s0[ii] = 0.0; s1[ii] = 0.0; }
    for (int b = 0; b < nblk; b += BATCH) {
      double t0[NE][BATCH], t1[NE][BATCH];
#pragma unroll
      for (int ii = 0; ii < NE; ++ii) {
        const int e = threadIdx.x + NTHR * ii;
#pragma unroll
        for (int q = 0; q < BATCH; ++q) {
          const bool in = e < KK && b + q < nblk;
          t0[ii][q] = in ? part[(size_t)(b + q) * stride + e] : 0.0;
          t1[ii][q] = (NMAT == 2 && in) ? part[(size_t)(b + q) * stride + KK + e] : 0.0;
        }
      }
#pragma unroll
      for (int ii = 0; ii < NE; ++ii)
#pragma unroll
        for (int q = 0; q < BATCH; ++q) { s0[ii] += t0[ii][q]; s1[ii] += t1[ii][q]; }
    }
#pragma unroll
    for (int ii = 0; ii < NE; ++ii) {
      const int e = threadIdx.x + NTHR * ii;
      if (e < KK) M0[e] = s0[ii];
      X1[ii] = s1[ii];
    }
    __syncthreads();
  } else {
    // k = 16 (K K < NTHR).  The job's length is its number of DEPENDENT memory round trips -- each
    // costs several microseconds while the pass saturates the memory system (tools/stamps.py) -- so
    // the loads are spread over all threads and issued in as few shots as registers allow:
    //   matrix values: T = NMAT K K per record; NTHR / T thread groups take interleaved records,
    //                  DEEP loads in flight per thread;
    //   column sums  : thread (record lane = tid / KP, column = tid % KP), records lane, lane + NTHR/KP, ...
    // Everything is combined through LDS in a fixed order (bitwise reproducible).
    constexpr int T = NMAT * KK;                  // 256 or 512
    constexpr int NG = NTHR / T;                  // 2 or 1
    constexpr int DEEP = 40;
    constexpr int NL = NTHR / KP;                 // record lanes of the column sums
    const int g = threadIdx.x / T, e = threadIdx.x % T;
    const bool on = g < NG;
    const int cl = threadIdx.x / KP, cc = threadIdx.x % KP;
    double sm = 0.0, sc = 0.0;
    // first shot: the column-sum records and DEEP matrix records leave together
    double tc[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) tc[q] = (cl + q * NL < nblk) ? part[(size_t)(cl + q * NL) * stride + T + cc] : 0.0;
    for (int b = g; b < nblk; b += NG * DEEP) {
      double t[DEEP];
#pragma unroll
      for (int q = 0; q < DEEP; ++q) t[q] = (on && b + q * NG < nblk) ? part[(size_t)(b + q * NG) * stride + e] : 0.0;
#pragma unroll
      for (int q = 0; q < DEEP; ++q) sm += t[q];
    }
#pragma unroll
    for (int q = 0; q < 8; ++q) sc += tc[q];
    for (int b = cl + 8 * NL; b < nblk; b += NL * 8) {       // more than 8 NL records (large n only)
      double t[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) t[q] = (b + q * NL < nblk) ? part[(size_t)(b + q * NL) * stride + T + cc] : 0.0;
#pragma unroll
      for (int q = 0; q < 8; ++q) sc += t[q];
    }
    tmp[threadIdx.x] = sm;
    tmp[NTHR + threadIdx.x] = sc;
    __syncthreads();
    X1[0] = 0.0;
    if (threadIdx.x < KK) {
      double r0 = 0.0, r1 = 0.0;
#pragma unroll
      for (int gg = 0; gg < NG; ++gg) {
        r0 += tmp[gg * T + threadIdx.x];
        if (NMAT == 2) r1 += tmp[gg * T + KK + threadIdx.x];
      }
      M0[threadIdx.x] = r0;
      X1[0] = r1;
    }
    if (threadIdx.x < KP) {
#pragma unroll
      for (int l = 0; l < NL; ++l) csum += tmp[NTHR + l * KP + threadIdx.x];
    }
    __syncthreads();
  }
  return csum;
}
template <int NTHR>
__device__ __forceinline__ double block_sum(double v, double* scratch /*[>= NTHR/64]*/) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = v;
  __syncthreads();
  double r = 0.0;
#pragma unroll
  for (int w = 0; w < NTHR / 64; ++w) r += scratch[w];
  __syncthreads();
  return r;
}

// --------------------------------------------------------------------------------------
// Factor update (fused numerator/denominator + multiplicative update epilogue), lean form.
//   IS_G = false : update_f  (R/update_steps.r:141-165)   W = F, product rows Pr = U = X G
//   IS_G = true  : update_g  (R/update_steps.r:180-207)   W = G, product rows Pr = T = X^T F'
//   new = | W o (Pr Ma + Phi) / (W Md + sigma W + 0.5 lm) |,   Ma, Md k x k from the k x k jobs:
//     F: Ma = S^T, Md = S (G^T G S^T)       G: Ma = S, Md = S^T (F'^T F' S)
//   (Md folds the reference's (W S)(Gram S^T) into W (S Gram S^T): fp reassociation only.)
//   Phi = star_prod_relevant (R/utils.r:63-78) through integer row maps.
// Writes the new fp64 rows, their f32 operand copy for the next streaming pass and -- G form -- the
// f32 copy of the reduced product rows T (operand of the T^T G' aux tile).
// The next row group's operands are requested before the current one is processed.
// --------------------------------------------------------------------------------------
#define RESNMTF_MAX_COUPLE 16
struct CoupleDesc {
  const double* W;     // the coupled view's factor [len_w][k] (running value)
  const int* map;      // [len]: row of the coupled view sharing this row's name, or -1; nullptr = identity
  double weight;       // vec[i] = phi[i, v]
  double n_other;      // nrow(mat_list[[i]])
};
struct UpdateArgs {
  int len, k;
  double* W;                  // [len][k] in/out
  float* W32;                 // [len_pad][ld32] f32 operand copy for the next streaming pass
  float* T32;                 // G form: [len_pad][ld32] f32 copy of T
  unsigned short* Wk;         // k > 16: K-packed bf16 pieces of the new rows (B operand of the next streaming pass), bk_store
  int ld32;                   // KP (mode A) or 64 (mode B)
  int kpack32;                // 1: W32 is the K-packed copy of the fp16 passes (k <= 16), T32 unchanged
  const float* P; int nsplit; int cols_pad;     // partials of the producing pass
  const double* Ma; const double* Md;           // [k][k] coefficients
  const double* lm;           // lambda (F) or mu (G), [k]
  double* part;               // EMIT form: [nblk][stride] fp64 partials: Gram [KP*KP], (G: cross [KP*KP]), colsum [KP]
  int gram_only;              // EMIT form, run prologue: update nothing, emit the partials of the CURRENT rows
  int rows_per_block;
  int restricted;             // 0: NaN->1 branch; 1: coupled formula (no NaN guard)
  double sigma;               // sum(vec)
  int n_couple;
  CoupleDesc couple[RESNMTF_MAX_COUPLE];
  const SweepCtl* ctl;
  int check_done;             // convergence mode only: leave when ctl->done
};

// EMIT (small problems, see resnmtf_hip.hip `kk_mode`): the workgroup also emits the fp64 partial
// Gram new^T new, column sums and -- G form -- cross product Pr^T new of its rows, which the
// k x k job (workgroup 0 of the next pass launch) sums; otherwise those products come from the
// MFMA aux tiles of that launch.
// (1024-thread workgroups of one 64-row group were measured slower at c2: 47.6 vs 46.3 us per sweep)
#define UPDATE_THREADS 512
// k > 32: 1024 threads = 16 rows per group.  The two [KP][KP] fp64 coefficient matrices alone take 64 KB of
// LDS there, so only one workgroup fits a CU either way; the larger one halves the groups (barriers) per
// workgroup and doubles the waves per CU (c5-sized view: F update 117 -> see DESIGN.md).
#ifndef RESNMTF_UPD16_THREADS      // k <= 16 (A/B builds: -DRESNMTF_UPD16_THREADS=256 | 1024; measured, tools/round3/upd_threads_ab.sh)
#define RESNMTF_UPD16_THREADS UPDATE_THREADS
#endif
constexpr int update_threads(int KP) { return KP >= 48 ? 1024 : (KP == 16 ? RESNMTF_UPD16_THREADS : UPDATE_THREADS); }
// the two body forms that follow from KP (and EMIT) alone, for resnmtf_update_plan; factor_update_body asserts that they are its own
constexpr bool update_mm64(int KP) {       // num and den of a row group on the fp64 MFMA: whole 16-row tiles, one wave per output tile
  return (KP == 16 || KP == 32 || KP == 64) && (update_threads(KP) / KP) % 16 == 0 &&
         (update_threads(KP) / KP / 16) * 2 * (KP / 16) <= update_threads(KP) / 64;
}
constexpr bool update_packk(int KP, bool emit) { return (KP == 32 || KP == 64) && !emit && update_threads(KP) / KP == 16; }
// the slab-prefetch depth PF of a launch: the bucket of its number of splits, as the end of factor_update_body dispatches it
constexpr int update_split_bucket(int nsplit) { return nsplit <= 4 ? 4 : nsplit <= 8 ? 8 : 16; }
// NCB: coupling-count bucket -- 0 = the unrestricted form (NaN -> 1 branch), else the restricted form with
// room for NCB coupled views in registers (4 keeps the gathered rows within the register budget)
// (the body is a device function: factor_update_kernel runs it per workgroup, pass_fused_kernel runs it in the first
// workgroups of the streaming-pass launch that consumes the updated factor)
template <int KP, bool IS_G, int NCB, bool EMIT>
__device__ __forceinline__ void factor_update_body(const UpdateArgs& a, const int blk, double* __restrict__ smem) {
  constexpr bool COUPLED = NCB > 0;
  constexpr int UT = update_threads(KP);
  constexpr int RG = UT / KP;                        // rows per group
  constexpr int KK = KP * KP;
  constexpr int NC = COUPLED ? NCB : 1;
  constexpr int NE = (KK + UT - 1) / UT;             // Gram entries per thread (KK >= UT)
  constexpr int NGRP = (KK < UT) ? UT / KK : 1;      // KK < UT: row slices of a group summed by NGRP thread groups
  constexpr int RSL = RG / NGRP;                     // rows per slice
  constexpr int PSTRIDE = (IS_G ? 2 : 1) * KK + KP;
  // k = 32 / 64 (16-row groups): the two products of a group, num = Pr Ma and den = W Md, run on the fp64
  // MFMA (v_mfma_f64_16x16x4_f64), one wave per 16 x 16 output tile: 2 LDS reads per MFMA instead of 2 per
  // FMA (the scalar form is LDS-bandwidth bound at k = 64: 50000 x 64 x 128 reads = 3.3 GB per launch).
  // LDS pitches are padded so that the operand reads of a half-wave hit 32 distinct 8-byte slots.
  constexpr int NRT = RG / 16;                       // 16-row tiles of a group
  constexpr bool MM64 = (KP == 16 || KP == 32 || KP == 64) && RG % 16 == 0 && NRT * 2 * (KP / 16) <= UT / 64;
  static_assert(MM64 == update_mm64(KP), "update_mm64 (what resnmtf_update_plan reports) has drifted from the body");
  constexpr int P16 = (KP % 32 == 0) ? KP + 16 : KP + 32;   // a pitch == 16 (mod 32) doubles
  constexpr int PMa = MM64 ? P16 : KP;               // pitch of Ma / Md       (B operand: lanes (j, k) -> slot j + 16 k)
  constexpr int PSU = MM64 ? KP + 2 : KP;            // pitch of sU / sW       (A operand: lanes (i, k) -> slot 2 i + k)
  constexpr int PNM = P16;                           // pitch of sNum / sDen   (D: lanes (p, q) -> slot p + 16 q)
  double* Ma = smem;                 // [KP][PMa]
  double* Md = Ma + KP * PMa;        // [KP][PMa]
  double* sU = Md + KP * PMa;        // [RG][PSU]  product rows
  double* sW = sU + RG * PSU;        // [RG][PSU]  old rows
  double* sN = sW + RG * PSU;        // [RG][KP]   new rows            (EMIT)
  double* sR = sN + RG * KP;         // [2][UT]    slice partials      (EMIT, KK < UT)
  double* sNum = sR + 2 * UT;        // [RG][PNM]  num, den of the group (MM64)
  double* sDen = sNum + RG * PNM;
  constexpr int SU = IS_G ? 8 : 0;     // stamp columns (diagnostic build)
  (void)SU;
  STAMP_U(SU + 0);
  const int k = a.k;
  const int rr = threadIdx.x / KP, i = threadIdx.x % KP;
  const bool lane_ok = (threadIdx.x < RG * KP) && (i < k);
  const int r_begin = blk * a.rows_per_block;
  const int r_end = min(r_begin + a.rows_per_block, a.len);

  // request the first group's operands, then the coefficients.  The product partials are kept RAW
  // (one register per split, up to PF) and summed when the group is processed, so that nothing
  // waits on these loads before the next barrier.  PF is the bucket (4 / 8 / 16) of the number of splits and the whole
  // body is instantiated per bucket: the PF loads of a request are then issued back to back, without a test between
  // them -- with one `if (q < nsplit)` per load the compiler waited for the first before testing for the second, and put
  // the loads of slabs 2.. of the NEXT group behind the end-of-trip barrier and a wait for this trip's stores (c2: F
  // update 5.9 -> see DESIGN.md section 5).  Slots of the bucket beyond nsplit re-read the last slab (a cache hit) and
  // are left out of the sum; nothing else touches a loaded value before it is needed.
  auto run = [&](auto pf_tag) {
  constexpr int PF = decltype(pf_tag)::value;
  const int ns = a.nsplit < PF ? a.nsplit : PF;
  double w = 0.0, cval[NC];
  float praw[PF];
  auto request = [&](int g0, float (&pr)[PF], double& w_, double (&cv)[NC]) {
    const int r = g0 + rr;
    w_ = 0.0;
#pragma unroll
    for (int q = 0; q < PF; ++q) pr[q] = 0.f;
    if (lane_ok && r < r_end) {
      w_ = a.W[(size_t)r * k + i];
      if (COUPLED)
#pragma unroll
        for (int c = 0; c < NC; ++c)
          if (c < a.n_couple) {
            const int* mp = a.couple[c].map;
            const int mr = mp ? mp[r] : r;                       // identity maps need no lookup
            cv[c] = (mr >= 0) ? a.couple[c].W[(size_t)mr * k + i] : w_;
          }
      const float* pp = a.P + (size_t)r * KP + i;
      const size_t ps = (size_t)a.cols_pad * KP;
#pragma unroll
      for (int q = 0; q < PF; ++q) pr[q] = pp[(size_t)(q < ns ? q : ns - 1) * ps];
    }
  };
  auto finish_u = [&](int g0, const float (&pr)[PF]) -> double {   // split order, fp64 accumulation
    double u_ = 0.0;
#pragma unroll
    for (int q = 0; q < PF; ++q) u_ += (q < ns) ? (double)pr[q] : 0.0;   // (slots beyond nsplit: zeros or re-reads)
    const int r = g0 + rr;
    if (a.nsplit > PF && lane_ok && r < r_end)
      u_ += sum_strided(a.P + ((size_t)PF * a.cols_pad + r) * KP + i, (size_t)a.cols_pad * KP, a.nsplit - PF);
    return u_;
  };
  request(r_begin, praw, w, cval);
  constexpr int NCO = (KK + UT - 1) / UT;
  double co_a[NCO], co_d[NCO];                                      // [k][k] global -> zero-padded [KP][PMa] LDS: every
#pragma unroll
  for (int ii = 0; ii < NCO; ++ii) {                                // load issued (entry 0 stands in where there is none)
    const int e = threadIdx.x + UT * ii, mi = e / KP, mj = e % KP;  // before the first is used -- `in ? load : 0` became
    const int src = (e < KK && mi < k && mj < k) ? mi * k + mj : 0; // one waited-for load per entry (8 round trips at k = 64)
    co_a[ii] = a.Ma[src]; co_d[ii] = a.Md[src];
  }
#pragma unroll
  for (int ii = 0; ii < NCO; ++ii) {
    const int e = threadIdx.x + UT * ii, mi = e / KP, mj = e % KP;
    if (e < KK) {
      const bool in = mi < k && mj < k;
      Ma[mi * PMa + mj] = in ? co_a[ii] : 0.0;
      Md[mi * PMa + mj] = in ? co_d[ii] : 0.0;
    }
  }
  const double half_lm = lane_ok ? 0.5 * a.lm[i] : 0.0;            // :151 / :188
  double gram[NE], cross[NE], colsum = 0.0;
#pragma unroll
  for (int ii = 0; ii < NE; ++ii) { gram[ii] = 0.0; cross[ii] = 0.0; }
  // k <= 16: the partial products of a group are ONE fp64 MFMA chain per matrix (v_mfma_f64_16x16x4_f64,
  // RG / 4 instructions): wave 0 the Gram new^T new, wave 1 the cross Pr^T new (G form), the next wave the
  // column sums (A = 1).  A[i][k] and B[k][j] of the Gram are the same register: lane (p, q) holds
  // new[4 s + q][p].  Accumulated over the groups in registers, no LDS reduction.
  constexpr bool MFMA64 = EMIT && KP == 16;
  constexpr bool PACKK = (KP == 32 || KP == 64) && !EMIT && RG == 16;   // bf16 pieces of a row group staged through LDS
  static_assert(PACKK == update_packk(KP, EMIT), "update_packk (what resnmtf_update_plan reports) has drifted from the body");
  f64x4 mg = {0.0, 0.0, 0.0, 0.0}, mc = {0.0, 0.0, 0.0, 0.0}, ms = {0.0, 0.0, 0.0, 0.0};

  for (int g0 = r_begin; g0 < r_end; g0 += RG) {
    const int r = g0 + rr;
    const bool ok = lane_ok && r < r_end;
    const double u_cur = finish_u(g0, praw), w_cur = w;
    if (threadIdx.x < RG * KP) { sU[rr * PSU + i] = u_cur; sW[rr * PSU + i] = w_cur; }
    double cv_cur[NC];
    if (COUPLED) {
#pragma unroll
      for (int c = 0; c < NC; ++c) cv_cur[c] = cval[c];
    }
    __syncthreads();                                   // also publishes Ma / Md on the first trip
    if (g0 == r_begin) STAMP_U(SU + 1);                  // first group's operands have arrived
    if (g0 + RG < r_end) request(g0 + RG, praw, w, cval);   // next group's loads fly during this one
    if (MM64) {
      // wave w: row tile w / (2 NTILES), product ((w / NTILES) & 1 ? den : num), column tile w % NTILES; K = KP in steps of 4
      constexpr int NTILES = KP / 16;
      const int wv = threadIdx.x >> 6, ln = threadIdx.x & 63, mp = ln & 15, mq = ln >> 4;
      if (wv < NRT * 2 * NTILES) {
        const int rt = wv / (2 * NTILES);
        const bool is_den = ((wv / NTILES) & 1) != 0;
        const int tile = wv % NTILES;
        const double* A_ = (is_den ? sW : sU) + rt * 16 * PSU;
        const double* B_ = is_den ? Md : Ma;
        f64x4 d = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int s4 = 0; s4 < KP / 4; ++s4)
          d = __builtin_amdgcn_mfma_f64_16x16x4f64(A_[mp * PSU + 4 * s4 + mq], B_[(4 * s4 + mq) * PMa + 16 * tile + mp], d, 0, 0, 0);
        double* O_ = (is_den ? sDen : sNum) + rt * 16 * PNM;
#pragma unroll
        for (int t = 0; t < 4; ++t) O_[(4 * t + mq) * PNM + 16 * tile + mp] = d[t];    // D: row 4 t + q, column p
      }
      __syncthreads();
    }
    double nw = (EMIT && a.gram_only) ? w_cur : 0.0;
    if (ok && !(EMIT && a.gram_only)) {
      double num = 0.0, den = 0.0;
      if (MM64) {
        num = sNum[rr * PNM + i];
        den = sDen[rr * PNM + i];
      } else {
#pragma unroll 16
        for (int j = 0; j < KP; ++j) {                 // padded extent: everything is zero beyond k
          num += sU[rr * PSU + j] * Ma[j * PMa + i];
          den += sW[rr * PSU + j] * Md[j * PMa + i];
        }
      }
      if (!COUPLED) {
        double ratio = num / (den + half_lm);                        // :153 / :191
        if (ratio != ratio) ratio = 1.0;                             // :154 / :192  NaN -> 1
        nw = fabs(w_cur * ratio);                                    // :155,:164 / :193,:206
      } else {
        double acc = 0.0;                                            // star_prod_relevant, utils.r:63-78
#pragma unroll
        for (int c = 0; c < NC; ++c)
          if (c < a.n_couple) acc = acc + (a.couple[c].weight * cv_cur[c]) * a.couple[c].n_other;   // utils.r:73
        const double phi_num = acc / (double)a.len;                  // utils.r:77
        nw = fabs(w_cur * ((num + phi_num) / (den + a.sigma * w_cur + half_lm)));  // :159-162 / :201-204
      }
      a.W[(size_t)r * k + i] = nw;
      // (k > 16: replicas of a view another rank owns pass no f32 copy, bf16 pieces or T32 -- only passes read them)
      if (KP == 16 || a.W32) a.W32[(KP == 16 && a.kpack32) ? kpack16(r, i) : (size_t)r * a.ld32 + fperm(i, KP / 16)] = (float)nw;
      if (KP > 16 && !PACKK && a.Wk) bk_store(a.Wk, r, i, KP / 16, (float)nw);
      if (IS_G && (KP == 16 || a.T32)) a.T32[(size_t)r * a.ld32 + fperm(i, KP / 16)] = (float)u_cur;
    }
    if (PACKK && a.Wk) {
      // k = 32 / 64: the K-packed bf16 pieces of the group's 16 rows (half a 32-row block: four of a fragment's eight
      // K-slots) leave as 8-byte stores, three per (N-tile, q, p), instead of three scattered 2-byte stores per entry
      // (c5-sized view: F update 68 -> see DESIGN.md section 5)
      float* sNf = reinterpret_cast<float*>(sN);
      if (threadIdx.x < RG * KP) sNf[rr * KP + i] = ok ? (float)nw : 0.f;
      __syncthreads();
      constexpr int NTL = KP / 16;
      if (threadIdx.x < NTL * 64) {
        const int nt = threadIdx.x >> 6, fq = (threadIdx.x >> 4) & 3, fp = threadIdx.x & 15, half = (g0 >> 4) & 1;
        float x[4];
#pragma unroll
        for (int uu = 0; uu < 4; ++uu) x[uu] = sNf[(4 * uu + fq) * KP + 16 * nt + fp];
        typedef unsigned int u32x2_t __attribute__((ext_vector_type(2)));
        u32x2_t ph, pm, pl;
#pragma unroll
        for (int d = 0; d < 2; ++d) {
          const float x0 = x[2 * d], x1 = x[2 * d + 1];
          ph[d] = pk_bf16(x0, x1);
          const float r0 = x0 - __uint_as_float(ph[d] << 16), r1 = x1 - __uint_as_float(ph[d] & 0xFFFF0000u);
          pm[d] = pk_bf16(r0, r1);
          pl[d] = pk_bf16(r0 - __uint_as_float(pm[d] << 16), r1 - __uint_as_float(pm[d] & 0xFFFF0000u));
        }
        // fragment (block, nt, piece, q, p) starts at bk_index(row with r % 4 = q and u = 0, column 16 nt + p); K-slots 4 half ..
        unsigned short* base = a.Wk + bk_index((g0 & ~31) + fq, 16 * nt + fp, NTL, 0) + 4 * half;
        *reinterpret_cast<u32x2_t*>(base) = ph;
        *reinterpret_cast<u32x2_t*>(base + 512) = pm;
        *reinterpret_cast<u32x2_t*>(base + 1024) = pl;
      }
    }
    if (g0 == r_begin) STAMP_U(SU + 2);                  // first group updated, stores issued
    if (EMIT) {
      if (threadIdx.x < RG * KP) sN[rr * KP + i] = ok ? nw : 0.0;
      __syncthreads();
      // partial Gram new^T new, cross Pr^T new (G form) and column sums over this group's rows
      if (MFMA64) {
        const int wv = threadIdx.x >> 6, ln = threadIdx.x & 63, p = ln & 15, q = ln >> 4;
        if (wv < (IS_G ? 3 : 2)) {
#pragma unroll
          for (int s4 = 0; s4 < RG / 4; ++s4) {
            const double nv = sN[(4 * s4 + q) * KP + p];
            if (wv == 0) mg = __builtin_amdgcn_mfma_f64_16x16x4f64(nv, nv, mg, 0, 0, 0);
            else if (IS_G && wv == 1) mc = __builtin_amdgcn_mfma_f64_16x16x4f64(sU[(4 * s4 + q) * PSU + p], nv, mc, 0, 0, 0);   // T^T G'
            else ms = __builtin_amdgcn_mfma_f64_16x16x4f64(1.0, nv, ms, 0, 0, 0);
          }
        }
      } else if (KK >= UT) {
#pragma unroll
        for (int ii = 0; ii < NE; ++ii) {
          const int e = threadIdx.x + UT * ii, ga = e / KP, gb = e % KP;
          if (e < KK) {
            double sg = 0.0, sc = 0.0;
#pragma unroll
            for (int t = 0; t < RG; ++t) {
              sg += sN[t * KP + ga] * sN[t * KP + gb];
              if (IS_G) sc += sU[t * PSU + ga] * sN[t * KP + gb];      // T^T G'
            }
            gram[ii] += sg; cross[ii] += sc;
          }
        }
      } else {
        const int gsl = threadIdx.x / KK, e = threadIdx.x % KK, ga = e / KP, gb = e % KP;
        double sg = 0.0, sc = 0.0;
        if (gsl < NGRP) {
#pragma unroll
          for (int t = 0; t < RSL; ++t) {
            const int row = gsl * RSL + t;
            sg += sN[row * KP + ga] * sN[row * KP + gb];
            if (IS_G) sc += sU[row * PSU + ga] * sN[row * KP + gb];    // T^T G'
          }
        }
        sR[threadIdx.x] = sg;
        if (IS_G) sR[UT + threadIdx.x] = sc;
      }
      if (!MFMA64 && threadIdx.x < KP) {
#pragma unroll 16
        for (int t = 0; t < RG; ++t) colsum += sN[t * KP + threadIdx.x];
      }
    }
    __syncthreads();                                   // sU / sW / sN are rewritten by the next trip
    if (EMIT && !MFMA64 && KK < UT && threadIdx.x < KK) {
#pragma unroll
      for (int gg = 0; gg < NGRP; ++gg) {
        gram[0] += sR[gg * KK + threadIdx.x];
        if (IS_G) cross[0] += sR[UT + gg * KK + threadIdx.x];
      }
      // sR is rewritten only after the next trip's barriers
    }
  }
  STAMP_U(SU + 3);                                       // all groups done
  if (MFMA64) {
    // D layout of the f64 16x16x4 (tools/micro/mfma64_layout.hip): register t of lane (p, q) = D[i = 4 t + q][j = p]
    // (interleaved -- not the 4 q + t of the f32 form)
    double* out = a.part + (size_t)blk * PSTRIDE;
    const int wv = threadIdx.x >> 6, ln = threadIdx.x & 63, p = ln & 15, q = ln >> 4;
    if (wv == 0) {
#pragma unroll
      for (int t = 0; t < 4; ++t) out[(4 * t + q) * KP + p] = mg[t];
    } else if (IS_G && wv == 1) {
#pragma unroll
      for (int t = 0; t < 4; ++t) out[KK + (4 * t + q) * KP + p] = mc[t];
    } else if (wv == (IS_G ? 2 : 1) && q == 0) {
      out[(IS_G ? 2 : 1) * KK + p] = ms[0];                                          // every row of D is the column sum
    }
  } else if (EMIT) {
    double* out = a.part + (size_t)blk * PSTRIDE;
#pragma unroll
    for (int ii = 0; ii < NE; ++ii) {
      const int e = threadIdx.x + UT * ii;
      if (e < KK) {
        out[e] = gram[ii];
        if (IS_G) out[KK + e] = cross[ii];
      }
    }
    if (threadIdx.x < KP) out[(IS_G ? 2 : 1) * KK + threadIdx.x] = colsum;
  }
  };   // run
  if (a.nsplit <= 4) run(std::integral_constant<int, 4>{});             // (update_split_bucket restates these three lines)
  else if (a.nsplit <= 8) run(std::integral_constant<int, 8>{});
  else run(std::integral_constant<int, 16>{});
  STAMP_U(SU + 4);
}
template <int KP, bool IS_G, int NCB, bool EMIT>
__global__ __launch_bounds__((update_threads(KP))) void factor_update_kernel(UpdateArgs a) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  if (a.check_done && a.ctl->done) return;
  factor_update_body<KP, IS_G, NCB, EMIT>(a, (int)blockIdx.x, smem);
}

// --------------------------------------------------------------------------------------
// The F updates of SEVERAL views in one launch (view-sharded runs with a replicated F chain, k <= 16).
// update_f of view w reads the running F of every phi-coupled view (R/update_steps.r:282-287: this sweep's
// for views before w, the previous sweep's for views after it).  When the coupled views share their rows in
// the same order (identity maps: auto-named views, R/utils.r:482-491) element (r, i) of F_w' depends only on
// elements (r, .) of the other views, so one thread walks the views in order with the running values of its
// element in registers: the chain of N dependent launches (N x (kernel + boundary), latency-bound) becomes one
// launch whose loads are all independent of the chain.  Same formulae, same association order as
// factor_update_kernel (num and den as scalar fp64 FMA chains over j instead of its fp64-MFMA tiles).
// Emits the f32 operand copy and the fp64 partial Gram / column sums (MFMA chain, as factor_update_kernel)
// only for the views this handle owns (at most four): nobody reads them for the others.
// --------------------------------------------------------------------------------------
template <int NVB>
struct ChainArgs {
  int len, k, n_views, rows_per_block;
  double* W[NVB];               // [len][k] in/out
  const float* U[NVB];          // [nsplit][len_pad][16] X.G slabs (replicate_f: the one folded slab of the exchange block)
  int nsplit[NVB]; size_t pstride;          // at most 4 splits per view; floats between the slabs of a view
  const double* Ma[NVB]; const double* Md[NVB]; const double* lm[NVB];
  int n_emit;                   // views this handle owns (at most 4 per chain): for them the kernel also emits
  float* W32e[4];               //   the f32 operand copy (pitch 16) and
  double* parte[4];             //   the [nblk][16*16 + 16] fp64 partials (Gram, column sums; G form: Gram, cross T^T G', column sums)
  float* T32e[4];               //   G form: the f32 copy of the product rows T (pitch 16)
  int emit_slot[NVB];           // view -> slot in the two arrays above, or -1
  int kpack32;                  // 1: the operand copies are K-packed (fp16 passes)
  const SweepCtl* ctl; int check_done;      // convergence mode only: leave when ctl->done
  double sigma[NVB];            // sum(phi[, w])
  double n_other[NVB];          // nrow of view c
  double weight[NVB][NVB];      // [w][c] = phi[c, w]
  unsigned cmask[NVB];          // bit c: view c is in view w's coupling list (weight != 0, shared rows not NA)
  unsigned restricted;          // bit w: restricted formula (sigma != 0), else the NaN -> 1 branch
};
template <int NVB>
constexpr size_t f_chain_smem_bytes() {
  constexpr int VB = NVB < 4 ? NVB : 4;
  return (size_t)(2 * NVB * 256 + 2 * VB * 32 * 18 + 2 * VB * 32 * 16 + 4 * 32 * 16 + 2 * 32 * 16) * sizeof(double);
}
// IS_G (k <= 16, replicated G chain, R/update_steps.r:195-204): the same walk for update_g of every view from the folded T
// slabs; the views this handle owns (at most two) also get the f32 copy of T and the cross product T^T G' among their
// partials, exactly as factor_update_kernel<16, true, ., true> emits them
template <int NVB, int PF, bool IS_G = false>   // PF: raw split slabs kept per view (1: the folded slab of an exchange block; 4: up to four splits)
__global__ __launch_bounds__(512) void f_chain_kernel(ChainArgs<NVB> a) {
  constexpr int KP = 16, RG = 32, UT = 512, KK = KP * KP, PSTRIDE = (IS_G ? 2 : 1) * KK + KP;
  constexpr int VB = NVB < 4 ? NVB : 4;  // views per batch of products
  constexpr int PSU = KP + 2;            // pitch of the A operand rows (conflict-free, as factor_update_kernel)
  extern __shared__ __attribute__((aligned(16))) double smem[];
  double* Ma = smem;                     // [NVB][KP][KP]
  double* Md = Ma + NVB * KK;            // [NVB][KP][KP]
  double* sU = Md + NVB * KK;            // [VB][RG][PSU]  product rows
  double* sW = sU + VB * RG * PSU;       // [VB][RG][PSU]  old rows
  double* sNum = sW + VB * RG * PSU;     // [VB][RG][KP]
  double* sDen = sNum + VB * RG * KP;    // [VB][RG][KP]
  double* sN = sDen + VB * RG * KP;      // [4][RG][KP]    new rows of the owned views
  double* sT = sN + 4 * RG * KP;         // [2][RG][KP]    G form: their product rows T
  if (a.check_done && a.ctl->done) return;
  const int k = a.k, nv = a.n_views;
  const int rr = threadIdx.x / KP, i = threadIdx.x % KP;
  const bool lane_ok = i < k;
  const int r_begin = blockIdx.x * a.rows_per_block;
  const int r_end = min(r_begin + a.rows_per_block, a.len);
  double fo[NVB];
  float uo[NVB][PF];
  auto request = [&](int g0, double (&f_)[NVB], float (&u_)[NVB][PF]) {
    const int r = g0 + rr;
    const bool ok = lane_ok && r < r_end;
    // (loads issued back to back, no test between them -- see factor_update_kernel: slots beyond a view's split count re-read
    // its last slab and are left out of the sum)
#pragma unroll
    for (int w = 0; w < NVB; ++w) {
      f_[w] = 0.0;
#pragma unroll
      for (int q = 0; q < PF; ++q) u_[w][q] = 0.f;
      if (w < nv && ok) {
        f_[w] = a.W[w][(size_t)r * k + i];
        const float* pp = a.U[w] + (size_t)r * KP + i;
        const int ns = a.nsplit[w] < PF ? a.nsplit[w] : PF;
#pragma unroll
        for (int q = 0; q < PF; ++q) u_[w][q] = pp[(size_t)(q < ns ? q : ns - 1) * a.pstride];
      }
    }
  };
  request(r_begin, fo, uo);
  // coefficients and lambda: every load issued before the first is used (entries that are not there re-read a valid
  // address and are zeroed at the store) -- one round trip instead of one per `in ? load : 0`
  constexpr int NCO = (NVB * KK + UT - 1) / UT;
  double co_a[NCO], co_d[NCO], lm_raw[NVB];
#pragma unroll
  for (int ii = 0; ii < NCO; ++ii) {
    const int e = threadIdx.x + UT * ii, w = e / KK, mi = (e % KK) / KP, mj = e % KP;
    const bool in = w < nv && mi < k && mj < k;
    const int wc = w < nv ? w : 0, src = in ? mi * k + mj : 0;
    co_a[ii] = a.Ma[wc][src]; co_d[ii] = a.Md[wc][src];
  }
#pragma unroll
  for (int w = 0; w < NVB; ++w) lm_raw[w] = a.lm[w < nv ? w : 0][lane_ok ? i : 0];
#pragma unroll
  for (int ii = 0; ii < NCO; ++ii) {
    const int e = threadIdx.x + UT * ii, w = e / KK, mi = (e % KK) / KP, mj = e % KP;
    if (e < nv * KK) {
      const bool in = mi < k && mj < k;
      Ma[e] = in ? co_a[ii] : 0.0;
      Md[e] = in ? co_d[ii] : 0.0;
    }
  }
  double half_lm[NVB];
#pragma unroll
  for (int w = 0; w < NVB; ++w) half_lm[w] = (w < nv && lane_ok) ? 0.5 * lm_raw[w] : 0.0;
  f64x4 mg = {0.0, 0.0, 0.0, 0.0};
  const int wv = threadIdx.x >> 6, ln = threadIdx.x & 63, mp = ln & 15, mq = ln >> 4;

  for (int g0 = r_begin; g0 < r_end; g0 += RG) {
    const int r = g0 + rr;
    const bool ok = lane_ok && r < r_end;
    double fcur[NVB], ucur[NVB];
#pragma unroll
    for (int w = 0; w < NVB; ++w) {
      fcur[w] = fo[w];
      double u_ = 0.0;
#pragma unroll
      for (int q = 0; q < PF; ++q) u_ += (w < nv && q < a.nsplit[w]) ? (double)uo[w][q] : 0.0;   // split order, fp64 accumulation
      ucur[w] = u_;
    }
    if (g0 + RG < r_end) request(g0 + RG, fo, uo);          // the next group's loads fly during this one
#pragma unroll
    for (int b0 = 0; b0 < NVB; b0 += VB) {
      if (b0 < nv) {
        // num = U Ma and den = F_old Md of up to VB views: independent of the chain, so all of them at once on the
        // fp64 MFMA -- task = (view, 16-row tile, num | den), 4 x VB tasks over the 8 waves, K = 16 in steps of 4
#pragma unroll
        for (int wl = 0; wl < VB; ++wl) {
          sU[(wl * RG + rr) * PSU + i] = ucur[b0 + wl];
          sW[(wl * RG + rr) * PSU + i] = fcur[b0 + wl];
        }
        __syncthreads();                                    // (the first one also publishes Ma / Md)
#pragma unroll
        for (int tt = 0; tt < (4 * VB + 7) / 8; ++tt) {
          const int task = wv + 8 * tt, wl = task >> 2, rt = (task >> 1) & 1;
          const bool is_den = (task & 1) != 0;
          if (task < 4 * VB && b0 + wl < nv) {
            const double* A_ = (is_den ? sW : sU) + (wl * RG + rt * 16) * PSU;
            const double* B_ = (is_den ? Md : Ma) + (b0 + wl) * KK;
            f64x4 d = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int s4 = 0; s4 < KP / 4; ++s4)
              d = __builtin_amdgcn_mfma_f64_16x16x4f64(A_[mp * PSU + 4 * s4 + mq], B_[(4 * s4 + mq) * KP + mp], d, 0, 0, 0);
            double* O_ = (is_den ? sDen : sNum) + (wl * RG + rt * 16) * KP;
#pragma unroll
            for (int t = 0; t < 4; ++t) O_[(4 * t + mq) * KP + mp] = d[t];       // D: row 4 t + q, column p
          }
        }
        __syncthreads();
        // the chain itself: the running values of this thread's element, in registers, no barrier
#pragma unroll
        for (int wl = 0; wl < VB; ++wl) {
          const int w = b0 + wl;
          if (w < nv) {
            const double w_cur = fcur[w];
            double nw = 0.0;
            if (ok) {
              const double num = sNum[(wl * RG + rr) * KP + i], den = sDen[(wl * RG + rr) * KP + i];
              if (!((a.restricted >> w) & 1u)) {
                double ratio = num / (den + half_lm[w]);                       // :153
                if (ratio != ratio) ratio = 1.0;                               // :154  NaN -> 1
                nw = fabs(w_cur * ratio);                                      // :155,:164
              } else {
                double acc = 0.0;                                              // star_prod_relevant, utils.r:63-78
#pragma unroll
                for (int c = 0; c < NVB; ++c)
                  if (c < nv && ((a.cmask[w] >> c) & 1u)) acc = acc + (a.weight[w][c] * fcur[c]) * a.n_other[c];   // utils.r:73
                const double phi_num = acc / (double)a.len;                    // utils.r:77
                nw = fabs(w_cur * ((num + phi_num) / (den + a.sigma[w] * w_cur + half_lm[w])));   // :159-162
              }
              a.W[w][(size_t)r * k + i] = nw;
              if (a.emit_slot[w] >= 0) a.W32e[a.emit_slot[w]][a.kpack32 ? kpack16(r, i) : (size_t)r * KP + i] = (float)nw;
              if (IS_G && a.emit_slot[w] >= 0) a.T32e[a.emit_slot[w]][(size_t)r * KP + i] = (float)ucur[w];
            }
            fcur[w] = nw;
            if (a.emit_slot[w] >= 0) sN[(a.emit_slot[w] * RG + rr) * KP + i] = ok ? nw : 0.0;
            if (IS_G && a.emit_slot[w] >= 0) sT[(a.emit_slot[w] * RG + rr) * KP + i] = ok ? ucur[w] : 0.0;
          }
        }
      }
    }
    __syncthreads();                                        // sN complete; sU / sW / sNum / sDen free for the next group
    // F form: wave 2 e = Gram of owned view e, wave 2 e + 1 = its column sums; G form: waves 3 e, 3 e + 1, 3 e + 2 = Gram,
    // cross T^T G' (A = the product rows), column sums -- the MFMA chains of factor_update_kernel, accumulated over the groups
    constexpr int ROLES = IS_G ? 3 : 2;
    if (wv < ROLES * a.n_emit) {
      const int slot = wv / ROLES, role = IS_G ? wv % ROLES : ((wv & 1) ? 2 : 0);
      const double* sNe = sN + slot * RG * KP;
#pragma unroll
      for (int s4 = 0; s4 < RG / 4; ++s4) {
        const double nvv = sNe[(4 * s4 + mq) * KP + mp];
        if (role == 0) mg = __builtin_amdgcn_mfma_f64_16x16x4f64(nvv, nvv, mg, 0, 0, 0);
        else if (role == 1) mg = __builtin_amdgcn_mfma_f64_16x16x4f64(sT[(slot * RG + 4 * s4 + mq) * KP + mp], nvv, mg, 0, 0, 0);   // T^T G'
        else mg = __builtin_amdgcn_mfma_f64_16x16x4f64(1.0, nvv, mg, 0, 0, 0);
      }
    }
  }
  constexpr int ROLES_O = IS_G ? 3 : 2;
  if (wv < ROLES_O * a.n_emit) {
    const int slot = wv / ROLES_O, role = IS_G ? wv % ROLES_O : ((wv & 1) ? 2 : 0);
    double* out = a.parte[slot] + (size_t)blockIdx.x * PSTRIDE;
    if (role < 2) {
#pragma unroll
      for (int t = 0; t < 4; ++t) out[role * KK + (4 * t + mq) * KP + mp] = mg[t];         // D[i = 4 t + q][j = p]
    } else if (mq == 0) {
      out[(IS_G ? 2 : 1) * KK + mp] = mg[0];                                    // every row of D is the column sum
    }
  }
}

// --------------------------------------------------------------------------------------
// The F (or G) updates of SEVERAL views in one launch at k = 32 / 64 (view-sharded runs with replicated chains).
// One launch per view reads the running factor of every coupled view again -- eight c5-sized views: 8 x 77 us, 326 MB
// each, of which 205 MB are the other views' rows.  Here a workgroup takes 32 rows at a time, loads them of EVERY view
// once (two elements per thread, all views in registers) and walks the views in the reference's order
// (R/update_steps.r:282-287 / :295-303); the two k x k coefficient matrices of the view being worked on sit in LDS
// and are replaced, through registers, while its products run (64 KB per view and row group from L2).  Per view:
// num = U Ma and den = W_old Md on the fp64 MFMA -- the very instruction sequence of factor_update_kernel, so the results
// are bitwise those of one launch per view (tests/test_sharded.py) -- then the element-wise rule with the running values.
// Needs what f_chain_kernel needs: equal lengths and k, identity row maps between coupled views, one folded product
// slab per view (the exchange blocks).  The f32 copy, the K-packed bf16 pieces and (G form) the f32 copy of T are
// written for the one view whose passes run on this rank.
// --------------------------------------------------------------------------------------
template <int NVB>
struct WideChainArgs {
  int len, k, n_views, ngroups, own;      // ngroups: 32-row groups; own: the view this rank streams X of, or -1
  int n_self;                             // nrow of the views (the 1 / n_v of star_prod_relevant, R/utils.r:77): = len, except
                                          // when the launch covers a ROW SLICE of the views (sliced chains)
  double* W[NVB];                         // [len][k] in / out
  float* O32; unsigned o32_stride;        // sliced chains: compact f32 copy [len][KP] of view w's new rows at O32 + w * o32_stride
                                          // (what travels back to the rank that streams X of view w), or nullptr
  float* O32v[NVB];                       // ... or (slice_p2p) straight into the memory of the rank that owns view w: its F_recv / G_recv
                                          // slot for this rank's slice, mapped through hipIpc (peer stores over xGMI); used when O32 == nullptr
  const float* U[NVB];                    // [len_pad][KP]: the folded product slab of the view
  const double* Ma[NVB]; const double* Md[NVB]; const double* lm[NVB];
  float* W32; unsigned short* Wk; float* T32; int ld32;        // of view `own`
  const SweepCtl* ctl; int check_done;
  double sigma[NVB];                      // sum(phi[, w]) (sum(psi[, w]))
  double n_other[NVB];                    // nrow of view c
  double weight[NVB][NVB];                // [w][c] = phi[c, w]
  unsigned cmask[NVB];                    // bit c: view c is in view w's coupling list
  unsigned restricted;                    // bit w: restricted formula, else the NaN -> 1 branch
};
__host__ __device__ constexpr int wide_chain_p16(int KP) { return (KP % 32 == 0) ? KP + 16 : KP + 32; }   // (a pitch == 16 (mod 32) doubles)
__host__ __device__ constexpr size_t wide_chain_smem_bytes(int KP) {
  return (size_t)(2 * KP * wide_chain_p16(KP) + 2 * 32 * (KP + 2) + 2 * 32 * wide_chain_p16(KP) + 8 * KP) * sizeof(double);
}
// SLICED: the launch covers a row slice of the views (sliced chains): no view's operand copies are written here, the new
// rows leave as compact f32 (O32) instead -- a variant of its own because registers decide this kernel (below)
template <int KP, bool IS_G, int NVB, bool SLICED = false>
__global__ __launch_bounds__(16 * KP) void wide_chain_kernel(WideChainArgs<NVB> a) {
  constexpr int UT = 16 * KP, RG = 32, NTL = KP / 16, KK = KP * KP;
  constexpr int PMa = wide_chain_p16(KP), PSU = KP + 2, PNM = wide_chain_p16(KP);   // the pitches of factor_update_kernel (conflict-free operand reads)
  constexpr int NCO = KK / UT;                                  // coefficient entries per thread and matrix
  static_assert(KP == 16 || KP == 32 || KP == 48 || KP == 64, "wide_chain_kernel: KP = 16 ... 64");
  static_assert(KK % UT == 0 && 4 * NTL == UT / 64, "one product task per wave");
  static_assert(NVB <= 8, "half_lm rows in LDS");
  extern __shared__ __attribute__((aligned(16))) double smem[];
  double* Ma = smem;                 // [KP][PMa]   coefficients of the view being worked on
  double* Md = Ma + KP * PMa;
  double* sU = Md + KP * PMa;        // [RG][PSU]   product rows of that view
  double* sW = sU + RG * PSU;        // [RG][PSU]   its old rows
  double* sNum = sW + RG * PSU;      // [RG][PNM]
  double* sDen = sNum + RG * PNM;
  double* sLm = sDen + RG * PNM;     // [8][KP]     lambda / 2 (mu / 2) of every view
  if (a.check_done && a.ctl->done) return;
  const int k = a.k, nv = a.n_views;
  const int rr = threadIdx.x / KP, i = threadIdx.x % KP;
  const bool lane_ok = i < k;
  const int wv = threadIdx.x >> 6, ln = threadIdx.x & 63, mp = ln & 15, mq = ln >> 4;
  // product stage: wave -> (16-row tile, num | den, 16-column tile); 4 NTL tasks = UT / 64 waves
  const int t_rt = wv / (2 * NTL), t_tile = wv % NTL;
  const bool t_den = ((wv / NTL) & 1) != 0;
  for (int e = threadIdx.x; e < 8 * KP; e += UT) {
    const int w = e / KP, c = e % KP;
    sLm[e] = (w < nv && c < k) ? 0.5 * a.lm[w][c] : 0.0;                        // :151 / :188
  }
  // Every load below is issued without a test on what an earlier one returned, and nothing touches a loaded value
  // before it is needed: slots of absent views or rows re-read a valid address (a cache hit) and are dropped where
  // they would be used.  Offsets are 32-bit (scalar base + vector offset addressing: one offset register for all views).
  // Registers decide this kernel: at 1024 threads a spill is a scratch access, i.e. a wait for EVERY load in flight
  // (vmcnt counts in order) at every step -- so the rows of the next group are not prefetched (its loads are exposed
  // once per group, 6 groups per workgroup at c5 size); the product rows and the coefficients are, one step ahead.
  float unext[2];
  double co_a[NCO], co_d[NCO];
  auto rows_of = [&](int g, unsigned (&at)[2], unsigned (&atu)[2], int (&r)[2], bool (&ok)[2]) {
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      r[e] = g * RG + rr + 16 * e; ok[e] = lane_ok && r[e] < a.len;
      const unsigned rc = (unsigned)min(r[e], a.len - 1);
      at[e] = rc * (unsigned)k + (unsigned)(lane_ok ? i : 0); atu[e] = rc * (unsigned)KP + (unsigned)i;
    }
  };
  auto request_u = [&](int g, int w) {                // the product rows of one view
#pragma unroll
    for (int e = 0; e < 2; ++e) unext[e] = a.U[w][(unsigned)min(g * RG + rr + 16 * e, a.len - 1) * (unsigned)KP + (unsigned)i];
  };
  auto request_co = [&](int w) {
#pragma unroll
    for (int ii = 0; ii < NCO; ++ii) {
      const int e = threadIdx.x + UT * ii, mi = e / KP, mj = e % KP;
      const unsigned src = (mi < k && mj < k) ? (unsigned)(mi * k + mj) : 0u;
      co_a[ii] = a.Ma[w][src]; co_d[ii] = a.Md[w][src];
    }
  };
  auto store_co = [&]() {
#pragma unroll
    for (int ii = 0; ii < NCO; ++ii) {
      const int e = threadIdx.x + UT * ii, mi = e / KP, mj = e % KP;
      const bool in = mi < k && mj < k;
      Ma[mi * PMa + mj] = in ? co_a[ii] : 0.0;
      Md[mi * PMa + mj] = in ? co_d[ii] : 0.0;
    }
  };
  int g = blockIdx.x;
  if (g >= a.ngroups) return;
  request_u(g, 0);
  request_co(0);
  store_co();
  for (; g < a.ngroups; g += gridDim.x) {
    int r[2]; bool ok[2]; unsigned at[2], atu[2];
    rows_of(g, at, atu, r, ok);
    double fcur[2][NVB];
#pragma unroll
    for (int e = 0; e < 2; ++e)
#pragma unroll
      for (int w = 0; w < NVB; ++w) fcur[e][w] = a.W[w < nv ? w : 0][at[e]];
    // (rows beyond len and columns beyond k hold re-read values instead of zeros: finite, they meet only the zero rows of
    // the padded coefficients or rows that are never stored -- and no select here means no wait for all 16 loads before
    // the first view's rows can go to LDS)
    const int gn = min(g + (int)gridDim.x, a.ngroups - 1);  // (the last trip re-requests its own group: harmless)
#pragma unroll
    for (int w = 0; w < NVB; ++w) {
      if (w < nv) {                                          // (uniform)
        double ucur[2];
#pragma unroll
        for (int e = 0; e < 2; ++e) {
          ucur[e] = ok[e] ? (double)unext[e] : 0.0;          // one slab: split order and fp64 accumulation are trivial
          sU[(rr + 16 * e) * PSU + i] = ucur[e];
          sW[(rr + 16 * e) * PSU + i] = fcur[e][w];          // (view w's rows are still the old ones)
        }
        const bool last = w + 1 >= nv;
        request_u(last ? gn : g, last ? 0 : w + 1);
        request_co(last ? 0 : w + 1);
        __syncthreads();                                     // sU / sW of this view, Ma / Md stored one step earlier
        {
          const double* A_ = (t_den ? sW : sU) + t_rt * 16 * PSU;
          const double* B_ = t_den ? Md : Ma;
          f64x4 d = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
          for (int s4 = 0; s4 < KP / 4; ++s4)
            d = __builtin_amdgcn_mfma_f64_16x16x4f64(A_[mp * PSU + 4 * s4 + mq], B_[(4 * s4 + mq) * PMa + 16 * t_tile + mp], d, 0, 0, 0);
          double* O_ = (t_den ? sDen : sNum) + t_rt * 16 * PNM;
#pragma unroll
          for (int t = 0; t < 4; ++t) O_[(4 * t + mq) * PNM + 16 * t_tile + mp] = d[t];    // D: row 4 t + q, column p
        }
        __syncthreads();
        // the next view's coefficients, before this step's stores are issued: behind conditional stores the compiler can
        // only wait for everything in flight (vmcnt counts loads and stores in order), i.e. for the stores' round trip
        store_co();                                          // (nobody reads Ma / Md until the next first barrier)
        const double half_lm = sLm[w * KP + i];
        float nwf[2];
#pragma unroll
        for (int e = 0; e < 2; ++e) {
          const double w_cur = fcur[e][w];
          double nw = 0.0;
          if (ok[e]) {
            const double num = sNum[(rr + 16 * e) * PNM + i], den = sDen[(rr + 16 * e) * PNM + i];
            if (!__builtin_amdgcn_readfirstlane((int)((a.restricted >> w) & 1u))) {         // (a scalar branch: one division, not both)
              double ratio = num / (den + half_lm);                              // :153 / :191
              if (ratio != ratio) ratio = 1.0;                                   // :154 / :192  NaN -> 1
              nw = fabs(w_cur * ratio);                                          // :155,:164 / :193,:206
            } else {
              double acc = 0.0;                                                  // star_prod_relevant, utils.r:63-78
#pragma unroll
              for (int c = 0; c < NVB; ++c)
                if (c < nv && ((a.cmask[w] >> c) & 1u)) acc = acc + (a.weight[w][c] * fcur[e][c]) * a.n_other[c];   // utils.r:73
              const double phi_num = acc / (double)a.n_self;                     // utils.r:77
              nw = fabs(w_cur * ((num + phi_num) / (den + a.sigma[w] * w_cur + half_lm)));        // :159-162 / :201-204
            }
            a.W[w][at[e]] = nw;
          }
          fcur[e][w] = nw;
          nwf[e] = (float)nw;
        }
        if (SLICED) {                                        // sliced chains: the rows travel to view w's rank as f32
#pragma unroll
          for (int e = 0; e < 2; ++e)                           // (row r[e], column i of a [len][KP] block = element
            if (ok[e]) (a.O32 ? a.O32 + (size_t)w * a.o32_stride : a.O32v[w])[(unsigned)((g * RG + 16 * e) * KP) + threadIdx.x] = nwf[e];   //  (g RG + 16 e) KP + thread index)
        }
        if (!SLICED && KP >= 32 && w == a.own) {
          // the operand copies of the view whose passes run here: f32 (Gram tiles), f32 T (G form), and the K-packed bf16
          // pieces of the 32-row block as 16-byte stores, three per (N-tile, q, p), staged through LDS as floats
#pragma unroll
          for (int e = 0; e < 2; ++e)
            if (ok[e]) {
              a.W32[(unsigned)r[e] * (unsigned)a.ld32 + (unsigned)fperm(i, NTL)] = nwf[e];
              if (IS_G) a.T32[(unsigned)r[e] * (unsigned)a.ld32 + (unsigned)fperm(i, NTL)] = (float)ucur[e];
            }
          __syncthreads();                                   // every thread has read its num / den
          float* sNf = reinterpret_cast<float*>(sNum);
#pragma unroll
          for (int e = 0; e < 2; ++e) sNf[(rr + 16 * e) * KP + i] = nwf[e];      // (zero for rows / columns that are not there)
          __syncthreads();
          if (threadIdx.x < NTL * 64) {
            const int nt = threadIdx.x >> 6, fq = (threadIdx.x >> 4) & 3, fp = threadIdx.x & 15;
            u32x4_t ph, pm, pl;
#pragma unroll
            for (int dd = 0; dd < 4; ++dd) {
              const float x0 = sNf[(8 * dd + fq) * KP + 16 * nt + fp], x1 = sNf[(8 * dd + 4 + fq) * KP + 16 * nt + fp];
              ph[dd] = pk_bf16(x0, x1);
              const float r0 = x0 - __uint_as_float(ph[dd] << 16), r1 = x1 - __uint_as_float(ph[dd] & 0xFFFF0000u);
              pm[dd] = pk_bf16(r0, r1);
              pl[dd] = pk_bf16(r0 - __uint_as_float(pm[dd] << 16), r1 - __uint_as_float(pm[dd] & 0xFFFF0000u));
            }
            unsigned short* base = a.Wk + bk_index(g * RG + fq, 16 * nt + fp, NTL, 0);
            *reinterpret_cast<u32x4_t*>(base) = ph;
            *reinterpret_cast<u32x4_t*>(base + 512) = pm;
            *reinterpret_cast<u32x4_t*>(base + 1024) = pl;
          }
          // (the next view's product stage writes sNum only after its first barrier)
        }
      }
    }
  }
}

// --------------------------------------------------------------------------------------
// Sliced chains, products first (slice_chain_kernel): the F (G) updates of EVERY view on a 16-row group of this rank's
// slice.  A slice gives a workgroup one or two row groups, so what counts is the LATENCY of a group, and walking the views
// one product stage at a time (wide_chain_kernel: barrier, 16 MFMAs, barrier, rule, per view) leaves a group at ~6 us per
// view.  But only the element-wise rule is a chain: num = U_w Ma_w and den = W_w,old Md_w do not depend on the other views'
// new rows (f_chain_kernel's observation).  So: the rows of all views go to LDS once (U as f32, old rows fp64); the 2 V
// products run two views at a time -- one 16 x 16 output tile per wave, v_mfma_f64_16x16x4_f64 over K = KP in the order of
// factor_update_kernel, hence the same bits -- with the B operand (the view's k x k coefficient matrix, L2-resident) read
// straight from global memory into the MFMA layout (no LDS copy of 2 x 32 KB per view) and requested while the previous
// pair's results cross LDS; then every thread walks the views for its element with all inputs in registers, no barrier.
// Same arguments as wide_chain_kernel (len = rows of the slice, n_self = rows of the views, O32 = the f32 rows that travel).
// --------------------------------------------------------------------------------------
__host__ __device__ constexpr size_t slice_chain_smem_bytes(int KP, int NVB) {
  return (size_t)NVB * 16 * (KP + 2) * 8 + (size_t)NVB * 16 * (KP + 2) * 4 + (size_t)4 * 16 * wide_chain_p16(KP) * 8 + (size_t)NVB * KP * 8 +
         (size_t)(NVB * NVB + NVB) * 8;
}
template <int KP, bool IS_G, int NVB>
__global__ __launch_bounds__(16 * KP) void slice_chain_kernel(WideChainArgs<NVB> a) {
  constexpr int UT = 16 * KP, NTL = KP / 16, PSU = KP + 2, PD = wide_chain_p16(KP), NB = NVB / 2;
  static_assert(NVB % 2 == 0 && (KP == 16 || KP == 32 || KP == 48 || KP == 64), "slice_chain_kernel");
  extern __shared__ __attribute__((aligned(16))) double smem[];
  double* sF = smem;                                            // [NVB][16][PSU]  old rows (A operand of den)
  float* sU = reinterpret_cast<float*>(sF + NVB * 16 * PSU);    // [NVB][16][PSU]  product rows, f32 (A operand of num)
  double* sD = reinterpret_cast<double*>(sU + NVB * 16 * PSU);  // [4][16][PD]     num | den of the pair of views in flight
  double* sLm = sD + 4 * 16 * PD;                               // [NVB][KP]       lambda / 2 (mu / 2)
  double* sCf = sLm + NVB * KP;                                 // [NVB][NVB]      coupling weight of view c in view w's rule (0: none)
  double* sNo = sCf + NVB * NVB;                                // [NVB]           nrow of view c
  if (a.check_done && a.ctl->done) return;
  const int k = a.k, nv = a.n_views;
  const int rr = threadIdx.x / KP, i = threadIdx.x % KP;
  const bool lane_ok = i < k;
  // (read from the kernel arguments inside the walk, the weights were scalar loads behind scalar branches -- one dependent
  // round trip per coupled view and step: ~1 us of the 2 us a walk step took, tools/stamps_slice_chain.py)
  for (int e = threadIdx.x; e < NVB * NVB + NVB; e += UT) {
    if (e < NVB * NVB) {
      const int w = e / NVB, c = e % NVB;
      sCf[e] = (w < nv && c < nv && ((a.cmask[w] >> c) & 1u)) ? a.weight[w][c] : 0.0;
    } else {
      sNo[e - NVB * NVB] = a.n_other[e - NVB * NVB < nv ? e - NVB * NVB : 0];
    }
  }
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));          // (uniform: the task's pointers stay scalar)
  const int ln = threadIdx.x & 63, mp = ln & 15, mq = ln >> 4;
  const int t_tile = wv % NTL, t_slot = wv / NTL;               // slot: view of the pair = slot >> 1, den = slot & 1
  for (int e = threadIdx.x; e < NVB * KP; e += UT) {
    const int w = e / KP, c = e % KP;
    sLm[e] = (w < nv && c < k) ? 0.5 * a.lm[w][c] : 0.0;                          // :151 / :188
  }
  const int ngroups = (a.len + 15) >> 4;
  const int ksteps = (k + 3) >> 2;                              // K-steps that hold a column < k (the others multiply zeros: skipped)
  const unsigned jc = (unsigned)min(16 * t_tile + mp, k - 1);   // (columns >= k: outputs nobody reads; a valid address)
  // per-lane offset of row q of a K-step; the step itself advances the (scalar) matrix pointer.  In the last step the
  // rows >= k re-read row k - 1: they meet the zero columns of A.  (One offset per K-step, all loop invariant, was 16
  // registers the compiler kept -- and spilled -- for the whole kernel.)
  const unsigned b_off = (unsigned)mq * (unsigned)k + jc;
  const unsigned b_off_last = (unsigned)min(mq, k - 1 - 4 * (ksteps - 1)) * (unsigned)k + jc;
  double bq[KP / 4];
  auto load_b = [&](int bt) {                                   // B fragment of this wave's task in pair bt: B[l = 4 s4 + q][j = 16 tile + p]
    const int w = min(2 * bt + (t_slot >> 1), nv - 1);
    const double* M = (t_slot & 1) ? a.Md[w] : a.Ma[w];         // (scalar)
#pragma unroll
    for (int s4 = 0; s4 < KP / 4; ++s4)
      if (s4 < ksteps) bq[s4] = (M + (size_t)(4 * s4) * k)[s4 == ksteps - 1 ? b_off_last : b_off];
  };
  // one row group per workgroup, no loop over groups: with a loop the compiler hoists everything group-invariant out of it
  // -- the 64 coupling weights as register pairs, a mask per coupling bit -- and then spills it (40 registers at k = 64)
  {
    const int g = blockIdx.x;
    if (g >= ngroups) return;
    constexpr int SU = IS_G ? 8 : 0;     // stamp columns (diagnostic build)
    (void)SU;
    STAMP_U(SU + 0);
    const int r = g * 16 + rr;
    const bool ok = lane_ok && r < a.len;
    const unsigned rc = (unsigned)min(r, a.len - 1);
    const unsigned at = rc * (unsigned)k + (unsigned)(lane_ok ? i : 0), atu = rc * (unsigned)KP + (unsigned)i;
    double fcur[NVB];
    float uc[NVB];
#pragma unroll
    for (int w = 0; w < NVB; ++w) { fcur[w] = a.W[w < nv ? w : 0][at]; uc[w] = a.U[w < nv ? w : 0][atu]; }
    load_b(0);
#pragma unroll
    for (int w = 0; w < NVB; ++w) {
      sF[(w * 16 + rr) * PSU + i] = ok ? fcur[w] : 0.0;
      sU[(w * 16 + rr) * PSU + i] = ok ? uc[w] : 0.f;
    }
    __syncthreads();                                            // (the first one also publishes sLm)
    STAMP_U(SU + 1);                                            // rows of every view in LDS
    // the element-wise rule of view w with the running values of this thread's element (R/update_steps.r:282-287 / :295-303)
    auto walk = [&](int w, double num, double den) {
      const double w_cur = fcur[w], half_lm = sLm[w * KP + i];
      double nw = 0.0;
      if (ok) {
        if (!__builtin_amdgcn_readfirstlane((int)((a.restricted >> w) & 1u))) {
          double ratio = num / (den + half_lm);                                  // :153 / :191
          if (ratio != ratio) ratio = 1.0;                                       // :154 / :192  NaN -> 1
          nw = fabs(w_cur * ratio);                                              // :155,:164 / :193,:206
        } else {
          double acc = 0.0;                                                      // star_prod_relevant, utils.r:63-78
#pragma unroll
          for (int c = 0; c < NVB; ++c) {
            const double cf = sCf[w * NVB + c];                                  // (0 where view c is not in view w's list)
            acc = (cf != 0.0) ? acc + (cf * fcur[c]) * sNo[c] : acc;             // utils.r:73
          }
          const double phi_num = acc / (double)a.n_self;                         // utils.r:77
          nw = fabs(w_cur * ((num + phi_num) / (den + a.sigma[w] * w_cur + half_lm)));            // :159-162 / :201-204
        }
        a.W[w][at] = nw;
        (a.O32 ? a.O32 + (size_t)w * a.o32_stride : a.O32v[w])[(unsigned)(g * 16 * KP) + threadIdx.x] = (float)nw;
      }
      fcur[w] = nw;
    };
#pragma unroll
    for (int bt = 0; bt < NB; ++bt) {
      if (2 * bt < nv) {                                        // (uniform)
        const int w = 2 * bt + (t_slot >> 1);
        f64x4 d = {0.0, 0.0, 0.0, 0.0};
        if (w < nv) {                                           // (wave-uniform)
          // A is exactly zero in the columns >= k (rows beyond the slice too), so the K-steps past k add exact zeros and are
          // skipped; in the last, partial step the lanes with l >= k pair a zero of A with a finite re-read of B
          if (t_slot & 1) {
            const double* A_ = sF + (w * 16 + mp) * PSU + mq;
#pragma unroll
            for (int s4 = 0; s4 < KP / 4; ++s4) {
              if (s4 < ksteps) d = __builtin_amdgcn_mfma_f64_16x16x4f64(A_[4 * s4], (4 * s4 + mq < k) ? bq[s4] : 0.0, d, 0, 0, 0);
              if (KP > 48 && (s4 & 3) == 3) __builtin_amdgcn_sched_barrier(0);      // (k = 64, 1024 threads: keep the A reads of at most
            }                                                                      //  four steps live -- registers decide, see above)
          } else {
            const float* A_ = sU + (w * 16 + mp) * PSU + mq;
#pragma unroll
            for (int s4 = 0; s4 < KP / 4; ++s4) {
              if (s4 < ksteps) d = __builtin_amdgcn_mfma_f64_16x16x4f64((double)A_[4 * s4], (4 * s4 + mq < k) ? bq[s4] : 0.0, d, 0, 0, 0);
              if (KP > 48 && (s4 & 3) == 3) __builtin_amdgcn_sched_barrier(0);
            }
          }
        }
        if (KP > 48) __builtin_amdgcn_sched_barrier(0);         // (... and the next pair's B loads behind the last MFMA: they reuse bq)
        __builtin_amdgcn_sched_barrier(0);
        if (bt + 1 < NB && 2 * (bt + 1) < nv) load_b(bt + 1);   // the next pair's B: in flight while this pair's results cross LDS
#pragma unroll
        for (int t = 0; t < 4; ++t) sD[(t_slot * 16 + 4 * t + mq) * PD + 16 * t_tile + mp] = d[t];      // D: row 4 t + q, column p
        if (bt == 0) STAMP_U(SU + 2);                           // first pair's MFMAs done, results stored
        __syncthreads();
        const double n0 = sD[(0 * 16 + rr) * PD + i], d0 = sD[(1 * 16 + rr) * PD + i];
        const double n1 = sD[(2 * 16 + rr) * PD + i], d1 = sD[(3 * 16 + rr) * PD + i];
        __syncthreads();                                        // sD is rewritten by the next pair (sF / sU by the next group)
        // the chain: views in order, this pair's two (the pairs come in view order; the rule reads the other views' running
        // values from registers -- new for the views before, old for those after)
        walk(2 * bt, n0, d0);
        if (2 * bt + 1 < nv) walk(2 * bt + 1, n1, d1);
        if (bt == 0) STAMP_U(SU + 3);                           // first pair walked
      }
    }
    STAMP_U(SU + 4);
  }
}

// --------------------------------------------------------------------------------------
// Sliced chains in two launches (slice_products_kernel + slice_walk_kernel).  slice_chain_kernel keeps a 16-row group in ONE
// workgroup, which then runs its V / 2 product stages one after the other: 16 x 64-cycle fp64 MFMAs per wave and stage on
// four waves per SIMD, each behind the L2 round trip of its B fragments -- ~7 us per pair of views at k = 64, 33 us for a
// group of c5's G slice, on 63 of 256 CUs.  But the products do not depend on the chain at all (only the element-wise rule
// does), so here every (row group, pair of views) is a workgroup of its own -- 4 x the workgroups, the whole chip -- that
// leaves num = U_w Ma_w and den = W_w,old Md_w in a scratch buffer (L2 / infinity-cache resident: 16 KB per view and
// group), and a second launch walks the views element by element with everything it needs in registers.  Same MFMA
// sequence per output tile and the same rule as slice_chain_kernel, hence the same bits.
//   ND: [view][num | den][rows16][KP] fp64, nd_stride = rows16 * KP
// --------------------------------------------------------------------------------------
template <int KP, int NVB>
__global__ __launch_bounds__(16 * KP) void slice_products_kernel(WideChainArgs<NVB> a, double* __restrict__ ND, unsigned nd_stride) {
  constexpr int UT = 16 * KP, NTL = KP / 16, PSU = KP + 2;
  __shared__ double sF[2 * 16 * PSU];                           // old rows of the pair's views (A operand of den)
  __shared__ float sU[2 * 16 * PSU];                            // their product rows, f32 (A operand of num)
  if (a.check_done && a.ctl->done) return;
  const int k = a.k, nv = a.n_views;
  const int g = blockIdx.x, bt = blockIdx.y;
  if (2 * bt >= nv || g * 16 >= a.len) return;
  const int rr = threadIdx.x / KP, i = threadIdx.x % KP;
  const bool lane_ok = i < k;
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int ln = threadIdx.x & 63, mp = ln & 15, mq = ln >> 4;
  const int t_tile = wv % NTL, t_slot = wv / NTL;               // slot: view of the pair = slot >> 1, den = slot & 1
  const int ksteps = (k + 3) >> 2;
  const unsigned jc = (unsigned)min(16 * t_tile + mp, k - 1);
  const unsigned b_off = (unsigned)mq * (unsigned)k + jc;
  const unsigned b_off_last = (unsigned)min(mq, k - 1 - 4 * (ksteps - 1)) * (unsigned)k + jc;
  const int r = g * 16 + rr;
  const bool ok = lane_ok && r < a.len;
  const unsigned rc = (unsigned)min(r, a.len - 1);
  const unsigned at = rc * (unsigned)k + (unsigned)(lane_ok ? i : 0), atu = rc * (unsigned)KP + (unsigned)i;
  const int w0 = 2 * bt, w1 = min(2 * bt + 1, nv - 1);
  const double f0 = a.W[w0][at], f1 = a.W[w1][at];
  const float u0 = a.U[w0][atu], u1 = a.U[w1][atu];
  const int w = min(2 * bt + (t_slot >> 1), nv - 1);
  double bq[KP / 4];
  {
    const double* M = (t_slot & 1) ? a.Md[w] : a.Ma[w];         // (scalar)
#pragma unroll
    for (int s4 = 0; s4 < KP / 4; ++s4)
      if (s4 < ksteps) bq[s4] = (M + (size_t)(4 * s4) * k)[s4 == ksteps - 1 ? b_off_last : b_off];
  }
  sF[(0 * 16 + rr) * PSU + i] = ok ? f0 : 0.0; sF[(1 * 16 + rr) * PSU + i] = ok ? f1 : 0.0;
  sU[(0 * 16 + rr) * PSU + i] = ok ? u0 : 0.f; sU[(1 * 16 + rr) * PSU + i] = ok ? u1 : 0.f;
  __syncthreads();
  if (2 * bt + (t_slot >> 1) >= nv) return;                     // (an odd number of views: the absent one's slots)
  f64x4 d = {0.0, 0.0, 0.0, 0.0};
  if (t_slot & 1) {
    const double* A_ = sF + ((t_slot >> 1) * 16 + mp) * PSU + mq;
#pragma unroll
    for (int s4 = 0; s4 < KP / 4; ++s4)
      if (s4 < ksteps) d = __builtin_amdgcn_mfma_f64_16x16x4f64(A_[4 * s4], (4 * s4 + mq < k) ? bq[s4] : 0.0, d, 0, 0, 0);
  } else {
    const float* A_ = sU + ((t_slot >> 1) * 16 + mp) * PSU + mq;
#pragma unroll
    for (int s4 = 0; s4 < KP / 4; ++s4)
      if (s4 < ksteps) d = __builtin_amdgcn_mfma_f64_16x16x4f64((double)A_[4 * s4], (4 * s4 + mq < k) ? bq[s4] : 0.0, d, 0, 0, 0);
  }
  double* O_ = ND + (size_t)(2 * w + (t_slot & 1)) * nd_stride + (size_t)(g * 16) * KP;
#pragma unroll
  for (int t = 0; t < 4; ++t) O_[(4 * t + mq) * KP + 16 * t_tile + mp] = d[t];      // D: row 4 t + q, column p
}

// (WR rows per workgroup: the walk is eight dependent fp64 divisions per element -- latency -- and a slice of c5's G has 1000
//  rows: 4-row workgroups put it on every CU instead of 63; 12.4 -> see profiles/r03_slice_split_ab.txt)
template <int KP, int NVB, int WR>
__global__ __launch_bounds__(WR * KP) void slice_walk_kernel(WideChainArgs<NVB> a, const double* __restrict__ ND, unsigned nd_stride) {
  constexpr int UT = WR * KP;
  __shared__ double sLm[NVB * KP];                              // lambda / 2 (mu / 2)
  __shared__ double sCf[NVB * NVB];                             // coupling weight of view c in view w's rule (0: none)
  __shared__ double sNo[NVB];                                   // nrow of view c
  if (a.check_done && a.ctl->done) return;
  const int k = a.k, nv = a.n_views;
  const int rr = threadIdx.x / KP, i = threadIdx.x % KP;
  const bool lane_ok = i < k;
  const int g = blockIdx.x;
  if (g * WR >= a.len) return;
  const int r = g * WR + rr;
  const bool ok = lane_ok && r < a.len;
  const unsigned rc = (unsigned)min(r, a.len - 1);
  const unsigned at = rc * (unsigned)k + (unsigned)(lane_ok ? i : 0);
  const unsigned an = rc * (unsigned)KP + (unsigned)i;
  double fcur[NVB], num[NVB], den[NVB];
#pragma unroll
  for (int w = 0; w < NVB; ++w) {
    const int wc = w < nv ? w : 0;
    fcur[w] = a.W[wc][at];
    num[w] = ND[(size_t)(2 * wc) * nd_stride + an]; den[w] = ND[(size_t)(2 * wc + 1) * nd_stride + an];
  }
  for (int e = threadIdx.x; e < NVB * NVB + NVB; e += UT) {
    if (e < NVB * NVB) {
      const int w = e / NVB, c = e % NVB;
      sCf[e] = (w < nv && c < nv && ((a.cmask[w] >> c) & 1u)) ? a.weight[w][c] : 0.0;
    } else {
      sNo[e - NVB * NVB] = a.n_other[e - NVB * NVB < nv ? e - NVB * NVB : 0];
    }
  }
  for (int e = threadIdx.x; e < NVB * KP; e += UT) {
    const int w = e / KP, c = e % KP;
    sLm[e] = (w < nv && c < k) ? 0.5 * a.lm[w][c] : 0.0;                          // :151 / :188
  }
  __syncthreads();
  // the element-wise rule, views in order (R/update_steps.r:282-287 / :295-303): the text of slice_chain_kernel's walk
#pragma unroll
  for (int w = 0; w < NVB; ++w) {
    if (w < nv) {                                               // (uniform)
      const double w_cur = fcur[w], half_lm = sLm[w * KP + i];
      double nw = 0.0;
      if (ok) {
        if (!__builtin_amdgcn_readfirstlane((int)((a.restricted >> w) & 1u))) {
          double ratio = num[w] / (den[w] + half_lm);                            // :153 / :191
          if (ratio != ratio) ratio = 1.0;                                       // :154 / :192  NaN -> 1
          nw = fabs(w_cur * ratio);                                              // :155,:164 / :193,:206
        } else {
          double acc = 0.0;                                                      // star_prod_relevant, utils.r:63-78
#pragma unroll
          for (int c = 0; c < NVB; ++c) {
            const double cf = sCf[w * NVB + c];                                  // (0 where view c is not in view w's list)
            acc = (cf != 0.0) ? acc + (cf * fcur[c]) * sNo[c] : acc;             // utils.r:73
          }
          const double phi_num = acc / (double)a.n_self;                         // utils.r:77
          nw = fabs(w_cur * ((num[w] + phi_num) / (den[w] + a.sigma[w] * w_cur + half_lm)));      // :159-162 / :201-204
        }
        a.W[w][at] = nw;
        (a.O32 ? a.O32 + (size_t)w * a.o32_stride : a.O32v[w])[(unsigned)(g * WR * KP) + threadIdx.x] = (float)nw;
      }
      fcur[w] = nw;
    }
  }
}

// --------------------------------------------------------------------------------------
// kk_f (last-arriving aux workgroup of the Xt.F launch): F'^T F' and colSums(F') from the aux
// slabs, then  FtF, FtFS = (F'^T F') S,  Ma_G = S,  Md_G = S^T ((F'^T F') S)   (R/update_steps.r:185-187)
// --------------------------------------------------------------------------------------
struct KKFArgs {
  int k;
  const double* part; int nblk;       // mode A: the F update's fp64 partials (nullptr in mode B)
  const double* S;                    // [k][k]
  double* FtF; double* FtFS; double* Ma_G; double* Md_G; double* cF;
};
template <int KP, int NTHR>
struct KKFPre { double s[(KP * KP + NTHR - 1) / NTHR]; };
template <int KP, int NTHR>
__device__ __forceinline__ void kk_f_prefetch(const KKFArgs& a, KKFPre<KP, NTHR>& p) {
#pragma unroll
  for (int ii = 0; ii < (KP * KP + NTHR - 1) / NTHR; ++ii) {
    const int e = threadIdx.x + NTHR * ii, i = e / KP, j = e % KP;
    p.s[ii] = a.S[(e < KP * KP && i < a.k && j < a.k) ? i * a.k + j : 0];      // raw: masked where it is stored to LDS (a select
  }                                                                            // here would be a wait for the load)
}
template <int KP, int NTHR, bool FROM_PART>
__device__ __forceinline__ void kk_f_body(const KKFArgs& a, const KKFPre<KP, NTHR>& pre, const float* __restrict__ Paux,
                                          int nsplit_aux, double* smem) {
  double* LA = smem; double* LB = LA + KP * KP; double* LC = LB + KP * KP; double* tmp = LC + KP * KP;
  const int k = a.k;
  double unused[(KP * KP + NTHR - 1) / NTHR];
  // LA = F'^T F', cf = colSums(F').  Mode B aux kinds: 0 = Gram (A = F32), 1 = ones
  // (nothing waits on the prefetched S before these loads have been issued)
  const double cf = FROM_PART ? kk_sum_partials<KP, NTHR, 1>(LA, unused, a.part, a.nblk, tmp)
                           : kk_sum_slabs<KP, NTHR, 1>(LA, unused, Paux, nsplit_aux, 1, k, tmp);
#pragma unroll
  for (int ii = 0; ii < (KP * KP + NTHR - 1) / NTHR; ++ii) {
    const int e = threadIdx.x + NTHR * ii;
    if (e < KP * KP) LB[e] = ((e / KP) < k && (e % KP) < k) ? pre.s[ii] : 0.0;   // LB = S
  }
  STAMP(13);
  __syncthreads();
  // (A operands that are symmetric bit for bit -- the Gram matrices -- are read TRANSPOSED: the plain form walks a column of the
  // row-major matrix, a 16-way LDS bank conflict per read that, with 8-16 waves on the CU's one LDS pipe, costs more than the
  // fp64 MFMAs themselves; same products in the same order, same bits -- see s_chain_kernel)
  kk_mm<KP, NTHR, true, false>(LC, LA, LB);                                      // LC = (F^T F) S        (:187)
  kk_store<KP, NTHR>(a.FtF, LA, k);
  kk_store<KP, NTHR>(a.Ma_G, LB, k);                                             // numerator (X^T F) S   (:185)
  if (threadIdx.x < (unsigned)k) a.cF[threadIdx.x] = cf;
  __syncthreads();
  kk_mm<KP, NTHR, true, false>(LA, LB, LC);                                      // LA = S^T ((F^T F) S)  (:186-187)
  // (F^T F) S goes to memory TRANSPOSED: its one reader, kk_s, uses it as the A operand of ((F^T F) S)(G^T G) and reads it
  // transposed (conflict-free) -- the value at [j][i] of the buffer is ((F^T F) S)[i][j]
#pragma unroll
  for (int ii = 0; ii < (KP * KP + NTHR - 1) / NTHR; ++ii) {
    const int e = threadIdx.x + NTHR * ii, i = e / KP, j = e % KP;
    if (e < KP * KP && i < k && j < k) a.FtFS[j * k + i] = LC[e];
  }
  __syncthreads();
  kk_store<KP, NTHR>(a.Md_G, LA, k);
}

// --------------------------------------------------------------------------------------
// kk_s (last-arriving aux workgroup of the X.G' launch): update_s (R/update_steps.r:220-240),
// update_lm x2 (:249-251,:312-313), calculate_error in trace form (R/utils.r:157-166)
//   ||X - F S G^T||^2 = ||X||^2 - 2 <S', F^T X G> + <(F^T F) S' (G^T G), S'>,
// the coefficients of the next F update  Ma_F = S'^T, Md_F = S' ((G^T G) S'^T)  (:146-148) and,
// on the last view in convergence mode, the stop test of R/main.r:55,77-80.
// mode 0 (run prologue): only the F coefficients, from the current S and G.
// --------------------------------------------------------------------------------------
struct SCouple { const double* S; double weight; };
struct KKSArgs {
  int k, mode;
  const double* part; int nblk;       // mode A: the G update's fp64 partials (nullptr in mode B)
  const double* FtF; const double* FtFS; const double* cF;
  double* S; double* lambda; double* mu;
  double* Ma_F; double* Md_F;
  const double* xnorm2;
  double* err; int err_stride; int err_col; int err_cap;   // err[sweep * stride + col]
  double* err_host; SweepCtl* ctl_host;                    // pinned host mirrors of err / ctl (device-mapped), or nullptr
  double* sblock;             // view-sharded runs with replicated G / S chains: mode 1 stops before the S rule and PUBLISHES
                              // its inputs here (sblock_layout); s_chain_kernel continues on every rank, for every view
  int restricted;             // sum(xi) != 0 (whole matrix, :226)
  double sigma;               // sum(xi[, v])
  int n_couple;
  SCouple couple[RESNMTF_MAX_COUPLE];
  SweepCtl* ctl;
  int last_view;              // 1: this job closes the sweep (counter, convergence test)
  int n_views; double tol;    // tol < 0: no test
};
// the inputs of kk_s that do not depend on the pass launch it rides in (register bundle, entry
// e = tid + NTHR ii).  In mode B every aux workgroup requests them BEFORE its slice of the aux pass,
// so that the last arriver finds them in registers.
template <int KP, int NTHR>
struct KKSPre {
  double sold[(KP * KP + NTHR - 1) / NTHR], ftfs[(KP * KP + NTHR - 1) / NTHR], ftf[(KP * KP + NTHR - 1) / NTHR],
      coup[(KP * KP + NTHR - 1) / NTHR];
  double lam, mu, cf, xn;
  int sweep;
};
template <int KP, int NTHR>
__device__ __forceinline__ void kk_s_prefetch(const KKSArgs& a, KKSPre<KP, NTHR>& p) {
  constexpr int NE = (KP * KP + NTHR - 1) / NTHR;
  const int k = a.k;
  p.sweep = a.ctl->sweep;
#pragma unroll
  for (int ii = 0; ii < NE; ++ii) {
    const int e = threadIdx.x + NTHR * ii, i = e / KP, j = e % KP;
    // RAW values: entries outside the k x k corner and lanes >= k re-read element 0 and are masked where they are used (a
    // select on a loaded value is a wait for it, and a load behind a per-lane test was a round trip of its own: lambda,
    // mu, colSums(F) and ||X||^2 cost four in a row, ~1.7 us each while the pass saturates the memory system)
    const int at = (e < KP * KP && i < k && j < k) ? i * k + j : 0;
    double acc = 0.0, s0 = a.S[at], f0 = 0.0, fs = 0.0;
    if (a.mode == 1) {                                                             // (uniform)
      f0 = a.FtF[at];
      fs = a.FtFS[at];
      if (a.restricted)                                                            // star_prod, utils.r:39-47
        for (int c = 0; c < a.n_couple; ++c) acc = acc + a.couple[c].weight * a.couple[c].S[at];
    }
    p.coup[ii] = acc; p.sold[ii] = s0; p.ftf[ii] = f0; p.ftfs[ii] = fs;
  }
  p.lam = p.mu = p.cf = 0.0; p.xn = 1.0;
  if (a.mode == 1) {
    const unsigned tx = threadIdx.x < (unsigned)k ? threadIdx.x : 0u;
    p.lam = a.lambda[tx]; p.mu = a.mu[tx]; p.cf = a.cF[tx]; p.xn = *a.xnorm2;
  }
}

template <int KP, int NTHR, bool FROM_PART>
__device__ __forceinline__ void kk_s_body(const KKSArgs& a, const KKSPre<KP, NTHR>& pre, const float* __restrict__ Paux,
                                          int nsplit_aux, double* smem) {
  constexpr int NE = (KP * KP + NTHR - 1) / NTHR;
  double* LA = smem; double* LB = LA + KP * KP; double* LC = LB + KP * KP; double* LD = LC + KP * KP;
  double* tmp = LD + KP * KP;        // [3 * NTHR]
  const int k = a.k;
  const int sweep = pre.sweep;       // index of the sweep being closed
  auto publish_pre = [&]() {         // after the sums: nothing waits on the prefetch before their loads are out
#pragma unroll
    for (int ii = 0; ii < NE; ++ii) {
      const int e = threadIdx.x + NTHR * ii;
      const bool corner = (e / KP) < k && (e % KP) < k;                             // (the prefetch holds raw values)
      if (e < KP * KP) { LB[e] = corner ? pre.sold[ii] : 0.0; LC[e] = corner ? pre.ftfs[ii] : 0.0; }   // LB = S, LC = (F^T F) S  (:224)
    }
    __syncthreads();
  };
  if (a.mode == 1) {
    double coup[NE], sold[NE], cross[NE], ftf[NE];
#pragma unroll
    for (int ii = 0; ii < NE; ++ii) { coup[ii] = pre.coup[ii]; sold[ii] = pre.sold[ii]; ftf[ii] = pre.ftf[ii]; cross[ii] = 0.0; }
    const double lam = pre.lam, mu = pre.mu, cf = pre.cf, xn = pre.xn;
    // LA = G'^T G', cross = T^T G' = (F^T X) G (:223), cg = colSums(G').
    // Mode B aux kinds: 0 = Gram (G32), 1 = cross (T32), 2 = ones
    const double cg = FROM_PART ? kk_sum_partials<KP, NTHR, 2>(LA, cross, a.part, a.nblk, tmp)
                             : kk_sum_slabs<KP, NTHR, 2>(LA, cross, Paux, nsplit_aux, 2, k, tmp);
    STAMP(5);
    publish_pre();
    kk_mm<KP, NTHR, true, false>(LD, LC, LA);                                      // LD = ((F^T F) S)(G^T G)   (LC holds ((F^T F) S)^T: kk_f stores it so)
    __syncthreads();
    if (a.sblock) {                                    // hand the S rule's inputs to s_chain_kernel (every rank, every view)
      const int kk = k * k;
      double* sb = a.sblock;
#pragma unroll
      for (int ii = 0; ii < NE; ++ii) {
        const int e = threadIdx.x + NTHR * ii, i = e / KP, j = e % KP;
        if (e < KP * KP && i < k && j < k) {
          const int at = i * k + j;
          sb[at] = sold[ii]; sb[kk + at] = cross[ii]; sb[2 * kk + at] = LD[e]; sb[3 * kk + at] = LA[e]; sb[4 * kk + at] = ftf[ii];
        }
      }
      if (threadIdx.x < (unsigned)k) { sb[5 * kk + threadIdx.x] = cg; sb[5 * kk + k + threadIdx.x] = cf; }
      if (threadIdx.x == 0) sb[5 * kk + 2 * k] = xn;
      return;
    }
    double tr1 = 0.0, snew[NE];
#pragma unroll
    for (int ii = 0; ii < NE; ++ii) {
      const int e = threadIdx.x + NTHR * ii, i = e / KP, j = e % KP;
      snew[ii] = 0.0;
      if (e < KP * KP && i < k && j < k) {
        const double s = sold[ii], num = cross[ii], den = LD[e];
        double ns;
        if (!a.restricted) {
          double ratio = num / den;                                                // :227
          if (ratio != ratio) ratio = 1.0;                                         // :228  NaN -> 1
          ns = fabs(s * ratio);                                                    // :229,:239
        } else {
          ns = fabs(s * ((num + coup[ii]) / (den + a.sigma * s)));                 // :234-237,:239
        }
        tr1 += ns * num;
        snew[ii] = ns;
      }
    }
    __syncthreads();                                   // every reader of LB (= old S) and LD is done
#pragma unroll
    for (int ii = 0; ii < NE; ++ii) {
      const int e = threadIdx.x + NTHR * ii, i = e / KP, j = e % KP;
      if (e < KP * KP) {
        LB[e] = snew[ii];                                                          // LB = S'
        LD[e] = (i < k && j < k) ? ftf[ii] : 0.0;                                  // LD = F^T F
        if (i < k && j < k) a.S[i * k + j] = snew[ii];
      }
    }
    tr1 = block_sum<NTHR>(tr1, tmp);                   // (barriers inside publish LB, LD)
    kk_mm<KP, NTHR, true, false>(LC, LB, LD);                                      // LC = S'^T (F^T F) = ((F^T F) S')^T   (as s_chain_kernel)
    __syncthreads();
    kk_mm<KP, NTHR, true, false>(LD, LC, LA);                                      // LD = (LC)^T (G^T G) = (F^T F) S' (G^T G)   (F^T F no longer needed)
    __syncthreads();
    double tr2 = 0.0;
#pragma unroll
    for (int ii = 0; ii < NE; ++ii) {
      const int e = threadIdx.x + NTHR * ii, i = e / KP, j = e % KP;
      if (e < KP * KP && i < k && j < k) tr2 += LD[e] * snew[ii];
    }
    tr2 = block_sum<NTHR>(tr2, tmp);
    if (threadIdx.x < (unsigned)k) {                                               // update_lm (:249-251)
      a.lambda[threadIdx.x] = cf * lam;
      a.mu[threadIdx.x] = cg * mu;
    }
    if (threadIdx.x == 0) {
      const double e_v = (xn - 2.0 * tr1 + tr2) / xn;
      a.err[(size_t)(sweep % a.err_cap) * a.err_stride + a.err_col] = e_v;
      if (a.err_host) a.err_host[(size_t)(sweep % a.err_cap) * a.err_stride + a.err_col] = e_v;
      if (a.last_view) {
        if (a.tol >= 0.0) {                            // R/main.r:77-80 and the while test of :55
          double sum = 0.0;                            // view order, as the host's mean
          for (int v = 0; v < a.n_views; ++v)
            sum += (v == a.err_col) ? e_v : a.err[(size_t)(sweep % a.err_cap) * a.err_stride + v];
          const double mean = sum / (double)a.n_views;
          const double diff = fabs(mean - a.ctl->prev_mean);
          a.ctl->prev_mean = mean;
          if (!(diff > a.tol)) {
            a.ctl->done = 1; a.ctl->stop_sweep = sweep + 1;
            if (a.ctl_host) { a.ctl_host->done = 1; a.ctl_host->stop_sweep = sweep + 1; }
          }
        }
        a.ctl->sweep = sweep + 1;
        if (a.ctl_host) {
          __threadfence_system();                      // the host may poll this counter: errors first
          a.ctl_host->sweep = sweep + 1;
        }
      }
    }
  } else {
    double unused[NE];                                                             // LA = G^T G (run prologue)
    if (FROM_PART) (void)kk_sum_partials<KP, NTHR, 2>(LA, unused, a.part, a.nblk, tmp);
    else (void)kk_sum_slabs<KP, NTHR, 1>(LA, unused, Paux, nsplit_aux, 2, k, tmp);
    publish_pre();
  }
  STAMP(6);
  // coefficients of the next F update:  Ma = S'^T,  Md = S' ((G^T G) S'^T)   (:146-148)
  kk_transpose<KP, NTHR>(LD, LB);                                                  // LD = S'^T (LD is free by now)
  __syncthreads();
  kk_mm<KP, NTHR, true, false>(LC, LA, LD);                                        // LC = (G^T G) S'^T   (G^T G symmetric: read transposed)
  __syncthreads();
  kk_mm<KP, NTHR, true, false>(LA, LD, LC);                                        // LA = (S'^T)^T LC = S' LC   (G^T G is no longer needed)
#pragma unroll
  for (int ii = 0; ii < NE; ++ii) {
    const int e = threadIdx.x + NTHR * ii, i = e / KP, j = e % KP;
    if (e < KP * KP && i < k && j < k) a.Ma_F[j * k + i] = LB[e];                  // Ma[j][i] = S'[i][j]
  }
  __syncthreads();
  kk_store<KP, NTHR>(a.Md_F, LA, k);
}

// --------------------------------------------------------------------------------------
// View-sharded runs with replicated chains: the second half of kk_s for EVERY view, on every rank.
// update_s of view w reads the running S of every xi-coupled view (R/update_steps.r:231-237, :305-311: this sweep's for
// views before w, the previous sweep's for views after it) -- a chain through the k x k matrices of all views, whose
// inputs (old S, numerator F^T X G, denominator (F^T F S)(G^T G), Gram matrices, column sums) each owner publishes
// (sblock_layout, kk_s_body) and one small all-gather hands to everybody.  The rule itself is element-wise, so workgroup
// w walks views 0 .. w with the running values of an entry in registers (same formulae, same order of additions as
// kk_s_prefetch / kk_s_body) and then finishes ITS view: S', lambda', mu', the error (trace form), Ma_F, Md_F -- the
// latter three straight into every rank's copy of the F / G exchange blocks.  Identical code on identical bytes:
// bitwise the same S, lambda, mu, coefficients on every rank.
//   sblock_layout (doubles): Sold [kk] | N [kk] | D [kk] | GtG [kk] | FtF [kk] | cG [k] | cF [k] | ||X||^2 [1]
// --------------------------------------------------------------------------------------
struct SChainArgs {
  int k, n_views;
  int* view_sweep;                                  // [n_views] device: sweeps closed per view since resnmtf_prepare -- each workgroup
                                                    // keeps its own, so the index never comes from the host (a captured launch replays)
  int* ticket;                                      // arrivals of this launch's workgroups: the last one closes the sweep (stop test)
  double tol; int check_done;                       // convergence mode (R/main.r:50-81): tol >= 0; check_done: leave when ctl->done
  const double* sblocks; size_t sblock_stride;      // doubles between the blocks of consecutive views
  double* S[RESNMTF_MAX_COUPLE + 1];                  // [k][k] per view, out
  double* lambda[RESNMTF_MAX_COUPLE + 1]; double* mu[RESNMTF_MAX_COUPLE + 1];      // [k] per view, in / out
  double* Ma_F[RESNMTF_MAX_COUPLE + 1]; double* Md_F[RESNMTF_MAX_COUPLE + 1];      // [k][k] per view, out
  double xi[RESNMTF_MAX_COUPLE + 1][RESNMTF_MAX_COUPLE + 1];                          // xi[c][w] = weight of view c in view w's rule (0 = none)
  double sigma[RESNMTF_MAX_COUPLE + 1];             // sum(xi[, w])
  int restricted;                                   // sum(xi) != 0 (whole matrix, R/update_steps.r:226)
  double* err; int err_stride; int err_cap; double* err_host;
  SweepCtl* ctl; SweepCtl* ctl_host;
};
// NVB: room for the running entries of NVB views in registers (the walk is unrolled NVB x NVB: with 17 x 17 the code of
// the k = 64 instance no longer fitted the instruction cache -- 283 us where its two halves measured 110 + 33)
constexpr int s_chain_threads(int KP) { return KP >= 48 ? 1024 : 512; }   // one wave per 16 x 16 tile of the k x k products at k = 64
template <int KP, int NVB>
__global__ __launch_bounds__(s_chain_threads(KP)) void s_chain_kernel(SChainArgs a) {
  constexpr int NTHR = s_chain_threads(KP), NE = (KP * KP + NTHR - 1) / NTHR;
  extern __shared__ __attribute__((aligned(16))) double smem[];
  double* LA = smem; double* LB = LA + KP * KP; double* LC = LB + KP * KP; double* LD = LC + KP * KP;
  double* tmp = LD + KP * KP;        // [3 * NTHR]
  if (a.check_done && a.ctl->done) return;
  const int k = a.k, kk = k * k, w = blockIdx.x, nv = a.n_views;
  const int sweep = a.view_sweep[w];                   // index of the sweep being closed (uniform; rewritten at the end)
  STAMP_U(5);                                          // (diagnostic build: columns 5 / 6 / 7 / 13 / 14 of tools/stamps_slice_chain.py)
  // the xi weights of the walk, once, into LDS: read from the kernel arguments inside the unrolled NVB x NVB walk they were
  // scalar loads behind scalar branches (`weight != 0`), one dependent round trip each
  __shared__ double sXi[NVB * NVB];                    // [c][j2] = weight of view j2 in view c's rule (0: none / absent)
  for (int e = threadIdx.x; e < NVB * NVB; e += NTHR) {
    const int c = e / NVB, j2 = e % NVB;
    sXi[e] = (j2 < nv && c < nv && j2 != c) ? a.xi[j2][c] : 0.0;
  }
  __syncthreads();
  const double* mine = a.sblocks + (size_t)w * a.sblock_stride;
  double tr1 = 0.0;
#pragma unroll 2
  for (int ii = 0; ii < NE; ++ii) {
    const int e = threadIdx.x + NTHR * ii, i = e / KP, j = e % KP;
    const bool on = e < KP * KP && i < k && j < k;
    const int at = on ? i * k + j : 0;
    // every load of the entry goes out before the first is used: slots of absent views and of entries outside the k x k
    // corner re-read a valid address and are dropped where they would be used (a load behind a test is a round trip of
    // its own here: 3 x 8 of them per entry at eight views)
    double run[NVB], numv[NVB], denv[NVB], s_w = 0.0, n_w = 0.0;
#pragma unroll
    for (int c = 0; c < NVB; ++c) {
      const double* blk = a.sblocks + (size_t)(c < nv ? c : 0) * a.sblock_stride;
      run[c] = blk[at]; numv[c] = blk[kk + at]; denv[c] = blk[2 * kk + at];
    }
    const double gtg_e = mine[3 * kk + at], ftf_e = mine[4 * kk + at];
#pragma unroll
    for (int c = 0; c < NVB; ++c) run[c] = (on && c < nv) ? run[c] : 0.0;
#pragma unroll
    for (int c = 0; c < NVB; ++c) {
      if (c <= w && on) {
        const double s = run[c], num = numv[c], den = denv[c];
        double ns;
        if (!a.restricted) {
          double ratio = num / den;                                                // :227
          if (ratio != ratio) ratio = 1.0;                                         // :228  NaN -> 1
          ns = fabs(s * ratio);                                                    // :229,:239
        } else {
          double acc = 0.0;                                                        // star_prod, utils.r:39-47
          asm volatile("" ::: "memory");              // (keep the NVB weight reads of this step here: hoisted above the walk,
#pragma unroll                                        //  NVB x NVB of them were live at once and spilled)
          for (int j2 = 0; j2 < NVB; ++j2) {
            const double wgt = sXi[c * NVB + j2];
            acc = (wgt != 0.0) ? acc + wgt * run[j2] : acc;                         // (vec[i] != 0, R/utils.r:42)
          }
          ns = fabs(s * ((num + acc) / (den + a.sigma[c] * s)));                   // :234-237,:239
        }
        run[c] = ns;
        if (c == w) { s_w = ns; n_w = num; }
      }
    }
    if (on) { a.S[w][at] = s_w; tr1 += s_w * n_w; }
    if (e < KP * KP) {
      LB[e] = s_w;                                                                 // LB = S'
      LA[e] = on ? gtg_e : 0.0;                                                    // LA = G'^T G'
      LD[e] = on ? ftf_e : 0.0;                                                    // LD = F'^T F'
    }
  }
  STAMP_U(6);                                          // walk done
  tr1 = block_sum<NTHR>(tr1, tmp);                     // (its barriers publish LA, LB, LD)
  // Every product below reads its A operand TRANSPOSED (kk_mm<TA = true>: A[l][i], consecutive lanes on consecutive words).
  // The plain form walks a column of a row-major [KP][KP] matrix -- a 16-way bank conflict per read, and with 16 waves on the
  // CU's one LDS pipe that, not the MFMA, set the pace: ~9 us per 64 x 64 x 64 product against ~2 (tools/stamps_slice_chain.py).
  // F^T F and G^T G are symmetric bit for bit (every entry the same products in the same order), so for them the transposed
  // read is the same matrix; where S' stands on the left, the product is formed transposed: ((F^T F) S')^T = S'^T (F^T F), each
  // entry the same products a b = b a in the same order of l -- the same bits as before.
  kk_mm<KP, NTHR, true, false>(LC, LB, LD);                                        // LC = S'^T (F^T F) = ((F^T F) S')^T
  __syncthreads();
  kk_mm<KP, NTHR, true, false>(LD, LC, LA);                                        // LD = (LC)^T (G^T G) = (F^T F) S' (G^T G)
  __syncthreads();
  STAMP_U(7);                                          // two k x k products done
  double tr2 = 0.0;
#pragma unroll
  for (int ii = 0; ii < NE; ++ii) {
    const int e = threadIdx.x + NTHR * ii, i = e / KP, j = e % KP;
    if (e < KP * KP && i < k && j < k) tr2 += LD[e] * LB[e];
  }
  tr2 = block_sum<NTHR>(tr2, tmp);
  if (threadIdx.x < (unsigned)k) {                                                 // update_lm (:249-251)
    a.lambda[w][threadIdx.x] = mine[5 * kk + k + threadIdx.x] * a.lambda[w][threadIdx.x];
    a.mu[w][threadIdx.x] = mine[5 * kk + threadIdx.x] * a.mu[w][threadIdx.x];
  }
  if (threadIdx.x == 0) {
    const double xn = mine[5 * kk + 2 * k];
    const double e_v = (xn - 2.0 * tr1 + tr2) / xn;
    const size_t row = (size_t)(sweep % a.err_cap) * a.err_stride;
    __hip_atomic_store(&a.err[row + w], e_v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (a.err_host) a.err_host[row + w] = e_v;
    a.view_sweep[w] = sweep + 1;                       // (every thread read it before the first barrier)
    // the workgroup that arrives last closes the sweep: counter, and -- convergence mode -- the stop test of R/main.r:55,77-80
    // on the mean over ALL views, summed in view order as the host's mean.  Every rank of a view-sharded run evaluates it on
    // the same bytes, so all ranks stop on the same sweep without a collective.
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (__hip_atomic_fetch_add(a.ticket, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == nv - 1) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      __hip_atomic_store(a.ticket, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // ready for the next launch
      if (a.tol >= 0.0) {
        double sum = 0.0;
        for (int v = 0; v < nv; ++v) sum += __hip_atomic_load(&a.err[row + v], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const double mean = sum / (double)nv;
        const double diff = fabs(mean - a.ctl->prev_mean);
        a.ctl->prev_mean = mean;
        if (!(diff > a.tol)) {
          a.ctl->done = 1; a.ctl->stop_sweep = sweep + 1;
          if (a.ctl_host) { a.ctl_host->done = 1; a.ctl_host->stop_sweep = sweep + 1; }
        }
      }
      a.ctl->sweep = sweep + 1;
      if (a.ctl_host) {
        __threadfence_system();                        // the host may poll this counter: errors first
        a.ctl_host->sweep = sweep + 1;
      }
    }
  }
  STAMP_U(13);                                         // error, lambda, mu, ticket done
  // coefficients of the next F update:  Ma = S'^T,  Md = S' ((G^T G) S'^T)   (:146-148)
  kk_transpose<KP, NTHR>(LD, LB);                                                  // LD = S'^T (LD is free by now)
  __syncthreads();
  kk_mm<KP, NTHR, true, false>(LC, LA, LD);                                        // LC = (G^T G) S'^T   (G^T G symmetric: A read transposed)
  __syncthreads();
  kk_mm<KP, NTHR, true, false>(LA, LD, LC);                                        // LA = (S'^T)^T LC = S' LC   (G^T G is no longer needed)
#pragma unroll
  for (int ii = 0; ii < NE; ++ii) {
    const int e = threadIdx.x + NTHR * ii, i = e / KP, j = e % KP;
    if (e < KP * KP && i < k && j < k) a.Ma_F[w][j * k + i] = LB[e];               // Ma[j][i] = S'[i][j]
  }
  __syncthreads();
  kk_store<KP, NTHR>(a.Md_F[w], LA, k);
  STAMP_U(14);
}

// --------------------------------------------------------------------------------------
// fp16 form of the streaming pass (k <= 16, hand-off mode A): A = the K-packed fp16 image of X (half the bytes),
// B = the K-packed f32 copy of the factor, split in registers into two fp16 pieces (x 2^13, hi + lo: 22 bits),
// products on v_mfma_f32_16x16x16_f16, f32 accumulate.  One wave-step = 16 contraction rows: lane (p, q) loads
// 32 B = [columns 4 p .. 4 p + 3][rows 4 (g + q) .. + 3] (the wave: 2 KB contiguous) and 16 B of B (1 KB
// contiguous); element block jj of A is the A operand (K = 4 q + u) of MFMA jj, which yields output rows 4 i + jj
// exactly as in the f32 form, so the epilogue (tree sum, slab layout) is shared.
// --------------------------------------------------------------------------------------
typedef _Float16 f16x4_t __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8_t __attribute__((ext_vector_type(8)));
#define RESNMTF_B16_SCALE 8192.0f
// U16: the image holds uniform 16-bit integers; they are widened exactly to f32 and multiplied on the f32 MFMA
// (v_mfma_f32_16x16x4_f32, B = the K-packed f32 copy as it is): MFMA (jj, u) has A = x[jj][u], B = b[u], K = q.
template <int NW, int UNROLL, bool U16>
__device__ __forceinline__ void pass_body_half(const _Float16* __restrict__ A, const float* __restrict__ B, int r_begin, int r_end,
                                               float out_scale, float* red, float* __restrict__ out /*[64][16]*/) {
  constexpr int KP = 16;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int p = lane & 15, q = lane >> 4;
  const int len = r_end - r_begin;
  const int nsteps = (len + 16 * NW - 1) / (16 * NW);          // workgroup steps of 16 NW rows
  const int nfull = len / (16 * NW);                           // steps whose rows are valid for every wave
  f32x4 acc[4];
#pragma unroll
  for (int jj = 0; jj < 4; ++jj) acc[jj] = (f32x4){0.f, 0.f, 0.f, 0.f};
  // row group of this lane at step 0: (r_begin + 16 wave) / 4 + q; a step advances 4 NW groups
  const size_t g0 = (size_t)(r_begin + 16 * wave) / 4 + q;
  const _Float16* a_ptr = A + (g0 * 64 + 4 * p) * 4;
  const float* b_ptr = B + (g0 * 16 + p) * 4;
  const size_t a_step = (size_t)4 * NW * 64 * 4, b_step = (size_t)4 * NW * 16 * 4;
  auto mma = [&](const f16x8_t (&a0)[UNROLL], const f16x8_t (&a1)[UNROLL], const f32x4 (&bv)[UNROLL]) {
    if (U16) {
      typedef unsigned int u32x4_t __attribute__((ext_vector_type(4)));
#pragma unroll
      for (int u = 0; u < UNROLL; ++u) {
        const u32x4_t w0 = __builtin_bit_cast(u32x4_t, a0[u]), w1 = __builtin_bit_cast(u32x4_t, a1[u]);
        // dword d of (w0 | w1) = column block jj = d / 2 of this lane, rows u = 2 (d % 2) (low half) and 2 (d % 2) + 1 (high half)
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
          const unsigned int lo2 = jj < 2 ? w0[2 * jj] : w1[2 * (jj - 2)], hi2 = jj < 2 ? w0[2 * jj + 1] : w1[2 * (jj - 2) + 1];
          const float x0 = (float)(lo2 & 0xFFFFu), x1 = (float)(lo2 >> 16), x2 = (float)(hi2 & 0xFFFFu), x3 = (float)(hi2 >> 16);
          acc[jj] = __builtin_amdgcn_mfma_f32_16x16x4f32(x0, bv[u][0], acc[jj], 0, 0, 0);
          acc[jj] = __builtin_amdgcn_mfma_f32_16x16x4f32(x1, bv[u][1], acc[jj], 0, 0, 0);
          acc[jj] = __builtin_amdgcn_mfma_f32_16x16x4f32(x2, bv[u][2], acc[jj], 0, 0, 0);
          acc[jj] = __builtin_amdgcn_mfma_f32_16x16x4f32(x3, bv[u][3], acc[jj], 0, 0, 0);
        }
      }
      return;
    }
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      f16x4_t bh, bl;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const float v = bv[u][t] * RESNMTF_B16_SCALE;
        const _Float16 h = (_Float16)fminf(v, 65504.0f);
        bh[t] = h;
        bl[t] = (_Float16)(v - (float)h);
      }
      const f16x4_t aj[4] = {{a0[u][0], a0[u][1], a0[u][2], a0[u][3]}, {a0[u][4], a0[u][5], a0[u][6], a0[u][7]},
                             {a1[u][0], a1[u][1], a1[u][2], a1[u][3]}, {a1[u][4], a1[u][5], a1[u][6], a1[u][7]}};
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) {
        acc[jj] = __builtin_amdgcn_mfma_f32_16x16x16f16(aj[jj], bl, acc[jj], 0, 0, 0);
        acc[jj] = __builtin_amdgcn_mfma_f32_16x16x16f16(aj[jj], bh, acc[jj], 0, 0, 0);
      }
    }
  };
  int i = 0;
  for (; i + UNROLL <= nfull; i += UNROLL) {                    // full trips: no predicate
    f16x8_t a0[UNROLL], a1[UNROLL];
    f32x4 bv[UNROLL];
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      const _Float16* ap = a_ptr + (size_t)(i + u) * a_step;
      a0[u] = *reinterpret_cast<const f16x8_t*>(ap);
      a1[u] = *reinterpret_cast<const f16x8_t*>(ap + 8);
      bv[u] = *reinterpret_cast<const f32x4*>(b_ptr + (size_t)(i + u) * b_step);
    }
    mma(a0, a1, bv);
  }
  for (; i < nsteps; i += UNROLL) {                              // ragged trips: clamped addresses, zeroed operands
    f16x8_t a0[UNROLL], a1[UNROLL];
    f32x4 bv[UNROLL];
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      const bool in = 16 * (NW * (i + u) + wave) < len;          // this wave's 16 rows of the step lie inside the split
      const _Float16* ap = in ? a_ptr + (size_t)(i + u) * a_step : A + ((size_t)(r_begin / 4 + q) * 64 + 4 * p) * 4;
      const float* bp = in ? b_ptr + (size_t)(i + u) * b_step : B + ((size_t)(r_begin / 4 + q) * 16 + p) * 4;
      const f16x8_t x0 = *reinterpret_cast<const f16x8_t*>(ap);
      const f16x8_t x1 = *reinterpret_cast<const f16x8_t*>(ap + 8);
      const f32x4 bb = *reinterpret_cast<const f32x4*>(bp);
      const f16x8_t z = {0, 0, 0, 0, 0, 0, 0, 0};
      a0[u] = in ? x0 : z;
      a1[u] = in ? x1 : z;
      bv[u] = in ? bb : (f32x4){0.f, 0.f, 0.f, 0.f};
    }
    mma(a0, a1, bv);
  }
  // tree sum over the waves and slab store: as pass_body (NT = 1), with the scales taken out
#pragma unroll
  for (int s = NW / 2; s >= 1; s >>= 1) {
    if (wave >= s && wave < 2 * s) {
      float* slot = red + (size_t)(wave - s) * 64 * KP;
#pragma unroll
      for (int jj = 0; jj < 4; ++jj)
#pragma unroll
        for (int t = 0; t < 4; ++t) slot[(jj * 4 + t) * 64 + lane] = acc[jj][t];
    }
    __syncthreads();
    if (wave < s) {
      const float* slot = red + (size_t)wave * 64 * KP;
#pragma unroll
      for (int jj = 0; jj < 4; ++jj)
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[jj][t] += slot[(jj * 4 + t) * 64 + lane];
    }
    __syncthreads();
  }
  if (wave == 0) {
#pragma unroll
    for (int jj = 0; jj < 4; ++jj)
#pragma unroll
      for (int t = 0; t < 4; ++t) red[(16 * q + 4 * t + jj) * KP + p] = acc[jj][t] * out_scale;
  }
  __syncthreads();
  for (int e = threadIdx.x * 4; e < 64 * KP; e += 256 * NW)
    *reinterpret_cast<f32x4*>(out + e) = *reinterpret_cast<const f32x4*>(&red[e]);
}

// --------------------------------------------------------------------------------------
// The pass launch.  Grid (1-D):  [naux * nsplit_aux aux workgroups][ntiles * nsplit main workgroups].
// Aux workgroups come first in dispatch order and cover few rows each, so they finish early; each
// publishes its slab (plain stores -> every wave drains vmcnt -> barrier -> one lane: agent-scope
// release fence, drained, then a relaxed agent-scope ticket).  The workgroup that draws the last
// ticket acquires (agent scope, one lane, drained, barrier), resets the counter for the next
// launch and runs the k x k job on the complete set of slabs.  Nothing ever waits on a flag, so
// placement and dispatch order cannot deadlock it; the results are consumed by the NEXT kernel.
// --------------------------------------------------------------------------------------
// resident workgroups per CU the pass kernels are compiled for: two 8-wave workgroups (128 VGPRs) at k <= 16, one
// (256 VGPRs: accumulators + two register buffers of A + the B pieces) above; the host's sizing counts on it
constexpr int pass_min_blocks(int NT, int NW) { return (NT <= 1 && NW <= 8) ? 2 : 1; }
template <int NT, int NW, int UNROLL, bool IS_XG, bool MODE_A, int SPLIT = 0>
// (HIP's second launch-bounds figure counts waves per SIMD: workgroups x NW waves over 4 SIMDs)
__global__ __launch_bounds__(64 * NW, (pass_min_blocks(NT, NW) * NW / 4 > 0 ? pass_min_blocks(NT, NW) * NW / 4 : 1)) void pass_kernel(PassArgs a, KKFArgs kf, KKSArgs ks) {
  constexpr int KP = 16 * NT;
  constexpr int SB = IS_XG ? 0 : 8;   // stamp columns (diagnostic build)
  (void)SB;
  if (a.check_done && a.ctl->done) return;
  extern __shared__ __attribute__((aligned(16))) double smem_d[];
  float* red = reinterpret_cast<float*>(smem_d);
  STAMP(SB + 0);
  if (MODE_A) {
    // mode A: the k x k job's inputs (fp64 partials of the preceding update kernel) are complete
    // before this launch starts; it runs in workgroup 0, concurrently with the whole pass
    if (blockIdx.x == 0) {
      if (a.fuse_zero && threadIdx.x < 2) __hip_atomic_store(a.fuse_zero + threadIdx.x, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (a.no_kk) return;
#ifdef RESNMTF_STAMPS
      {   // how long does ONE dependent load take from here?
        const double probe = IS_XG ? ks.part[threadIdx.x] : kf.part[threadIdx.x];
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (probe == 1.2345e300) smem_d[0] = 1.0;
        STAMP(SB + 7);
      }
#endif
      if (IS_XG) { KKSPre<KP, 64 * NW> pre; kk_s_prefetch<KP, 64 * NW>(ks, pre); kk_s_body<KP, 64 * NW, true>(ks, pre, a.Paux, a.nsplit_aux, smem_d); }
      else { KKFPre<KP, 64 * NW> pre; kk_f_prefetch<KP, 64 * NW>(kf, pre); kk_f_body<KP, 64 * NW, true>(kf, pre, a.Paux, a.nsplit_aux, smem_d); }
      STAMP(SB + 4);
      return;
    }
    const int b = blockIdx.x - 1;
    if (SPLIT >= 2 && NW == 8) {
      const int bx = xcd_order(a, b, (int)blockIdx.x);
      const int tg = bx % a.ntg, split = bx / a.ntg;
      const int r_begin = split * a.rows_per_split;
      if (a.tw == 8)
        pass_body_wide<NT, 1>(a.A, a.tile_stride, a.ntiles, tg * 8, a.Bk, r_begin, min(r_begin + a.rows_per_split, a.rows_pad),
                              reinterpret_cast<u32x4_t*>(smem_d), a.P + (size_t)split * a.cols_pad * KP);
      else
        pass_body_wide<NT, 2>(a.A, a.tile_stride, a.ntiles, tg * 4, a.Bk, r_begin, min(r_begin + a.rows_per_split, a.rows_pad),
                              reinterpret_cast<u32x4_t*>(smem_d), a.P + (size_t)split * a.cols_pad * KP);
      STAMP(SB + 1);
      return;
    }
    const int tile = b % a.ntiles, split = b / a.ntiles;
    const int r_begin = split * a.rows_per_split;
      pass_body<NT, NW, UNROLL>(a.A + (size_t)tile * a.tile_stride, a.lda, a.B, a.ldb, r_begin, min(r_begin + a.rows_per_split, a.rows_pad), red,
                                a.P + ((size_t)split * a.cols_pad + (size_t)tile * 64) * KP);
    STAMP(SB + 1);
    return;
  }
  const int naux_blocks = a.naux * a.nsplit_aux;
  if ((int)blockIdx.x >= naux_blocks) {
    const int b = blockIdx.x - naux_blocks;
    if (SPLIT >= 2 && NW == 8) {
      const int bx = xcd_order(a, b, (int)blockIdx.x);
      const int tg = bx % a.ntg, split = bx / a.ntg;
      const int r_begin = split * a.rows_per_split;
      if (a.tw == 8)
        pass_body_wide<NT, 1>(a.A, a.tile_stride, a.ntiles, tg * 8, a.Bk, r_begin, min(r_begin + a.rows_per_split, a.rows_pad),
                              reinterpret_cast<u32x4_t*>(smem_d), a.P + (size_t)split * a.cols_pad * KP);
      else
        pass_body_wide<NT, 2>(a.A, a.tile_stride, a.ntiles, tg * 4, a.Bk, r_begin, min(r_begin + a.rows_per_split, a.rows_pad),
                              reinterpret_cast<u32x4_t*>(smem_d), a.P + (size_t)split * a.cols_pad * KP);
      STAMP(SB + 1);
      return;
    }
    const int tile = b % a.ntiles, split = b / a.ntiles;
    const int r_begin = split * a.rows_per_split;
      pass_body<NT, NW, UNROLL>(a.A + (size_t)tile * a.tile_stride, a.lda, a.B, a.ldb, r_begin, min(r_begin + a.rows_per_split, a.rows_pad), red,
                                a.P + ((size_t)split * a.cols_pad + (size_t)tile * 64) * KP);
    STAMP(SB + 1);
    return;
  }
  const int kind = blockIdx.x / a.nsplit_aux, split = blockIdx.x % a.nsplit_aux;
  const int r_begin = split * a.rows_per_split_aux;
  // the k x k job's slab-independent inputs are requested now (small k only: they stay in registers
  // across the aux pass); whichever aux workgroup turns out to be the last arriver has them at hand
  constexpr bool PREFETCH = (KP * KP <= 2 * 64 * NW);
  KKSPre<KP, 64 * NW> pre_s; KKFPre<KP, 64 * NW> pre_f;
  if (PREFETCH) { if (IS_XG) kk_s_prefetch<KP, 64 * NW>(ks, pre_s); else kk_f_prefetch<KP, 64 * NW>(kf, pre_f); }
  pass_body<NT, NW, UNROLL>(a.aux[kind], 64, a.B, a.ldb, r_begin, min(r_begin + a.rows_per_split_aux, a.rows_pad), red,
                            a.Paux + ((size_t)kind * a.nsplit_aux + split) * 64 * KP);
  STAMP(SB + 1);
  // ---- publish the slab, draw a ticket
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // every storing wave
  __syncthreads();                                     // (also: everyone is done reading `red`)
  volatile int* ticket_slot = reinterpret_cast<volatile int*>(red);
  if (threadIdx.x == 0) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // keep: the compiler may drop the fence's own wait
    *ticket_slot = __hip_atomic_fetch_add(a.aux_cnt, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __syncthreads();
  const int ticket = *ticket_slot;
  STAMP(SB + 2);
  if (ticket != naux_blocks - 1) return;
  // ---- last arriver: every aux slab of this launch is published
  if (threadIdx.x == 0) {
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __hip_atomic_store(a.aux_cnt, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // ready for the next launch
  }
  __syncthreads();
  STAMP(SB + 3);
  if (IS_XG) { if (!PREFETCH) kk_s_prefetch<KP, 64 * NW>(ks, pre_s); kk_s_body<KP, 64 * NW, false>(ks, pre_s, a.Paux, a.nsplit_aux, smem_d); }
  else { if (!PREFETCH) kk_f_prefetch<KP, 64 * NW>(kf, pre_f); kk_f_body<KP, 64 * NW, false>(kf, pre_f, a.Paux, a.nsplit_aux, smem_d); }
  STAMP(SB + 4);
}

// fp16 form of the mode A pass launch (k <= 16): workgroup 0 = the k x k job, the others pass_body_half
template <int UNROLL, bool IS_XG, bool U16>
__global__ __launch_bounds__(512, 4) void pass_half_kernel(PassArgs a, KKFArgs kf, KKSArgs ks) {
  constexpr int KP = 16, NW = 8;
  if (a.check_done && a.ctl->done) return;
  extern __shared__ __attribute__((aligned(16))) double smem_d[];
  float* red = reinterpret_cast<float*>(smem_d);
  if (blockIdx.x == 0) {
    if (a.no_kk) return;
    if (IS_XG) { KKSPre<KP, 64 * NW> pre; kk_s_prefetch<KP, 64 * NW>(ks, pre); kk_s_body<KP, 64 * NW, true>(ks, pre, a.Paux, a.nsplit_aux, smem_d); }
    else { KKFPre<KP, 64 * NW> pre; kk_f_prefetch<KP, 64 * NW>(kf, pre); kk_f_body<KP, 64 * NW, true>(kf, pre, a.Paux, a.nsplit_aux, smem_d); }
    return;
  }
  const int b = blockIdx.x - 1;
  const int tile = b % a.ntiles, split = b / a.ntiles;
  const int r_begin = split * a.rows_per_split;
  pass_body_half<NW, UNROLL, U16>(a.A16 + (size_t)tile * a.tile_stride16, a.B, r_begin, min(r_begin + a.rows_per_split, a.rows_pad),
                             a.out_scale, red, a.P + ((size_t)split * a.cols_pad + (size_t)tile * 64) * KP);
}

// --------------------------------------------------------------------------------------
// Mode A pass launch (k <= 16, f32 images) with the factor update that FEEDS it fused in (R/update_steps.r:146-164 ->
// crossprod(x, f), :185-206 -> x %*% g): workgroup 0 is the k x k job as before, the first n_upd of the others run
// factor_update_body for one row block each (the unrestricted form: the coupled forms do not fit the pass's register
// budget), publish it (stores drained, agent-scope release, relaxed arrival counter) and then join the rest, which went
// straight to the wait: one bounded spin of thread 0 per workgroup on the counter, acquire, barrier.  Everything that
// waits is resident while every updater is (updaters head the grid and wait for nothing), so dispatch order cannot
// deadlock it; a spin that runs out raises fz.err instead of hanging (the host reports it).  Saves the update kernel's
// own launch ramp / drain and the kernel boundary: the pass workgroups are resident and start streaming the moment the
// last row block is published.  The counter of THIS launch is zeroed by the sibling launch of the pair (Xt.F <-> X.G),
// which cannot overlap it in stream order.  Same update code on the same bytes: bitwise the unfused sweep.
// --------------------------------------------------------------------------------------
struct FuseArgs {
  int* cnt_own;                       // arrivals of this launch's update blocks (zeroed by the sibling launch: PassArgs.fuse_zero)
  int n_upd;                          // update blocks = workgroups 1 .. n_upd
  int* err;                           // set to 1 when a wait ran out
  int nap;                            // s_sleep(8) periods (~0.2 us each) between two looks at the flag
};
template <int UNROLL, bool IS_XG, bool PRE>
__global__ __launch_bounds__(512, 4) void pass_fused_kernel(PassArgs a, KKFArgs kf, KKSArgs ks, UpdateArgs u, FuseArgs fz) {
  constexpr int KP = 16, NT = 1, NW = 8;
  constexpr int SB = IS_XG ? 0 : 8;   // stamp columns (diagnostic build)
  (void)SB;
  if (a.check_done && a.ctl->done) return;
  extern __shared__ __attribute__((aligned(16))) double smem_d[];
  float* red = reinterpret_cast<float*>(smem_d);
  STAMP(SB + 0);
  const int b = (int)blockIdx.x - 1;
  KKSPre<KP, 64 * NW> pre_s; KKFPre<KP, 64 * NW> pre_f;
  if (b < 0) {
    if (a.fuse_zero && threadIdx.x < 2) __hip_atomic_store(a.fuse_zero + threadIdx.x, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (!a.no_kk) {        // what the k x k job reads besides the update's partials: in flight while the update runs
      if (IS_XG) kk_s_prefetch<KP, 64 * NW>(ks, pre_s); else kk_f_prefetch<KP, 64 * NW>(kf, pre_f);
    }
  } else if (b < fz.n_upd) {
    factor_update_body<KP, IS_XG, 0, true>(u, b, smem_d);          // the X.G' launch consumes G', the Xt.F launch F'
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");               // every storing wave
    __syncthreads();                                               // (also: the update is done with the LDS)
    STAMP(SB + 5);
    if (threadIdx.x == 0) {
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      // the last block to arrive raises the flag the waiters poll (cnt_own[1]): 480 workgroups polling the very word the
      // updaters increment put those increments behind a queue of reads
      if (__hip_atomic_fetch_add(fz.cnt_own, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == fz.n_upd - 1)
        __hip_atomic_store(fz.cnt_own + 1, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  // PRE: the first trip of X rows (they do not depend on the update) is requested now and lands while the workgroup waits
  f32x4 pre_av[UNROLL];
  const int tile = b < 0 ? 0 : b % a.ntiles, split = b < 0 ? 0 : b / a.ntiles;
  const int r_begin = split * a.rows_per_split, r_end = min(r_begin + a.rows_per_split, a.rows_pad);
  bool pre_ok = false;
  if (PRE && b >= 0) pre_ok = pass_prefetch_a<NW, UNROLL>(a.A + (size_t)tile * a.tile_stride, a.lda, r_begin, r_end, pre_av);
  if (threadIdx.x == 0) {
    int spins = 0;
    while (__hip_atomic_load(fz.cnt_own + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0) {
      for (int z = 0; z < fz.nap; ++z) __builtin_amdgcn_s_sleep(8);
      if (++spins > (1 << 19)) { __hip_atomic_store(fz.err, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); break; }   // (>= 0.1 s)
    }
#ifdef RESNMTF_FUSE_ACQUIRE
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#endif
  }
  // No cache invalidate here (an agent-scope acquire is buffer_inv sc1: it drops the L2 of the whole XCD, and with one per
  // workgroup -- 60 per XCD while X streams through that L2 -- the launch took 31 / 37 us instead of 17 + 5).  It is not
  // needed: this CU's L1 and this XCD's L2 were invalidated when the launch began (every kernel starts with that acquire, or
  // results of earlier kernels on other XCDs could not be read at all), and nothing in this launch reads the updated factor,
  // its f32 copy or the partials before this point -- the waiters touch only X (and the k x k job S-side inputs) until
  // the counter is complete -- so no stale line of them can sit in either cache; the buffers are allocations of their own
  // (no line shared with data that is read earlier).  The writers' side is a full agent-scope release (L2 write-back) before
  // the relaxed increment, the counter itself is read at agent scope.  The barrier below orders every wave's loads behind
  // thread 0's last look at the counter.
  asm volatile("" ::: "memory");
  __syncthreads();
  STAMP(SB + 6);
  if (b < 0) {
    if (a.no_kk) return;
    if (IS_XG) kk_s_body<KP, 64 * NW, true>(ks, pre_s, a.Paux, a.nsplit_aux, smem_d);
    else kk_f_body<KP, 64 * NW, true>(kf, pre_f, a.Paux, a.nsplit_aux, smem_d);
    STAMP(SB + 4);
    return;
  }
  float* out = a.P + ((size_t)split * a.cols_pad + (size_t)tile * 64) * KP;
  if (PRE && pre_ok) pass_body<NT, NW, UNROLL, true>(a.A + (size_t)tile * a.tile_stride, a.lda, a.B, a.ldb, r_begin, r_end, red, out, pre_av);
  else pass_body<NT, NW, UNROLL>(a.A + (size_t)tile * a.tile_stride, a.lda, a.B, a.ldb, r_begin, r_end, red, out);
  STAMP(SB + 1);
}

#ifndef RESNMTF_TEMPLATES_ONLY
// --------------------------------------------------------------------------------------
// Row-sliced chains (view-sharded runs, resnmtf_options.slice_chains): star_prod_relevant is row-local by NAME
// (R/utils.r:67-73: row r of view v reads only the same-named row of view i) and ordered over the views
// (R/update_steps.r:282-303), so a rank can walk the F (G) chain of ALL views for the 1 / V of the shared rows (columns)
// it is assigned -- one view's worth of element-wise work instead of V views' -- given the same rows of every view's
// product U = X G (T = X^T F').  Two small kernels stand at the seams:
//   slice_pack_kernel    the split slabs of the own view's pass, folded exactly as slab_fold_kernel folds them (fp64 sum in
//                        split order, rounded to f32 once), written as V chunks [rows_per_slice][KP] -- chunk c is what the
//                        all-to-all hands to rank c -- each followed by a copy of a small fp64 tail (the own view's k x k
//                        coefficient matrices: what every rank's chain step of this view needs besides the rows);
//                        G form: also the f32 copy of T in the operand layout (A operand of the T^T G' aux tile);
//   slice_unpack_kernel  the own view's new rows, as they arrive from the V slice holders (compact f32, natural column
//                        order), into the operand layouts of the next streaming pass: the f32 copy (columns interleaved,
//                        fperm) and -- k > 16 -- the K-packed bf16 pieces, 16-byte stores staged through LDS exactly as
//                        wide_chain_kernel writes them for a view it owns (same roundings: bitwise the same operands).
// --------------------------------------------------------------------------------------
struct SlicePackArgs {
  const float* P; int nsplit; int rows_pad;       // [nsplit][rows_pad][KP] split slabs of the pass
  int KP, NT;
  int rows_per_slice, n_slices;
  char* out; size_t chunk_bytes;                  // chunk c at out + c * chunk_bytes: [rows_per_slice][KP] f32, then the tail
  char* outv[8];                                  // slice_p2p (out == nullptr): chunk c goes straight to rank c -- its U_recv / T_recv slot
                                                  // for this rank, mapped through hipIpc (peer stores over xGMI)
  const double* tail[2]; int tail_count;          // tail = tail[0][0 .. count) | tail[1][0 .. count)  (count = 0: none)
  double* tailv[8];                               // slice_p2p: the tail of chunk c goes HERE instead of behind the chunk (rank c's slot of
                                                  // this view's S block), or nullptr
  float* T32; int ld32;                           // G form: [rows_pad][ld32] f32 operand copy of the folded rows, or nullptr
  const SweepCtl* ctl; int check_done;
};
static __global__ __launch_bounds__(256) void slice_pack_kernel(SlicePackArgs a) {
  if (a.check_done && a.ctl->done) return;
  const int qpr = a.KP / 4;                                                   // quads per row
  const size_t quads_all = (size_t)a.n_slices * a.rows_per_slice * qpr;
  const size_t slab_quads = (size_t)a.rows_pad * qpr;
  for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < quads_all; idx += (size_t)gridDim.x * 256) {
    const int row = (int)(idx / qpr), q = (int)(idx % qpr);
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    if (row < a.rows_pad) {
      const float4* p = reinterpret_cast<const float4*>(a.P) + idx;
      for (int sp = 0; sp < a.nsplit; sp += 4) {                              // (the loop of slab_fold_kernel)
        float4 t[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) t[u] = (sp + u < a.nsplit) ? p[(size_t)(sp + u) * slab_quads] : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int u = 0; u < 4; ++u) { s0 += (double)t[u].x; s1 += (double)t[u].y; s2 += (double)t[u].z; s3 += (double)t[u].w; }
      }
    }
    const float4 v = make_float4((float)s0, (float)s1, (float)s2, (float)s3);
    const int c = row / a.rows_per_slice, lr = row % a.rows_per_slice;
    reinterpret_cast<float4*>(a.out ? a.out + (size_t)c * a.chunk_bytes : a.outv[c])[(size_t)lr * qpr + q] = v;
    if (a.T32 && row < a.rows_pad) {
      float* t = a.T32 + (size_t)row * a.ld32;
      t[fperm(4 * q, a.NT)] = v.x; t[fperm(4 * q + 1, a.NT)] = v.y; t[fperm(4 * q + 2, a.NT)] = v.z; t[fperm(4 * q + 3, a.NT)] = v.w;
    }
  }
  const size_t tails = (size_t)a.n_slices * 2 * a.tail_count;
  const size_t slice_bytes = (size_t)a.rows_per_slice * a.KP * sizeof(float);
  for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < tails; idx += (size_t)gridDim.x * 256) {
    const int c = (int)(idx / (2 * (size_t)a.tail_count)), j = (int)(idx % (2 * (size_t)a.tail_count));
    double* dst = a.tailv[c] ? a.tailv[c] : reinterpret_cast<double*>((a.out ? a.out + (size_t)c * a.chunk_bytes : a.outv[c]) + slice_bytes);
    dst[j] = a.tail[j / a.tail_count][j % a.tail_count];
  }
}

// slice_p2p: after a producing kernel, in stream order: one arrival per peer on the counter word of this exchange (the
// consumer's stream waits for V arrivals per sweep with hipStreamWaitValue32 -- no device-side spin anywhere).  The producing
// kernel has completed (its peer stores are flushed) before this one starts; the fence orders this kernel's own view of it.
struct SliceSignalArgs { unsigned int* flag[8]; int n; };
static __global__ void slice_signal_kernel(SliceSignalArgs a) {
  if ((int)threadIdx.x < a.n) {
    __threadfence_system();
    (void)__hip_atomic_fetch_add(a.flag[threadIdx.x], 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

// slice_p2p without slice_chains (replicated-chain layouts): up to two byte ranges of this rank's exchange block -> the same
// offsets of every peer's arena (16-byte stores over the IPC mappings; the ranges are multiples of 16 bytes, 256-aligned)
struct BlockPushArgs {
  const char* src;            // own arena
  char* dst[8]; int n_dst;    // the peers' arenas (the own rank left out)
  size_t off[2], bytes[2];
};
static __global__ __launch_bounds__(256) void block_push_kernel(BlockPushArgs a) {
  for (int s = 0; s < 2; ++s) {
    const size_t quads = a.bytes[s] / 16;
    const uint4* src = reinterpret_cast<const uint4*>(a.src + a.off[s]);
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < quads; i += (size_t)gridDim.x * 256) {
      const uint4 q = src[i];
      for (int c = 0; c < a.n_dst; ++c) reinterpret_cast<uint4*>(a.dst[c] + a.off[s])[i] = q;
    }
  }
}

// slice_p2p = 2: the wait of a phase as a one-wave kernel instead of hipStreamWaitValue32 -- a kernel node, so whole sweeps can be
// captured in a graph and replayed.  The number of the wait comes from a device counter of its call site (a replay advances it),
// the spin is bounded (error word in pinned host memory, reported by resnmtf_synchronize) and sleeps between polls; one wave, so
// the producers it waits for -- other devices, or other processes on this one -- are never kept off the machine by it.
struct P2pWaitArgs { const unsigned int* flag; unsigned int* site; unsigned int per_wait, add; int* err; };
static __global__ void p2p_wait_kernel(P2pWaitArgs a) {
  if (threadIdx.x != 0) return;
  const unsigned int n = *a.site;
  *a.site = n + 1;
  const unsigned int target = a.per_wait * (n + a.add);
  for (long long spins = 0; __hip_atomic_load(a.flag, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_SYSTEM) < target; ++spins) {
    if (spins > 30000000ll) { *a.err = 2; break; }      // (tens of seconds)
    __builtin_amdgcn_s_sleep(16);
  }
}

// resnmtf_p2p_selftest: 256 words that name their writer and their position into every peer's probe region
struct P2pProbeArgs { unsigned int* dst[8]; int n_dst; unsigned int tag; };
static __global__ void p2p_probe_kernel(P2pProbeArgs a) {
  for (int c = 0; c < a.n_dst; ++c) a.dst[c][threadIdx.x] = a.tag | threadIdx.x;
}

// ... and the reader: a KERNEL behind the stream wait, as in a sweep (a copy engine would not go through this device's caches).
// Counts the words that differ from what rank c must have stored; the second round of the self-test re-reads lines the first
// round left in this device's L2 -- if the wait + kernel-start acquire does not drop them, the old pattern shows here.
struct P2pCheckArgs { const unsigned int* src[8]; unsigned int tag[8]; int n_src; int* bad; };
static __global__ void p2p_check_kernel(P2pCheckArgs a) {
  int bad = 0;
  for (int c = 0; c < a.n_src; ++c) bad += a.src[c][threadIdx.x] != (a.tag[c] | threadIdx.x);
  if (bad) atomicAdd(a.bad, bad);
}

struct SliceUnpackArgs {
  const float* in;            // [>= round_up(len, 32)][KP] f32, natural column order (the received chunks, back to back)
  int len, k;
  float* W32; int ld32;       // [len_pad][ld32] operand copy, columns interleaved (fperm)
  unsigned short* Wk;         // KP > 16: K-packed bf16 pieces (bk_index)
  const SweepCtl* ctl; int check_done;
};
template <int KP>
__global__ __launch_bounds__(256) void slice_unpack_kernel(SliceUnpackArgs a) {
  constexpr int NTL = KP / 16, PER = 32 * KP / 256;                           // values per thread of a 32-row block
  __shared__ float sNf[32 * KP];
  if (a.check_done && a.ctl->done) return;
  const int r0 = blockIdx.x * 32;
  float x[PER];
#pragma unroll
  for (int u = 0; u < PER; ++u) x[u] = a.in[(size_t)r0 * KP + threadIdx.x + 256 * u];     // (coalesced; masked below)
#pragma unroll
  for (int u = 0; u < PER; ++u) {
    const int e = threadIdx.x + 256 * u, lr = e / KP, i = e % KP;
    const float v = (r0 + lr < a.len && i < a.k) ? x[u] : 0.f;
    sNf[e] = v;
    a.W32[(size_t)(r0 + lr) * a.ld32 + fperm(i, NTL)] = v;
  }
  if (KP > 16 && a.Wk) {
    __syncthreads();
    if (threadIdx.x < NTL * 64) {
      const int nt = threadIdx.x >> 6, fq = (threadIdx.x >> 4) & 3, fp = threadIdx.x & 15;
      u32x4_t ph, pm, pl;
#pragma unroll
      for (int dd = 0; dd < 4; ++dd) {
        const float x0 = sNf[(8 * dd + fq) * KP + 16 * nt + fp], x1 = sNf[(8 * dd + 4 + fq) * KP + 16 * nt + fp];
        ph[dd] = pk_bf16(x0, x1);
        const float q0 = x0 - __uint_as_float(ph[dd] << 16), q1 = x1 - __uint_as_float(ph[dd] & 0xFFFF0000u);
        pm[dd] = pk_bf16(q0, q1);
        pl[dd] = pk_bf16(q0 - __uint_as_float(pm[dd] << 16), q1 - __uint_as_float(pm[dd] & 0xFFFF0000u));
      }
      unsigned short* base = a.Wk + bk_index(r0 + fq, 16 * nt + fp, NTL, 0);
      *reinterpret_cast<u32x4_t*>(base) = ph;
      *reinterpret_cast<u32x4_t*>(base + 512) = pm;
      *reinterpret_cast<u32x4_t*>(base + 1024) = pl;
    }
  }
}

// --------------------------------------------------------------------------------------
// SVD initialisation (SURVEY 8(f1); init_mats_inner, R/update_steps.r:78-125): the reference takes the
// top-k singular triplets of X from a full svd().  Here: randomized subspace iteration whose two big
// products per iteration are the streaming passes above (X.Omega and X^T.Q with L <= 64 columns);
// the tall-skinny helpers below are the rest of the device work, the L x L factorisations (Cholesky,
// Jacobi) run on the host in fp64 (resnmtf_hip.hip, resnmtf_init_svd).
// --------------------------------------------------------------------------------------
// Y[r][c] = (double) A32(r, c)   (thin views: the tile-major f32 image widened for the fp64 Gram)
static __global__ __launch_bounds__(256) void widen_rows_kernel(const float* __restrict__ A32, size_t ts, int len, int cols,
                                                         double* __restrict__ Y) {
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (size_t)len * cols) return;
  const int r = (int)(idx / cols), c = (int)(idx % cols);
  Y[idx] = (double)A32[xidx(r, c, ts)];
}
// Y[r][j] = sum over splits of the pass slabs P[s][r][j]   (f32 -> fp64)
static __global__ __launch_bounds__(256) void slab_sum_kernel(const float* __restrict__ P, int nsplit, int rows_pad, int L,
                                                       int len, double* __restrict__ Y) {
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (size_t)len * L) return;
  const int r = (int)(idx / L), j = (int)(idx % L);
  Y[idx] = sum_strided(P + (size_t)r * L + j, (size_t)rows_pad * L, nsplit);
}
// out = the nsplit f32 slabs of a pass summed in split order (fp64 accumulation, as the update kernels
// sum them), rounded to f32 once: the compact form of the X.G result that travels between ranks
static __global__ __launch_bounds__(256) void slab_fold_kernel(const float* __restrict__ P, int nsplit, int quads,
                                                        float* __restrict__ out) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= quads) return;
  const float4* p = reinterpret_cast<const float4*>(P) + idx;
  double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
  for (int sp = 0; sp < nsplit; sp += 4) {
    float4 t[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) t[q] = (sp + q < nsplit) ? p[(size_t)(sp + q) * quads] : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int q = 0; q < 4; ++q) { s0 += (double)t[q].x; s1 += (double)t[q].y; s2 += (double)t[q].z; s3 += (double)t[q].w; }
  }
  reinterpret_cast<float4*>(out)[idx] = make_float4((float)s0, (float)s1, (float)s2, (float)s3);
}
// part[b][i L + j] = sum over the rows of block b of Y[r][i] Y[r][j]   (fp64)
static __global__ __launch_bounds__(256) void ts_gram_kernel(const double* __restrict__ Y, int len, int L, int rows_per_block,
                                                      double* __restrict__ part) {
  __shared__ double tile[16 * 64];
  const int r0 = blockIdx.x * rows_per_block, r1 = min(r0 + rows_per_block, len);
  double acc[16];
#pragma unroll
  for (int ii = 0; ii < 16; ++ii) acc[ii] = 0.0;
  for (int g0 = r0; g0 < r1; g0 += 16) {
    for (int e = threadIdx.x; e < 16 * L; e += 256) {
      const int r = g0 + e / L;
      tile[e] = r < r1 ? Y[(size_t)r * L + e % L] : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int ii = 0; ii < 16; ++ii) {
      const int e = threadIdx.x + 256 * ii;
      if (e < L * L) {
        const int i = e / L, j = e % L;
        double s = 0.0;
#pragma unroll
        for (int t = 0; t < 16; ++t) s += tile[t * L + i] * tile[t * L + j];
        acc[ii] += s;
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int ii = 0; ii < 16; ++ii) {
    const int e = threadIdx.x + 256 * ii;
    if (e < L * L) part[(size_t)blockIdx.x * L * L + e] = acc[ii];
  }
}
// out[e] = sum_b part[b][e]   (block order)
static __global__ __launch_bounds__(256) void reduce_records_kernel(const double* __restrict__ part, int nblk, int count,
                                                             double* __restrict__ out) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e < count) out[e] = sum_strided(part + e, (size_t)count, nblk);
}
// Q = Y M  (M row-major L x L fp64); optionally also the f32 operand copy of Q (pitch ld, interleaved)
static __global__ __launch_bounds__(256) void ts_apply_kernel(const double* __restrict__ Y, int len, int L,
                                                       const double* __restrict__ M, double* __restrict__ Q,
                                                       float* __restrict__ W32, int ld, int nt) {
  __shared__ double Ms[64 * 64];
  for (int e = threadIdx.x; e < L * L; e += 256) Ms[e] = M[e];
  __syncthreads();
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (size_t)len * L) return;
  const int r = (int)(idx / L), j = (int)(idx % L);
  double s = 0.0;
  for (int i = 0; i < L; ++i) s += Y[(size_t)r * L + i] * Ms[i * L + j];
  Q[idx] = s;
  if (W32) W32[(size_t)r * ld + fperm(j, nt)] = (float)s;
}

// --------------------------------------------------------------------------------------
// Finalise: normalisation_check (R/utils.r:176-195) + binary clusters (R/obtain_bicl.r:162-180)
// outputs are written COLUMN-MAJOR fp64 (R layout) into staging buffers.
// --------------------------------------------------------------------------------------
static __global__ __launch_bounds__(256) void colsum_kernel(const double* __restrict__ W, int len, int k,
                                                     double* __restrict__ out) {
  __shared__ double red[256];
  const int j = blockIdx.x;
  double s = 0.0;
  for (int r = threadIdx.x; r < len; r += 256) s += W[(size_t)r * k + j];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int st = 128; st > 0; st >>= 1) {
    if ((int)threadIdx.x < st) red[threadIdx.x] += red[threadIdx.x + st];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[j] = red[0];
}

// S_out[i][j] = S[i][j] * cF[j] * cG[j]  (utils.r:178-181); relations[j] = which.max(S_out[, j])
static __global__ void finalise_s_kernel(const double* __restrict__ S, int k, const double* __restrict__ cF,
                                  const double* __restrict__ cG, double* __restrict__ S_out_colmajor,
                                  int* __restrict__ relations) {
  const int j = threadIdx.x;
  if (j >= k) return;
  const double sc = cF[j] * cG[j];
  int best = 0; double bv = 0.0;
  for (int i = 0; i < k; ++i) {
    const double v = S[i * k + j] * sc;
    S_out_colmajor[(size_t)j * k + i] = v;
    if (i == 0 || v > bv) { bv = v; best = i; }     // first maximum, like which.max
  }
  relations[j] = best;
}

// W_out[, j] = W[, j] / c[j] (utils.r:182-189); clusters[, j] = (W_out[, src_j] > 1/len), src_j =
// relations[j] for row clusters (obtain_bicl.r:180) and j for column clusters.
static __global__ __launch_bounds__(256) void finalise_factor_kernel(const double* __restrict__ W, int len, int k,
                                                              const double* __restrict__ c,
                                                              const int* __restrict__ relations,
                                                              double* __restrict__ W_out, double* __restrict__ cl_out) {
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (size_t)len * k) return;
  const int j = (int)(idx / len), r = (int)(idx % len);    // column-major output index
  W_out[idx] = W[(size_t)r * k + j] / c[j];
  const int src = relations ? relations[j] : j;
  const double v = W[(size_t)r * k + src] / c[src];
  cl_out[idx] = (v > (1.0 / (double)len)) ? 1.0 : 0.0;
}

// --------------------------------------------------------------------------------------
// Relevance of a sub-sample biclustering against the original one: relevance_results (R/stability_analysis.r:45-67)
// with jaccard_main (:16-33), cart_prod and jaccard_func (R/utils.r:117-145).  Bicluster i is the pair set R_i x C_i, so
// |pairs_i ^ pairs_j| = |R_i ^ TR_j| |C_i ^ TC_j| and |pairs_i| = |R_i| |C_i|: the Jaccard index is a function of integer
// counts per side.  relevance_count_kernel counts ONE side (rows or columns) per launch: a wave takes 64 lines at a time,
// forms the membership masks of the sub-sample's clusters (the comparison of finalise_factor_kernel, bit for bit: same
// W / c[src] > 1/len) and of the reference's clusters gathered through idx with __ballot, and adds popcounts of the
// ANDed masks into LDS counters, then into `counts` -- integer atomics only, so the counts do not depend on the order
// in which workgroups or waves run.
// counts (per side, unsigned): [k * k: |A_i ^ B_j| at i * k + j] [k: |A_i|] [k: |B_j|]   (A = sub-sample, B = reference)
// ref: the reference's clusters of this side as 0 / 1 bytes, [len_ref][k] row-major; idx: len indices into its rows
// (validated on the host).
// MASKED (resnmtf_relevance_masked): the sub-sample's cluster i counts as empty when flags[drop_rel[i]] is set -- flags
// are indexed by F column and drop_rel is finalise_s_kernel's relations, for the row and the column launch alike (the
// column zeroing of the spurious-bicluster removal, R/obtain_bicl.r:176-188).
// --------------------------------------------------------------------------------------
template <bool MASKED>
static __global__ __launch_bounds__(256) void relevance_count_kernel(const double* __restrict__ W, int len, int k,
                                                                     const double* __restrict__ c,
                                                                     const int* __restrict__ relations,
                                                                     const unsigned char* __restrict__ ref,
                                                                     const int* __restrict__ idx,
                                                                     unsigned int* __restrict__ counts,
                                                                     const int* __restrict__ drop_rel,
                                                                     const unsigned char* __restrict__ flags) {
  __shared__ unsigned int cnt[RESNMTF_MAX_K * RESNMTF_MAX_K + 2 * RESNMTF_MAX_K];
  const int total = k * k + 2 * k;
  for (int t = threadIdx.x; t < total; t += 256) cnt[t] = 0u;
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int chunks = (len + 63) / 64;
  const double thr = 1.0 / (double)len;
  for (int ch = blockIdx.x * 4 + wave; ch < chunks; ch += gridDim.x * 4) {
    const int r = ch * 64 + lane;
    const bool valid = r < len;
    const int rr = valid ? r : len - 1;      // lanes past the end address the last line and vote 0
    const unsigned char* refrow = ref + (size_t)idx[rr] * k;
    unsigned long long mine = 0ull;          // lane j < k: the reference's cluster j over these 64 lines
    for (int j = 0; j < k; ++j) {
      const unsigned long long b = __ballot(valid && refrow[j] != 0);
      if (lane == j) mine = b;
    }
    if (lane < k && mine) atomicAdd(&cnt[k * k + k + lane], (unsigned int)__popcll(mine));
    for (int i = 0; i < k; ++i) {
      if constexpr (MASKED) {
        if (flags[drop_rel[i]]) continue;                            // a removed cluster: no member (wave-uniform)
      }
      const int src = relations ? relations[i] : i;
      const unsigned long long a = __ballot(valid && (W[(size_t)rr * k + src] / c[src] > thr));
      if (a == 0ull) continue;                                       // (wave-uniform)
      if (lane == 0) atomicAdd(&cnt[k * k + i], (unsigned int)__popcll(a));
      if (lane < k) {
        const unsigned int p = (unsigned int)__popcll(a & mine);
        if (p) atomicAdd(&cnt[i * k + lane], p);
      }
    }
  }
  __syncthreads();
  for (int t = threadIdx.x; t < total; t += 256)
    if (cnt[t]) atomicAdd(&counts[t], cnt[t]);
}

// relevance[j] = max_i J(i, j) (apply(jac_mat, 2, max)), J = I / U, I = rI * cI, U = |R_i| |C_i| + |TR_j| |TC_j| - I,
// 0 when U == 0 -- after the edge cases of relevance_results, decided on the ROW clusters alone (m_0 / n_0 = non-empty
// columns of row_c / true_r): exactly one of them 0 -> 0, both 0 -> 1, broadcast over j.  Integer products (exact in
// int64 and, below 2^53, in fp64) and one correctly rounded division per pair: bitwise the fp64 host restatement.
static __global__ void relevance_epilogue_kernel(int k, const unsigned int* __restrict__ rows_cnt,
                                                 const unsigned int* __restrict__ cols_cnt, double* __restrict__ out) {
  const int j = threadIdx.x;
  if (j >= k) return;
  const unsigned int *rI = rows_cnt, *rA = rows_cnt + k * k, *rB = rA + k;
  const unsigned int *cI = cols_cnt, *cA = cols_cnt + k * k, *cB = cA + k;
  int m0 = 0, n0 = 0;
  for (int t = 0; t < k; ++t) { m0 += rA[t] != 0u; n0 += rB[t] != 0u; }
  if ((m0 == 0) != (n0 == 0)) { out[j] = 0.0; return; }     // R/stability_analysis.r:57-59
  if (m0 == 0) { out[j] = 1.0; return; }                     // :62-64
  double best = 0.0;
  for (int i = 0; i < k; ++i) {
    const long long inter = (long long)rI[i * k + j] * (long long)cI[i * k + j];
    const long long uni = (long long)rA[i] * (long long)cA[i] + (long long)rB[j] * (long long)cB[j] - inter;
    const double jac = uni == 0 ? 0.0 : (double)inter / (double)uni;      // jaccard_func, R/utils.r:117-126
    if (i == 0 || jac > best) best = jac;
  }
  out[j] = best;
}
#endif      // RESNMTF_TEMPLATES_ONLY
