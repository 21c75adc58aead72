// Device-wide fp64 factorisation (resnmtf_fp64_run, DESIGN.md section 21): the arithmetic of resnmtf_group.hip.inc --
// res_nmtf_inner (R/main.r:32-140) in fp64, line by line -- spread over the whole device.  One sweep of one view is a
// short sequence of ordinary launches on one stream; kernel boundaries are the only synchronisation (no atomics, no
// flags, no spins: nothing here can wait on another workgroup).
//
// Per view: X (column-major, leading dimension ldx = f64_ld(n), columns rounded up to 64, zero-filled) and its
// transpose in the same form; F (n x k) and G (m x k) column-major, updated in place; S, lambda, mu and the k x k
// temporaries in a small work area; X^T F (m x k, read again by update_s) and F S (n x k, for the error) in two scratch
// matrices of max(n, m) k doubles; the product slabs [split][rows][KP] and the per-workgroup partials of every sum.
//
// Determinism: every sum runs in an order fixed by (n, m, k): per thread in sequence, fixed trees in LDS, slabs and
// partials summed in split / workgroup order by their consumer.  Two runs of one job give the same bits.

typedef double f64x4 __attribute__((ext_vector_type(4)));

#include "resnmtf_fp64_job.h"   // the shape constants (F64_THREADS, F64_ROWS, ...) and the shape-only plans: host code, no HIP

#define F64_GRAM_STAGE 32
#define F64_RES_LD 80         // LDS stride of a column of the residual's F S tile (80 = 16 mod 32 doubles: the four
                              // k-slices of an MFMA operand read fall on disjoint halves of the banks)
#define F64_MAX_VIEWS 8

// sum of one value per thread by a fixed tree; thread 0 gets the total
__device__ inline double f64_block_sum(double x, double* red) {
  const int t = threadIdx.x;
  red[t] = x;
  __syncthreads();
  for (int s = F64_THREADS / 2; s > 0; s >>= 1) {
    if (t < s) red[t] += red[t + s];
    __syncthreads();
  }
  const double r = red[0];
  __syncthreads();
  return r;
}

// ---- tall-skinny product: slab[split][i][c] = sum over the split's j of X[i, j] O[j, c] ----
// X column-major with leading dimension ldx (a multiple of 32) and whole F64_JC-column stages, zero-filled; O (contr x k)
// column-major.  Wave w of workgroup b owns rows 128 b + 32 w .. + 31 as two MFMA tiles: lane (p, q) loads the row pair
// (2 p, 2 p + 1) of column j + q in one 16-byte load, tile 0 takes the even rows and tile 1 the odd ones
// (v_mfma_f64_16x16x4_f64: lane (p, q) supplies A[p][q] and B[q][p], register t of the result is C[4 t + q][p]).
template <int KP>
__global__ __launch_bounds__(F64_THREADS) void fp64_product_kernel(const double* __restrict__ X, size_t ldx,
                                                                   const double* __restrict__ O, int contr, int k, int chunk,
                                                                   int contr_pad, double* __restrict__ slab) {
  constexpr int KPL = KP + 1, NTC = KP / 16;
  __shared__ double Ol[F64_JC * KPL];
  const int wv = threadIdx.x >> 6, ln = threadIdx.x & 63, p = ln & 15, q = ln >> 4;
  const size_t i0 = (size_t)blockIdx.x * F64_ROWS + (size_t)wv * 32;
  const bool live = i0 < ldx;
  const int jb = blockIdx.y * chunk, je = min(jb + chunk, contr_pad);
  f64x4 acc[2][NTC];
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int tc = 0; tc < NTC; ++tc) acc[h][tc] = f64x4{0.0, 0.0, 0.0, 0.0};
  for (int j0 = jb; j0 < je; j0 += F64_JC) {
    __syncthreads();
    for (int e = threadIdx.x; e < F64_JC * KP; e += F64_THREADS) {
      const int jj = e % F64_JC, c = e / F64_JC, j = j0 + jj;
      Ol[jj * KPL + c] = (j < contr && c < k) ? O[(size_t)j + (size_t)c * contr] : 0.0;
    }
    __syncthreads();
    if (live) {
      const double* xp = X + i0 + 2 * p + (size_t)(j0 + q) * ldx;
#pragma unroll
      for (int s = 0; s < F64_JC / 4; ++s) {
        const double2 x = *reinterpret_cast<const double2*>(xp + (size_t)(4 * s) * ldx);
#pragma unroll
        for (int tc = 0; tc < NTC; ++tc) {
          const double b = Ol[(4 * s + q) * KPL + 16 * tc + p];
          acc[0][tc] = __builtin_amdgcn_mfma_f64_16x16x4f64(x.x, b, acc[0][tc], 0, 0, 0);
          acc[1][tc] = __builtin_amdgcn_mfma_f64_16x16x4f64(x.y, b, acc[1][tc], 0, 0, 0);
        }
      }
    }
  }
  if (live) {
    double* out = slab + ((size_t)blockIdx.y * ldx + i0) * KP;
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int tc = 0; tc < NTC; ++tc)
#pragma unroll
        for (int t = 0; t < 4; ++t) out[(size_t)(2 * (4 * t + q) + h) * KP + 16 * tc + p] = acc[h][tc][t];
  }
}

// ---- Gram partials: part[b][a + c ka] = sum over the rows of workgroup b of A[i, a] B[i, c] ----
// blockIdx.y picks one of up to two (A, B) pairs of one length.  Rows go through LDS in stages of 32; thread t owns the
// outputs t, t + 256, ... and sums its rows in order.
struct F64GramArgs {
  const double* A[2];
  const double* B[2];
  double* part[2];
  int len, k;
};
__global__ __launch_bounds__(F64_THREADS) void fp64_gram_kernel(F64GramArgs a) {
  constexpr int LD = 65, NQ = 16;
  __shared__ double Al[F64_GRAM_STAGE * LD], Bl[F64_GRAM_STAGE * LD];
  const int y = blockIdx.y, k = a.k, Q = k * k, t = threadIdx.x;
  const double* A = a.A[y];
  const double* B = a.B[y];
  const size_t r_begin = (size_t)blockIdx.x * F64_GRAM_ROWS;
  const size_t r_end = min(r_begin + (size_t)F64_GRAM_ROWS, (size_t)a.len);
  double acc[NQ];
  int ia[NQ], ib[NQ];
#pragma unroll
  for (int u = 0; u < NQ; ++u) {
    const int qq = min(t + F64_THREADS * u, Q - 1);
    acc[u] = 0.0; ia[u] = qq % k; ib[u] = qq / k;
  }
  for (size_t r0 = r_begin; r0 < r_end; r0 += F64_GRAM_STAGE) {
    __syncthreads();
    for (int e = t; e < F64_GRAM_STAGE * k; e += F64_THREADS) {
      const int r = e % F64_GRAM_STAGE, c = e / F64_GRAM_STAGE;
      const size_t i = r0 + r;
      Al[r * LD + c] = i < r_end ? A[i + (size_t)c * a.len] : 0.0;
      Bl[r * LD + c] = i < r_end ? B[i + (size_t)c * a.len] : 0.0;
    }
    __syncthreads();
    for (int r = 0; r < F64_GRAM_STAGE; ++r) {
#pragma unroll
      for (int u = 0; u < NQ; ++u)
        if (F64_THREADS * u < Q) acc[u] = fma(Al[r * LD + ia[u]], Bl[r * LD + ib[u]], acc[u]);
    }
  }
  double* out = a.part[y] + (size_t)blockIdx.x * Q;
#pragma unroll
  for (int u = 0; u < NQ; ++u)
    if (t + F64_THREADS * u < Q) out[t + F64_THREADS * u] = acc[u];
}

// ---- row-local update: update_f (R/update_steps.r:141-165) or update_g (:180-207) of one view, in place ----
// One thread per row.  For the G form the roles swap as in grp_update_side: rows = columns of X, "F" = G, S^T for S, mu
// for lambda, psi for phi, column maps for row maps.  The product comes from the slab, summed in split order, and is
// kept in xo (the G form's X^T F is read again by update_s).  Each workgroup leaves the column sums of its new rows.
struct F64UpdArgs {
  int n, k, KP, V, nsplit, unrestricted;
  size_t ldx;                             // rows of one slab split
  const double* slab;
  double* P;                              // the factor updated (n x k)
  double* xo;                             // n x k
  double* ps;                             // n x k
  const double* S;                        // k x k of this view
  const double* W;                        // F form: (G^T G) S^T; G form: (F^T F) S
  const double* lm;                       // lambda / mu of this view
  double rsum;                            // sum(phi[, v]) / sum(psi[, v])
  double r[F64_MAX_VIEWS];                // phi[w, v] / psi[w, v]
  const int* map[F64_MAX_VIEWS];          // row of view w for every row of v, or -1; nullptr = NA
  const double* Pw[F64_MAX_VIEWS];
  int nw[F64_MAX_VIEWS];
  double* colpart;                        // [workgroup][k]
};
template <bool G_FORM>
__global__ __launch_bounds__(F64_UPD_ROWS) void fp64_update_kernel(F64UpdArgs a) {
  const int k = a.k, n = a.n;
  const size_t i = (size_t)blockIdx.x * F64_UPD_ROWS + threadIdx.x;
  const size_t sn = (size_t)n;
  if (i < sn) {
    for (int c = 0; c < k; ++c) {
      double acc = 0.0;
      for (int s = 0; s < a.nsplit; ++s) acc += a.slab[((size_t)s * a.ldx + i) * a.KP + c];
      a.xo[i + (size_t)c * sn] = acc;
    }
    for (int c = 0; c < k; ++c) {                 // P S (F form) or G S^T (G form), row i
      double acc = 0.0;
      for (int e = 0; e < k; ++e) acc = fma(a.P[i + (size_t)e * sn], G_FORM ? a.S[c + e * k] : a.S[e + c * k], acc);
      a.ps[i + (size_t)c * sn] = acc;
    }
    for (int c = 0; c < k; ++c) {
      double num = 0.0, den = 0.0;                // numerator: F form (X G) S^T, G form (X^T F) S
      for (int e = 0; e < k; ++e) num = fma(a.xo[i + (size_t)e * sn], G_FORM ? a.S[e + c * k] : a.S[c + e * k], num);
      for (int e = 0; e < k; ++e) den = fma(a.ps[i + (size_t)e * sn], a.W[e + c * k], den);
      const double p = a.P[i + (size_t)c * sn];
      const double half = 0.5 * a.lm[c];
      double out;
      if (a.unrestricted) {                       // :152 / :190
        double mat = num / (den + half);
        if (isnan(mat)) mat = 1.0;
        out = p * mat;
      } else {                                    // star_prod_relevant (R/utils.r:63-78)
        double acc = 0.0;
        for (int w = 0; w < a.V; ++w) {
          const double r = a.r[w];
          if (r == 0.0 || a.map[w] == nullptr) continue;
          const int row = a.map[w][i];
          const double val = row >= 0 ? a.Pw[w][(size_t)row + (size_t)c * a.nw[w]] : p;
          acc = acc + r * val * (double)a.nw[w];
        }
        const double np = acc / (double)n;
        out = p * ((num + np) / (den + a.rsum * p + half));
      }
      a.P[i + (size_t)c * sn] = fabs(out);
    }
  }
  __syncthreads();                                // (a workgroup's own global writes are visible to it past the barrier)
  if ((int)threadIdx.x < k) {
    const size_t r0 = (size_t)blockIdx.x * F64_UPD_ROWS, r1 = min(r0 + (size_t)F64_UPD_ROWS, sn);
    double acc = 0.0;
    for (size_t r = r0; r < r1; ++r) acc += a.P[r + (size_t)threadIdx.x * sn];
    a.colpart[(size_t)blockIdx.x * k + threadIdx.x] = acc;
  }
}

// F S (n x k) for the error (calculate_error, R/utils.r:157-166: x_hat = (F S) G^T)
__global__ __launch_bounds__(F64_UPD_ROWS) void fp64_fs_kernel(const double* __restrict__ F, const double* __restrict__ S,
                                                               int n, int k, double* __restrict__ fs) {
  const size_t i = (size_t)blockIdx.x * F64_UPD_ROWS + threadIdx.x, sn = (size_t)n;
  if (i >= sn) return;
  for (int c = 0; c < k; ++c) {
    double acc = 0.0;
    for (int e = 0; e < k; ++e) acc = fma(F[i + (size_t)e * sn], S[e + c * k], acc);
    fs[i + (size_t)c * sn] = acc;
  }
}

// ---- residual partials: part[split][tile] = sum over the tile's rows and the split's columns of (X - (F S) G^T)^2 ----
// The workgroup keeps its 64 rows of F S in LDS (column c at stride F64_RES_LD) and forms x_hat^T in 16 x 16 MFMA tiles:
// A = 16 rows of G, B = (F S)^T, so register t of lane (p, q) is x_hat[i(p), j0 + 4 t + q] and the matching X entries of a
// row pair are one 16-byte load.  Padded rows, columns and k-slots are zero on both sides and add nothing.
template <int KP>
__global__ __launch_bounds__(F64_THREADS) void fp64_resid_kernel(const double* __restrict__ X, size_t ldx,
                                                                 const double* __restrict__ FS, int n,
                                                                 const double* __restrict__ G, int m, int k, int chunk,
                                                                 double* __restrict__ part) {
  __shared__ double FSl[KP * F64_RES_LD];
  __shared__ double red[F64_THREADS];
  const int wv = threadIdx.x >> 6, ln = threadIdx.x & 63, p = ln & 15, q = ln >> 4;
  const size_t i0 = (size_t)blockIdx.x * F64_RES_ROWS;
  for (int e = threadIdx.x; e < KP * F64_RES_ROWS; e += F64_THREADS) {
    const int r = e % F64_RES_ROWS, c = e / F64_RES_ROWS;
    FSl[c * F64_RES_LD + r] = (i0 + r < (size_t)n && c < k) ? FS[i0 + r + (size_t)c * n] : 0.0;
  }
  __syncthreads();
  const int m16 = (m + 15) / 16 * 16;
  const int jb = blockIdx.y * chunk, je = min(jb + chunk, m16);
  double acc = 0.0;
  for (int j0 = jb + 16 * wv; j0 < je; j0 += 64) {
    double av[KP / 4];
#pragma unroll
    for (int s = 0; s < KP / 4; ++s)
      av[s] = (j0 + p < m && 4 * s + q < k) ? G[(size_t)(j0 + p) + (size_t)(4 * s + q) * m] : 0.0;
#pragma unroll
    for (int pg = 0; pg < 2; ++pg) {
      if (i0 + 32 * pg >= ldx) continue;          // (rows that were never allocated)
      f64x4 d0 = {0.0, 0.0, 0.0, 0.0}, d1 = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int s = 0; s < KP / 4; ++s) {
        const double b0 = FSl[(4 * s + q) * F64_RES_LD + 32 * pg + 2 * p];
        const double b1 = FSl[(4 * s + q) * F64_RES_LD + 32 * pg + 2 * p + 1];
        d0 = __builtin_amdgcn_mfma_f64_16x16x4f64(av[s], b0, d0, 0, 0, 0);
        d1 = __builtin_amdgcn_mfma_f64_16x16x4f64(av[s], b1, d1, 0, 0, 0);
      }
      const double* xp = X + i0 + 32 * pg + 2 * p + (size_t)(j0 + q) * ldx;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const double2 x = *reinterpret_cast<const double2*>(xp + (size_t)(4 * t) * ldx);
        const double r0 = x.x - d0[t], r1 = x.y - d1[t];
        acc = fma(r0, r0, acc);
        acc = fma(r1, r1, acc);
      }
    }
  }
  const double sq = f64_block_sum(acc, red);
  if (threadIdx.x == 0) part[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = sq;
}

// ||X||_F^2 partials over the padded image (the padding is zero): workgroup b sums entries [b, b + 1) F64_NORM_CHUNK
__global__ __launch_bounds__(F64_THREADS) void fp64_norm_kernel(const double* __restrict__ X, size_t total,
                                                                double* __restrict__ part) {
  __shared__ double red[F64_THREADS];
  const size_t b0 = (size_t)blockIdx.x * F64_NORM_CHUNK, b1 = min(b0 + (size_t)F64_NORM_CHUNK, total);
  double acc = 0.0;
  for (size_t e = b0 + threadIdx.x; e < b1; e += F64_THREADS) acc = fma(X[e], X[e], acc);
  const double sq = f64_block_sum(acc, red);
  if (threadIdx.x == 0) part[blockIdx.x] = sq;
}

// ---- the k x k job: one workgroup reduces the partials of the launch before it, in workgroup order, and does the
// small algebra of the step.  Its temporaries are global (a workgroup sees its own writes past a barrier). ----
enum { F64_KK_SIDE_F = 0, F64_KK_SIDE_G = 1, F64_KK_S = 2, F64_KK_ERR = 3, F64_KK_NORM = 4 };
struct F64KKArgs {
  int mode, k, V, v;
  int nblk_a, nblk_b;                     // workgroups behind part_a / part_b (S: also behind col_f / col_g)
  int nblk_f, nblk_g;
  const double* part_a;                   // SIDE: O^T O; S: (F^T X) G; ERR / NORM: the scalar partials
  const double* part_b;                   // S: G^T G
  const double* col_f;                    // S: column-sum partials of the new F / G
  const double* col_g;
  double *kkA, *kkB, *kkC, *kkD;          // k x k each; kkA carries F^T F from SIDE_G to S
  double* S;                              // every view's S (V k^2)
  double *lam, *mu;                       // this view's lambda / mu
  double *cf, *cg;                        // this view's column sums of F / G (kept for normalisation_check)
  double *norms, *errs;                   // per view
  double* err_out;                        // ERR, last view: where the sweep's mean error goes
  int xi_zero;                            // every entry of xi is zero (:226)
  double xsum;                            // sum(xi[, v])
  double xi[F64_MAX_VIEWS];               // xi[w, v]
};

__device__ inline void f64_kk_reduce(double* out, const double* part, int nblk, int Q) {
  for (int q = threadIdx.x; q < Q; q += F64_THREADS) {
    double acc = 0.0;
    for (int b = 0; b < nblk; ++b) acc += part[(size_t)b * Q + q];
    out[q] = acc;
  }
  __syncthreads();
}
// C = A op(B), k x k column-major
__device__ inline void f64_kk_mul(const double* A, const double* B, bool tB, int k, double* C) {
  for (int q = threadIdx.x; q < k * k; q += F64_THREADS) {
    const int r = q % k, c = q / k;
    double acc = 0.0;
    for (int e = 0; e < k; ++e) acc = fma(A[r + e * k], tB ? B[c + e * k] : B[e + c * k], acc);
    C[q] = acc;
  }
  __syncthreads();
}
// numpy's sum of a short vector (pairwise_sum: sequential below 8 entries, the 8-accumulator form at 8)
__device__ inline double f64_vec_sum(const double* a, int n) {
  if (n < 8) {
    double r = 0.0;
    for (int i = 0; i < n; ++i) r += a[i];
    return r;
  }
  return ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]));
}

__global__ __launch_bounds__(F64_THREADS) void fp64_kk_kernel(F64KKArgs a) {
  __shared__ double red[F64_THREADS];
  const int k = a.k, Q = k * k, t = threadIdx.x;
  double* S = a.S + (size_t)a.v * Q;
  if (a.mode == F64_KK_SIDE_F || a.mode == F64_KK_SIDE_G) {
    // F form: W = (G^T G) S^T -> den = (F S) W;   G form: W = (F^T F) S -> den = (G S^T) W
    f64_kk_reduce(a.kkA, a.part_a, a.nblk_a, Q);
    f64_kk_mul(a.kkA, S, a.mode == F64_KK_SIDE_F, k, a.kkB);
  } else if (a.mode == F64_KK_S) {                // update_s (R/update_steps.r:220-240), then update_lm (:249-251, :312-313)
    f64_kk_reduce(a.kkC, a.part_a, a.nblk_a, Q);  // (F^T X) G
    f64_kk_reduce(a.kkD, a.part_b, a.nblk_b, Q);  // G^T G
    f64_kk_reduce(a.cf, a.col_f, a.nblk_f, k);
    f64_kk_reduce(a.cg, a.col_g, a.nblk_g, k);
    f64_kk_mul(a.kkA, S, false, k, a.kkB);        // (F^T F) S
    f64_kk_mul(a.kkB, a.kkD, false, k, a.kkA);    // ((F^T F) S) (G^T G)
    for (int q = t; q < Q; q += F64_THREADS) {
      const double s = S[q];
      double out;
      if (a.xi_zero) {
        double mat = a.kkC[q] / a.kkA[q];
        if (isnan(mat)) mat = 1.0;
        out = s * mat;
      } else {                                    // star_prod (R/utils.r:39-47)
        double acc = 0.0;
        for (int w = 0; w < a.V; ++w)
          if (a.xi[w] != 0.0) acc = acc + a.xi[w] * a.S[(size_t)w * Q + q];
        out = s * ((a.kkC[q] + acc) / (a.kkA[q] + a.xsum * s));
      }
      S[q] = fabs(out);                           // (every S_w read above belongs to another view: xi's diagonal is zero)
    }
    for (int c = t; c < k; c += F64_THREADS) {
      a.lam[c] = a.cf[c] * a.lam[c];
      a.mu[c] = a.cg[c] * a.mu[c];
    }
  } else {                                        // ERR / NORM: a sum of squares as norm()^2
    double acc = 0.0;
    for (int b = t; b < a.nblk_a; b += F64_THREADS) acc += a.part_a[b];
    const double sq = f64_block_sum(acc, red);
    if (t == 0) {
      const double nrm = sqrt(sq);
      if (a.mode == F64_KK_NORM) {
        a.norms[a.v] = nrm * nrm;                 // R/main.r:48
      } else {
        a.errs[a.v] = (nrm * nrm) / a.norms[a.v];
        if (a.v == a.V - 1) *a.err_out = f64_vec_sum(a.errs, a.V) / (double)a.V;   // (errs of the earlier views: earlier launches)
      }
    }
  }
}

// normalisation_check (R/utils.r:176-195) of one view: S columns by cF * cG, then F / cF, G / cG
__global__ __launch_bounds__(F64_THREADS) void fp64_normalise_kernel(double* F, double* G, double* S, const double* cf,
                                                                     const double* cg, int n, int m, int k) {
  const size_t nf = (size_t)n * k, ng = (size_t)m * k, ns = (size_t)k * k, total = nf + ng + ns;
  for (size_t e = (size_t)blockIdx.x * F64_THREADS + threadIdx.x; e < total; e += (size_t)gridDim.x * F64_THREADS) {
    if (e < nf) F[e] = F[e] / cf[e / (size_t)n];
    else if (e < nf + ng) G[e - nf] = G[e - nf] / cg[(e - nf) / (size_t)m];
    else { const size_t q = e - nf - ng; S[q] = S[q] * (cf[q / k] * cg[q / k]); }
  }
}

// ---- launchers of the templated kernels: one instance per padded k (16 / 32 / 48 / 64) ----
template <int KP>
static void fp64_product_kp(hipStream_t st, const F64ProductPlan& p, const double* X, size_t ldx, const double* O, int contr,
                     int k, size_t contr_pad, double* slab) {
  hipLaunchKernelGGL(fp64_product_kernel<KP>, dim3(p.tiles, p.splits), dim3(F64_THREADS), 0, st, X, ldx, O, contr, k,
                     p.chunk, (int)contr_pad, slab);
}
static void fp64_product(hipStream_t st, int KP, const F64ProductPlan& p, const double* X, size_t ldx, const double* O,
                  int contr, int k, size_t contr_pad, double* slab) {
  switch (KP) {
    case 16: fp64_product_kp<16>(st, p, X, ldx, O, contr, k, contr_pad, slab); break;
    case 32: fp64_product_kp<32>(st, p, X, ldx, O, contr, k, contr_pad, slab); break;
    case 48: fp64_product_kp<48>(st, p, X, ldx, O, contr, k, contr_pad, slab); break;
    default: fp64_product_kp<64>(st, p, X, ldx, O, contr, k, contr_pad, slab); break;
  }
}
template <int KP>
static void fp64_resid_kp(hipStream_t st, const F64ProductPlan& p, const double* X, size_t ldx, const double* FS, int n,
                   const double* G, int m, int k, double* part) {
  hipLaunchKernelGGL(fp64_resid_kernel<KP>, dim3(p.tiles, p.splits), dim3(F64_THREADS), 0, st, X, ldx, FS, n, G, m, k,
                     p.chunk, part);
}
static void fp64_resid(hipStream_t st, int KP, const F64ProductPlan& p, const double* X, size_t ldx, const double* FS, int n,
                const double* G, int m, int k, double* part) {
  switch (KP) {
    case 16: fp64_resid_kp<16>(st, p, X, ldx, FS, n, G, m, k, part); break;
    case 32: fp64_resid_kp<32>(st, p, X, ldx, FS, n, G, m, k, part); break;
    case 48: fp64_resid_kp<48>(st, p, X, ldx, FS, n, G, m, k, part); break;
    default: fp64_resid_kp<64>(st, p, X, ldx, FS, n, G, m, k, part); break;
  }
}
