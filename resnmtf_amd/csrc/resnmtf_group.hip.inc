// Grouped small factorisations (resnmtf_group_run, DESIGN.md section 12): one persistent 256-thread workgroup per
// job runs the whole of res_nmtf_inner (R/main.r:32-140) for that job -- every sweep, the error, the stop test and
// normalisation_check -- in fp64, from its initial factors to the end.  Workgroups never wait on each other.
//
// Per job: X_v (column-major n x m) and its transpose (column-major m x n) are read-only inputs; F_v (n x k) and G_v
// (m x k), column-major, live in the job's output region and are updated in place; S_v, lambda_v, mu_v and every k x k
// temporary live in LDS; XtF (m x k, the X^T F of the G update, reused by the S update) and F S (n x k, for the
// error) share one per-job global scratch.
//
// Determinism: every sum runs in an order fixed by the job's own shapes (sequential per thread, then fixed trees in
// LDS); no atomics.  A job's output bits depend only on its own inputs.

#define GRP_THREADS 256
#define GRP_MAX_VIEWS 8
#define GRP_MAX_K 32

struct GroupDesc {
  int V, k, n_iters, cap;                  // n_iters 0 = convergence; cap = number of sweeps allowed (<= max_iters)
  int id, pad;                             // the job's index in the caller's list
  int n[GRP_MAX_VIEWS], m[GRP_MAX_VIEWS];
  long long x[GRP_MAX_VIEWS];              // offsets in doubles from the buffer base: X_v, column-major n x m
  long long xt[GRP_MAX_VIEWS];             // X_v^T, column-major m x n
  long long f[GRP_MAX_VIEWS], g[GRP_MAX_VIEWS];   // live F_v / G_v (initial values on entry, normalised on exit)
  long long s, lam, mu;                    // S (V k^2, view-major, each column-major), lambda (V k), mu (V k)
  long long err, err_stride;               // mean error of sweep t at err + t * err_stride (cap entries)
  long long scratch, scratch2;             // two regions of max_v max(n_v, m_v) * k doubles each
  long long rmap[GRP_MAX_VIEWS][GRP_MAX_VIEWS];   // int offsets: row i of view v -> shared row of view w or -1;
  long long cmap[GRP_MAX_VIEWS][GRP_MAX_VIEWS];   //   -1 = NA (no shared names)
  double tol;
  double phi[GRP_MAX_VIEWS * GRP_MAX_VIEWS];      // [w * 8 + v] = phi[w, v] (symmetrised, zero diagonal)
  double xi[GRP_MAX_VIEWS * GRP_MAX_VIEWS];
  double psi[GRP_MAX_VIEWS * GRP_MAX_VIEWS];
};

// LDS doubles a job needs: S, lambda, mu of every view, four k x k temporaries, the reduction tree, per-view values
__host__ __device__ inline int group_lds_doubles(int V, int k) {
  return V * k * k + 2 * V * k + 4 * k * k + GRP_THREADS + 2 * GRP_MAX_VIEWS;
}

// sum of one value per thread by a fixed tree; every thread gets the total
__device__ inline double grp_block_sum(double x, double* red) {
  const int t = threadIdx.x;
  red[t] = x;
  __syncthreads();
  for (int s = GRP_THREADS / 2; s > 0; s >>= 1) {
    if (t < s) red[t] += red[t + s];
    __syncthreads();
  }
  const double r = red[0];
  __syncthreads();
  return r;
}

// out[a + b * ka] = sum_i A[i + a * len] * B[i + b * len]  (B == nullptr: column sums of A, kb = 1).  With
// Q = ka * kb <= 256 outputs, T = the largest power of two with T * Q <= 256 threads share one output (thread l of
// the T sums rows l, l + T, ... in order), then a fixed tree over the T; above 256 outputs one thread per output.
__device__ inline void grp_gram(const double* A, const double* B, int len, int ka, int kb, double* out, double* red) {
  const int Q = ka * kb, t = threadIdx.x;
  if (Q <= GRP_THREADS) {
    int T = 1;
    while (T * 2 * Q <= GRP_THREADS) T *= 2;
    const int q = t / T, l = t - q * T;
    double acc = 0.0;
    if (q < Q) {
      const int a = q % ka, b = q / ka;
      const double* pa = A + (size_t)a * len;
      if (B) {
        const double* pb = B + (size_t)b * len;
#pragma unroll 4
        for (int i = l; i < len; i += T) acc = fma(pa[i], pb[i], acc);
      } else {
#pragma unroll 4
        for (int i = l; i < len; i += T) acc += pa[i];
      }
    }
    red[t] = acc;
    __syncthreads();
    for (int s = T / 2; s > 0; s >>= 1) {
      if (q < Q && l < s) red[t] += red[t + s];
      __syncthreads();
    }
    if (q < Q && l == 0) out[q] = red[t];
    __syncthreads();
  } else {
    for (int q = t; q < Q; q += GRP_THREADS) {
      const int a = q % ka, b = q / ka;
      const double* pa = A + (size_t)a * len;
      const double* pb = B + (size_t)b * len;
      double acc = 0.0;
      for (int i = 0; i < len; ++i) acc = fma(pa[i], pb[i], acc);
      out[q] = acc;
    }
    __syncthreads();
  }
}

// C = op(A) op(B), k x k column-major in LDS; op = transpose when the flag is set
__device__ inline void grp_kk(const double* A, bool tA, const double* B, bool tB, int k, double* C) {
  for (int q = threadIdx.x; q < k * k; q += GRP_THREADS) {
    const int r = q % k, c = q / k;
    double acc = 0.0;
    for (int e = 0; e < k; ++e)
      acc = fma(tA ? A[e + r * k] : A[r + e * k], tB ? B[c + e * k] : B[e + c * k], acc);
    C[q] = acc;
  }
  __syncthreads();
}

// numpy's sum of a short vector (pairwise_sum: sequential below 8 entries, the 8-accumulator form at 8)
__device__ inline double grp_vec_sum(const double* a, int stride, int n) {
  if (n < 8) {
    double r = 0.0;
    for (int i = 0; i < n; ++i) r += a[i * stride];
    return r;
  }
  return ((a[0] + a[stride]) + (a[2 * stride] + a[3 * stride])) + ((a[4 * stride] + a[5 * stride]) + (a[6 * stride] + a[7 * stride]));
}

// every entry of a V x V restriction is zero (the whole-matrix branch tests of update_g / update_s; the entries are
// checked non-negative on the host, so this is sum(M) == 0)
__device__ inline bool grp_all_zero(const double* M, int V) {
  for (int w = 0; w < V; ++w)
    for (int v = 0; v < V; ++v)
      if (M[w * GRP_MAX_VIEWS + v] != 0.0) return false;
  return true;
}

// update_f (R/update_steps.r:141-165) or update_g (:180-207) of view v, in place.  For the G form the roles swap:
// rows = columns of X (read through X^T), "F" = G, S^T for S, mu for lambda, psi for phi, column maps for row maps,
// and the branch tests the whole psi; the G form also keeps X^T F in the scratch for update_s.
template <int KM, bool G_FORM>
__device__ void grp_update_side(const GroupDesc& d, double* base, const int* ibase, int v, double* lS, double* lLM,
                                double* kkA, double* kkB, double* red) {
  const int k = d.k, V = d.V;
  const int n = G_FORM ? d.m[v] : d.n[v];         // rows of the factor being updated
  const int m = G_FORM ? d.n[v] : d.m[v];         // rows of the other factor
  double* P = base + (G_FORM ? d.g[v] : d.f[v]);  // factor updated (n x k)
  const double* O = base + (G_FORM ? d.f[v] : d.g[v]);   // the other factor (m x k)
  const double* X = base + (G_FORM ? d.xt[v] : d.x[v]);  // n x m column-major
  const double* S = lS + v * k * k;
  const double* lm = lLM + v * k;
  const double* R = G_FORM ? d.psi : d.phi;
  double* xo = base + d.scratch;                  // X O (n x k); the G form's X^T F is read again by update_s
  double* ps = base + d.scratch2;                 // P S / G S^T (n x k)

  grp_gram(O, O, m, k, k, kkA, red);              // O^T O
  // F form: W = (G^T G) S^T  -> den = (F S) W;   G form: W = (F^T F) S -> den = (G S^T) W
  grp_kk(kkA, false, S, !G_FORM, k, kkB);
  double rsum = grp_vec_sum(R + v, GRP_MAX_VIEWS, V);                    // sum(phi[, v]) / sum(psi[, v])
  const bool unrestricted = G_FORM ? grp_all_zero(R, V) : (rsum == 0.0); // :152 / :190

  for (int i = threadIdx.x; i < n; i += GRP_THREADS) {
    double xo_r[KM];
#pragma unroll
    for (int c = 0; c < KM; ++c) xo_r[c] = 0.0;
    constexpr int kColUnroll = KM == 8 ? 4 : (KM == 16 ? 2 : 1);   // (4 at k = 32 costs 256 VGPRs)
#pragma unroll kColUnroll
    for (int j = 0; j < m; ++j) {                 // (X O)[i, :]  (unrolled: several columns' loads in flight)
      const double x = X[i + (size_t)j * n];
#pragma unroll
      for (int c = 0; c < KM; ++c)
        if (c < k) xo_r[c] = fma(x, O[j + (size_t)c * m], xo_r[c]);
    }
#pragma unroll
    for (int c = 0; c < KM; ++c)
      if (c < k) xo[i + (size_t)c * n] = xo_r[c];
    for (int c = 0; c < k; ++c) {                 // P S (F form) or G S^T (G form), row i
      double acc = 0.0;
      for (int e = 0; e < k; ++e) acc = fma(P[i + (size_t)e * n], G_FORM ? S[c + e * k] : S[e + c * k], acc);
      ps[i + (size_t)c * n] = acc;
    }
    for (int c = 0; c < k; ++c) {
      double num = 0.0, den = 0.0;                // numerator: F form (X G) S^T, G form (X^T F) S
      for (int e = 0; e < k; ++e) num = fma(xo[i + (size_t)e * n], G_FORM ? S[e + c * k] : S[c + e * k], num);
      for (int e = 0; e < k; ++e) den = fma(ps[i + (size_t)e * n], kkB[e + c * k], den);
      const double p = P[i + (size_t)c * n];
      const double half = 0.5 * lm[c];
      double out;
      if (unrestricted) {
        double mat = num / (den + half);
        if (isnan(mat)) mat = 1.0;
        out = p * mat;
      } else {                                    // star_prod_relevant (R/utils.r:63-78)
        double acc = 0.0;
        for (int w = 0; w < V; ++w) {
          const double r = R[w * GRP_MAX_VIEWS + v];
          const long long mo = G_FORM ? d.cmap[v][w] : d.rmap[v][w];
          if (r == 0.0 || mo < 0) continue;
          const int nw = G_FORM ? d.m[w] : d.n[w];
          const int row = ibase[mo + i];
          const double* Pw = base + (G_FORM ? d.g[w] : d.f[w]);
          const double val = row >= 0 ? Pw[row + (size_t)c * nw] : p;
          acc = acc + r * val * (double)nw;
        }
        const double np = acc / (double)n;
        out = p * ((num + np) / (den + rsum * p + half));
      }
      P[i + (size_t)c * n] = fabs(out);
    }
  }
  __syncthreads();
}

// update_s (R/update_steps.r:220-240) of view v, in place in LDS; kkA holds F^T F, the scratch X^T F
template <int KM>
__device__ void grp_update_s(const GroupDesc& d, double* base, int v, double* lS, double* kkA, double* kkB,
                             double* kkC, double* kkD, double* red) {
  const int k = d.k, V = d.V, m = d.m[v];
  const double* G = base + d.g[v];
  const double* xo = base + d.scratch;
  double* S = lS + v * k * k;
  grp_gram(xo, G, m, k, k, kkC, red);             // (F^T X) G
  grp_gram(G, G, m, k, k, kkD, red);              // G^T G
  grp_kk(kkA, false, S, false, k, kkB);           // (F^T F) S
  grp_kk(kkB, false, kkD, false, k, kkA);         // ((F^T F) S) (G^T G)
  const bool unrestricted = grp_all_zero(d.xi, V);                      // :226
  const double xsum = grp_vec_sum(d.xi + v, GRP_MAX_VIEWS, V);
  for (int q = threadIdx.x; q < k * k; q += GRP_THREADS) {
    const double s = S[q];
    double out;
    if (unrestricted) {
      double mat = kkC[q] / kkA[q];
      if (isnan(mat)) mat = 1.0;
      out = s * mat;
    } else {                                      // star_prod (R/utils.r:39-47)
      double acc = 0.0;
      for (int w = 0; w < V; ++w) {
        const double x = d.xi[w * GRP_MAX_VIEWS + v];
        if (x != 0.0) acc = acc + x * lS[w * k * k + q];
      }
      out = s * ((kkC[q] + acc) / (kkA[q] + xsum * s));
    }
    S[q] = fabs(out);
  }
  __syncthreads();
}

// ||X - F S G^T||_F^2 of view v (calculate_error, R/utils.r:157-166: x_hat = (F S) G^T), as norm()^2
template <int KM>
__device__ double grp_view_error(const GroupDesc& d, double* base, int v, const double* lS, double* red) {
  const int k = d.k, n = d.n[v], m = d.m[v];
  const double* F = base + d.f[v];
  const double* G = base + d.g[v];
  const double* X = base + d.x[v];
  const double* S = lS + v * k * k;
  double* fs = base + d.scratch2;
  for (int i = threadIdx.x; i < n; i += GRP_THREADS) {
#pragma unroll
    for (int c = 0; c < KM; ++c) {
      if (c >= k) continue;
      double acc = 0.0;
      for (int e = 0; e < k; ++e) acc = fma(F[i + (size_t)e * n], S[e + c * k], acc);
      fs[i + (size_t)c * n] = acc;
    }
  }
  __syncthreads();
  const unsigned total = (unsigned)n * (unsigned)m;
  double acc = 0.0;
#pragma unroll 2
  for (unsigned e = threadIdx.x; e < total; e += GRP_THREADS) {
    const unsigned j = e / (unsigned)n, i = e - j * (unsigned)n;
    double xh = 0.0;
#pragma unroll
    for (int c = 0; c < KM; ++c)
      if (c < k) xh = fma(fs[i + (size_t)c * n], G[j + (size_t)c * m], xh);
    const double r = X[e] - xh;
    acc = fma(r, r, acc);
  }
  const double sq = grp_block_sum(acc, red);      // (every thread is past its fs reads here)
  const double nrm = sqrt(sq);
  return nrm * nrm;
}

template <int KM>
__device__ void grp_run_job(const GroupDesc& d, double* base, const int* ibase, int* sweeps, double* lds) {
  const int V = d.V, k = d.k, t = threadIdx.x;
  double* lS = lds;
  double* lLam = lS + V * k * k;
  double* lMu = lLam + V * k;
  double* kkA = lMu + V * k;
  double* kkB = kkA + k * k;
  double* kkC = kkB + k * k;
  double* kkD = kkC + k * k;
  double* red = kkD + k * k;
  double* norms = red + GRP_THREADS;              // ||X_v||_F^2 (norm()^2, R/main.r:48)
  double* errs = norms + GRP_MAX_VIEWS;

  for (int q = t; q < V * k * k; q += GRP_THREADS) lS[q] = base[d.s + q];
  for (int q = t; q < V * k; q += GRP_THREADS) { lLam[q] = base[d.lam + q]; lMu[q] = base[d.mu + q]; }
  for (int v = 0; v < V; ++v) {
    const double* X = base + d.x[v];
    const unsigned total = (unsigned)d.n[v] * (unsigned)d.m[v];
    double acc = 0.0;
    for (unsigned e = t; e < total; e += GRP_THREADS) acc = fma(X[e], X[e], acc);
    const double sq = grp_block_sum(acc, red);
    const double nrm = sqrt(sq);
    if (t == 0) norms[v] = nrm * nrm;
  }
  __syncthreads();

  double err_temp = 0.0;                          // R/main.r:53-54
  int it = 0;
  while (it < d.cap) {
    for (int v = 0; v < V; ++v) {                 // update_matrices (R/update_steps.r:272-319), Gauss-Seidel
      grp_update_side<KM, false>(d, base, ibase, v, lS, lLam, kkA, kkB, red);
      grp_update_side<KM, true>(d, base, ibase, v, lS, lMu, kkA, kkB, red);   // leaves F^T F in kkA
      grp_update_s<KM>(d, base, v, lS, kkA, kkB, kkC, kkD, red);
      grp_gram(base + d.f[v], nullptr, d.n[v], k, 1, kkA, red);             // update_lm (:249-251, :312-313)
      grp_gram(base + d.g[v], nullptr, d.m[v], k, 1, kkB, red);
      for (int c = t; c < k; c += GRP_THREADS) {
        lLam[v * k + c] = kkA[c] * lLam[v * k + c];
        lMu[v * k + c] = kkB[c] * lMu[v * k + c];
      }
      __syncthreads();
    }
    for (int v = 0; v < V; ++v) {
      const double e = grp_view_error<KM>(d, base, v, lS, red);
      if (t == 0) errs[v] = e / norms[v];
    }
    __syncthreads();
    const double mean = grp_vec_sum(errs, 1, V) / (double)V;
    if (t == 0) base[d.err + (long long)it * d.err_stride] = mean;
    ++it;
    if (d.n_iters == 0) {                         // R/main.r:55, 79-80
      const double diff = fabs(mean - err_temp);
      err_temp = mean;
      if (!(diff > d.tol)) break;
    }
  }

  // normalisation_check (R/utils.r:176-195): S columns by cF * cG, then F / cF, G / cG
  for (int v = 0; v < V; ++v) {
    const int n = d.n[v], m = d.m[v];
    double* F = base + d.f[v];
    double* G = base + d.g[v];
    grp_gram(F, nullptr, n, k, 1, kkA, red);
    grp_gram(G, nullptr, m, k, 1, kkB, red);
    for (int q = t; q < k * k; q += GRP_THREADS) {
      const int c = q / k;
      lS[v * k * k + q] = lS[v * k * k + q] * (kkA[c] * kkB[c]);
    }
    for (int q = t; q < n * k; q += GRP_THREADS) F[q] = F[q] / kkA[q / n];
    for (int q = t; q < m * k; q += GRP_THREADS) G[q] = G[q] / kkB[q / m];
    __syncthreads();
  }
  for (int q = t; q < V * k * k; q += GRP_THREADS) base[d.s + q] = lS[q];
  for (int q = t; q < V * k; q += GRP_THREADS) { base[d.lam + q] = lLam[q]; base[d.mu + q] = lMu[q]; }
  if (t == 0) sweeps[d.id] = it;
}

// one instance per k class (k <= 8, 16, 32): a job runs in the instance of its own k, whatever else is in the batch
template <int KM>
__global__ __launch_bounds__(GRP_THREADS) void group_kernel(const GroupDesc* __restrict__ descs, double* base,
                                                            const int* ibase, int* sweeps) {
  extern __shared__ double group_lds[];
  grp_run_job<KM>(descs[blockIdx.x], base, ibase, sweeps, group_lds);
}

__host__ __device__ inline int group_k_class(int k) { return k <= 8 ? 8 : (k <= 16 ? 16 : 32); }
