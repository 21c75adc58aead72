// resnmtf_jsd.hip.inc -- Jensen-Shannon scores of column pairs (resnmtf_jsd_pairs): jsd_calc (R/utils.r:95-106) for
// every pair of a list, as check_biclusters / get_thresholds (R/obtain_bicl.r:55-133) call it.  Included by
// resnmtf_hip.hip; fp64 throughout (the removal rule compares near-equal statistics).  DESIGN.md section 11.
//
// jsd_calc(x1, x2): both sides get stats::density(c, from = 0, to = M), M = max(x1, x2), n = 512 (R <= 4.3's
// old.coords form), their values beyond max(c) are zeroed, and philentropy::JSD(unit = "log2", est.prob = "empirical")
// compares the two.  Three kernels:
//   jsd_tile_sort_kernel / jsd_merge_kernel  every column sorted ascending once: 2048-entry tiles by a bitonic network in
//                                            LDS, then merge passes whose every entry finds its place by a binary search
//                                            of the partner run (ties: the left run first).  -0 is stored as +0.
//   jsd_stats_kernel                         per column: bw.nrd0 (sd: R's refined mean, then a second pass; type-7 quartiles off the sorted
//                                            column, the fallbacks) and the maximum.
//   jsd_pair_kernel                          one workgroup per pair, both sides in LDS: BinDist from the sorted column,
//                                            the 512 x 512 Toeplitz sum with the Gaussian table, the clamp, approx, the
//                                            zeroing, the normalisation and the JSD reduction.
// Determinism: every sum has an order fixed by n alone (chunks of ceil(n / 512) sorted entries, chunk order, fixed
// reduction trees), no atomics; a column's sort and statistics depend on that column only, and a pair's value on its
// two columns only -- not on the other pairs of the launch, their order or the grid.

#include <cfloat>

namespace {

constexpr int JSD_N = 512;            // density()'s n
constexpr int JSD_TILE = 2048;        // entries of one LDS-sorted tile
constexpr int JSD_SORT_THREADS = 1024;
constexpr int JSD_KEY_LOW = -2;       // bin keys outside [-1, 511] (no contribution) are clamped to -2 / 512
constexpr int JSD_KEY_HIGH = 512;     // (jsd_pair_kernel bins x <= M < up = M + 4 bw with bw > 0, so xpos < 511: key 510 is the
                                      // highest any input reaches; 511 and JSD_KEY_HIGH are kept for BinDist's form only)
constexpr int JSD_KEY_EMPTY = 1 << 30;

__device__ __forceinline__ double jsd_canon(double v) { return v == 0.0 ? 0.0 : v; }

__global__ void __launch_bounds__(JSD_SORT_THREADS)
jsd_tile_sort_kernel(const double* __restrict__ src, double* __restrict__ dst, int n) {
  __shared__ double s[JSD_TILE];
  const size_t col = (size_t)blockIdx.y * n;
  const int base = blockIdx.x * JSD_TILE;
  const int cnt = min(JSD_TILE, n - base);
  for (int i = threadIdx.x; i < JSD_TILE; i += JSD_SORT_THREADS)
    s[i] = i < cnt ? jsd_canon(src[col + base + i]) : INFINITY;      // finite inputs (host check): padding sorts last
  __syncthreads();
  for (int k = 2; k <= JSD_TILE; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      const int t = threadIdx.x;
      const int i = 2 * t - (t & (j - 1));
      const bool up = (i & k) == 0;
      const double a = s[i], b = s[i + j];
      if ((a > b) == up) { s[i] = b; s[i + j] = a; }
      __syncthreads();
    }
  }
  for (int i = threadIdx.x; i < cnt; i += JSD_SORT_THREADS) dst[col + base + i] = s[i];
}

// merge runs [2r w, (2r + 1) w) and [(2r + 1) w, (2r + 2) w) of every column (clipped to n) from src into dst
__global__ void __launch_bounds__(256)
jsd_merge_kernel(const double* __restrict__ src, double* __restrict__ dst, int n, int width) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const size_t col = (size_t)blockIdx.y * n;
  const double key = src[col + i];
  const int run = i / width;
  const int base = (run & ~1) * width;
  const bool left = (run & 1) == 0;
  const int pb = left ? base + width : base;                  // partner run [pb, pe)
  const int pe = left ? min(base + 2 * width, n) : base + width;
  const int own = left ? i - base : i - (base + width);
  int lo = pb, hi = max(pb, pe);
  while (lo < hi) {                                           // left: #partner < key; right: #partner <= key
    const int mid = (lo + hi) >> 1;
    const double v = src[col + mid];
    if (left ? (v < key) : (v <= key)) lo = mid + 1; else hi = mid;
  }
  dst[col + base + own + (lo - pb)] = key;
}

__device__ double jsd_block_sum256(double v, double* red) {   // fixed tree over 256 lanes (4 waves)
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  const int w = threadIdx.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[w] = v;
  __syncthreads();
  return ((red[0] + red[1]) + (red[2] + red[3]));
}

// per column: bw.nrd0 (stats::bw.nrd0) and the maximum; sorted = the sorted columns, orig = the columns as given
// (bw.nrd0's abs(x[1]) fallback reads the first entry in the caller's order).  n_pow = n^-0.2 from the host's pow, the
// one R's length(x)^(-0.2) calls: the device's pow is a last bit off it at some n (511, 2048, 2049, 6145 among the
// tested sizes), which a constant column's bandwidth 0.9 |x[1]| n^-0.2 shows bit for bit
__global__ void __launch_bounds__(256)
jsd_stats_kernel(const double* __restrict__ sorted, const double* __restrict__ orig, int n, double n_pow,
                 double* __restrict__ stats) {
  __shared__ double red[4];
  const size_t col = (size_t)blockIdx.x * n;
  const double* x = sorted + col;
  double s = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) s += x[i];
  const double mean0 = jsd_block_sum256(s, red) / n;
  double sd0 = 0.0;                                           // R's refinement of the mean (cov.c): a constant column
  for (int i = threadIdx.x; i < n; i += 256) sd0 += x[i] - mean0;    // gets sd = 0 exactly, hence bw.nrd0's fallbacks
  const double mean = mean0 + jsd_block_sum256(sd0, red) / n;
  double ss = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) { const double d = x[i] - mean; ss += d * d; }
  const double var = jsd_block_sum256(ss, red) / (n - 1);
  if (threadIdx.x != 0) return;
  const double hi = sqrt(var);
  double q[2];
  const double probs[2] = {0.25, 0.75};
  for (int t = 0; t < 2; ++t) {                               // quantile(type = 7): index = 1 + (n - 1) p
    const double index = 1.0 + (double)(n - 1) * probs[t];
    const double flo = floor(index), fhi = ceil(index);
    const int l = (int)flo - 1, h = (int)fhi - 1;
    double qs = x[l];
    if (index > flo && x[h] != qs) { const double hh = index - flo; qs = (1.0 - hh) * qs + hh * x[h]; }
    q[t] = qs;
  }
  double lo = fmin(hi, (q[1] - q[0]) / 1.34);
  if (lo == 0.0) {
    lo = hi;
    if (lo == 0.0) { lo = fabs(orig[col]); if (lo == 0.0) lo = 1.0; }
  }
  stats[2 * blockIdx.x] = 0.9 * lo * n_pow;
  stats[2 * blockIdx.x + 1] = x[n - 1];
}

// stats::dnorm(x, 0, sigma) (nmath/dnorm.c, the accurate branch for |x| / sigma >= 5)
__device__ __forceinline__ double jsd_dnorm(double x, double sigma) {
  const double M_1_SQRT_2PI_ = 0.398942280401432677939946059934;
  x = fabs(x / sigma);
  if (x >= 2.0 * sqrt(DBL_MAX)) return 0.0;
  if (x < 5.0) return M_1_SQRT_2PI_ * exp(-0.5 * x * x) / sigma;
  if (x > sqrt(-2.0 * 0.693147180559945309417232121458 * (DBL_MIN_EXP + 1 - DBL_MANT_DIG))) return 0.0;
  const double x1 = ldexp(rint(ldexp(x, 16)), -16);
  const double x2 = x - x1;
  return M_1_SQRT_2PI_ / sigma * (exp(-0.5 * x1 * x1) * exp((-0.5 * x2 - x1) * x2));
}

// seq.int(from, to, length.out = 512), entry i (R's symmetric form, src/main/seq.c)
__device__ __forceinline__ double jsd_seq(double from, double to, int i) {
  if (i == 0) return from;
  if (i == JSD_N - 1) return to;
  const double by = (to - from) / (double)(JSD_N - 1);
  return i < JSD_N / 2 ? from + (double)i * by : to - (double)(JSD_N - 1 - i) * by;
}

struct JsdPairShared {
  double y[2][JSD_N];                 // binned mass, then the density on xords
  double g[2][JSD_N];                 // Gaussian table dnorm(d * 2 (up - lo) / 1023, bw)
  double a[JSD_N + 1], b[JSD_N + 1];  // per bin key (-1 .. 511, index key + 1): sum of w (1 - fx) / of w fx
  double ha[JSD_N], hb[JSD_N], ta[JSD_N], tb[JSD_N];   // per chunk: head / tail run partials
  int hk[JSD_N], tk[JSD_N];           // per chunk: head / tail run keys
  double red[8];
};

__device__ __forceinline__ double jsd_block_sum512(double v, double* red) {   // fixed tree over 512 lanes (8 waves)
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((red[0] + red[1]) + (red[2] + red[3])) + ((red[4] + red[5]) + (red[6] + red[7]));
}

// BinDist(x, rep(1/n, n), lo, up, 512) (src/library/stats/src/massdist.c) of one sorted column into sh.y[side].
// Entry x has key ix = floor((x - lo) / xdelta) and fx = the fraction: w (1 - fx) goes to bin ix (0 <= ix <= 511),
// w fx to bin ix + 1 (-1 <= ix <= 510).  ix is monotone along the sorted column, so every key's entries are one
// contiguous run: chunk t = entries [t L, (t + 1) L), L = ceil(n / 512), sums its runs in order; a run strictly inside
// a chunk is that key's whole sum, the first and last run of a chunk are partials, summed over the chunks in order.
__device__ void jsd_bin(const double* __restrict__ x, int n, double lo, double xdelta, JsdPairShared& sh, int side) {
  const int t = threadIdx.x;
  const double w = 1.0 / (double)n;
  sh.a[t] = 0.0; sh.b[t] = 0.0;
  if (t == 0) { sh.a[JSD_N] = 0.0; sh.b[JSD_N] = 0.0; }
  __syncthreads();
  const int L = (n + JSD_N - 1) / JSD_N;
  const int beg = t * L, end = min(n, beg + L);
  if (beg >= n) {
    sh.hk[t] = JSD_KEY_EMPTY; sh.tk[t] = JSD_KEY_EMPTY;
    sh.ha[t] = sh.hb[t] = sh.ta[t] = sh.tb[t] = 0.0;
  } else {
    int cur = 0;
    double sa = 0.0, sb = 0.0;
    bool head = false;
    for (int i = beg; i < end; ++i) {
      const double xpos = (x[i] - lo) / xdelta;
      int key;
      double ca = 0.0, cb = 0.0;
      if (xpos < -1.0) key = JSD_KEY_LOW;
      else if (xpos >= 512.0) key = JSD_KEY_HIGH;
      else {
        key = (int)floor(xpos);
        const double fx = xpos - (double)key;
        if (key >= 0) ca = w * (1.0 - fx);
        if (key <= JSD_N - 2) cb = w * fx;
      }
      if (i == beg) cur = key;
      if (key != cur) {
        if (!head) { sh.hk[t] = cur; sh.ha[t] = sa; sh.hb[t] = sb; head = true; }
        else if (cur >= -1 && cur < JSD_N) { sh.a[cur + 1] = sa; sh.b[cur + 1] = sb; }   // the whole run of key cur
        cur = key; sa = 0.0; sb = 0.0;
      }
      sa += ca; sb += cb;
    }
    if (!head) { sh.hk[t] = cur; sh.ha[t] = sa; sh.hb[t] = sb; sh.tk[t] = cur; sh.ta[t] = 0.0; sh.tb[t] = 0.0; }
    else { sh.tk[t] = cur; sh.ta[t] = sa; sh.tb[t] = sb; }
  }
  __syncthreads();
  for (int q = t; q <= JSD_N; q += JSD_N) {                   // key = q - 1 in [-1, 511]
    const int key = q - 1;
    int l = 0, h = JSD_N;                                     // first chunk whose tail key >= key
    while (l < h) { const int m = (l + h) >> 1; if (sh.tk[m] < key) l = m + 1; else h = m; }
    bool found = false;
    double sa = 0.0, sb = 0.0;
    for (int c = l; c < JSD_N && sh.hk[c] <= key; ++c) {
      if (sh.hk[c] == key) { sa += sh.ha[c]; sb += sh.hb[c]; found = true; }
      else if (sh.tk[c] == key) { sa += sh.ta[c]; sb += sh.tb[c]; found = true; }
    }
    if (found) { sh.a[q] = sa; sh.b[q] = sb; }
  }
  __syncthreads();
  sh.y[side][t] = sh.a[t + 1] + sh.b[t];                      // bin t: w (1 - fx) of key t, w fx of key t - 1
  __syncthreads();
}

// out[p] = jsd_calc(cols[:, pairs[2p]], cols[:, pairs[2p + 1]]); dens (nullable, [n_pairs][2][512], resnmtf_jsd_stages)
// receives both sides' densities on xout after the zeroing, before the normalisation
__global__ void __launch_bounds__(JSD_N)
jsd_pair_kernel(const double* __restrict__ sorted, const double* __restrict__ stats, int n,
                const int* __restrict__ pairs, double* __restrict__ out, double* __restrict__ dens) {
  __shared__ JsdPairShared sh;
  const int t = threadIdx.x;
  const int p = blockIdx.x;
  const int c[2] = {pairs[2 * p], pairs[2 * p + 1]};
  const double bw[2] = {stats[2 * c[0]], stats[2 * c[1]]};
  const double mx[2] = {stats[2 * c[0] + 1], stats[2 * c[1] + 1]};
  const double M = fmax(mx[0], mx[1]);
  double lo[2], up[2];
  for (int s = 0; s < 2; ++s) {
    lo[s] = 0.0 - 4.0 * bw[s];                                // density.default: lo = from - 4 bw, up = to + 4 bw
    up[s] = M + 4.0 * bw[s];
    jsd_bin(sorted + (size_t)c[s] * n, n, lo[s], (up[s] - lo[s]) / (double)(JSD_N - 1), sh, s);
    const double by = (2.0 * (up[s] - lo[s])) / (double)(2 * JSD_N - 1);   // kords = seq(0, 2 (up - lo), length 1024)
    sh.g[s][t] = jsd_dnorm((double)t * by, bw[s]);
  }
  __syncthreads();
  // Re(fft^-1(fft(y) Conj(fft(kords))))[0:512] / 1024 with y's upper half zero = this direct sum, then pmax(0, .)
  double acc0 = 0.0, acc1 = 0.0;
  for (int a = 0; a < JSD_N; ++a) {
    const int d = a > t ? a - t : t - a;
    const double y0 = sh.y[0][a], y1 = sh.y[1][a];
    if (y0 != 0.0) acc0 += y0 * sh.g[0][d];
    if (y1 != 0.0) acc1 += y1 * sh.g[1][d];
  }
  __syncthreads();
  sh.y[0][t] = fmax(0.0, acc0);
  sh.y[1][t] = fmax(0.0, acc1);
  __syncthreads();
  // approx(xords = seq(lo, up, 512), y, xout = seq(0, M, 512)) (stats/src/approx.c), then y[x > max(c)] <- 0
  const double v = jsd_seq(0.0, M, t);
  double yv[2];
  for (int s = 0; s < 2; ++s) {
    const double* ys = sh.y[s];
    int i = 0, j = JSD_N - 1;
    double r;
    if (v < jsd_seq(lo[s], up[s], i) || v > jsd_seq(lo[s], up[s], j)) r = NAN;
    else {
      while (i < j - 1) { const int ij = (i + j) / 2; if (v < jsd_seq(lo[s], up[s], ij)) j = ij; else i = ij; }
      const double xi = jsd_seq(lo[s], up[s], i), xj = jsd_seq(lo[s], up[s], j);
      if (v == xj) r = ys[j];
      else if (v == xi) r = ys[i];
      else r = ys[i] + (ys[j] - ys[i]) * ((v - xi) / (xj - xi));
    }
    yv[s] = v > mx[s] ? 0.0 : r;
    if (dens) dens[((size_t)p * 2 + s) * JSD_N + t] = yv[s];
  }
  const double s0 = jsd_block_sum512(yv[0], sh.red);
  const double s1 = jsd_block_sum512(yv[1], sh.red);
  // philentropy::JSD(rbind(P, Q), unit = "log2", est.prob = "empirical"): terms with P = 0 (Q = 0) skipped
  const double P = yv[0] / s0, Q = yv[1] / s1, PQ = P + Q;
  const double t1 = (P == 0.0 || PQ == 0.0) ? 0.0 : P * log2((2.0 * P) / PQ);
  const double t2 = (Q == 0.0 || PQ == 0.0) ? 0.0 : Q * log2((2.0 * Q) / PQ);
  const double sum1 = jsd_block_sum512(t1, sh.red);
  const double sum2 = jsd_block_sum512(t2, sh.red);
  if (t == 0) out[p] = 0.5 * (sum1 + sum2);
}


// ---- resnmtf_spurious_scores: the pool is gathered on the device (colsum_kernel + finalise_factor_kernel per handle) --
// flag[0] = 1 when an entry of the pool is not finite (a plain store of one value: no sum, no atomic)
__global__ void __launch_bounds__(256)
jsd_finite_kernel(const double* __restrict__ x, size_t total, int* __restrict__ flag) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256)
    if (!isfinite(x[i])) flag[0] = 1;
}

// NumPy's pairwise summation (pairwise_sum of numpy/_core/src/umath/loops_utils.h.src, the order np.mean uses along a
// contiguous axis): below 8 entries in order from 0; up to 128 eight strided accumulators, combined as
// ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)), then the tail in order; above, split at n / 2 rounded down to a
// multiple of 8.  D bounds the depth at compile time (n < 2^31 needs 24 levels).
__device__ double jsd_np_pairwise_leaf(const double* a, long long n) {
  if (n < 8) {
    double r = 0.0;
    for (long long i = 0; i < n; ++i) r += a[i];
    return r;
  }
  double r[8];
  for (int j = 0; j < 8; ++j) r[j] = a[j];
  long long i = 8;
  for (; i < n - (n % 8); i += 8)
    for (int j = 0; j < 8; ++j) r[j] += a[i + j];
  double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
  for (; i < n; ++i) res += a[i];
  return res;
}

template <int D>
__device__ double jsd_np_pairwise(const double* a, long long n) {
  if constexpr (D == 0) {
    return jsd_np_pairwise_leaf(a, n);
  } else {
    if (n <= 128) return jsd_np_pairwise_leaf(a, n);
    long long n2 = n / 2;
    n2 -= n2 % 8;
    return jsd_np_pairwise<D - 1>(a, n2) + jsd_np_pairwise<D - 1>(a + n2, n - n2);
  }
}

// score[k] = mean(vals[k * RK .. (k + 1) * RK)) as np.mean(vals.reshape(K, RK), axis=1) computes it: one thread per k
__global__ void __launch_bounds__(64)
jsd_score_mean_kernel(const double* __restrict__ vals, int K, int RK, double* __restrict__ score) {
  const int k = blockIdx.x * 64 + threadIdx.x;
  if (k >= K) return;
  score[k] = jsd_np_pairwise<24>(vals + (size_t)k * RK, RK) / (double)RK;
}

}  // namespace
