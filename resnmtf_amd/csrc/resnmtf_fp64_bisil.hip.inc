// resnmtf_fp64_bisil.hip.inc -- per-member silhouettes of a view's biclusters in double precision (resnmtf_fp64_bisil,
// DESIGN.md section 26): the score of R/obtain_bicl.r:189-199 computed on the numbers that precision="fp64" factorised.
// Included by resnmtf_fp64.hip only.
//
// This file is the TWIN of resnmtf_bisil.hip.inc.  The definition is DESIGN.md section 13, unchanged, and the launch
// structure per side and active bicluster is that file's: gather -> (cosine) norms -> distance tiles contracted with the
// membership bits -> epilogue.  The norm, distance and epilogue arithmetic below is stated a second time, line for line,
// with one difference: the restricted block G[f][u] = X(U[u], J_k[f]) is a `double` array, so no value passes through
// fp32.  (The two cannot share the text without making the existing kernels templates over G's type, which renames them
// and risks their instruction text; a change to the arithmetic of either file is a change to both.)  On data that fp32
// holds exactly the two give the same bits: widening is exact and every sum keeps its order -- features ascending, the
// 64-wide tiles of U ascending inside a chunk, chunk partials in chunk order, the member skipped by index.  No
// floating-point atomics, no waits between workgroups.
//
// The gather is the new kernel work: it reads X where it lies -- a resnmtf_device_matrix of fp64 / fp32 / fp16 / bf16
// with any strides >= 0 -- with no image in between.  Two forms, chosen per side from the strides alone
// (f64_bisil_gather_form, resnmtf_bisil_plan.h):
//   fp64_bisil_gather_pts_kernel<DT>   the point stride is the smaller: lanes along the points u, G written directly
//                                      (neighbouring lanes on neighbouring doubles of G, and on neighbouring points of X
//                                      as far as U is dense in them).
//   fp64_bisil_gather_lds_kernel<DT>   the feature stride is the smaller: a 32 (features) x 32 (points) tile through
//                                      LDS.  256 threads are 32 lanes (tx) x 8 (ty); lane tx reads feature f0 + tx of
//                                      point u0 + j into tile[j][tx] (32 lanes on 32 consecutive doubles), and after the
//                                      barrier writes G[(f0 + j) upad + u0 + tx] = tile[tx][j].  tile[32][33] doubles: a
//                                      pitch of 66 dwords, so the 32 lanes of a half wave sit on the bank pairs
//                                      (2 tx + 2 j) mod 64 -- 32 distinct pairs, no conflict (ds_read_b64 banks per
//                                      32-lane half over 64 dwords) --, the layout of fp64_images_kernel (section 23).
// Neither side of a row-major or a column-major source is read at a stride.  Both zero-fill U's padding n_u <= u < upad.
// Offsets are size_t throughout.

constexpr int F64_BISIL_TILE = BISIL_PLAN_TILE;    // members per workgroup = others per distance tile
constexpr int F64_BISIL_FT = 32;                   // features per LDS stage
constexpr int F64_BISIL_THREADS = 256;
enum { F64_BISIL_EUCLIDEAN = 0, F64_BISIL_MANHATTAN = 1, F64_BISIL_COSINE = 2 };

// G[f * upad + u] = X(pts[u], feat[f]) for u < n_u, 0 for n_u <= u < upad; X(p, f) = src[p * ps + f * fs]
template <int DT>
static __global__ void __launch_bounds__(256)
fp64_bisil_gather_pts_kernel(const void* __restrict__ src, size_t ps, size_t fs, const int* __restrict__ feat, int nf,
                             const int* __restrict__ pts, int n_u, int upad, double* __restrict__ G) {
  const size_t total = (size_t)nf * upad;
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
    const int f = (int)(e / upad), u = (int)(e % upad);
    G[e] = u < n_u ? f64_load_wide<DT>(src, (size_t)pts[u] * ps + (size_t)feat[f] * fs) : 0.0;
  }
}

// the same block through LDS; one workgroup per tile, tiles numbered along the points first (upad / 32 of them)
template <int DT>
static __global__ void __launch_bounds__(256)
fp64_bisil_gather_lds_kernel(const void* __restrict__ src, size_t ps, size_t fs, const int* __restrict__ feat, int nf,
                             const int* __restrict__ pts, int n_u, int upad, double* __restrict__ G) {
  __shared__ double tile[F64_DEV_TILE][F64_DEV_TILE + 1];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const unsigned tiles_u = (unsigned)(upad / F64_DEV_TILE);
  const int u0 = (int)(blockIdx.x % tiles_u) * F64_DEV_TILE, f0 = (int)(blockIdx.x / tiles_u) * F64_DEV_TILE;
  const int fr = f0 + tx;
  const size_t foff = fr < nf ? (size_t)feat[fr] * fs : 0;
  for (int j = ty; j < F64_DEV_TILE; j += 8) {
    const int u = u0 + j;
    tile[j][tx] = (u < n_u && fr < nf) ? f64_load_wide<DT>(src, (size_t)pts[u] * ps + foff) : 0.0;
  }
  __syncthreads();
  for (int j = ty; j < F64_DEV_TILE; j += 8) {
    const int f = f0 + j, u = u0 + tx;                      // (u < upad: upad is a multiple of 64)
    if (f < nf) G[(size_t)f * upad + u] = tile[tx][j];
  }
}

static __global__ void __launch_bounds__(256)
fp64_bisil_norm_kernel(const double* __restrict__ G, int nf, int upad, double* __restrict__ norm2) {
  const int u = blockIdx.x * 256 + threadIdx.x;
  if (u >= upad) return;
  double s = 0.0;
  for (int f = 0; f < nf; ++f) { const double x = G[(size_t)f * upad + u]; s = fma(x, x, s); }
  norm2[u] = s;
}

struct F64BisilShared {
  union {
    struct { double a[F64_BISIL_FT][F64_BISIL_TILE]; double b[F64_BISIL_FT][F64_BISIL_TILE]; } f;   // member / other features
    double d[F64_BISIL_TILE][F64_BISIL_TILE + 1];                                                   // distance tile (padded rows)
  };
  unsigned long long msk[F64_BISIL_TILE];   // membership bits of the tile's others
  int mp[F64_BISIL_TILE];                   // the workgroup's members as positions in U
};

// partial[((chunk * n_mem) + member) * K + l] = sum of d(member, u) over the u of this chunk with bit l set, u != member
template <int METRIC, int KQ>
static __global__ void __launch_bounds__(F64_BISIL_THREADS)
fp64_bisil_dist_kernel(const double* __restrict__ G, int nf, int upad, int n_u, const int* __restrict__ mpos, int n_mem,
                       const unsigned long long* __restrict__ umask, const double* __restrict__ norm2, int K,
                       int chunk_tiles, double* __restrict__ partial) {
  __shared__ F64BisilShared sh;
  const int t = threadIdx.x;
  const int m0 = blockIdx.x * F64_BISIL_TILE;
  const int chunk = blockIdx.y;
  const int tile_beg = chunk * chunk_tiles;
  const int tile_end = min(upad / F64_BISIL_TILE, tile_beg + chunk_tiles);
  if (t < F64_BISIL_TILE) sh.mp[t] = m0 + t < n_mem ? mpos[m0 + t] : 0;   // (out-of-range members: position 0, discarded)
  const int tm = t & 15, to = t >> 4;                                      // distances: members tm + 16 a, others to + 16 b
  const int ci = t >> 2, cq = t & 3;                                       // contraction: member ci, biclusters cq + 4 s
  double sums[KQ];
#pragma unroll
  for (int s = 0; s < KQ; ++s) sums[s] = 0.0;
  __syncthreads();
  for (int tile = tile_beg; tile < tile_end; ++tile) {
    const int u0 = tile * F64_BISIL_TILE;
    double acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b = 0; b < 4; ++b) acc[a][b] = 0.0;
    for (int f0 = 0; f0 < nf; f0 += F64_BISIL_FT) {
#pragma unroll
      for (int r = 0; r < F64_BISIL_FT * F64_BISIL_TILE / F64_BISIL_THREADS; ++r) {
        const int e = t + r * F64_BISIL_THREADS, f = e >> 6, c = e & 63;
        const bool in = f0 + f < nf;
        const size_t row = (size_t)min(f0 + f, nf - 1) * upad;     // (clamped: every load stays inside G)
        sh.f.a[f][c] = in ? G[row + sh.mp[c]] : 0.0;
        sh.f.b[f][c] = in ? G[row + u0 + c] : 0.0;
      }
      __syncthreads();
#pragma unroll 4
      for (int f = 0; f < F64_BISIL_FT; ++f) {
        double xa[4], xb[4];
#pragma unroll
        for (int a = 0; a < 4; ++a) xa[a] = sh.f.a[f][tm + 16 * a];
#pragma unroll
        for (int b = 0; b < 4; ++b) xb[b] = sh.f.b[f][to + 16 * b];
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
          for (int b = 0; b < 4; ++b) {
            if (METRIC == F64_BISIL_EUCLIDEAN) { const double df = xa[a] - xb[b]; acc[a][b] = fma(df, df, acc[a][b]); }
            else if (METRIC == F64_BISIL_MANHATTAN) acc[a][b] += fabs(xa[a] - xb[b]);
            else acc[a][b] = fma(xa[a], xb[b], acc[a][b]);
          }
      }
      __syncthreads();
    }
    // the feature stages are done (last barrier above): the distance tile takes their place
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      const int ma = tm + 16 * a;
      const int pa = sh.mp[ma];
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const int ob = to + 16 * b, u = u0 + ob;
        double d;
        if (METRIC == F64_BISIL_EUCLIDEAN) d = sqrt(fmax(acc[a][b], 0.0));
        else if (METRIC == F64_BISIL_MANHATTAN) d = acc[a][b];
        else {
          const double na = norm2[pa], nb = norm2[u];
          if (na == 0.0 && nb == 0.0) d = 0.0;
          else if (na == 0.0 || nb == 0.0) d = 1.0;
          else d = 1.0 - acc[a][b] / (sqrt(na) * sqrt(nb));
        }
        sh.d[ma][ob] = (u == pa || u >= n_u) ? 0.0 : d;
      }
    }
    if (t < F64_BISIL_TILE) sh.msk[t] = u0 + t < n_u ? umask[u0 + t] : 0ull;
    __syncthreads();
    for (int u = 0; u < F64_BISIL_TILE; ++u) {
      const double d = sh.d[ci][u];
      const unsigned long long mk = sh.msk[u] >> cq;
#pragma unroll
      for (int s = 0; s < KQ; ++s) sums[s] += ((mk >> (4 * s)) & 1ull) ? d : 0.0;
    }
    __syncthreads();
  }
  if (m0 + ci < n_mem) {
    double* out = partial + ((size_t)chunk * n_mem + m0 + ci) * K;
#pragma unroll
    for (int s = 0; s < KQ; ++s)
      if (cq + 4 * s < K) out[cq + 4 * s] = sums[s];
  }
}

// per member of bicluster k: a = mean over I_k \ {i}, b = min over the other active l with I_l \ {i} non-empty,
// s = (b - a) / max(a, b); 0 for a singleton I_k, no l left or max(a, b) = 0.  sil[k * n_pts + point] = s.
// One wave per member, lane l sums bicluster l's chunk partials in chunk order (coalesced over l); lane 0 then takes
// a and b from the K means in bicluster order.
static __global__ void __launch_bounds__(256)
fp64_bisil_epilogue_kernel(const double* __restrict__ partial, int n_chunks, int n_mem, int K, int k,
                           const int* __restrict__ mpos, const unsigned long long* __restrict__ umask,
                           const int* __restrict__ upts, const int* __restrict__ cnt, unsigned long long active, int n_pts,
                           double* __restrict__ sil) {
  __shared__ double mean_s[4][64];
  __shared__ int ok_s[4][64];
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
  const int m = blockIdx.x * 4 + w;
  double mean = 0.0;
  int ok = 0;
  if (m < n_mem && l < K && ((active >> l) & 1ull)) {
    const int c = cnt[l] - (int)((umask[mpos[m]] >> l) & 1ull);
    if (c > 0) {
      double s = 0.0;
      for (int ch = 0; ch < n_chunks; ++ch) s += partial[((size_t)ch * n_mem + m) * K + l];
      mean = s / (double)c;
      ok = 1;
    }
  }
  mean_s[w][l] = mean;
  ok_s[w][l] = ok;
  __syncthreads();
  if (l != 0 || m >= n_mem) return;
  double a = 0.0, b = 0.0;
  bool has_a = false, has_b = false;
  for (int j = 0; j < K; ++j) {
    if (!ok_s[w][j]) continue;
    if (j == k) { a = mean_s[w][j]; has_a = true; }
    else if (!has_b || mean_s[w][j] < b) { b = mean_s[w][j]; has_b = true; }
  }
  double s = 0.0;
  if (has_a && has_b) {
    const double mx = fmax(a, b);
    if (mx != 0.0) s = (b - a) / mx;
  }
  sil[(size_t)k * n_pts + upts[mpos[m]]] = s;
}

// ---- launches ----
template <int DT>
void f64_bisil_launch_gather(hipStream_t st, int form, const void* src, size_t ps, size_t fs, const int* feat, int nf,
                             const int* pts, int n_u, int upad, double* G) {
  if (form == F64_BISIL_GATHER_POINTS) {
    const size_t total = (size_t)nf * upad;
    hipLaunchKernelGGL((fp64_bisil_gather_pts_kernel<DT>), dim3((unsigned)std::min<size_t>((total + 255) / 256, 8192)), dim3(256), 0,
                       st, src, ps, fs, feat, nf, pts, n_u, upad, G);
  } else {
    const unsigned tiles = (unsigned)(upad / F64_DEV_TILE) * (unsigned)((nf + F64_DEV_TILE - 1) / F64_DEV_TILE);
    hipLaunchKernelGGL((fp64_bisil_gather_lds_kernel<DT>), dim3(tiles), dim3(256), 0, st, src, ps, fs, feat, nf, pts, n_u, upad, G);
  }
}
// side sd of x: the points are its rows (sd = 0) or its columns
inline void fp64_bisil_gather(hipStream_t st, const resnmtf_device_matrix& x, int sd, const int* feat, int nf, const int* pts,
                              int n_u, int upad, double* G) {
  const size_t ps = (size_t)(sd == 0 ? x.row_stride : x.col_stride), fs = (size_t)(sd == 0 ? x.col_stride : x.row_stride);
  const int form = f64_bisil_side_form(sd, x.row_stride, x.col_stride);
  switch (x.dtype) {
    case RESNMTF_DTYPE_F64: f64_bisil_launch_gather<RESNMTF_DTYPE_F64>(st, form, x.ptr, ps, fs, feat, nf, pts, n_u, upad, G); break;
    case RESNMTF_DTYPE_F32: f64_bisil_launch_gather<RESNMTF_DTYPE_F32>(st, form, x.ptr, ps, fs, feat, nf, pts, n_u, upad, G); break;
    case RESNMTF_DTYPE_F16: f64_bisil_launch_gather<RESNMTF_DTYPE_F16>(st, form, x.ptr, ps, fs, feat, nf, pts, n_u, upad, G); break;
    default: f64_bisil_launch_gather<RESNMTF_DTYPE_BF16>(st, form, x.ptr, ps, fs, feat, nf, pts, n_u, upad, G); break;
  }
}

struct F64BisilDistArgs {
  const double* G; int nf, upad, n_u; const int* mpos; int n_mem; const unsigned long long* umask; const double* norm2;
  int K, chunk_tiles; double* partial;
};
template <int METRIC, int KQ>
void f64_bisil_launch_dist_kq(dim3 grid, hipStream_t st, const F64BisilDistArgs& a) {
  hipLaunchKernelGGL((fp64_bisil_dist_kernel<METRIC, KQ>), grid, dim3(F64_BISIL_THREADS), 0, st, a.G, a.nf, a.upad, a.n_u, a.mpos,
                     a.n_mem, a.umask, a.norm2, a.K, a.chunk_tiles, a.partial);
}
template <int METRIC>
void f64_bisil_launch_dist_m(int kq, dim3 grid, hipStream_t st, const double* G, int nf, int upad, int n_u, const int* mpos,
                             int n_mem, const unsigned long long* umask, const double* norm2, int K, int chunk_tiles,
                             double* partial) {
  const F64BisilDistArgs a{G, nf, upad, n_u, mpos, n_mem, umask, norm2, K, chunk_tiles, partial};
  switch (kq) {                               // (bisil_kq gives no other value)
    case 1: f64_bisil_launch_dist_kq<METRIC, 1>(grid, st, a); break;
    case 2: f64_bisil_launch_dist_kq<METRIC, 2>(grid, st, a); break;
    case 4: f64_bisil_launch_dist_kq<METRIC, 4>(grid, st, a); break;
    case 8: f64_bisil_launch_dist_kq<METRIC, 8>(grid, st, a); break;
    case 16: f64_bisil_launch_dist_kq<METRIC, 16>(grid, st, a); break;
    default: break;
  }
}
inline void fp64_bisil_dist(int metric, int kq, dim3 grid, hipStream_t st, const double* G, int nf, int upad, int n_u,
                            const int* mpos, int n_mem, const unsigned long long* umask, const double* norm2, int K,
                            int chunk_tiles, double* partial) {
  if (metric == F64_BISIL_EUCLIDEAN) f64_bisil_launch_dist_m<F64_BISIL_EUCLIDEAN>(kq, grid, st, G, nf, upad, n_u, mpos, n_mem, umask, norm2, K, chunk_tiles, partial);
  else if (metric == F64_BISIL_MANHATTAN) f64_bisil_launch_dist_m<F64_BISIL_MANHATTAN>(kq, grid, st, G, nf, upad, n_u, mpos, n_mem, umask, norm2, K, chunk_tiles, partial);
  else f64_bisil_launch_dist_m<F64_BISIL_COSINE>(kq, grid, st, G, nf, upad, n_u, mpos, n_mem, umask, norm2, K, chunk_tiles, partial);
}
