// resnmtf_bisil.hip.inc -- per-member silhouettes of a view's biclusters (resnmtf_bisil), the device side of the
// bisilhouette score that res_nmtf_inner reports as `bisil` (R/obtain_bicl.r:189-199) and that the k sweep of
// apply_resnmtf ranks (R/main.r:291-312).  Included by resnmtf_hip.hip; fp64 arithmetic over the fp32 image values.
// DESIGN.md section 13 holds the definition; this unit and resnmtf_amd/bisil.py are its only two statements.
// resnmtf_fp64_bisil.hip.inc (the fp64 unit, section 26) is this file's TWIN: the norm, distance and epilogue arithmetic
// stated a second time over a `double` G.  A change to the arithmetic here is a change there.
//
// One side (rows, or columns with the roles swapped) of one active bicluster k is three or four launches:
//   bisil_gather_kernel   G[f][u] = X(U[u], J_k[f]) as fp32, feature-major [|J_k|][U_pad]: U = the union of the active
//                         biclusters' members (the only points a silhouette compares with), zero-padded to 64.
//                         A sparse view (resnmtf_bisil_sparse) has no image: G is zero-filled and bisil_scatter_kernel
//                         writes the stored entries of the feature lines (CSC columns / CSR rows) that fall in U --
//                         the same fp32 values at the same places, so everything below gives the same bits.
//   bisil_norm_kernel     (cosine) ||G[:, u]||^2 in fp64, features in ascending order.
//   bisil_dist_kernel     one workgroup per (64 members of I_k) x (one chunk of U's 64-wide tiles): a 64 x 64 distance
//                         tile on fp64 VALU (4 x 4 per thread over a 32-feature LDS stage), then contracted at once with
//                         the 0/1 membership bits of the 64 others: every member keeps its K per-bicluster sums in
//                         registers (K / 4 per thread).  The member itself is skipped by index, so d(i, i) never enters.
//   bisil_epilogue_kernel one wave per member: the chunk partials summed in chunk order (a lane per bicluster), a,
//                         b and s.
// Determinism: every sum has an order fixed by the shapes and the clusters alone (features ascending, tiles ascending
// inside a chunk, chunks ascending), no atomics -- two calls give bitwise equal silhouettes.

namespace {

constexpr int BISIL_TILE = 64;        // members per workgroup = others per distance tile
constexpr int BISIL_FT = 32;          // features per LDS stage
constexpr int BISIL_THREADS = 256;
enum { BISIL_EUCLIDEAN = 0, BISIL_MANHATTAN = 1, BISIL_COSINE = 2 };

// G[f * upad + u] = img(pts[u], feat[f]) for u < n_u, 0 for n_u <= u < upad; img is tile-major with stride ld
// (the row side reads Xt32 (column feat, row pts), the column side X32 (row feat, column pts): xidx(feat, pts, ld))
__global__ void __launch_bounds__(256)
bisil_gather_kernel(const float* __restrict__ img, size_t ld, const int* __restrict__ feat, int nf,
                    const int* __restrict__ pts, int n_u, int upad, float* __restrict__ G) {
  const size_t total = (size_t)nf * upad;
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
    const int f = (int)(e / upad), u = (int)(e % upad);
    G[e] = u < n_u ? img[xidx(feat[f], pts[u], ld)] : 0.f;
  }
}

// sparse views: G (zero-filled by the caller) [f * upad + rank[idx[e]]] = val[e] over the stored entries e of line
// feat[f] whose point is in U (rank >= 0, the position in U; < upad).  ptr / idx / val: the CSC (row side: lines are
// columns, idx rows) or the CSR (column side).  One wave per feature line, lanes striding its entries -- a dense line
// among sparse ones costs its own wave len / 64 steps, not one thread len steps; indices are strictly increasing within
// a line (checked at upload), so no two lanes write one element.
__global__ void __launch_bounds__(BISIL_THREADS)
bisil_scatter_kernel(const long long* __restrict__ ptr, const int* __restrict__ idx, const float* __restrict__ val,
                     const int* __restrict__ feat, int nf, const int* __restrict__ rank, int upad, float* __restrict__ G) {
  const int lane = threadIdx.x & 63;
  const int waves = BISIL_THREADS / 64;
  for (int f = blockIdx.x * waves + (threadIdx.x >> 6); f < nf; f += (int)gridDim.x * waves) {
    const int line = feat[f];
    const long long p1 = ptr[line + 1];
    float* __restrict__ g = G + (size_t)f * upad;
    for (long long e = ptr[line] + lane; e < p1; e += 64) {
      const int r = rank[idx[e]];
      if (r >= 0) g[r] = val[e];
    }
  }
}

__global__ void __launch_bounds__(256)
bisil_norm_kernel(const float* __restrict__ G, int nf, int upad, double* __restrict__ norm2) {
  const int u = blockIdx.x * 256 + threadIdx.x;
  if (u >= upad) return;
  double s = 0.0;
  for (int f = 0; f < nf; ++f) { const double x = (double)G[(size_t)f * upad + u]; s = fma(x, x, s); }
  norm2[u] = s;
}

struct BisilShared {
  union {
    struct { double a[BISIL_FT][BISIL_TILE]; double b[BISIL_FT][BISIL_TILE]; } f;   // member / other features
    double d[BISIL_TILE][BISIL_TILE + 1];                                             // distance tile (padded rows)
  };
  unsigned long long msk[BISIL_TILE];   // membership bits of the tile's others
  int mp[BISIL_TILE];                   // the workgroup's members as positions in U
};

// partial[((chunk * n_mem) + member) * K + l] = sum of d(member, u) over the u of this chunk with bit l set, u != member
template <int METRIC, int KQ>
__global__ void __launch_bounds__(BISIL_THREADS)
bisil_dist_kernel(const float* __restrict__ G, int nf, int upad, int n_u, const int* __restrict__ mpos, int n_mem,
                  const unsigned long long* __restrict__ umask, const double* __restrict__ norm2, int K,
                  int chunk_tiles, double* __restrict__ partial) {
  __shared__ BisilShared sh;
  const int t = threadIdx.x;
  const int m0 = blockIdx.x * BISIL_TILE;
  const int chunk = blockIdx.y;
  const int tile_beg = chunk * chunk_tiles;
  const int tile_end = min(upad / BISIL_TILE, tile_beg + chunk_tiles);
  if (t < BISIL_TILE) sh.mp[t] = m0 + t < n_mem ? mpos[m0 + t] : 0;   // (out-of-range members: position 0, discarded)
  const int tm = t & 15, to = t >> 4;                                  // distances: members tm + 16 a, others to + 16 b
  const int ci = t >> 2, cq = t & 3;                                   // contraction: member ci, biclusters cq + 4 s
  double sums[KQ];
#pragma unroll
  for (int s = 0; s < KQ; ++s) sums[s] = 0.0;
  __syncthreads();
  for (int tile = tile_beg; tile < tile_end; ++tile) {
    const int u0 = tile * BISIL_TILE;
    double acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b = 0; b < 4; ++b) acc[a][b] = 0.0;
    for (int f0 = 0; f0 < nf; f0 += BISIL_FT) {
#pragma unroll
      for (int r = 0; r < BISIL_FT * BISIL_TILE / BISIL_THREADS; ++r) {
        const int e = t + r * BISIL_THREADS, f = e >> 6, c = e & 63;
        const bool in = f0 + f < nf;
        const size_t row = (size_t)min(f0 + f, nf - 1) * upad;     // (clamped: every load stays inside G)
        sh.f.a[f][c] = in ? (double)G[row + sh.mp[c]] : 0.0;
        sh.f.b[f][c] = in ? (double)G[row + u0 + c] : 0.0;
      }
      __syncthreads();
#pragma unroll 4
      for (int f = 0; f < BISIL_FT; ++f) {
        double xa[4], xb[4];
#pragma unroll
        for (int a = 0; a < 4; ++a) xa[a] = sh.f.a[f][tm + 16 * a];
#pragma unroll
        for (int b = 0; b < 4; ++b) xb[b] = sh.f.b[f][to + 16 * b];
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
          for (int b = 0; b < 4; ++b) {
            if (METRIC == BISIL_EUCLIDEAN) { const double df = xa[a] - xb[b]; acc[a][b] = fma(df, df, acc[a][b]); }
            else if (METRIC == BISIL_MANHATTAN) acc[a][b] += fabs(xa[a] - xb[b]);
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
        if (METRIC == BISIL_EUCLIDEAN) d = sqrt(fmax(acc[a][b], 0.0));
        else if (METRIC == BISIL_MANHATTAN) d = acc[a][b];
        else {
          const double na = norm2[pa], nb = norm2[u];
          if (na == 0.0 && nb == 0.0) d = 0.0;
          else if (na == 0.0 || nb == 0.0) d = 1.0;
          else d = 1.0 - acc[a][b] / (sqrt(na) * sqrt(nb));
        }
        sh.d[ma][ob] = (u == pa || u >= n_u) ? 0.0 : d;
      }
    }
    if (t < BISIL_TILE) sh.msk[t] = u0 + t < n_u ? umask[u0 + t] : 0ull;
    __syncthreads();
    for (int u = 0; u < BISIL_TILE; ++u) {
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
__global__ void __launch_bounds__(256)
bisil_epilogue_kernel(const double* __restrict__ partial, int n_chunks, int n_mem, int K, int k,
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

// (the host's lists of a call -- U, the masks, every bicluster's members and features -- are BisilHostLists,
// resnmtf_bisil_plan.h, shared with resnmtf_fp64_bisil)
static_assert(BISIL_TILE == BISIL_PLAN_TILE, "the chunk rule of resnmtf_bisil_plan.h counts this kernel's tiles");

template <int METRIC>
void bisil_launch_dist_m(int kq, dim3 grid, hipStream_t st, const float* G, int nf, int upad, int n_u, const int* mpos,
                         int n_mem, const unsigned long long* umask, const double* norm2, int K, int chunk_tiles,
                         double* partial) {
  switch (kq) {
#define BISIL_CASE(KQ) case KQ: hipLaunchKernelGGL((bisil_dist_kernel<METRIC, KQ>), grid, dim3(BISIL_THREADS), 0, st, G, nf, \
                                                   upad, n_u, mpos, n_mem, umask, norm2, K, chunk_tiles, partial); break;
    BISIL_CASE(1) BISIL_CASE(2) BISIL_CASE(4) BISIL_CASE(8) BISIL_CASE(16)
#undef BISIL_CASE
    default: break;
  }
}

// kq = ceil(K / 4) rounded up to a power of two: the per-thread bicluster sums of bisil_dist_kernel
void bisil_launch_dist(int metric, int kq, dim3 grid, hipStream_t st, const float* G, int nf, int upad, int n_u,
                       const int* mpos, int n_mem, const unsigned long long* umask, const double* norm2, int K,
                       int chunk_tiles, double* partial) {
  if (metric == BISIL_EUCLIDEAN) bisil_launch_dist_m<BISIL_EUCLIDEAN>(kq, grid, st, G, nf, upad, n_u, mpos, n_mem, umask, norm2, K, chunk_tiles, partial);
  else if (metric == BISIL_MANHATTAN) bisil_launch_dist_m<BISIL_MANHATTAN>(kq, grid, st, G, nf, upad, n_u, mpos, n_mem, umask, norm2, K, chunk_tiles, partial);
  else bisil_launch_dist_m<BISIL_COSINE>(kq, grid, st, G, nf, upad, n_u, mpos, n_mem, umask, norm2, K, chunk_tiles, partial);
}

// ---- resnmtf_bisil_device (DESIGN.md section 19): the cluster matrices are in device memory, so the lists above are
// built there, each in the order bisil_impl builds it on the host, and the score is combined there too.
//   bisil_words_kernel        one wave per 64 points: the u64 membership word of every point (bit j = entry (p, j) != 0),
//                             the refusal bit of an entry other than 0 / 1 (x != 0.0 && x != 1.0: NaN is refused, -0.0 is
//                             0) and the member counts of the k biclusters (integer atomics: exact in any order).  A
//                             source whose row stride is the smaller is read with lanes along the points, any other with
//                             lanes along the biclusters and a ballot per point.
//   bisil_union_kernel        one workgroup per side: the active mask from the counts, then U as an ordered compaction
//                             of the points with an active bit -- upts ascending, umask, (sparse) rank -- and |U|.
//   bisil_members_kernel      one workgroup per (active bicluster j, side): the ordered compaction of U's positions with
//                             bit j (mpos_j, ascending) and, through upts, of those points (the other side's feat_j).
//   bisil_member_mean_kernel  one workgroup per (active bicluster, side): the members' silhouettes gathered in ascending
//                             point order, then their mean in NumPy's order (bisil_np_sum) by one thread.
//   bisil_score_kernel        sigma_l = 0.5 (row mean + column mean) per active l, their mean in NumPy's order; 0 with
//                             fewer than two active biclusters: bisil.view_score, bit for bit.
// The compactions are chunked scans inside one workgroup (bisil_scan_step: a ballot per wave, the wave totals through
// LDS): positions depend on the flags alone.  No spins, no waits between workgroups, no floating-point atomics.
// Every kernel here is a template (<int UNUSED> where it has no parameter of its own): instantiations are emitted after
// the existing code, so no existing kernel is displaced in the code object (profiles/kernel_fingerprint.txt).

constexpr int BISIL_SCAN_THREADS = 1024;
constexpr int BISIL_NP_BLOCK = 8192;      // NumPy reduces a long 1-D array in buffers of 8192 entries, summed in order

// hdr, the ints the host reads back: [0] the refusal bits (1: the row matrix, 2: the column matrix), [1] |U| of the rows,
// [2] of the columns, [3 .. 3 + k) the row counts, [3 + k .. 3 + 2 k) the column counts
constexpr int BISIL_HDR_COUNTS = 3;

struct BisilSideMeta {                    // one side's arrays in device memory
  const unsigned long long* words;        // [n_pts]
  int n_pts;
  unsigned long long* umask;              // [n_pts] (|U| used)
  int* upts;                              // [n_pts] (|U| used)
  int* rank;                              // [n_pts] or NULL (dense views)
};

struct BisilOffsets {                     // per side and bicluster: where its lists start (ints of `lists`, doubles of `vals`)
  int mpos[2][RESNMTF_MAX_K];
  int feat[2][RESNMTF_MAX_K];
  int val[2][RESNMTF_MAX_K];
};

template <int DT, bool ALONG_R>
__global__ void __launch_bounds__(256)
bisil_words_kernel(const void* __restrict__ src, long long rs, long long cs, int len, int k, int bad_bit,
                   unsigned long long* __restrict__ words, int* __restrict__ count, int* __restrict__ refusal) {
  const int lane = threadIdx.x & 63;
  const long long p0 = ((long long)blockIdx.x * 4 + (threadIdx.x >> 6)) * 64;
  if (p0 >= len) return;                                   // (the whole wave)
  unsigned long long word = 0ull;
  bool bad = false;
  if constexpr (ALONG_R) {
    const long long p = p0 + lane;
    if (p < len)
      for (int j = 0; j < k; ++j) {
        const double x = load_wide<DT>(src, p * rs + (long long)j * cs);
        bad |= x != 0.0 && x != 1.0;
        word |= (unsigned long long)(x != 0.0) << j;
      }
  } else {
    for (int i = 0; i < 64; ++i) {
      const long long p = p0 + i;
      double x = 0.0;
      if (p < len && lane < k) x = load_wide<DT>(src, p * rs + (long long)lane * cs);
      bad |= x != 0.0 && x != 1.0;
      const unsigned long long b = __ballot(x != 0.0);
      if (lane == i) word = b;
    }
  }
  if (__ballot(bad) != 0ull && lane == 0) atomicOr(refusal, bad_bit);
  if (p0 + lane < len) words[p0 + lane] = word;
  int mine = 0;
  for (int j = 0; j < k; ++j) {
    const int c = __popcll(__ballot((word >> j) & 1ull));
    if (lane == j) mine = c;
  }
  if (mine > 0) atomicAdd(count + lane, mine);
}

// one step of a workgroup's ordered compaction (every thread calls it): the position of this thread's element among
// the flagged ones, `running` advanced by the step's count
__device__ __forceinline__ int bisil_scan_step(bool flag, int& running, int* __restrict__ wsum) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const unsigned long long b = __ballot(flag);
  if (lane == 0) wsum[w] = __popcll(b);
  __syncthreads();
  int before = 0, total = 0;
  for (int i = 0; i < BISIL_SCAN_THREADS / 64; ++i) {
    const int c = wsum[i];
    if (i < w) before += c;
    total += c;
  }
  __syncthreads();                                         // (wsum is written again by the next step)
  const int pos = running + before + __popcll(b & ((1ull << lane) - 1ull));
  running += total;
  return pos;
}

template <int UNUSED>
__global__ void __launch_bounds__(BISIL_SCAN_THREADS)
bisil_union_kernel(BisilSideMeta rows, BisilSideMeta cols, int k, int* __restrict__ hdr) {
  __shared__ int wsum[BISIL_SCAN_THREADS / 64];
  __shared__ unsigned long long active_s;
  if (hdr[0] != 0) return;                                 // refused: nothing is built
  const BisilSideMeta s = blockIdx.x == 0 ? rows : cols;
  const int t = threadIdx.x;
  if (t < 64) {
    const bool on = t < k && hdr[BISIL_HDR_COUNTS + t] > 0 && hdr[BISIL_HDR_COUNTS + k + t] > 0;
    const unsigned long long a = __ballot(on);
    if (t == 0) active_s = a;
  }
  __syncthreads();
  const unsigned long long active = active_s;
  int running = 0;
  for (int base = 0; base < s.n_pts; base += BISIL_SCAN_THREADS) {
    const int p = base + t;
    const unsigned long long b = p < s.n_pts ? s.words[p] & active : 0ull;
    const int pos = bisil_scan_step(b != 0ull, running, wsum);
    if (b != 0ull) { s.upts[pos] = p; s.umask[pos] = b; }
    if (s.rank && p < s.n_pts) s.rank[p] = b != 0ull ? pos : -1;
  }
  if (t == 0) hdr[1 + blockIdx.x] = running;
}

template <int UNUSED>
__global__ void __launch_bounds__(BISIL_SCAN_THREADS)
bisil_members_kernel(const unsigned long long* __restrict__ umask_r, const int* __restrict__ upts_r, int n_u_r,
                     const unsigned long long* __restrict__ umask_c, const int* __restrict__ upts_c, int n_u_c,
                     unsigned long long active, BisilOffsets off, int* __restrict__ lists) {
  __shared__ int wsum[BISIL_SCAN_THREADS / 64];
  const int j = blockIdx.x, sd = blockIdx.y, t = threadIdx.x;
  if (!((active >> j) & 1ull)) return;
  const unsigned long long* __restrict__ umask = sd == 0 ? umask_r : umask_c;
  const int* __restrict__ upts = sd == 0 ? upts_r : upts_c;
  const int n_u = sd == 0 ? n_u_r : n_u_c;
  int* __restrict__ mpos = lists + off.mpos[sd][j];
  int* __restrict__ feat = lists + off.feat[1 - sd][j];    // this side's members are the other side's features
  int running = 0;
  for (int base = 0; base < n_u; base += BISIL_SCAN_THREADS) {
    const int u = base + t;
    const bool in = u < n_u && ((umask[u] >> j) & 1ull);
    const int pos = bisil_scan_step(in, running, wsum);
    if (in) { mpos[pos] = u; feat[pos] = upts[u]; }
  }
}

// ndarray.mean()'s sum of a contiguous 1-D fp64 array: buffers of 8192 entries, each summed pairwise
// (jsd_np_pairwise, resnmtf_jsd.hip.inc), the buffer sums added in order; tests/test_post_on_device_host.py restates it
__device__ double bisil_np_sum(const double* a, long long n) {
  double s = jsd_np_pairwise<8>(a, n < BISIL_NP_BLOCK ? n : (long long)BISIL_NP_BLOCK);
  for (long long i = BISIL_NP_BLOCK; i < n; i += BISIL_NP_BLOCK)
    s += jsd_np_pairwise<8>(a + i, n - i < BISIL_NP_BLOCK ? n - i : (long long)BISIL_NP_BLOCK);
  return s;
}

// sil: [n k] row silhouettes then [m k] column silhouettes, column-major; cnt: [k] row counts then [k] column counts
template <int UNUSED>
__global__ void __launch_bounds__(256)
bisil_member_mean_kernel(const double* __restrict__ sil, int n, int m, int k, const int* __restrict__ cnt,
                         unsigned long long active, BisilOffsets off, const int* __restrict__ lists,
                         double* __restrict__ vals, double* __restrict__ means) {
  const int j = blockIdx.x, sd = blockIdx.y;
  if (!((active >> j) & 1ull)) return;
  const int c = cnt[sd * k + j], n_pts = sd == 0 ? n : m;
  const double* __restrict__ s = sil + (sd == 0 ? (size_t)0 : (size_t)n * k) + (size_t)j * n_pts;
  const int* __restrict__ pts = lists + off.feat[1 - sd][j];
  double* v = vals + off.val[sd][j];
  for (int i = threadIdx.x; i < c; i += 256) v[i] = s[pts[i]];
  __syncthreads();
  if (threadIdx.x == 0) means[sd * RESNMTF_MAX_K + j] = bisil_np_sum(v, c) / (double)c;
}

template <int UNUSED>
__global__ void __launch_bounds__(64)
bisil_score_kernel(const double* __restrict__ means, int k, unsigned long long active, double* __restrict__ score) {
  __shared__ double sigma[RESNMTF_MAX_K];
  if (threadIdx.x != 0) return;
  int n_act = 0;
  for (int l = 0; l < k; ++l)
    if ((active >> l) & 1ull) sigma[n_act++] = 0.5 * (means[l] + means[RESNMTF_MAX_K + l]);
  score[0] = n_act < 2 ? 0.0 : bisil_np_sum(sigma, n_act) / (double)n_act;
}

}  // namespace
