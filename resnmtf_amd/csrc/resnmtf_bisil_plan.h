// The host-only half of a bisilhouette call (DESIGN.md sections 13 and 26): what depends on nothing but the shapes, the
// 0 / 1 cluster matrices and the strides.  No HIP: it compiles with a plain C++17 compiler against include/resnmtf_hip.h
// alone, which is how tests/host/fp64_bisil_check.cpp runs it.  Two translation units include it and so share one
// statement of
//   - the index lists of a call (bisil_build_lists): the membership words, the member counts, the active biclusters, per
//     side the union U, its masks and every bicluster's members as positions in U, and through them its features;
//   - the chunk rule (bisil_chunk_rule) and the kq table (bisil_kq) of the distance kernel;
// resnmtf_hip.hip (resnmtf_bisil, resnmtf_bisil_sparse: the fp32 images) and resnmtf_fp64.hip (resnmtf_fp64_bisil: X read
// where it lies, every value carried in fp64), which adds its workspace (f64_bisil_plan) and the choice of its gather
// kernel (f64_bisil_gather_form), and resnmtf_fp64_bisil_sparse's rank tables (f64_bisil_ranks) and workspace
// (f64_bisil_sparse_plan; section 29).
#ifndef RESNMTF_BISIL_PLAN_H
#define RESNMTF_BISIL_PLAN_H

#include <algorithm>
#include <cstddef>
#include <cstring>
#include <vector>

#include "resnmtf_hip.h"

constexpr int BISIL_PLAN_TILE = 64;          // members per workgroup = others per distance tile (BISIL_TILE)
constexpr int BISIL_PLAN_WORKGROUPS = 2048;  // workgroups one distance launch aims for (a constant: never the device's)

// kq = ceil(K / 4) rounded up to a power of two: the per-thread bicluster sums of the distance kernel
inline int bisil_kq(int k) { return k <= 4 ? 1 : k <= 8 ? 2 : k <= 16 ? 4 : k <= 32 ? 8 : 16; }

// One side of one active bicluster: the others (U, n_u points) are split into chunks of whole 64-wide tiles, enough of
// them to fill the device with the bicluster's ceil(n_mem / 64) member tiles; the chunk partials are summed in chunk
// order later.  A function of the two counts alone.
// (tests/test_gpu_bisil_forms.py restates this rule and the kq table above: change them together)
struct BisilChunks { int chunk_tiles, chunks; };
inline BisilChunks bisil_chunk_rule(int n_u, int n_mem) {
  const int tiles_u = (n_u + BISIL_PLAN_TILE - 1) / BISIL_PLAN_TILE, tiles_m = (n_mem + BISIL_PLAN_TILE - 1) / BISIL_PLAN_TILE;
  const int want = std::max(1, std::min(tiles_u, (BISIL_PLAN_WORKGROUPS + tiles_m - 1) / tiles_m));
  BisilChunks c;
  c.chunk_tiles = (tiles_u + want - 1) / want;
  c.chunks = (tiles_u + c.chunk_tiles - 1) / c.chunk_tiles;
  return c;
}

// one side of a call: points = rows (features = columns) or the reverse; every list is 0-based
struct BisilHostSide {
  int n_pts = 0;
  std::vector<int> upts;                      // U: the points in an active bicluster, ascending
  std::vector<unsigned long long> umask;      // their active-bicluster bits
  std::vector<std::vector<int>> mpos;         // per bicluster: its members as positions in U, ascending
  std::vector<int> cnt;                       // per bicluster: its members, active or not
};
struct BisilHostLists {
  unsigned long long active = 0ull;           // biclusters with rows and columns
  BisilHostSide side[2];                      // [0] rows, [1] columns
  // per side: the features of bicluster j are the other side's members of j, as point indices
  std::vector<int> features(int sd, int j) const {
    std::vector<int> f;
    const BisilHostSide& o = side[1 - sd];
    for (int p : o.mpos[j]) f.push_back(o.upts[p]);
    return f;
  }
};

// The lists of row_clusters (n x k) and col_clusters (m x k), column-major 0 / 1.  Returns 0, or which matrix holds the
// first entry other than 0 or 1 in bicluster order, the rows of a bicluster before its columns: 1 = row_clusters,
// 2 = col_clusters (NaN is refused, -0.0 is 0); `out` is then unspecified.
inline int bisil_build_lists(int n, int m, int k, const double* row_clusters, const double* col_clusters, BisilHostLists& out) {
  std::vector<unsigned long long> bits[2] = {std::vector<unsigned long long>((size_t)n, 0ull), std::vector<unsigned long long>((size_t)m, 0ull)};
  std::vector<int> count[2] = {std::vector<int>((size_t)k, 0), std::vector<int>((size_t)k, 0)};
  for (int j = 0; j < k; ++j) {
    for (int r = 0; r < n; ++r) {
      const double x = row_clusters[(size_t)j * n + r];
      if (x != 0.0 && x != 1.0) return 1;
      if (x != 0.0) { bits[0][r] |= 1ull << j; ++count[0][j]; }
    }
    for (int c = 0; c < m; ++c) {
      const double x = col_clusters[(size_t)j * m + c];
      if (x != 0.0 && x != 1.0) return 2;
      if (x != 0.0) { bits[1][c] |= 1ull << j; ++count[1][j]; }
    }
  }
  out.active = 0ull;
  for (int j = 0; j < k; ++j) if (count[0][j] > 0 && count[1][j] > 0) out.active |= 1ull << j;
  for (int sd = 0; sd < 2; ++sd) {
    BisilHostSide& s = out.side[sd];
    s = BisilHostSide();
    s.n_pts = sd == 0 ? n : m; s.cnt = count[sd]; s.mpos.resize((size_t)k);
    for (int p = 0; p < s.n_pts; ++p) {
      const unsigned long long b = bits[sd][p] & out.active;
      if (!b) continue;
      for (int j = 0; j < k; ++j) if ((b >> j) & 1ull) s.mpos[j].push_back((int)s.upts.size());
      s.upts.push_back(p); s.umask.push_back(b);
    }
  }
  return 0;
}

// ---- resnmtf_fp64_bisil ----

// Which gather kernel builds G[f][u] = X(U[u], J[f]) for a side whose points lie `pt_stride` elements apart in the
// source and whose features `ft_stride`: lanes along the points when the point stride is the smaller (a tie: the
// points), else a 32 x 32 tile through LDS, read with lanes along the features.  From the strides alone.
enum { F64_BISIL_GATHER_POINTS = 0, F64_BISIL_GATHER_LDS = 1 };
inline int f64_bisil_gather_form(long long pt_stride, long long ft_stride) {
  return pt_stride <= ft_stride ? F64_BISIL_GATHER_POINTS : F64_BISIL_GATHER_LDS;
}
// side 0: the points are rows; side 1: columns
inline int f64_bisil_side_form(int sd, long long row_stride, long long col_stride) {
  return sd == 0 ? f64_bisil_gather_form(row_stride, col_stride) : f64_bisil_gather_form(col_stride, row_stride);
}

// The sizes of one call, from the counts (n_u: |U| per side; cnt[sd][j]: the members of bicluster j on side sd) and the
// shapes, and the layout of its one device buffer, in doubles from its start:
//   [g: G, the largest |J_l| x U_pad block][norm2: U_pad][partial: chunks x members x k of one bicluster]
//   [sil: n k, then m k][meta: the lists, 8-byte words][x: n m, a host X alone]
struct F64BisilPlan {
  size_t g_dbl = 1, part_dbl = 1, upad_max = BISIL_PLAN_TILE;
  int chunks[2][RESNMTF_MAX_K] = {}, chunk_tiles[2][RESNMTF_MAX_K] = {};
  int kq = 1;
  size_t norm2 = 0, partial = 0, sil = 0, meta = 0, x = 0, total = 0;       // offsets, and the size of the buffer
};
inline void f64_bisil_plan(int n, int m, int k, unsigned long long active, const int n_u[2], const int* const cnt[2],
                           size_t meta_words, bool host_x, F64BisilPlan& p) {
  p = F64BisilPlan();
  for (int sd = 0; sd < 2; ++sd) {
    const size_t upad = (size_t)(n_u[sd] + BISIL_PLAN_TILE - 1) / BISIL_PLAN_TILE * BISIL_PLAN_TILE;
    p.upad_max = std::max(p.upad_max, upad);
    for (int j = 0; j < k; ++j) {
      if (!((active >> j) & 1ull)) continue;
      const BisilChunks c = bisil_chunk_rule(n_u[sd], cnt[sd][j]);
      p.chunk_tiles[sd][j] = c.chunk_tiles;
      p.chunks[sd][j] = c.chunks;
      p.g_dbl = std::max(p.g_dbl, (size_t)cnt[1 - sd][j] * upad);
      p.part_dbl = std::max(p.part_dbl, (size_t)c.chunks * cnt[sd][j] * k);
    }
  }
  p.kq = bisil_kq(k);
  p.norm2 = p.g_dbl;
  p.partial = p.norm2 + p.upad_max;
  p.sil = p.partial + p.part_dbl;
  p.meta = p.sil + (size_t)n * k + (size_t)m * k;
  p.x = p.meta + meta_words;
  p.total = p.x + (host_x ? (size_t)n * m : 0);
}

// The lists as the device holds them: 8-byte words [umask rows | umask columns | ints], the ints per side [upts | cnt |
// per active j: mpos_j | feat_j]; the offsets count words (mask) and ints from the buffer's start (the rest).
struct F64BisilMeta {
  std::vector<unsigned long long> words;
  size_t mask[2] = {}, pts[2] = {}, cnt[2] = {}, mpos[2][RESNMTF_MAX_K] = {}, feat[2][RESNMTF_MAX_K] = {};
};
inline void f64_bisil_pack(int k, const BisilHostLists& L, F64BisilMeta& M) {
  M = F64BisilMeta();
  std::vector<int> ints;
  auto put = [&](const std::vector<int>& a) { const size_t o = ints.size(); ints.insert(ints.end(), a.begin(), a.end()); return o; };
  const size_t n_mask = L.side[0].umask.size() + L.side[1].umask.size();
  for (int sd = 0; sd < 2; ++sd) {
    const BisilHostSide& s = L.side[sd];
    M.pts[sd] = 2 * n_mask + put(s.upts);
    M.cnt[sd] = 2 * n_mask + put(s.cnt);
    for (int j = 0; j < k; ++j) {
      if (!((L.active >> j) & 1ull)) continue;
      M.mpos[sd][j] = 2 * n_mask + put(s.mpos[j]);
      M.feat[sd][j] = 2 * n_mask + put(L.features(sd, j));
    }
  }
  if (ints.size() % 2) ints.push_back(0);
  M.words.resize(n_mask + ints.size() / 2);
  M.mask[0] = 0; M.mask[1] = L.side[0].umask.size();
  std::copy(L.side[0].umask.begin(), L.side[0].umask.end(), M.words.begin());
  std::copy(L.side[1].umask.begin(), L.side[1].umask.end(), M.words.begin() + M.mask[1]);
  if (!ints.empty()) std::memcpy(M.words.data() + n_mask, ints.data(), ints.size() * sizeof(int));
}

// ---- resnmtf_fp64_bisil_sparse ----

// The rank tables of the scatter, n + m ints, the rows' table first: rank[p] = the position of point p in U of its
// side, or -1 when p is in no active bicluster.
inline void f64_bisil_ranks(const BisilHostLists& L, std::vector<int>& rank) {
  const size_t n = (size_t)L.side[0].n_pts, m = (size_t)L.side[1].n_pts;
  rank.assign(n + m, -1);
  for (int sd = 0; sd < 2; ++sd) {
    int* r = rank.data() + (sd == 0 ? 0 : n);
    const std::vector<int>& u = L.side[sd].upts;
    for (size_t i = 0; i < u.size(); ++i) r[u[i]] = (int)i;
  }
}

// The one device buffer of a sparse call, in doubles from its start: the dense call's regions without a copy of X
// (`dense`: G, norm2, partial, sil, meta), then
//   [rank: n + m ints, rows first][cptr: m + 1 int64][cval: nnz][cidx: nnz ints][rptr: n + 1 int64][rval: nnz][ridx: nnz ints]
// -- the CSC and the CSR copy of X as section 22 stores a sparse view: 24 bytes per stored entry plus the pointers.
struct F64BisilSparsePlan {
  F64BisilPlan dense;
  size_t rank = 0, cptr = 0, cval = 0, cidx = 0, rptr = 0, rval = 0, ridx = 0, total = 0;   // offsets, and the size of the buffer
  size_t copies_dbl = 0;                                                                   // of them the two sparse copies
};
inline void f64_bisil_sparse_plan(int n, int m, int k, unsigned long long active, const int n_u[2], const int* const cnt[2],
                                  size_t meta_words, size_t nnz, F64BisilSparsePlan& p) {
  p = F64BisilSparsePlan();
  f64_bisil_plan(n, m, k, active, n_u, cnt, meta_words, false, p.dense);
  const size_t idx_dbl = (nnz + 1) / 2;
  size_t off = p.dense.total;
  p.rank = off; off += ((size_t)n + (size_t)m + 1) / 2;
  p.cptr = off; off += (size_t)m + 1;
  p.cval = off; off += nnz;
  p.cidx = off; off += idx_dbl;
  p.rptr = off; off += (size_t)n + 1;
  p.rval = off; off += nnz;
  p.ridx = off; off += idx_dbl;
  p.total = off;
  p.copies_dbl = p.total - p.cptr;
}

#endif
