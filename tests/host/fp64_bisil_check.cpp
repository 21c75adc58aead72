// Stand-alone host check of csrc/resnmtf_bisil_plan.h: the index lists of a bisilhouette call,
// the chunk rule, the kq table, the choice of the gather kernel, the workspace of resnmtf_fp64_bisil and the packing of
// its lists, each against brute force.  No HIP call; built with a plain C++17 compiler by
// tests/test_fp64_bisil_check_host.py.  Exits non-zero at the first condition that does not hold.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <set>
#include <vector>

#include "resnmtf_bisil_plan.h"

#define CHECK(cond)                                                                 \
  do {                                                                              \
    if (!(cond)) {                                                                  \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);                 \
      std::exit(1);                                                                 \
    }                                                                               \
  } while (0)

namespace {
int ceil_div(int a, int b) { return (a + b - 1) / b; }

// the chunk rule by search: the smallest chunk length (in tiles) whose chunk count, times the member tiles, does not
// exceed what ceil(2048 / tiles_m) chunks would launch -- and never more chunks than tiles
void check_chunk_rule(int n_u, int n_mem) {
  const BisilChunks c = bisil_chunk_rule(n_u, n_mem);
  const int tiles_u = ceil_div(n_u, 64), tiles_m = ceil_div(n_mem, 64);
  int want = ceil_div(2048, tiles_m);
  if (want > tiles_u) want = tiles_u;
  if (want < 1) want = 1;
  int len = 1;
  while (ceil_div(tiles_u, len) > want) ++len;            // brute force: the first length that needs at most `want` chunks
  CHECK(c.chunk_tiles == len);
  CHECK(c.chunks == ceil_div(tiles_u, len));
  CHECK(c.chunks >= 1 && c.chunks <= tiles_u);
  CHECK((long long)c.chunks * c.chunk_tiles >= tiles_u);                  // the chunks cover U
  CHECK((long long)(c.chunks - 1) * c.chunk_tiles < tiles_u);             // and the last one is not empty
}

struct Clusters {
  int n, m, k;
  std::vector<double> rc, cc;
};

Clusters random_clusters(int n, int m, int k, double fill, unsigned seed, int empty_rows_of = -1, int empty_cols_of = -1) {
  std::mt19937 gen(seed);
  std::uniform_real_distribution<double> u(0.0, 1.0);
  Clusters c{n, m, k, std::vector<double>((size_t)n * k, 0.0), std::vector<double>((size_t)m * k, 0.0)};
  for (int j = 0; j < k; ++j) {
    for (int r = 0; r < n; ++r) c.rc[(size_t)j * n + r] = (j != empty_rows_of && u(gen) < fill) ? 1.0 : 0.0;
    for (int q = 0; q < m; ++q) c.cc[(size_t)j * m + q] = (j != empty_cols_of && u(gen) < fill) ? 1.0 : 0.0;
  }
  return c;
}

// the lists against their definition, entry by entry
void check_lists(const Clusters& c, bool host_x) {
  BisilHostLists L;
  CHECK(bisil_build_lists(c.n, c.m, c.k, c.rc.data(), c.cc.data(), L) == 0);
  const std::vector<double>* mat[2] = {&c.rc, &c.cc};
  const int len[2] = {c.n, c.m};
  unsigned long long active = 0ull;
  for (int j = 0; j < c.k; ++j) {
    bool any[2] = {false, false};
    for (int sd = 0; sd < 2; ++sd)
      for (int p = 0; p < len[sd]; ++p) any[sd] = any[sd] || (*mat[sd])[(size_t)j * len[sd] + p] != 0.0;
    if (any[0] && any[1]) active |= 1ull << j;
  }
  CHECK(L.active == active);
  for (int sd = 0; sd < 2; ++sd) {
    const BisilHostSide& s = L.side[sd];
    CHECK(s.n_pts == len[sd] && (int)s.cnt.size() == c.k && (int)s.mpos.size() == c.k);
    CHECK(s.upts.size() == s.umask.size());
    size_t u = 0;
    for (int p = 0; p < len[sd]; ++p) {                    // U: ascending, exactly the points with an active bit
      unsigned long long b = 0ull;
      for (int j = 0; j < c.k; ++j)
        if ((*mat[sd])[(size_t)j * len[sd] + p] != 0.0) b |= 1ull << j;
      b &= active;
      if (!b) continue;
      CHECK(u < s.upts.size() && s.upts[u] == p && s.umask[u] == b);
      ++u;
    }
    CHECK(u == s.upts.size());
    for (int j = 0; j < c.k; ++j) {
      int count = 0;
      for (int p = 0; p < len[sd]; ++p) count += (*mat[sd])[(size_t)j * len[sd] + p] != 0.0 ? 1 : 0;
      CHECK(s.cnt[j] == count);
      if (!((active >> j) & 1ull)) { CHECK(s.mpos[j].empty()); continue; }
      CHECK((int)s.mpos[j].size() == count);               // an active bicluster: every member is in U
      for (size_t i = 0; i < s.mpos[j].size(); ++i) {
        const int pos = s.mpos[j][i];
        CHECK(pos >= 0 && pos < (int)s.upts.size());
        CHECK(i == 0 || s.mpos[j][i - 1] < pos);
        CHECK((*mat[sd])[(size_t)j * len[sd] + s.upts[pos]] == 1.0);
      }
    }
  }
  for (int sd = 0; sd < 2; ++sd)                           // features: the other side's members as point indices
    for (int j = 0; j < c.k; ++j) {
      if (!((active >> j) & 1ull)) continue;
      const std::vector<int> f = L.features(sd, j);
      std::vector<int> want;
      for (int p = 0; p < len[1 - sd]; ++p)
        if ((*mat[1 - sd])[(size_t)j * len[1 - sd] + p] != 0.0) want.push_back(p);
      CHECK(f == want);
    }

  // the packed lists and the workspace: every region inside the buffer, disjoint, and large enough for its consumer
  F64BisilMeta M;
  f64_bisil_pack(c.k, L, M);
  const int n_u[2] = {(int)L.side[0].upts.size(), (int)L.side[1].upts.size()};
  const int* const cnt[2] = {L.side[0].cnt.data(), L.side[1].cnt.data()};
  F64BisilPlan P;
  f64_bisil_plan(c.n, c.m, c.k, active, n_u, cnt, M.words.size(), host_x, P);
  const int* ints = reinterpret_cast<const int*>(M.words.data());
  const size_t n_ints = 2 * M.words.size();
  std::set<size_t> used;                                   // ints of the packed lists, each claimed once
  auto claim = [&](size_t off, size_t count) {
    CHECK(off + count <= n_ints);
    for (size_t i = off; i < off + count; ++i) CHECK(used.insert(i).second);
  };
  for (int sd = 0; sd < 2; ++sd) {
    const BisilHostSide& s = L.side[sd];
    claim(2 * M.mask[sd], 2 * s.umask.size());
    for (size_t u = 0; u < s.umask.size(); ++u) CHECK(M.words[M.mask[sd] + u] == s.umask[u]);
    claim(M.pts[sd], s.upts.size());
    for (size_t u = 0; u < s.upts.size(); ++u) CHECK(ints[M.pts[sd] + u] == s.upts[u]);
    claim(M.cnt[sd], (size_t)c.k);
    for (int j = 0; j < c.k; ++j) CHECK(ints[M.cnt[sd] + j] == s.cnt[j]);
    for (int j = 0; j < c.k; ++j) {
      if (!((active >> j) & 1ull)) continue;
      const std::vector<int> f = L.features(sd, j);
      claim(M.mpos[sd][j], s.mpos[j].size());
      claim(M.feat[sd][j], f.size());
      for (size_t i = 0; i < f.size(); ++i) CHECK(ints[M.feat[sd][j] + i] == f[i]);
      for (size_t i = 0; i < s.mpos[j].size(); ++i) CHECK(ints[M.mpos[sd][j] + i] == s.mpos[j][i]);
    }
  }
  size_t g = 1, part = 1, upad_max = 64;
  for (int sd = 0; sd < 2; ++sd) {
    const size_t upad = (size_t)ceil_div(n_u[sd], 64) * 64;
    if (upad > upad_max) upad_max = upad;
    for (int j = 0; j < c.k; ++j) {
      if (!((active >> j) & 1ull)) continue;
      const BisilChunks ch = bisil_chunk_rule(n_u[sd], cnt[sd][j]);
      CHECK(P.chunks[sd][j] == ch.chunks && P.chunk_tiles[sd][j] == ch.chunk_tiles);
      CHECK(P.g_dbl >= (size_t)cnt[1 - sd][j] * upad);                       // G of this side and bicluster fits
      CHECK(P.part_dbl >= (size_t)ch.chunks * cnt[sd][j] * c.k);             // and so do its partials
      if ((size_t)cnt[1 - sd][j] * upad > g) g = (size_t)cnt[1 - sd][j] * upad;
      if ((size_t)ch.chunks * cnt[sd][j] * c.k > part) part = (size_t)ch.chunks * cnt[sd][j] * c.k;
    }
  }
  CHECK(P.g_dbl == g && P.part_dbl == part && P.upad_max == upad_max && P.kq == bisil_kq(c.k));
  const size_t sil = (size_t)c.n * c.k + (size_t)c.m * c.k;
  CHECK(P.norm2 == g && P.partial == P.norm2 + upad_max && P.sil == P.partial + part && P.meta == P.sil + sil);
  CHECK(P.x == P.meta + M.words.size());
  CHECK(P.total == P.x + (host_x ? (size_t)c.n * c.m : 0));
}
}  // namespace

int main() {
  // kq: ceil(K / 4) rounded up to a power of two
  for (int k = 1; k <= 64; ++k) {
    int q = 1;
    while (q < ceil_div(k, 4)) q *= 2;
    CHECK(bisil_kq(k) == q);
  }
  // the chunk rule over a grid of counts, the edges of a tile and the documented plans among them
  int rules = 0;
  for (int n_u : {1, 63, 64, 65, 127, 128, 129, 1000, 2945, 2950, 3008, 5000, 10000, 131072, 200000})
    for (int n_mem : {1, 63, 64, 65, 128, 129, 1000, 2945, 4000, 10000, 131072, 200000})
      if (n_mem <= n_u) { check_chunk_rule(n_u, n_mem); ++rules; }
  { const BisilChunks c = bisil_chunk_rule(2950, 2945); CHECK(c.chunk_tiles == 2 && c.chunks == 24); }
  { const BisilChunks c = bisil_chunk_rule(5000, 4000); CHECK(c.chunk_tiles == 3 && c.chunks == 27); }
  { const BisilChunks c = bisil_chunk_rule(150, 20); CHECK(c.chunk_tiles == 1 && c.chunks == 3); }
  // the gather form: lanes along the smaller stride, a tie along the points; per side the roles swap
  for (long long rs : {0LL, 1LL, 2LL, 90LL, 4096LL})
    for (long long cs : {0LL, 1LL, 3LL, 90LL, 150LL}) {
      CHECK(f64_bisil_side_form(0, rs, cs) == (rs <= cs ? F64_BISIL_GATHER_POINTS : F64_BISIL_GATHER_LDS));
      CHECK(f64_bisil_side_form(1, rs, cs) == (cs <= rs ? F64_BISIL_GATHER_POINTS : F64_BISIL_GATHER_LDS));
    }
  CHECK(f64_bisil_side_form(0, 90, 1) == F64_BISIL_GATHER_LDS && f64_bisil_side_form(1, 90, 1) == F64_BISIL_GATHER_POINTS);    // row-major
  CHECK(f64_bisil_side_form(0, 1, 150) == F64_BISIL_GATHER_POINTS && f64_bisil_side_form(1, 1, 150) == F64_BISIL_GATHER_LDS);  // column-major
  // the lists, their packing and the workspace
  int cases = 0;
  struct Shape { int n, m, k; double fill; int er, ec; };
  const Shape shapes[] = {{40, 30, 1, 0.3, -1, -1}, {40, 30, 3, 0.3, -1, -1},  {150, 90, 5, 0.2, 1, 3}, {150, 90, 17, 0.1, -1, -1},
                          {150, 97, 64, 0.05, 63, 0}, {330, 150, 12, 0.4, -1, -1}, {2950, 60, 3, 0.9, -1, -1}, {7, 5, 4, 0.0, -1, -1},
                          {64, 64, 2, 1.0, -1, -1},   {65, 33, 9, 0.5, 8, 8}};
  for (const Shape& s : shapes)
    for (int host_x = 0; host_x < 2; ++host_x) {
      check_lists(random_clusters(s.n, s.m, s.k, s.fill, 1000u + (unsigned)cases, s.er, s.ec), host_x != 0);
      ++cases;
    }
  // refusals: the first offender in bicluster order, the rows of a bicluster before its columns; NaN refused, -0.0 is 0
  {
    Clusters c = random_clusters(20, 10, 3, 0.5, 7u);
    BisilHostLists L;
    c.cc[(size_t)0 * 10 + 4] = 2.0;
    c.rc[(size_t)1 * 20 + 3] = 0.5;
    CHECK(bisil_build_lists(c.n, c.m, c.k, c.rc.data(), c.cc.data(), L) == 2);
    c.rc[(size_t)0 * 20 + 19] = std::nan("");
    CHECK(bisil_build_lists(c.n, c.m, c.k, c.rc.data(), c.cc.data(), L) == 1);
    Clusters z = random_clusters(20, 10, 3, 0.5, 7u);
    BisilHostLists A, B;
    CHECK(bisil_build_lists(z.n, z.m, z.k, z.rc.data(), z.cc.data(), A) == 0);
    for (double& x : z.rc) if (x == 0.0) x = -0.0;
    CHECK(bisil_build_lists(z.n, z.m, z.k, z.rc.data(), z.cc.data(), B) == 0);
    CHECK(A.active == B.active && A.side[0].upts == B.side[0].upts && A.side[0].umask == B.side[0].umask);
  }
  std::printf("fp64_bisil_check: %d chunk rules, %d list cases, all checks passed\n", rules, cases);
  return 0;
}
