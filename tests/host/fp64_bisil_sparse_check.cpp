// Stand-alone host check of what resnmtf_fp64_bisil_sparse decides without a device: the rank
// tables of the scatter (f64_bisil_ranks) against their definition, the layout of the call's one buffer
// (f64_bisil_sparse_plan: every region claimed once, each large enough for every side and bicluster) and the CSR copy of
// crafted CSCs (fp64_check_csc + fp64_csr_from_csc) against a direct transpose.  No HIP call; built with a plain C++17
// compiler by tests/test_fp64_bisil_sparse_check_host.py.  Exits non-zero at the first condition that does not hold.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <utility>
#include <vector>

#include "resnmtf_bisil_plan.h"
#include "resnmtf_fp64_job.h"

#define CHECK(cond)                                                                 \
  do {                                                                              \
    if (!(cond)) {                                                                  \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);                 \
      std::exit(1);                                                                 \
    }                                                                               \
  } while (0)

namespace {
int g_rank_cases = 0, g_plan_cases = 0, g_csr_cases = 0;

struct Clusters {
  int n, m, k;
  std::vector<double> rc, cc;
};

// k biclusters at `fill`; bicluster `no_rows` has no row, bicluster `no_cols` no column (-1: none)
Clusters random_clusters(int n, int m, int k, double fill, unsigned seed, int no_rows = -1, int no_cols = -1) {
  std::mt19937 gen(seed);
  std::uniform_real_distribution<double> u(0.0, 1.0);
  Clusters c{n, m, k, std::vector<double>((size_t)n * k, 0.0), std::vector<double>((size_t)m * k, 0.0)};
  for (int j = 0; j < k; ++j) {
    for (int r = 0; r < n; ++r) c.rc[(size_t)j * n + r] = (j != no_rows && u(gen) < fill) ? 1.0 : 0.0;
    for (int q = 0; q < m; ++q) c.cc[(size_t)j * m + q] = (j != no_cols && u(gen) < fill) ? 1.0 : 0.0;
  }
  return c;
}

// rank[p] = the number of points below p that are in an active bicluster when p is in one itself, else -1: the
// definition, from the cluster matrices alone
void check_ranks(const Clusters& c) {
  BisilHostLists L;
  CHECK(bisil_build_lists(c.n, c.m, c.k, c.rc.data(), c.cc.data(), L) == 0);
  std::vector<int> rank;
  f64_bisil_ranks(L, rank);
  CHECK(rank.size() == (size_t)c.n + (size_t)c.m);
  unsigned long long active = 0ull;
  for (int j = 0; j < c.k; ++j) {
    bool rows = false, cols = false;
    for (int r = 0; r < c.n; ++r) rows = rows || c.rc[(size_t)j * c.n + r] != 0.0;
    for (int q = 0; q < c.m; ++q) cols = cols || c.cc[(size_t)j * c.m + q] != 0.0;
    if (rows && cols) active |= 1ull << j;
  }
  CHECK(active == L.active);
  const std::vector<double>* mat[2] = {&c.rc, &c.cc};
  const int len[2] = {c.n, c.m};
  for (int sd = 0; sd < 2; ++sd) {
    const int* r = rank.data() + (sd == 0 ? 0 : c.n);
    int seen = 0;
    for (int p = 0; p < len[sd]; ++p) {
      bool in_u = false;
      for (int j = 0; j < c.k; ++j) in_u = in_u || (((active >> j) & 1ull) && (*mat[sd])[(size_t)j * len[sd] + p] != 0.0);
      CHECK(r[p] == (in_u ? seen : -1));
      if (in_u) {
        CHECK(L.side[sd].upts[(size_t)seen] == p);        // the inverse of U
        ++seen;
      }
    }
    CHECK(seen == (int)L.side[sd].upts.size());
  }
  ++g_rank_cases;
}

// every region of the buffer: inside it, disjoint from every other, and as large as its largest use
void check_plan(const Clusters& c, size_t nnz) {
  BisilHostLists L;
  CHECK(bisil_build_lists(c.n, c.m, c.k, c.rc.data(), c.cc.data(), L) == 0);
  F64BisilMeta M;
  f64_bisil_pack(c.k, L, M);
  const int n_u[2] = {(int)L.side[0].upts.size(), (int)L.side[1].upts.size()};
  const int* const cnt[2] = {L.side[0].cnt.data(), L.side[1].cnt.data()};
  F64BisilSparsePlan p;
  f64_bisil_sparse_plan(c.n, c.m, c.k, L.active, n_u, cnt, M.words.size(), nnz, p);
  F64BisilPlan d;
  f64_bisil_plan(c.n, c.m, c.k, L.active, n_u, cnt, M.words.size(), false, d);
  CHECK(p.dense.total == d.total && p.dense.g_dbl == d.g_dbl && p.dense.meta == d.meta && p.dense.x == d.total);   // no copy of X
  const size_t n = (size_t)c.n, m = (size_t)c.m, k = (size_t)c.k;
  // what every region must hold, in bytes
  size_t g_need = 0, norm_need = 0, part_need = 0;
  for (int sd = 0; sd < 2; ++sd) {
    const size_t upad = (size_t)(n_u[sd] + 63) / 64 * 64;
    norm_need = std::max(norm_need, upad);
    for (int j = 0; j < c.k; ++j) {
      if (!((L.active >> j) & 1ull)) continue;
      g_need = std::max(g_need, (size_t)cnt[1 - sd][j] * upad);                        // features x padded members
      part_need = std::max(part_need, (size_t)p.dense.chunks[sd][j] * cnt[sd][j] * k);
      CHECK((size_t)p.dense.chunks[sd][j] * p.dense.chunk_tiles[sd][j] * 64 >= upad);   // the chunks cover U
    }
  }
  struct Region { const char* name; size_t begin, bytes; };
  const Region regions[] = {
      {"g", 0, g_need * 8},
      {"norm2", p.dense.norm2 * 8, norm_need * 8},
      {"partial", p.dense.partial * 8, part_need * 8},
      {"sil", p.dense.sil * 8, (n * k + m * k) * 8},
      {"meta", p.dense.meta * 8, M.words.size() * 8},
      {"rank", p.rank * 8, (n + m) * 4},
      {"cptr", p.cptr * 8, (m + 1) * 8},
      {"cval", p.cval * 8, nnz * 8},
      {"cidx", p.cidx * 8, nnz * 4},
      {"rptr", p.rptr * 8, (n + 1) * 8},
      {"rval", p.rval * 8, nnz * 8},
      {"ridx", p.ridx * 8, nnz * 4},
  };
  const size_t count = sizeof(regions) / sizeof(regions[0]);
  for (size_t a = 0; a < count; ++a) {
    CHECK(regions[a].begin % 8 == 0);
    CHECK(regions[a].begin + regions[a].bytes <= p.total * 8);
    if (a + 1 < count) CHECK(regions[a].begin + regions[a].bytes <= regions[a + 1].begin);   // in order, so pairwise disjoint
  }
  CHECK(p.copies_dbl == p.total - p.cptr);
  CHECK(p.copies_dbl * 8 >= 24 * nnz + 8 * (n + m + 2));                 // 24 bytes per stored entry plus the pointers
  CHECK(p.copies_dbl * 8 <= 24 * nnz + 8 * (n + m + 2) + 16);            // (two index arrays rounded up to 8 bytes)
  ++g_plan_cases;
}

struct Csc {
  int n, m;
  std::vector<long long> ptr;
  std::vector<int> idx;
  std::vector<double> val;
};

// a CSC with `len(c)` stored entries in column c, at the rows a seeded draw picks, ascending
template <class Len>
Csc make_csc(int n, int m, unsigned seed, Len len) {
  std::mt19937 gen(seed);
  Csc a{n, m, {0}, {}, {}};
  a.idx.reserve(1); a.val.reserve(1);                     // (never a NULL pointer, as the callers of the entry do)
  std::vector<int> rows((size_t)n);
  for (int c = 0; c < m; ++c) {
    for (int i = 0; i < n; ++i) rows[(size_t)i] = i;
    std::shuffle(rows.begin(), rows.end(), gen);
    const int l = std::min(n, len(c));
    std::sort(rows.begin(), rows.begin() + l);
    for (int e = 0; e < l; ++e) {
      a.idx.push_back(rows[(size_t)e]);
      a.val.push_back(1.0 + (double)(gen() % 1000) / 1024.0 + (double)c);
    }
    a.ptr.push_back((long long)a.idx.size());
  }
  return a;
}

// the CSR copy against a direct transpose: (row, column, value) triples sorted by row, then column
void check_csr(const Csc& a) {
  F64SparseShape sh;
  CHECK(fp64_check_csc(a.n, a.m, a.ptr.data(), a.idx.data(), a.val.data(), sh).empty());
  CHECK(sh.nnz == a.idx.size());
  std::vector<long long> rp;
  std::vector<int> ci;
  std::vector<double> rv;
  fp64_csr_from_csc(a.n, a.m, a.ptr.data(), a.idx.data(), a.val.data(), rp, ci, rv);
  struct Entry { int r, c; double v; };
  std::vector<Entry> all;
  for (int c = 0; c < a.m; ++c)
    for (long long e = a.ptr[(size_t)c]; e < a.ptr[(size_t)c + 1]; ++e) all.push_back({a.idx[(size_t)e], c, a.val[(size_t)e]});
  std::stable_sort(all.begin(), all.end(), [](const Entry& x, const Entry& y) { return x.r != y.r ? x.r < y.r : x.c < y.c; });
  CHECK(rp.size() == (size_t)a.n + 1 && ci.size() == all.size() && rv.size() == all.size());
  CHECK(rp[0] == 0 && rp[(size_t)a.n] == (long long)all.size());
  long long longest_row = 0, longest_col = 0;
  size_t e = 0;
  for (int r = 0; r < a.n; ++r) {
    CHECK(rp[(size_t)r] == (long long)e);
    while (e < all.size() && all[e].r == r) {
      CHECK(ci[e] == all[e].c && rv[e] == all[e].v);
      if (e > (size_t)rp[(size_t)r]) CHECK(ci[e] > ci[e - 1]);          // columns ascend strictly within a row
      ++e;
    }
    longest_row = std::max(longest_row, (long long)e - rp[(size_t)r]);
  }
  CHECK(e == all.size());
  for (int c = 0; c < a.m; ++c) longest_col = std::max(longest_col, a.ptr[(size_t)c + 1] - a.ptr[(size_t)c]);
  CHECK(sh.longest_row == longest_row && sh.longest_col == longest_col);
  ++g_csr_cases;
}
}  // namespace

int main() {
  // ---- the rank tables ----
  const int shapes[][3] = {{1, 1, 1}, {7, 5, 1}, {64, 64, 3}, {65, 63, 5}, {150, 90, 5}, {150, 90, 64}, {40, 700, 1}, {300, 17, 12}};
  unsigned seed = 1;
  for (const auto& s : shapes)
    for (double fill : {0.05, 0.45, 1.0}) {
      check_ranks(random_clusters(s[0], s[1], s[2], fill, seed++));
      if (s[2] >= 3) check_ranks(random_clusters(s[0], s[1], s[2], fill, seed++, 1, 2));     // inactive biclusters
    }
  {
    Clusters none = random_clusters(20, 30, 4, 0.0, 99);                  // no active bicluster: every rank is -1
    BisilHostLists L;
    CHECK(bisil_build_lists(none.n, none.m, none.k, none.rc.data(), none.cc.data(), L) == 0 && L.active == 0ull);
    std::vector<int> rank;
    f64_bisil_ranks(L, rank);
    CHECK(rank.size() == 50 && std::count(rank.begin(), rank.end(), -1) == 50);
    ++g_rank_cases;
  }

  // ---- the workspace ----
  for (const auto& s : shapes)
    for (double fill : {0.05, 0.45, 1.0})
      for (size_t nnz : {(size_t)0, (size_t)1, (size_t)2, (size_t)(s[0] * s[1] / 3), (size_t)s[0] * (size_t)s[1]}) {
        check_plan(random_clusters(s[0], s[1], s[2], fill, seed++), nnz);
        if (s[2] >= 3) check_plan(random_clusters(s[0], s[1], s[2], fill, seed++, 0, 2), nnz);
      }
  check_plan(random_clusters(2950, 60, 3, 0.9, seed++), 17700);           // 24 chunks on the row side
  {
    // the shape the entry must refuse: 200000 x 200000, one bicluster holding everything -- G alone is 320 GB, and the
    // arithmetic of the plan holds it
    const int n = 200000;
    Clusters all{n, n, 1, std::vector<double>((size_t)n, 1.0), std::vector<double>((size_t)n, 1.0)};
    BisilHostLists L;
    CHECK(bisil_build_lists(n, n, 1, all.rc.data(), all.cc.data(), L) == 0);
    F64BisilMeta M;
    f64_bisil_pack(1, L, M);
    const int n_u[2] = {n, n};
    const int* const cnt[2] = {L.side[0].cnt.data(), L.side[1].cnt.data()};
    F64BisilSparsePlan p;
    f64_bisil_sparse_plan(n, n, 1, L.active, n_u, cnt, M.words.size(), 5, p);
    CHECK(p.dense.g_dbl == (size_t)n * 200000);
    CHECK(p.total * 8 >= 320000000000ull);
    ++g_plan_cases;
  }

  // ---- the CSR copy ----
  check_csr(make_csc(1, 1, 1, [](int) { return 1; }));
  check_csr(make_csc(5, 4, 2, [](int) { return 0; }));                                          // no stored entry
  check_csr(make_csc(150, 9, 3, [](int c) { const int l[] = {0, 1, 63, 64, 65, 129, 150, 2, 0}; return l[c]; }));
  check_csr(make_csc(9, 150, 4, [](int c) { return c % 10; }));                                 // 9: dense columns
  check_csr(make_csc(64, 64, 5, [](int c) { return c == 7 ? 64 : (c % 3 == 0 ? 0 : 3); }));     // a dense line among sparse ones
  check_csr(make_csc(200, 90, 6, [](int c) { return 1 + (c * 37) % 50; }));
  {
    Csc bad = make_csc(10, 3, 7, [](int) { return 4; });                  // the refusals come before any copy is built
    F64SparseShape sh;
    std::swap(bad.idx[0], bad.idx[1]);
    CHECK(!fp64_check_csc(bad.n, bad.m, bad.ptr.data(), bad.idx.data(), bad.val.data(), sh).empty());
    std::swap(bad.idx[0], bad.idx[1]);
    bad.idx[5] = 10;
    CHECK(!fp64_check_csc(bad.n, bad.m, bad.ptr.data(), bad.idx.data(), bad.val.data(), sh).empty());
  }

  std::printf("fp64_bisil_sparse_check: %d rank cases, %d workspace cases, %d CSR cases, all checks passed\n", g_rank_cases,
              g_plan_cases, g_csr_cases);
  return 0;
}
