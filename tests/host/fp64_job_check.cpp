// Stand-alone host check of csrc/resnmtf_fp64_job.h: the layout of the fp64 job's one device
// buffer, the CSC check, the CSR build, the two struct checks that need no device and the restriction column sums.  No
// HIP call; built with a plain C++17 compiler by tests/test_fp64_job_check_host.py.  Prints every offset of every job (the printout of two builds is
// compared when the layout code moves) and exits non-zero at the first condition that does not hold.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>

#include "resnmtf_fp64_job.h"

#define CHECK(cond)                                                                 \
  do {                                                                              \
    if (!(cond)) {                                                                  \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);                 \
      std::exit(1);                                                                 \
    }                                                                               \
  } while (0)

namespace {
typedef resnmtf_group_job Job;

// a CSC structure with values, and what a brute-force pass over its dense form says of it
struct Csc {
  int n = 0, m = 0;
  std::vector<long long> ptr;
  std::vector<int> idx;
  std::vector<double> val;
};

Csc csc_of_dense(int n, int m, const std::vector<double>& a) {     // a column-major, zeros not stored
  Csc c;
  c.n = n; c.m = m; c.ptr.assign(1, 0);
  c.idx.reserve(1); c.val.reserve(1);       // (no stored entry: the arrays are still there, a NULL one is refused)
  for (int col = 0; col < m; ++col) {
    for (int i = 0; i < n; ++i)
      if (a[(size_t)i + (size_t)col * n] != 0.0) { c.idx.push_back(i); c.val.push_back(a[(size_t)i + (size_t)col * n]); }
    c.ptr.push_back((long long)c.idx.size());
  }
  return c;
}

std::vector<double> random_dense(int n, int m, double fill, unsigned seed) {
  std::mt19937 gen(seed);
  std::uniform_real_distribution<double> u(0.0, 1.0);
  std::vector<double> a((size_t)n * m, 0.0);
  for (double& x : a)
    if (u(gen) < fill) x = 0.5 + u(gen);
  return a;
}

F64SparseShape shape_of(const Csc& c) {
  F64SparseShape sh;
  CHECK(fp64_check_csc(c.n, c.m, c.ptr.data(), c.idx.data(), c.val.data(), sh).empty());
  return sh;
}

struct Case {
  const char* name;
  Job j;
  int cap;
  F64Source src[RESNMTF_GROUP_MAX_VIEWS];
  F64SparseShape shapes[RESNMTF_GROUP_MAX_VIEWS];
};

Case make_case(const char* name, int k, int cap, std::vector<std::pair<int, int>> dims) {
  Case c;
  std::memset(&c.j, 0, sizeof(c.j));
  c.name = name; c.cap = cap;
  c.j.struct_size = (int)sizeof(Job);
  c.j.n_views = (int)dims.size(); c.j.k = k; c.j.n_iters = cap;
  for (int v = 0; v < RESNMTF_GROUP_MAX_VIEWS; ++v) {
    c.src[v] = F64Source::HostDense;
    for (int w = 0; w < RESNMTF_GROUP_MAX_VIEWS; ++w) c.j.row_count[v][w] = c.j.col_count[v][w] = -1;
  }
  for (size_t v = 0; v < dims.size(); ++v) { c.j.n_rows[v] = dims[v].first; c.j.n_cols[v] = dims[v].second; }
  return c;
}

void make_sparse(Case& c, int v, F64Source src, const Csc& m) {
  CHECK(m.n == c.j.n_rows[v] && m.m == c.j.n_cols[v]);
  c.src[v] = src;
  c.shapes[v] = shape_of(m);
}

struct Region { std::string name; size_t begin, extent; };

size_t cdiv(size_t a, size_t b) { return (a + b - 1) / b; }

// Every region with the extent its consumer addresses -- read off fp64_enqueue_sweep, the upload and the norm launches
// in csrc/resnmtf_fp64.hip and the kernels they start, not off fp64_layout.
std::vector<Region> regions_of(const Case& c, const F64Layout& L) {
  const size_t k = (size_t)L.k, V = (size_t)L.V, KP = (size_t)L.KP;
  std::vector<Region> r;
  size_t big = 0, slab = 0, spart = 0;
  bool any_sparse = false;
  for (int v = 0; v < L.V; ++v) {
    const F64View& w = L.vw[v];
    const size_t n = (size_t)w.n, m = (size_t)w.m;
    const std::string p = "view" + std::to_string(v) + ".";
    if (w.sparse()) {                       // the upload: m + 1 and n + 1 pointers, nnz values, nnz ints two per double
      any_sparse = true;
      const size_t ints = cdiv(w.nnz * sizeof(int), sizeof(double));
      r.push_back({p + "cptr", w.cptr, m + 1}); r.push_back({p + "cval", w.cval, w.nnz}); r.push_back({p + "cidx", w.cidx, ints});
      r.push_back({p + "rptr", w.rptr, n + 1}); r.push_back({p + "rval", w.rval, w.nnz}); r.push_back({p + "ridx", w.ridx, ints});
      // fp64_spmm: slab[(split ldx + line) KP + c]; fp64_norm_kernel over the nnz CSC values
      slab = std::max(slab, std::max((size_t)w.sxg.splits * w.ldn, (size_t)w.sxtf.splits * w.ldm) * KP);
      spart = std::max(spart, cdiv(w.nnz, F64_NORM_CHUNK));
    } else {                                // fp64_product_kernel reads ldx rows of contr_pad columns; slab[(split ldx + i) KP + c]
      r.push_back({p + "x", w.x, w.ldn * w.mpad}); r.push_back({p + "xt", w.xt, w.ldm * w.npad});
      slab = std::max(slab, std::max((size_t)w.xg.splits * w.ldn, (size_t)w.xtf.splits * w.ldm) * KP);
      // fp64_resid: one partial per (tile, split); fp64_norm_kernel: one per chunk of the image of X
      spart = std::max(spart, std::max((size_t)w.res.tiles * w.res.splits, cdiv(w.ldn * w.mpad, F64_NORM_CHUNK)));
    }
    r.push_back({p + "f", w.f, n * k}); r.push_back({p + "g", w.g, m * k});
    big = std::max(big, std::max(n, m));
  }
  r.push_back({"s", L.s, V * k * k}); r.push_back({"lam", L.lam, V * k}); r.push_back({"mu", L.mu, V * k});
  r.push_back({"kk", L.kk, 4 * k * k});     // kkA, kkB, kkC, kkD
  r.push_back({"cf", L.cf, V * k}); r.push_back({"cg", L.cg, V * k});
  r.push_back({"norms", L.norms, V}); r.push_back({"errs", L.errs, V});
  r.push_back({"scratch", L.scratch, big * k});       // fp64_update_kernel's xo: the rows of the side updated, k columns
  r.push_back({"scratch2", L.scratch2, big * k});     // its ps, and F S of fp64_fs_kernel
  r.push_back({"slab", L.slab, slab});
  r.push_back({"part0", L.part0, cdiv(big, F64_GRAM_ROWS) * k * k});      // fp64_gram_kernel: one k x k per 256 rows
  r.push_back({"part1", L.part1, cdiv(big, F64_GRAM_ROWS) * k * k});
  r.push_back({"colf", L.colf, cdiv(big, F64_UPD_ROWS) * k});             // colpart[block k + c], 64 rows per block
  r.push_back({"colg", L.colg, cdiv(big, F64_UPD_ROWS) * k});
  r.push_back({"spart", L.spart, std::max<size_t>(spart, 1)});
  r.push_back({"err", L.err, (size_t)c.cap});                             // err_out = err + it, it < cap
  if (any_sparse) {
    r.push_back({"slots", L.slots, V * 3 * k * k});                       // three k x k per view
    r.push_back({"ot", L.ot, big * KP});                                  // fp64_sp_operand_kernel: OT[j KP + c], j < len
  }
  r.push_back({"maps", L.maps, L.total - L.maps});
  return r;
}

void check_layout(const Case& c) {
  F64Layout L;
  fp64_layout(c.j, c.cap, L, c.src, c.shapes);
  std::printf("job %s: V %d k %d KP %d cap %d\n", c.name, L.V, L.k, L.KP, L.cap);
  for (int v = 0; v < L.V; ++v) {
    const F64View& w = L.vw[v];
    std::printf("  view %d: n %d m %d ldn %zu mpad %zu ldm %zu npad %zu x %zu xt %zu f %zu g %zu nnz %zu cptr %zu cval %zu cidx %zu "
                "rptr %zu rval %zu ridx %zu\n", v, w.n, w.m, w.ldn, w.mpad, w.ldm, w.npad, w.x, w.xt, w.f, w.g, w.nnz, w.cptr, w.cval,
                w.cidx, w.rptr, w.rval, w.ridx);
    if (w.sparse())
      std::printf("    sxg %d %lld %lld sxtf %d %lld %lld\n", w.sxg.splits, w.sxg.piece, w.sxg.longest, w.sxtf.splits, w.sxtf.piece,
                  w.sxtf.longest);
    else
      std::printf("    xg %d %d %d xtf %d %d %d res %d %d %d\n", w.xg.tiles, w.xg.splits, w.xg.chunk, w.xtf.tiles, w.xtf.splits,
                  w.xtf.chunk, w.res.tiles, w.res.splits, w.res.chunk);
  }
  std::printf("  out_begin %zu out_end %zu s %zu lam %zu mu %zu kk %zu cf %zu cg %zu norms %zu errs %zu scratch %zu scratch2 %zu slab %zu\n",
              L.out_begin, L.out_end, L.s, L.lam, L.mu, L.kk, L.cf, L.cg, L.norms, L.errs, L.scratch, L.scratch2, L.slab);
  std::printf("  part0 %zu part1 %zu colf %zu colg %zu spart %zu err %zu slots %zu ot %zu maps %zu total %zu\n", L.part0, L.part1,
              L.colf, L.colg, L.spart, L.err, L.slots, L.ot, L.maps, L.total);
  for (int v = 0; v < L.V; ++v)
    for (int w = 0; w < L.V; ++w)
      if (L.rmap[v][w] >= 0 || L.cmap[v][w] >= 0) std::printf("  map %d %d: rows %lld cols %lld\n", v, w, L.rmap[v][w], L.cmap[v][w]);

  // every region inside [0, total), pairwise disjoint at the extent its consumer addresses
  std::vector<Region> r = regions_of(c, L);
  std::sort(r.begin(), r.end(), [](const Region& a, const Region& b) { return a.begin != b.begin ? a.begin < b.begin : a.extent < b.extent; });
  for (size_t i = 0; i < r.size(); ++i) {
    CHECK(r[i].begin + r[i].extent <= L.total);
    if (i + 1 < r.size() && r[i].begin + r[i].extent > r[i + 1].begin) {
      std::printf("FAILED: job %s: %s [%zu, +%zu) overlaps %s at %zu\n", c.name, r[i].name.c_str(), r[i].begin, r[i].extent,
                  r[i + 1].name.c_str(), r[i + 1].begin);
      std::exit(1);
    }
  }
  // [out_begin, out_end) is exactly F and G per view, then S, then lambda, then mu
  const size_t k = (size_t)L.k, V = (size_t)L.V;
  size_t off = L.out_begin;
  for (int v = 0; v < L.V; ++v) {
    CHECK(L.vw[v].f == off); off += (size_t)L.vw[v].n * k;
    CHECK(L.vw[v].g == off); off += (size_t)L.vw[v].m * k;
  }
  CHECK(L.s == off); off += V * k * k;
  CHECK(L.lam == off); off += V * k;
  CHECK(L.mu == off); off += V * k;
  CHECK(L.out_end == off);
  for (int f = 0; f < 2 * F64_OUT_SET; ++f)           // the table's pieces are those five, at the same places
    for (int v = 0; v < L.V; ++v) {
      const F64OutField& o = F64_OUT_FIELDS[f];
      const size_t at = fp64_piece_offset(L, v, o.piece), cnt = o.count((size_t)L.vw[v].n, (size_t)L.vw[v].m, k);
      CHECK(at >= L.out_begin && at + cnt <= L.out_end);
    }
  // the int maps: from 2 maps on, one after the other, within 2 total
  size_t ioff = 2 * L.maps;
  for (int v = 0; v < RESNMTF_GROUP_MAX_VIEWS; ++v)
    for (int w = 0; w < RESNMTF_GROUP_MAX_VIEWS; ++w) {
      const bool pair = v < L.V && w < L.V && v != w;
      CHECK((L.rmap[v][w] >= 0) == (pair && c.j.row_count[v][w] > 0));
      CHECK((L.cmap[v][w] >= 0) == (pair && c.j.col_count[v][w] > 0));
      if (L.rmap[v][w] >= 0) { CHECK((size_t)L.rmap[v][w] == ioff); ioff += (size_t)L.vw[v].n; }
      if (L.cmap[v][w] >= 0) { CHECK((size_t)L.cmap[v][w] == ioff); ioff += (size_t)L.vw[v].m; }
    }
  CHECK(ioff <= 2 * L.total);
  // slots and ot exist only with a sparse view
  bool any_sparse = false;
  for (int v = 0; v < L.V; ++v) any_sparse = any_sparse || L.vw[v].sparse();
  if (!any_sparse) CHECK(L.slots == 0 && L.ot == 0);
  else CHECK(L.slots >= L.err + (size_t)c.cap && L.ot >= L.slots + V * 3 * k * k);
}

int check_layouts() {
  std::vector<Case> cases;
  cases.push_back(make_case("1: 1x1 k1", 1, 7, {{1, 1}}));
  cases.push_back(make_case("2: 33x257 k17", 17, 7, {{33, 257}}));
  cases.push_back(make_case("3: 257x33 k33", 33, 7, {{257, 33}}));
  cases.push_back(make_case("4: 1024x64 k16", 16, 7, {{1024, 64}}));
  CHECK(f64_ld(1024) == 1056);
  {
    std::vector<std::pair<int, int>> dims;
    for (int v = 0; v < RESNMTF_GROUP_MAX_VIEWS; ++v) dims.push_back({40 + v, 30 + 2 * v});
    Case c = make_case("5: 8 views, every pair mapped", 3, 7, dims);
    for (int v = 0; v < 8; ++v)
      for (int w = 0; w < 8; ++w)
        if (v != w) { c.j.row_count[v][w] = 5 + v; c.j.col_count[v][w] = 4 + w; }
    cases.push_back(c);
  }
  {
    Case c = make_case("6: dense and sparse mixed", 5, 7, {{50, 70}, {70, 50}, {50, 70}, {64, 64}});
    make_sparse(c, 1, F64Source::HostCsc, csc_of_dense(70, 50, random_dense(70, 50, 0.2, 1)));
    make_sparse(c, 2, F64Source::DeviceSparse, csc_of_dense(50, 70, random_dense(50, 70, 0.1, 2)));
    c.src[3] = F64Source::DeviceDense;
    c.j.row_count[0][2] = c.j.row_count[2][0] = 50;
    c.j.col_count[0][2] = c.j.col_count[2][0] = 9;
    cases.push_back(c);
  }
  {
    Case c = make_case("7: sparse, nnz 0", 4, 7, {{20, 30}});
    make_sparse(c, 0, F64Source::HostCsc, csc_of_dense(20, 30, std::vector<double>(600, 0.0)));
    CHECK(c.shapes[0].nnz == 0);
    cases.push_back(c);
  }
  {
    Case c = make_case("8: sparse, odd nnz", 2, 7, {{9, 7}});
    std::vector<double> a(63, 0.0);
    for (int e = 0; e < 13; ++e) a[(size_t)(e * 5) % 63] = 1.0 + e;
    make_sparse(c, 0, F64Source::HostCsc, csc_of_dense(9, 7, a));
    CHECK(c.shapes[0].nnz == 13);
    cases.push_back(c);
  }
  {
    Case c = make_case("9: sparse, a line beyond 16 x 256 entries", 2, 7, {{5000, 20}});
    std::vector<double> a((size_t)5000 * 20, 0.0);
    for (int i = 0; i < 5000; ++i) a[(size_t)i] = 1.0;                    // column 0 is full
    for (int col = 1; col < 20; ++col) a[(size_t)col + (size_t)col * 5000] = 2.0;
    make_sparse(c, 0, F64Source::HostCsc, csc_of_dense(5000, 20, a));
    CHECK(c.shapes[0].longest_col == 5000 && c.shapes[0].longest_col > (long long)F64_SP_MAX_SPLITS * F64_SP_PIECE);
    CHECK(f64_plan_sparse(c.shapes[0].longest_col).splits == F64_SP_MAX_SPLITS);
    cases.push_back(c);
  }
  cases.push_back(make_case("10: cap 1", 17, 1, {{33, 257}}));
  for (const Case& c : cases) {
    CHECK(fp64_shapes_ok(c.j));
    check_layout(c);
  }
  return (int)cases.size();
}

// ---- fp64_check_csc: each refusal once by a minimal offender; a valid structure against a brute-force count ----
void check_csc() {
  F64SparseShape sh;
  auto refusal = [&](int n, int m, std::vector<long long> ptr, std::vector<int> idx, std::vector<double> val) {
    return fp64_check_csc(n, m, ptr.data(), idx.data(), val.empty() ? nullptr : val.data(), sh);
  };
  const long long p0[2] = {0, 0};
  const int i0[1] = {0};
  CHECK(fp64_check_csc(2, 1, nullptr, i0, nullptr, sh) == "col_ptr / row_idx is NULL");
  CHECK(fp64_check_csc(2, 1, p0, nullptr, nullptr, sh) == "col_ptr / row_idx is NULL");
  CHECK(refusal(2, 1, {1, 1}, {0}, {}) == "col_ptr[0] must be 0 (0-based CSC)");
  CHECK(refusal(2, 2, {0, 1, 0}, {0}, {}) == "col_ptr is not monotone (column 1)");
  CHECK(refusal(2, 1, {0, 1}, {2}, {}) == "row index out of range in column 0");
  CHECK(refusal(2, 1, {0, 1}, {-1}, {}) == "row index out of range in column 0");
  CHECK(refusal(2, 2, {0, 0, 2}, {1, 1}, {}) == "row indices must be strictly increasing within a column (column 1)");
  CHECK(refusal(2, 1, {0, 1}, {0}, {std::nan("")}) == "non-finite entry in column 0");
  CHECK(refusal(2, 1, {0, 1}, {0}, {-1.0}) == "negative entry in column 0");
  for (unsigned seed = 0; seed < 4; ++seed) {
    const int n = 13 + 5 * (int)seed, m = 11 + 3 * (int)seed;
    const std::vector<double> a = random_dense(n, m, 0.3, 10 + seed);
    const Csc c = csc_of_dense(n, m, a);
    CHECK(fp64_check_csc(n, m, c.ptr.data(), c.idx.data(), c.val.data(), sh).empty());
    size_t nnz = 0;
    long long longest_row = 0, longest_col = 0;
    for (int col = 0; col < m; ++col) {
      long long cnt = 0;
      for (int i = 0; i < n; ++i) cnt += a[(size_t)i + (size_t)col * n] != 0.0;
      longest_col = std::max(longest_col, cnt); nnz += (size_t)cnt;
    }
    for (int i = 0; i < n; ++i) {
      long long cnt = 0;
      for (int col = 0; col < m; ++col) cnt += a[(size_t)i + (size_t)col * n] != 0.0;
      longest_row = std::max(longest_row, cnt);
    }
    CHECK(sh.nnz == nnz && sh.longest_row == longest_row && sh.longest_col == longest_col);

    // fp64_csr_from_csc: the CSR read off the dense matrix, rows in order, columns ascending within a row
    std::vector<long long> rp, want_rp(1, 0);
    std::vector<int> ci, want_ci;
    std::vector<double> rv, want_rv;
    fp64_csr_from_csc(n, m, c.ptr.data(), c.idx.data(), c.val.data(), rp, ci, rv);
    for (int i = 0; i < n; ++i) {
      for (int col = 0; col < m; ++col)
        if (a[(size_t)i + (size_t)col * n] != 0.0) { want_ci.push_back(col); want_rv.push_back(a[(size_t)i + (size_t)col * n]); }
      want_rp.push_back((long long)want_ci.size());
    }
    CHECK(rp == want_rp && ci == want_ci && rv == want_rv);
  }
}

// ---- the two struct checks, called directly: the cases of tests/test_fp64_device_host.py::
// test_c_entry_refuses_a_malformed_device_struct, the same texts ----
double g_there[4];                          // (addresses that are never read through)

Job small_job(int V) {                      // n = 10, m = 8, k = 2, every host pointer set
  Job j;
  std::memset(&j, 0, sizeof(j));
  j.struct_size = (int)sizeof(Job); j.n_views = V; j.k = 2; j.n_iters = 5;
  for (int v = 0; v < V; ++v) {
    j.n_rows[v] = 10; j.n_cols[v] = 8;
    j.x[v] = j.f0[v] = j.s0[v] = j.g0[v] = g_there;
    j.f_out[v] = j.s_out[v] = j.g_out[v] = j.lambda_out[v] = j.mu_out[v] = g_there;
  }
  return j;
}

resnmtf_device_matrix mat(int dtype = RESNMTF_DTYPE_F64, long long rs = 1, long long cs = 10) {
  resnmtf_device_matrix a;
  std::memset(&a, 0, sizeof(a));
  a.ptr = g_there; a.dtype = dtype; a.row_stride = rs; a.col_stride = cs;
  return a;
}

std::string device_refusal(const Job& j, const resnmtf_fp64_device& d) {
  F64Source src[RESNMTF_GROUP_MAX_VIEWS];
  F64DeviceUse use;
  fp64_resolve_sources(nullptr, &d, nullptr, src);
  return fp64_check_device_struct(j, d, src, use);
}

bool starts(const std::string& text, const char* prefix) { return text.rfind(prefix, 0) == 0; }

void check_device_struct() {
  resnmtf_fp64_device fresh;
  std::memset(&fresh, 0, sizeof(fresh));
  fresh.struct_size = (int)sizeof(fresh);
  Job j = small_job(1);
  resnmtf_fp64_device d = fresh;
  CHECK(device_refusal(j, d).empty());

  d = fresh; d.x[0] = mat();                                              // both
  CHECK(starts(device_refusal(j, d), "view 0: x is given both in the job (job->x) and in device memory (dev->x)"));
  d = fresh; j = small_job(1); j.x[0] = nullptr;                          // neither
  CHECK(starts(device_refusal(j, d), "view 0: x is given neither in the job (job->x) nor in device memory (dev->x)"));
  d = fresh; j = small_job(1); d.f0[0] = mat(); d.g0[0] = mat(RESNMTF_DTYPE_F64, 1, 8);      // partial factors
  j.f0[0] = j.s0[0] = j.g0[0] = nullptr;
  CHECK(starts(device_refusal(j, d), "view 0: f0 / s0 / g0 are given partly in device memory (dev->s0 NULL)"));
  d = fresh; j = small_job(1); d.f0[0] = mat(); d.s0[0] = mat(RESNMTF_DTYPE_F64, 1, 2); d.g0[0] = mat(RESNMTF_DTYPE_F64, 1, 8);   // factors twice
  CHECK(starts(device_refusal(j, d), "view 0: f0 / s0 / g0 are given in device memory: job->f0 / s0 / g0 / lambda0 / mu0 must be NULL"));
  d = fresh; d.lambda0[0] = mat();                                        // lambda0 alone
  CHECK(starts(device_refusal(j, d), "view 0: dev->lambda0 / dev->mu0 need f0 / s0 / g0 in device memory"));
  d = fresh; d.f_out[0] = d.s_out[0] = d.lambda_out[0] = d.mu_out[0] = g_there;             // partial outputs
  CHECK(starts(device_refusal(j, d), "view 0: dev->g_out is NULL while other device outputs are given"));
  d = fresh; d.state_f[0] = g_there;                                      // partial state
  CHECK(starts(device_refusal(j, d), "view 0: dev->state_s is NULL while other device state outputs are given"));
  d = fresh; j = small_job(1); j.x[0] = nullptr; d.x[0] = mat(RESNMTF_DTYPE_F64, -1);       // negative stride
  CHECK(starts(device_refusal(j, d), "view 0: dev->x has a negative stride"));
  d = fresh; d.x[0] = mat(4);                                             // unknown dtype
  CHECK(starts(device_refusal(j, d), "view 0: dev->x has an unknown dtype (4)"));
  d = fresh; j = small_job(1); d.struct_size = (int)sizeof(d) - 8;       // struct_size
  CHECK(device_refusal(j, d) == "resnmtf_fp64_device struct_size mismatch");
  d = fresh; d.x[1] = mat();                                              // beyond n_views
  CHECK(starts(device_refusal(j, d), "view 1: dev->x is given beyond n_views"));
  d = fresh; j = small_job(2);                                            // a set over one of two views
  for (int f = 0; f < F64_OUT_SET; ++f) (d.*F64_OUT_FIELDS[f].member)[0] = g_there;
  CHECK(starts(device_refusal(j, d), "view 1: dev->f_out is NULL while other device outputs are given"));

  // a full struct: what the checks leave in `use`, and the sources resolved
  d = fresh; j = small_job(1); j.x[0] = nullptr; d.x[0] = mat();
  for (const F64OutField& o : F64_OUT_FIELDS) (d.*o.member)[0] = g_there;
  F64Source src[RESNMTF_GROUP_MAX_VIEWS];
  F64DeviceUse use;
  fp64_resolve_sources(nullptr, &d, nullptr, src);
  CHECK(src[0] == F64Source::DeviceDense && src[1] == F64Source::HostDense && fp64_x_elsewhere(src) == 1u);
  CHECK(fp64_check_device_struct(j, d, src, use).empty() && use.out && use.state && use.factors == 0);
}

void check_sparse_device_struct() {
  resnmtf_fp64_sparse_device fresh;
  std::memset(&fresh, 0, sizeof(fresh));
  fresh.struct_size = (int)sizeof(fresh);
  resnmtf_fp64_sparse_device_view good;
  std::memset(&good, 0, sizeof(good));
  good.layout = RESNMTF_SPARSE_CSC; good.index_type = RESNMTF_INDEX_I32; good.dtype = RESNMTF_DTYPE_F64;
  good.ptr_or_rows = good.idx_or_cols = good.values = g_there; good.nnz = 3;
  Job j = small_job(1);
  j.x[0] = nullptr;
  resnmtf_fp64_sparse_device d = fresh;
  d.view[0] = good;
  CHECK(fp64_check_sparse_device_struct(j, nullptr, nullptr, d).empty());
  F64Source src[RESNMTF_GROUP_MAX_VIEWS];
  fp64_resolve_sources(nullptr, nullptr, &d, src);
  CHECK(src[0] == F64Source::DeviceSparse && f64_is_sparse(src[0]) && src[1] == F64Source::HostDense);

  const Job with_x = small_job(1);
  CHECK(starts(fp64_check_sparse_device_struct(with_x, nullptr, nullptr, d),
               "view 0: x is given in two places, in sparse device arrays (spd->view) and in the job (job->x)"));
  CHECK(fp64_check_sparse_device_struct(j, nullptr, nullptr, fresh) == "view 0: x is given in none of job->x, sp, dev->x and spd");
  d = fresh; d.view[0] = good; d.view[1] = good;
  CHECK(fp64_check_sparse_device_struct(j, nullptr, nullptr, d) == "view 1: spd->view is given beyond n_views");
  resnmtf_fp64_device dev;
  std::memset(&dev, 0, sizeof(dev));
  dev.struct_size = (int)sizeof(dev); dev.stream = g_there;
  d = fresh; d.view[0] = good;
  CHECK(starts(fp64_check_sparse_device_struct(j, nullptr, &dev, d), "dev->stream and spd->stream differ"));
  d.view[0].layout = 7;
  CHECK(fp64_check_sparse_device_struct(j, nullptr, nullptr, d) == "view 0: spd->view: unknown layout: one of RESNMTF_SPARSE_CSC / _CSR / _COO");
  d.view[0] = good; d.view[0].index_type = 7;
  CHECK(fp64_check_sparse_device_struct(j, nullptr, nullptr, d) == "view 0: spd->view: unknown index type: RESNMTF_INDEX_I32 or _I64");
  d.view[0] = good; d.view[0].dtype = 9;
  CHECK(fp64_check_sparse_device_struct(j, nullptr, nullptr, d) == "view 0: spd->view: unknown dtype: one of RESNMTF_DTYPE_F64 / _F32 / _F16 / _BF16");
  d.view[0] = good; d.view[0].nnz = -1;
  CHECK(fp64_check_sparse_device_struct(j, nullptr, nullptr, d) == "view 0: spd->view: nnz is negative");
  d.view[0] = good; d.view[0].values = nullptr;
  CHECK(fp64_check_sparse_device_struct(j, nullptr, nullptr, d) == "view 0: spd->view: ptr_or_rows / idx_or_cols / values is NULL");
}
// ---- fp64_col_sum / fp64_all_zero: the restriction column sums that decide the branch and scale the denominator ----
// R[w, v] = 1 / (3 + 6 w + 10 v) (odd denominators: no entry is dyadic), column-major V x V, for V = 1 .. 8: one correctly
// rounded division per entry, so tests/test_fp64_job_check_host.py rebuilds the same doubles and requires every printed
// sum to be numpy's, bit for bit (sequential below 8 entries, the 8-accumulator pairwise form at 8).
void check_col_sums() {
  for (int V = 1; V <= RESNMTF_GROUP_MAX_VIEWS; ++V) {
    std::vector<double> r((size_t)V * V);
    for (int v = 0; v < V; ++v)
      for (int w = 0; w < V; ++w) r[(size_t)w + (size_t)v * V] = 1.0 / (double)(3 + 6 * w + 10 * v);
    for (int v = 0; v < V; ++v) std::printf("colsum V %d v %d: %a\n", V, v, fp64_col_sum(r.data(), V, v));
    CHECK(!fp64_all_zero(r.data(), V));
    std::vector<double> z((size_t)V * V, 0.0);
    CHECK(fp64_all_zero(z.data(), V));
    for (int v = 0; v < V; ++v) CHECK(fp64_col_sum(z.data(), V, v) == 0.0);
    z[(size_t)V * V - 1] = 0x1p-1074;                   // the last entry alone, the smallest double there is
    CHECK(!fp64_all_zero(z.data(), V) && fp64_col_sum(z.data(), V, V - 1) == 0x1p-1074);
    if (V > 1) CHECK(fp64_col_sum(z.data(), V, 0) == 0.0);
    CHECK(fp64_all_zero(nullptr, V) && fp64_col_sum(nullptr, V, V - 1) == 0.0);
  }
}
}  // namespace

int main() {
  const int jobs = check_layouts();
  check_csc();
  check_device_struct();
  check_sparse_device_struct();
  check_col_sums();
  std::printf("fp64_job_check: %d jobs, all checks passed\n", jobs);
  return 0;
}
