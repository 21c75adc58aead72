// Stand-alone host check of csrc/resnmtf_fp64_shuffle_sparse_job.h: the struct checks of
// resnmtf_fp64_shuffle_sparse that need no device, the extents of its outputs and of a device view's arrays, the overlap
// test, the workspace regions (each claimed once and large enough) with the transient byte count, and the ordered column
// sum -- equal, bit for bit, to fp64_shuffle_stats_kernel's 256-lane order (restated here statement by statement) on
// densified random columns of length 1 .. 1100, explicit zeros, -0.0 and the lengths 0, 1, 255, 256, 257 included.  No HIP
// call; built with a plain C++17 compiler by tests/test_fp64_shuffle_sparse_check_host.py (and under
// -fsanitize=address,undefined).  Exits non-zero at the first condition that does not hold.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "resnmtf_fp64_shuffle_sparse_job.h"

#define CHECK(cond)                                                                 \
  do {                                                                              \
    if (!(cond)) {                                                                  \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);                 \
      std::exit(1);                                                                 \
    }                                                                               \
  } while (0)

namespace {
// (stand-ins: the struct checks compare pointers with NULL and read nothing)
long long host_ptr[4], dev_ptr[4], out_ptr[4], out_idx[6];
int host_idx[6];
double host_val[6], out_val[6];
float dev_val[6];
int counts[2];

resnmtf_fp64_shuffle_sparse_job sound_host_job() {
  resnmtf_fp64_shuffle_sparse_job j;
  std::memset(&j, 0, sizeof(j));
  j.struct_size = (int)sizeof(j);
  j.n = 5; j.m = 3; j.normalise = 1; j.seed = 7;
  j.x.col_ptr = host_ptr; j.x.row_idx = host_idx; j.x.values = host_val;
  j.out_col_ptr = out_ptr; j.out_row_idx = out_idx; j.out_values = out_val;
  j.n_empty_rows = &counts[0]; j.n_empty_cols = &counts[1];
  return j;
}
resnmtf_fp64_shuffle_sparse_job sound_device_job() {
  resnmtf_fp64_shuffle_sparse_job j = sound_host_job();
  j.x.col_ptr = nullptr; j.x.row_idx = nullptr; j.x.values = nullptr;
  j.x_dev.layout = RESNMTF_SPARSE_CSC; j.x_dev.index_type = RESNMTF_INDEX_I64; j.x_dev.dtype = RESNMTF_DTYPE_F32;
  j.x_dev.ptr_or_rows = dev_ptr; j.x_dev.idx_or_cols = out_idx; j.x_dev.values = dev_val; j.x_dev.nnz = 6;
  return j;
}
bool refused(const resnmtf_fp64_shuffle_sparse_job& j, const char* part) {
  const char* why = f64_shuffle_sparse_check_job(&j);
  return why && std::strstr(why, part);
}

int check_struct() {
  int cases = 0;
  resnmtf_fp64_shuffle_sparse_job j = sound_host_job();
  CHECK(f64_shuffle_sparse_check_job(&j) == nullptr);
  j = sound_device_job();
  CHECK(f64_shuffle_sparse_check_job(&j) == nullptr);
  CHECK(std::string(f64_shuffle_sparse_check_job(nullptr)) == "job is NULL"); ++cases;
  j = sound_host_job(); j.struct_size -= 1; CHECK(refused(j, "resnmtf_fp64_shuffle_sparse_job struct_size mismatch")); ++cases;
  j = sound_host_job(); j.struct_size = (int)sizeof(resnmtf_fp64_shuffle_job); CHECK(refused(j, "struct_size mismatch")); ++cases;
  j = sound_host_job(); j.n = 0; CHECK(refused(j, "view dimensions must be positive")); ++cases;
  j = sound_device_job(); j.m = -4; CHECK(refused(j, "view dimensions must be positive")); ++cases;
  j = sound_device_job(); j.x.col_ptr = host_ptr; CHECK(refused(j, "X is given in two places (job->x and job->x_dev)")); ++cases;
  j = sound_host_job(); j.x_dev.nnz = 1; CHECK(refused(j, "X is given in two places")); ++cases;       // (any of the seven fields)
  j = sound_host_job(); j.x.col_ptr = nullptr; CHECK(refused(j, "X is given in no place (job->x or job->x_dev)")); ++cases;
  j = sound_host_job(); j.out_col_ptr = nullptr; CHECK(refused(j, "out_col_ptr is NULL")); ++cases;
  j = sound_host_job(); j.n_empty_rows = nullptr; CHECK(refused(j, "n_empty_rows / n_empty_cols are NULL")); ++cases;
  j = sound_device_job(); j.n_empty_cols = nullptr; CHECK(refused(j, "n_empty_rows / n_empty_cols are NULL")); ++cases;
  // the two arrays of nnz may be NULL for a view without a stored entry, and only then
  j = sound_host_job(); j.out_row_idx = nullptr;
  CHECK(f64_shuffle_sparse_check_job(&j) == nullptr && f64_shuffle_sparse_check_nnz(j, 0) == nullptr);
  CHECK(std::string(f64_shuffle_sparse_check_nnz(j, 1)) == "out_row_idx / out_values are NULL"); ++cases;
  j = sound_host_job(); j.out_values = nullptr;
  CHECK(std::string(f64_shuffle_sparse_check_nnz(j, 6)) == "out_row_idx / out_values are NULL"); ++cases;
  j = sound_host_job(); CHECK(f64_shuffle_sparse_check_nnz(j, 6) == nullptr);
  // the masks and the stream may be NULL; what a device view holds is judged by the run's own checks, not here
  j = sound_device_job(); j.x_dev.layout = 9; j.x_dev.dtype = 17; CHECK(f64_shuffle_sparse_check_job(&j) == nullptr);
  // n m never exceeds the Feistel domain for int extents: the largest is (2^31 - 1)^2 < 2^62
  j = sound_host_job(); j.n = 2147483647; j.m = 2147483647; CHECK(f64_shuffle_sparse_check_job(&j) == nullptr);
  CHECK((unsigned long long)j.n * (unsigned long long)j.m < F64_SHUFFLE_MAX_COUNT);
  return cases;
}

void check_extents() {
  resnmtf_fp64_shuffle_sparse_job j = sound_device_job();       // 5 x 3, nnz 6, CSC int64 fp32
  F64ShuffleSparseRange out[3], in[3];
  f64_shuffle_sparse_outputs(j, 6, out);
  CHECK(out[0].ptr == out_ptr && out[0].bytes == 4 * 8 && out[1].ptr == out_idx && out[1].bytes == 6 * 8);
  CHECK(out[2].ptr == out_val && out[2].bytes == 6 * 8 && std::string(out[2].name) == "out_values");
  f64_shuffle_sparse_outputs(j, 0, out);
  CHECK(out[0].bytes == 4 * 8 && out[1].bytes == 0 && out[2].bytes == 0);
  f64_shuffle_sparse_sources(j, in);
  CHECK(in[0].bytes == 4 * 8 && in[1].bytes == 6 * 8 && in[2].bytes == 6 * 4);
  j.x_dev.layout = RESNMTF_SPARSE_CSR; j.x_dev.index_type = RESNMTF_INDEX_I32; j.x_dev.dtype = RESNMTF_DTYPE_BF16;
  f64_shuffle_sparse_sources(j, in);
  CHECK(in[0].bytes == 6 * 4 && in[1].bytes == 6 * 4 && in[2].bytes == 6 * 2);
  j.x_dev.layout = RESNMTF_SPARSE_COO; j.x_dev.dtype = RESNMTF_DTYPE_F64;
  f64_shuffle_sparse_sources(j, in);
  CHECK(in[0].bytes == 6 * 4 && in[1].bytes == 6 * 4 && in[2].bytes == 6 * 8);
  j.n = 200000; j.m = 20000;
  f64_shuffle_sparse_outputs(j, 40000000ull, out);
  CHECK(out[0].bytes == 20001ull * 8 && out[1].bytes == 320000000ull && out[2].bytes == 320000000ull);

  // overlaps: the outputs with each other, then with the arrays of a device view; none with a host view
  char buf[256];
  const char *a = nullptr, *b = nullptr;
  auto ranges = [&](size_t o0, size_t o1, size_t o2, size_t len) {
    out[0] = {"out_col_ptr", buf + o0, len}; out[1] = {"out_row_idx", buf + o1, len}; out[2] = {"out_values", buf + o2, len};
  };
  ranges(0, 32, 64, 32);
  CHECK(!f64_shuffle_sparse_overlap(out, nullptr, a, b));
  ranges(0, 31, 64, 32);
  CHECK(f64_shuffle_sparse_overlap(out, nullptr, a, b) && std::string(a) == "out_col_ptr" && std::string(b) == "out_row_idx");
  ranges(0, 32, 63, 32);
  CHECK(f64_shuffle_sparse_overlap(out, nullptr, a, b) && std::string(a) == "out_row_idx" && std::string(b) == "out_values");
  ranges(64, 32, 95, 32);
  CHECK(f64_shuffle_sparse_overlap(out, nullptr, a, b) && std::string(a) == "out_col_ptr" && std::string(b) == "out_values");
  ranges(0, 32, 64, 32);
  in[0] = {"x_dev.ptr_or_rows", buf + 96, 32}; in[1] = {"x_dev.idx_or_cols", buf + 128, 32}; in[2] = {"x_dev.values", buf + 160, 32};
  CHECK(!f64_shuffle_sparse_overlap(out, in, a, b));
  in[2].ptr = buf + 95;
  CHECK(f64_shuffle_sparse_overlap(out, in, a, b) && std::string(a) == "out_values" && std::string(b) == "x_dev.values");
  in[2].ptr = buf + 160; in[0].ptr = buf + 8; in[0].bytes = 1;
  CHECK(f64_shuffle_sparse_overlap(out, in, a, b) && std::string(a) == "out_col_ptr" && std::string(b) == "x_dev.ptr_or_rows");
  // empty ranges and NULL pointers overlap nothing (nnz = 0; a COO without rows)
  out[1].bytes = 0; out[2].bytes = 0; out[1].ptr = buf; out[2].ptr = buf;
  in[0] = {"x_dev.ptr_or_rows", nullptr, 0}; in[1].bytes = 0; in[1].ptr = buf; in[2].bytes = 0; in[2].ptr = buf;
  CHECK(!f64_shuffle_sparse_overlap(out, in, a, b));
}

// the regions of the workspace: each inside [0, total), pairwise disjoint, aligned, and as large as its user needs
int check_workspace() {
  int cases = 0;
  for (int n : {1, 7, 255, 256, 257, 70000}) {
    for (int m : {1, 3, 8, 9, 65536}) {
      const F64ShuffleSparsePlan p = f64_shuffle_sparse_plan(n, m);
      struct Region { size_t at, bytes, align; };
      const Region r[3] = {{p.colsum, (size_t)m * sizeof(double), 8}, {p.ints, 4 * sizeof(int), 4}, {p.mask, (size_t)n + (size_t)m, 1}};
      for (int x = 0; x < 3; ++x) {
        CHECK(r[x].at % r[x].align == 0 && r[x].at + r[x].bytes <= p.total);
        for (int y = x + 1; y < 3; ++y) CHECK(r[x].at + r[x].bytes <= r[y].at || r[y].at + r[y].bytes <= r[x].at);
      }
      CHECK(p.total % 8 == 0 && p.total < p.mask + (size_t)n + (size_t)m + 8);
      ++cases;
    }
  }
  // the transient memory: 68 bytes per stored entry, the pointers and the flag words beside them
  CHECK(F64_SHUFFLE_SPARSE_BYTES_PER_ENTRY == (8 + 4) + (4 + 4) + (5 * 8 + 2 * 4));
  CHECK(f64_shuffle_sparse_transient_bytes(5, 3, 0) == (2 * 4 + 6) * 8 + 48);
  CHECK(f64_shuffle_sparse_transient_bytes(5, 3, 10) == f64_shuffle_sparse_transient_bytes(5, 3, 0) + 680);
  CHECK(f64_shuffle_sparse_transient_bytes(200000, 20000, 40000000ull) == 40000000ull * 68 + (2 * 20001ull + 200001ull) * 8 + 48);
  return cases;
}

// fp64_shuffle_stats_kernel on one dense column, statement by statement: lane t of 256 takes rows t, t + 256, ..., then the
// 256-wide tree, for the minimum and then for sum(x + shift)
double dense_lane_sum(const std::vector<double>& col) {
  const long long n = (long long)col.size();
  double red[256];
  for (int t = 0; t < 256; ++t) {
    double mn = 0.0;
    for (long long r = t; r < n; r += 256) mn = std::fmin(mn, col[(size_t)r]);
    red[t] = mn;
  }
  for (int s = 128; s > 0; s >>= 1)
    for (int t = 0; t < s; ++t) red[t] = std::fmin(red[t], red[t + s]);
  const double sh = std::fabs(red[0]);
  for (int t = 0; t < 256; ++t) {
    double sum = 0.0;
    for (long long r = t; r < n; r += 256) sum += col[(size_t)r] + sh;
    red[t] = sum;
  }
  for (int s = 128; s > 0; s >>= 1)
    for (int t = 0; t < s; ++t) red[t] += red[t + s];
  return red[0];
}

unsigned long long next_random(unsigned long long& state) {      // splitmix64
  unsigned long long z = (state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

int check_column_sum() {
  int columns = 0;
  unsigned long long state = 12345;
  const double fill[4] = {0.01, 0.3, 0.6, 1.0};
  for (int n = 1; n <= 1100; ++n) {
    for (int f = 0; f < 4; ++f) {
      std::vector<double> dense((size_t)n, 0.0), vals;
      std::vector<int> rows;
      for (int r = 0; r < n; ++r) {
        if ((double)(next_random(state) >> 11) * 0x1p-53 >= fill[f]) continue;
        // magnitudes spread over 2^-20 .. 2^20 so that the order of the additions shows in the last bits
        double v = ((double)(next_random(state) >> 11) * 0x1p-53 + 0.5) * std::ldexp(1.0, (int)(next_random(state) % 41) - 20);
        const unsigned long long kind = next_random(state) % 50;
        if (kind == 0) v = 0.0;                                  // an explicit zero
        if (kind == 1) v = -0.0;                                 // (passes the ">= 0" check; x + 0.0 makes it +0.0 on both sides)
        dense[(size_t)r] = v; rows.push_back(r); vals.push_back(v);
      }
      const double want = dense_lane_sum(dense);
      const double got = f64_shuffle_sparse_colsum_host(rows.data(), vals.data(), (long long)rows.size());
      CHECK(std::memcmp(&want, &got, sizeof(double)) == 0);
      ++columns;
    }
  }
  // a column with exactly 0, 1, 255, 256 and 257 stored entries among 600 rows, and a full block followed by one entry
  for (int count : {0, 1, 255, 256, 257}) {
    std::vector<double> dense(600, 0.0), vals;
    std::vector<int> rows;
    for (int r = 0; r < 600 && (int)rows.size() < count; ++r) {
      if (count < 255 || r % 2 == 0 || 600 - r <= count - (int)rows.size()) {
        const double v = (double)(next_random(state) >> 11) * 0x1p-53 + 0x1p-30;
        dense[(size_t)r] = v; rows.push_back(r); vals.push_back(v);
      }
    }
    CHECK((int)rows.size() == count);
    const double want = dense_lane_sum(dense);
    const double got = f64_shuffle_sparse_colsum_host(rows.data(), vals.data(), (long long)rows.size());
    CHECK(std::memcmp(&want, &got, sizeof(double)) == 0);
    ++columns;
  }
  // the order matters: the plain entry-order sum of such a column differs somewhere (else the check above shows nothing)
  bool differs = false;
  for (int trial = 0; trial < 50 && !differs; ++trial) {
    std::vector<double> dense(700, 0.0);
    double plain = 0.0;
    for (int r = 0; r < 700; ++r) { dense[(size_t)r] = (double)(next_random(state) >> 11) * 0x1p-53; plain += dense[(size_t)r]; }
    const double lanes = dense_lane_sum(dense);
    differs = std::memcmp(&lanes, &plain, sizeof(double)) != 0;
  }
  CHECK(differs);
  return columns;
}
}  // namespace

int main() {
  const int cases = check_struct();
  check_extents();
  const int work = check_workspace();
  const int columns = check_column_sum();
  std::printf("fp64_shuffle_sparse_check: %d refusals, %d workspace cases, %d column sums, all checks passed\n", cases, work, columns);
  return 0;
}
