// Stand-alone host check of csrc/resnmtf_fp64_subsample_job.h: the struct checks of
// resnmtf_fp64_subsample and resnmtf_fp64_relevance that need no device, the range / duplicate checks of the index lists,
// the extents and the overlap test, the gather-form chooser and both workspace layouts.  No HIP call; built with a plain
// C++17 compiler by tests/test_fp64_subsample_check_host.py (and under -fsanitize=address,undefined).  Exits non-zero at
// the first condition that does not hold.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "resnmtf_fp64_subsample_job.h"

#define CHECK(cond)                                                                 \
  do {                                                                              \
    if (!(cond)) {                                                                  \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);                 \
      std::exit(1);                                                                 \
    }                                                                               \
  } while (0)

namespace {
double host_x[6], dev_out[6], rel[4];   // (stand-ins: the struct checks compare pointers with NULL and read nothing)
float dev_x[6];
int counts[2];
const int rows2[2] = {2, 0}, cols2[2] = {1, 0};

resnmtf_fp64_subsample_job sound_host_job() {
  resnmtf_fp64_subsample_job j;
  std::memset(&j, 0, sizeof(j));
  j.struct_size = (int)sizeof(j);
  j.n = 3; j.m = 2; j.n_sub = 2; j.m_sub = 2;
  j.rows = rows2; j.cols = cols2;
  j.x = host_x;
  j.out = dev_out;
  j.n_empty_rows = &counts[0]; j.n_empty_cols = &counts[1];
  return j;
}
resnmtf_fp64_subsample_job sound_device_job() {
  resnmtf_fp64_subsample_job j = sound_host_job();
  j.x = nullptr;
  j.x_dev.ptr = dev_x; j.x_dev.dtype = RESNMTF_DTYPE_F32; j.x_dev.row_stride = 2; j.x_dev.col_stride = 1;
  return j;
}
bool refused(const resnmtf_fp64_subsample_job& j, const char* part) {
  const char* why = f64_subsample_check_job(&j);
  return why && std::strstr(why, part);
}

int check_struct() {
  int cases = 0;
  resnmtf_fp64_subsample_job j = sound_host_job();
  CHECK(f64_subsample_check_job(&j) == nullptr);
  j = sound_device_job();
  CHECK(f64_subsample_check_job(&j) == nullptr);
  CHECK(std::string(f64_subsample_check_job(nullptr)) == "job is NULL"); ++cases;
  j = sound_host_job(); j.struct_size -= 1; CHECK(refused(j, "struct_size mismatch")); ++cases;
  j = sound_host_job(); j.struct_size = 0; CHECK(refused(j, "struct_size mismatch")); ++cases;
  j = sound_host_job(); j.n = 0; CHECK(refused(j, "dimensions must be positive")); ++cases;
  j = sound_host_job(); j.m = -4; CHECK(refused(j, "dimensions must be positive")); ++cases;
  j = sound_host_job(); j.n_sub = 0; CHECK(refused(j, "n_sub must be in [1, n]")); ++cases;
  j = sound_host_job(); j.n_sub = 4; CHECK(refused(j, "n_sub must be in [1, n]")); ++cases;
  j = sound_host_job(); j.m_sub = -1; CHECK(refused(j, "m_sub must be in [1, m]")); ++cases;
  j = sound_host_job(); j.m_sub = 3; CHECK(refused(j, "m_sub must be in [1, m]")); ++cases;
  j = sound_host_job(); j.rows = nullptr; CHECK(refused(j, "rows / cols are NULL")); ++cases;
  j = sound_host_job(); j.cols = nullptr; CHECK(refused(j, "rows / cols are NULL")); ++cases;
  j = sound_host_job(); j.x_dev.ptr = dev_x; CHECK(refused(j, "X is given in two places")); ++cases;
  j = sound_host_job(); j.x = nullptr; CHECK(refused(j, "X is given in no place")); ++cases;
  j = sound_host_job(); j.out = nullptr; CHECK(refused(j, "out is NULL")); ++cases;
  j = sound_device_job(); j.out = nullptr; CHECK(refused(j, "out is NULL")); ++cases;
  j = sound_host_job(); j.n_empty_rows = nullptr; CHECK(refused(j, "n_empty_rows / n_empty_cols are NULL")); ++cases;
  j = sound_host_job(); j.n_empty_cols = nullptr; CHECK(refused(j, "n_empty_rows / n_empty_cols are NULL")); ++cases;
  j = sound_device_job(); j.x_dev.dtype = 4; CHECK(refused(j, "unknown dtype")); ++cases;
  j = sound_device_job(); j.x_dev.dtype = -1; CHECK(refused(j, "unknown dtype")); ++cases;
  j = sound_device_job(); j.x_dev.row_stride = -1; CHECK(refused(j, "strides must be >= 0")); ++cases;
  j = sound_device_job(); j.x_dev.col_stride = -2; CHECK(refused(j, "strides must be >= 0")); ++cases;
  // (the dtype and the strides of x_dev are not read for a host X)
  j = sound_host_job(); j.x_dev.dtype = 9; j.x_dev.row_stride = -1; CHECK(f64_subsample_check_job(&j) == nullptr);
  // masks and the stream may be NULL; strides of 0 (an expanded tensor) are sound; the whole view is a sub-sample
  j = sound_device_job(); j.x_dev.row_stride = 0; j.x_dev.col_stride = 0; CHECK(f64_subsample_check_job(&j) == nullptr);
  j = sound_host_job(); j.n_sub = 3; CHECK(f64_subsample_check_job(&j) == nullptr);
  return cases;
}

int check_indices() {
  int cases = 0;
  const int perm[5] = {4, 0, 3, 1, 2};
  CHECK(f64_subsample_check_indices("rows", perm, 5, 5).empty());
  CHECK(f64_subsample_check_indices("rows", perm, 3, 5).empty());
  CHECK(f64_subsample_check_indices("rows", perm, 1, 5).empty());
  const int one[1] = {0};
  CHECK(f64_subsample_check_indices("cols", one, 1, 1).empty());
  CHECK(f64_subsample_check_indices("rows", perm, 5, 4) == "rows[0] = 4 is out of range [0, 4)"); ++cases;
  const int neg[3] = {1, -1, 0};
  CHECK(f64_subsample_check_indices("cols", neg, 3, 5) == "cols[1] = -1 is out of range [0, 5)"); ++cases;
  const int twice[4] = {2, 0, 2, 0};
  CHECK(f64_subsample_check_indices("rows", twice, 4, 5) == "rows[2] = 2 occurs twice"); ++cases;
  CHECK(f64_subsample_check_indices("rows", twice, 2, 5).empty());            // (only the first `count` are read)
  const int edge[2] = {6, 7};
  CHECK(f64_subsample_check_indices("cols", edge, 2, 7) == "cols[1] = 7 is out of range [0, 7)"); ++cases;
  // the range is tested before the duplicate: an index past the end never indexes the seen-table
  const int both[3] = {9, 9, 1};
  CHECK(f64_subsample_check_indices("rows", both, 3, 5) == "rows[0] = 9 is out of range [0, 5)"); ++cases;
  return cases;
}

void check_extents() {
  resnmtf_fp64_subsample_job j = sound_device_job();        // 3 x 2 fp32 row-major: the last element is 2 * 2 + 1 = 5
  CHECK(f64_matrix_bytes(j.x_dev, j.n, j.m) == 6 * 4);
  CHECK(f64_array_bytes(j.n_sub, j.m_sub) == 4 * 8);
  j.x_dev.row_stride = 0; j.x_dev.col_stride = 0; j.x_dev.dtype = RESNMTF_DTYPE_BF16;
  CHECK(f64_matrix_bytes(j.x_dev, j.n, j.m) == 2);                 // expanded: one element
  j.x_dev.row_stride = 5; j.x_dev.col_stride = 40; j.x_dev.dtype = RESNMTF_DTYPE_F64;
  CHECK(f64_matrix_bytes(j.x_dev, j.n, j.m) == (2 * 5 + 40 + 1) * 8);
  CHECK(f64_array_bytes(50000, 8000) == 3200000000ull);
  CHECK(!f64_array_bytes_overflow(50000, 8000));
  CHECK(f64_array_bytes_overflow(2147483647, 2147483647));               // 8 n m does not fit 64 bits
  CHECK(!f64_array_bytes_overflow(1 << 30, 1 << 30) && f64_array_bytes(1 << 30, 1 << 30) == (1ull << 63));
  CHECK(f64_array_bytes_overflow(1 << 30, (1 << 30) + 1));

  char buf[64];
  CHECK(f64_ranges_overlap(buf, 16, buf + 8, 16));
  CHECK(f64_ranges_overlap(buf + 8, 16, buf, 16));
  CHECK(f64_ranges_overlap(buf, 64, buf + 10, 1));
  CHECK(f64_ranges_overlap(buf, 16, buf + 15, 1));
  CHECK(!f64_ranges_overlap(buf, 16, buf + 16, 16));
  CHECK(!f64_ranges_overlap(buf + 16, 16, buf, 16));

  for (int n : {1, 7, 255, 256, 257}) {
    for (int m : {1, 3, 8, 9}) {
      const F64SubsamplePlan p = f64_subsample_plan(n, m);
      CHECK(p.ints == 0 && p.rows == 16 && p.cols == p.rows + (size_t)n * 4 && p.mask == p.cols + (size_t)m * 4);
      CHECK(p.rows % 4 == 0 && p.cols % 4 == 0);
      CHECK(p.total >= p.mask + (size_t)n + (size_t)m && p.total % 8 == 0 && p.total < p.mask + (size_t)n + (size_t)m + 8);
    }
  }
}

void check_form() {
  // lanes along the destination rows where the source's row stride is the smaller (column-major, a host X) ...
  CHECK(f64_subsample_form(1, 300) == 0);
  CHECK(f64_subsample_form(1, 1) == 0);                     // a single line
  CHECK(f64_subsample_form(0, 0) == 0);                     // expanded both ways
  CHECK(f64_subsample_form(0, 1) == 0);                     // one row expanded over the rows
  CHECK(f64_subsample_form(2, 600) == 0);                   // a strided slice of a column-major tensor
  // ... and the LDS transpose where the column stride is the smaller (row-major)
  CHECK(f64_subsample_form(70, 1) == 1);
  CHECK(f64_subsample_form(140, 2) == 1);
  CHECK(f64_subsample_form(1, 0) == 1);                     // one column expanded over the columns
  // the tiles: the gather's block is whole waves, its LDS tile divides the block, the column sums' tile is one trip
  static_assert(F64_SUB_BLOCK % 64 == 0 && F64_SUB_BLOCK % F64_SUB_TILE == 0, "gather block");
  static_assert(F64_SUB_COLSUM_ROWS * F64_SUB_COLSUM_COLS % F64_SUB_BLOCK == 0 && F64_SUB_BLOCK % F64_SUB_COLSUM_ROWS == 0, "column-sum tile");
  static_assert(F64_SUB_COLSUM_COLS <= 64, "one lane per column of the tile, in one wave");
}

int check_relevance() {
  int cases = 0;
  auto sound = [] {
    resnmtf_fp64_relevance_job j;
    std::memset(&j, 0, sizeof(j));
    j.struct_size = (int)sizeof(j);
    j.n = 3; j.m = 2; j.n_sub = 2; j.m_sub = 2; j.k = 2; j.k_ref = 3;
    j.row_c.ptr = dev_x; j.row_c.dtype = RESNMTF_DTYPE_F32; j.row_c.row_stride = 1; j.row_c.col_stride = 2;
    j.col_c = j.row_c;
    j.true_r = host_x; j.true_c_dev = j.row_c;
    j.rows = rows2; j.cols = cols2;
    j.relevance = rel;
    return j;
  };
  auto refused_rel = [](const resnmtf_fp64_relevance_job& j, const char* part) {
    const char* why = f64_relevance_check_job(&j);
    return why && std::strstr(why, part);
  };
  resnmtf_fp64_relevance_job j = sound();
  CHECK(f64_relevance_check_job(&j) == nullptr);
  CHECK(std::string(f64_relevance_check_job(nullptr)) == "job is NULL"); ++cases;
  j = sound(); j.struct_size += 8; CHECK(refused_rel(j, "struct_size mismatch")); ++cases;
  j = sound(); j.n = 0; CHECK(refused_rel(j, "dimensions must be positive")); ++cases;
  j = sound(); j.n_sub = 4; CHECK(refused_rel(j, "n_sub must be in [1, n]")); ++cases;
  j = sound(); j.m_sub = 0; CHECK(refused_rel(j, "m_sub must be in [1, m]")); ++cases;
  j = sound(); j.k = 0; CHECK(refused_rel(j, "k must be in [1, 64]")); ++cases;
  j = sound(); j.k = 65; CHECK(refused_rel(j, "k must be in [1, 64]")); ++cases;
  j = sound(); j.k_ref = 65; CHECK(refused_rel(j, "k_ref must be in [1, 64]")); ++cases;
  j = sound(); j.k = 64; j.k_ref = 64; CHECK(f64_relevance_check_job(&j) == nullptr);
  j = sound(); j.cols = nullptr; CHECK(refused_rel(j, "rows / cols are NULL")); ++cases;
  j = sound(); j.relevance = nullptr; CHECK(refused_rel(j, "relevance is NULL")); ++cases;
  j = sound(); j.col_c.ptr = nullptr; CHECK(refused_rel(j, "row_c / col_c are NULL")); ++cases;
  j = sound(); j.true_r_dev = j.row_c; CHECK(refused_rel(j, "true_r is given in two places")); ++cases;
  j = sound(); j.true_r = nullptr; CHECK(refused_rel(j, "true_r is given in no place")); ++cases;
  j = sound(); j.true_c = host_x; CHECK(refused_rel(j, "true_c is given in two places")); ++cases;
  j = sound(); j.true_c_dev.ptr = nullptr; CHECK(refused_rel(j, "true_c is given in no place")); ++cases;
  j = sound(); j.row_c.dtype = 7; CHECK(refused_rel(j, "row_c: unknown dtype")); ++cases;
  j = sound(); j.col_c.col_stride = -1; CHECK(refused_rel(j, "col_c: strides must be >= 0")); ++cases;
  j = sound(); j.true_c_dev.dtype = -2; CHECK(refused_rel(j, "true_c_dev: unknown dtype")); ++cases;
  j = sound(); j.true_r_dev.dtype = 9; CHECK(f64_relevance_check_job(&j) == nullptr);      // (not read for a host true_r)

  const double good[6] = {0, 1, 1, 0, 0, 1}, bad[6] = {0, 1, 1, 0.5, 2, 1};
  CHECK(f64_relevance_bad_entry(good, 3, 2) == -1);
  CHECK(f64_relevance_bad_entry(bad, 3, 2) == 3);                // the lowest column-major position: row 0, column 1
  const double nan_in[2] = {0, std::strtod("nan", nullptr)};
  CHECK(f64_relevance_bad_entry(nan_in, 2, 1) == 1);

  j = sound();                                                   // true_r staged (3 x 3 doubles), true_c in place
  F64RelevancePlan p = f64_relevance_plan(j);
  CHECK(p.side_counts == 2 * 3 + 2 + 3);
  CHECK(p.bad == 0 && p.out == 32 && p.true_r == p.out + 3 * 8 && p.true_c == p.true_r + 9 * 8 && p.counts == p.true_c);
  CHECK(p.rows == p.counts + 2 * p.side_counts * 4 && p.cols == p.rows + 2 * 4);
  CHECK(p.total >= p.cols + 2 * 4 && p.total % 8 == 0 && p.counts % 8 == 0 && p.rows % 4 == 0);
  j.true_r = nullptr; j.true_r_dev = j.row_c; j.true_c = host_x; j.true_c_dev.ptr = nullptr;
  p = f64_relevance_plan(j);
  CHECK(p.true_c == p.true_r && p.counts == p.true_c + 2 * 3 * 8);
  j.k = 64; j.k_ref = 64;
  p = f64_relevance_plan(j);
  CHECK(p.side_counts == 64 * 64 + 128);
  return cases;
}
}  // namespace

int main() {
  const int cases = check_struct();
  const int lists = check_indices();
  check_extents();
  check_form();
  const int rel_cases = check_relevance();
  std::printf("fp64_subsample_check: %d refusals, %d index-list refusals, %d relevance refusals, all checks passed\n", cases, lists, rel_cases);
  return 0;
}
