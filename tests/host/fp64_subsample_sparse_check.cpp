// Stand-alone host check of csrc/resnmtf_fp64_subsample_sparse_job.h: the struct checks of
// resnmtf_fp64_subsample_sparse that need no device, count mode against fill mode, the index-list checks it shares with
// resnmtf_fp64_subsample, the extents of its outputs and of a device view's arrays, the overlap test, the workspace
// regions (each claimed once and large enough) and the transient byte count.  No HIP call; built with a plain C++17
// compiler by tests/test_fp64_subsample_sparse_check_host.py (and under -fsanitize=address,undefined).  Exits non-zero at
// the first condition that does not hold.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "resnmtf_fp64_subsample_sparse_job.h"

#define CHECK(cond)                                                                 \
  do {                                                                              \
    if (!(cond)) {                                                                  \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);                 \
      std::exit(1);                                                                 \
    }                                                                               \
  } while (0)

namespace {
// (stand-ins: the struct checks compare pointers with NULL and read nothing)
long long host_ptr[4], dev_ptr[4], out_ptr[3], out_idx[6], kept;
int host_idx[6], rows[4] = {4, 0, 2, 1}, cols[2] = {2, 0};
double host_val[6], out_val[6];
float dev_val[6];
int counts[2];

resnmtf_fp64_subsample_sparse_job sound_host_job() {
  resnmtf_fp64_subsample_sparse_job j;
  std::memset(&j, 0, sizeof(j));
  j.struct_size = (int)sizeof(j);
  j.n = 5; j.m = 3; j.n_sub = 4; j.m_sub = 2;
  j.rows = rows; j.cols = cols;
  j.x.col_ptr = host_ptr; j.x.row_idx = host_idx; j.x.values = host_val;
  j.out_col_ptr = out_ptr; j.out_row_idx = out_idx; j.out_values = out_val; j.out_capacity = 6;
  j.nnz_sub = &kept;
  j.n_empty_rows = &counts[0]; j.n_empty_cols = &counts[1];
  return j;
}
resnmtf_fp64_subsample_sparse_job sound_device_job() {
  resnmtf_fp64_subsample_sparse_job j = sound_host_job();
  j.x.col_ptr = nullptr; j.x.row_idx = nullptr; j.x.values = nullptr;
  j.x_dev.layout = RESNMTF_SPARSE_CSC; j.x_dev.index_type = RESNMTF_INDEX_I64; j.x_dev.dtype = RESNMTF_DTYPE_F32;
  j.x_dev.ptr_or_rows = dev_ptr; j.x_dev.idx_or_cols = out_idx; j.x_dev.values = dev_val; j.x_dev.nnz = 6;
  return j;
}
resnmtf_fp64_subsample_sparse_job count_job() {
  resnmtf_fp64_subsample_sparse_job j = sound_host_job();
  j.out_col_ptr = nullptr; j.out_row_idx = nullptr; j.out_values = nullptr; j.out_capacity = 0;
  return j;
}
bool refused(const resnmtf_fp64_subsample_sparse_job& j, const char* text) {
  const char* why = f64_subsample_sparse_check_job(&j);
  return why && std::string(why) == text;
}

int check_struct() {
  int cases = 0;
  resnmtf_fp64_subsample_sparse_job j = sound_host_job();
  CHECK(f64_subsample_sparse_check_job(&j) == nullptr && !f64_subsample_sparse_count_mode(j));
  j = sound_device_job();
  CHECK(f64_subsample_sparse_check_job(&j) == nullptr);
  j = count_job();
  CHECK(f64_subsample_sparse_check_job(&j) == nullptr && f64_subsample_sparse_count_mode(j));
  CHECK(std::string(f64_subsample_sparse_check_job(nullptr)) == "job is NULL"); ++cases;
  j = sound_host_job(); j.struct_size -= 1; CHECK(refused(j, "resnmtf_fp64_subsample_sparse_job struct_size mismatch")); ++cases;
  j = sound_host_job(); j.struct_size = (int)sizeof(resnmtf_fp64_subsample_job);
  CHECK(refused(j, "resnmtf_fp64_subsample_sparse_job struct_size mismatch")); ++cases;
  // the extents and the lists: resnmtf_fp64_subsample's texts
  resnmtf_fp64_subsample_job dense;
  std::memset(&dense, 0, sizeof(dense));
  dense.struct_size = (int)sizeof(dense);
  j = sound_host_job(); j.n = 0; CHECK(refused(j, "view dimensions must be positive")); ++cases;
  CHECK(std::string(f64_subsample_check_job(&dense)) == "view dimensions must be positive");
  j = sound_device_job(); j.m = -4; CHECK(refused(j, "view dimensions must be positive")); ++cases;
  dense.n = 5; dense.m = 3;
  j = sound_host_job(); j.n_sub = 0; CHECK(refused(j, "n_sub must be in [1, n]")); ++cases;
  CHECK(std::string(f64_subsample_check_job(&dense)) == "n_sub must be in [1, n]");
  j = sound_host_job(); j.n_sub = 6; CHECK(refused(j, "n_sub must be in [1, n]")); ++cases;
  dense.n_sub = 4;
  j = sound_host_job(); j.m_sub = 4; CHECK(refused(j, "m_sub must be in [1, m]")); ++cases;
  CHECK(std::string(f64_subsample_check_job(&dense)) == "m_sub must be in [1, m]");
  j = sound_host_job(); j.m_sub = 0; CHECK(refused(j, "m_sub must be in [1, m]")); ++cases;
  dense.m_sub = 2;
  j = sound_host_job(); j.rows = nullptr; CHECK(refused(j, "rows / cols are NULL")); ++cases;
  CHECK(std::string(f64_subsample_check_job(&dense)) == "rows / cols are NULL");
  j = sound_device_job(); j.cols = nullptr; CHECK(refused(j, "rows / cols are NULL")); ++cases;
  // the source and the outputs: resnmtf_fp64_shuffle_sparse's texts
  j = sound_device_job(); j.x.col_ptr = host_ptr; CHECK(refused(j, "X is given in two places (job->x and job->x_dev)")); ++cases;
  j = sound_host_job(); j.x_dev.nnz = 1; CHECK(refused(j, "X is given in two places (job->x and job->x_dev)")); ++cases;
  j = sound_host_job(); j.x.col_ptr = nullptr; CHECK(refused(j, "X is given in no place (job->x or job->x_dev)")); ++cases;
  j = sound_host_job(); j.out_capacity = -1; CHECK(refused(j, "out_capacity is negative")); ++cases;
  j = sound_host_job(); j.out_col_ptr = nullptr; CHECK(refused(j, "out_col_ptr is NULL")); ++cases;           // fill mode: the others are given
  j = count_job(); j.out_capacity = 3; CHECK(refused(j, "out_col_ptr is NULL")); ++cases;                     // a capacity alone is fill mode
  j = sound_host_job(); j.out_row_idx = nullptr; CHECK(refused(j, "out_row_idx / out_values are NULL")); ++cases;
  j = sound_device_job(); j.out_values = nullptr; CHECK(refused(j, "out_row_idx / out_values are NULL")); ++cases;
  // with a capacity of 0 the two arrays may be NULL in fill mode: the pointers are still written
  j = sound_host_job(); j.out_row_idx = nullptr; j.out_values = nullptr; j.out_capacity = 0;
  CHECK(f64_subsample_sparse_check_job(&j) == nullptr && !f64_subsample_sparse_count_mode(j));
  j = sound_host_job(); j.nnz_sub = nullptr; CHECK(refused(j, "nnz_sub is NULL")); ++cases;
  j = count_job(); j.nnz_sub = nullptr; CHECK(refused(j, "nnz_sub is NULL")); ++cases;
  j = sound_host_job(); j.n_empty_rows = nullptr; CHECK(refused(j, "n_empty_rows / n_empty_cols are NULL")); ++cases;
  j = count_job(); j.n_empty_cols = nullptr; CHECK(refused(j, "n_empty_rows / n_empty_cols are NULL")); ++cases;
  // the masks and the stream may be NULL; what a device view holds is judged by the run's own checks, not here
  j = sound_device_job(); j.x_dev.layout = 9; j.x_dev.dtype = 17; CHECK(f64_subsample_sparse_check_job(&j) == nullptr);
  return cases;
}

int check_lists() {
  int cases = 0;
  const int good[4] = {4, 0, 2, 1};
  CHECK(f64_subsample_check_indices("rows", good, 4, 5).empty());
  const int high[3] = {0, 5, 1};
  CHECK(f64_subsample_check_indices("rows", high, 3, 5) == "rows[1] = 5 is out of range [0, 5)"); ++cases;
  const int low[2] = {-1, 0};
  CHECK(f64_subsample_check_indices("cols", low, 2, 3) == "cols[0] = -1 is out of range [0, 3)"); ++cases;
  const int twice[4] = {2, 0, 1, 0};
  CHECK(f64_subsample_check_indices("cols", twice, 4, 3) == "cols[3] = 0 occurs twice"); ++cases;
  return cases;
}

void check_extents() {
  resnmtf_fp64_subsample_sparse_job j = sound_device_job();       // 4 x 2 of 5 x 3, capacity 6, CSC int64 fp32
  F64ShuffleSparseRange out[3], in[3];
  f64_subsample_sparse_outputs(j, out);
  CHECK(out[0].ptr == out_ptr && out[0].bytes == 3 * 8 && out[1].ptr == out_idx && out[1].bytes == 6 * 8);
  CHECK(out[2].ptr == out_val && out[2].bytes == 6 * 8 && std::string(out[2].name) == "out_values");
  j.out_capacity = 0;
  f64_subsample_sparse_outputs(j, out);
  CHECK(out[0].bytes == 3 * 8 && out[1].bytes == 0 && out[2].bytes == 0);
  resnmtf_fp64_subsample_sparse_job c = count_job();
  f64_subsample_sparse_outputs(c, out);
  CHECK(out[0].bytes == 0 && out[1].bytes == 0 && out[2].bytes == 0);
  // the arrays of a device view are those of the n x m source, not of the sub-sample
  f64_subsample_sparse_sources(j, in);
  CHECK(in[0].ptr == dev_ptr && in[0].bytes == 4 * 8 && in[1].bytes == 6 * 8 && in[2].bytes == 6 * 4);
  j.x_dev.layout = RESNMTF_SPARSE_CSR; j.x_dev.index_type = RESNMTF_INDEX_I32; j.x_dev.dtype = RESNMTF_DTYPE_BF16;
  f64_subsample_sparse_sources(j, in);
  CHECK(in[0].bytes == 6 * 4 && in[1].bytes == 6 * 4 && in[2].bytes == 6 * 2);
  j.x_dev.layout = RESNMTF_SPARSE_COO; j.x_dev.dtype = RESNMTF_DTYPE_F64;
  f64_subsample_sparse_sources(j, in);
  CHECK(in[0].bytes == 6 * 4 && in[1].bytes == 6 * 4 && in[2].bytes == 6 * 8 && std::string(in[2].name) == "x_dev.values");
  j = sound_host_job(); j.n = 200000; j.m = 20000; j.n_sub = 180000; j.m_sub = 18000; j.out_capacity = 40000000ll;
  f64_subsample_sparse_outputs(j, out);
  CHECK(out[0].bytes == 18001ull * 8 && out[1].bytes == 320000000ull && out[2].bytes == 320000000ull);
  // the bound of the kept entries: every stored entry or every position, 64-bit
  CHECK(f64_subsample_sparse_bound(4, 2, 6) == 6 && f64_subsample_sparse_bound(4, 2, 9) == 8 && f64_subsample_sparse_bound(4, 2, 0) == 0);
  CHECK(f64_subsample_sparse_bound(70000, 70000, 5000000000ull) == 4900000000ull);

  // overlaps: the outputs with each other, then with the arrays of a device view (section 30's test, on these ranges)
  char buf[256];
  const char *a = nullptr, *b = nullptr;
  out[0] = {"out_col_ptr", buf, 32}; out[1] = {"out_row_idx", buf + 32, 32}; out[2] = {"out_values", buf + 64, 32};
  CHECK(!f64_shuffle_sparse_overlap(out, nullptr, a, b));
  out[1].ptr = buf + 31;
  CHECK(f64_shuffle_sparse_overlap(out, nullptr, a, b) && std::string(a) == "out_col_ptr" && std::string(b) == "out_row_idx");
  out[1].ptr = buf + 32;
  in[0] = {"x_dev.ptr_or_rows", buf + 96, 32}; in[1] = {"x_dev.idx_or_cols", buf + 128, 32}; in[2] = {"x_dev.values", buf + 95, 32};
  CHECK(f64_shuffle_sparse_overlap(out, in, a, b) && std::string(a) == "out_values" && std::string(b) == "x_dev.values");
  in[2].ptr = buf + 160;
  CHECK(!f64_shuffle_sparse_overlap(out, in, a, b));
  // count mode: no output range, so nothing overlaps whatever the view's arrays are
  f64_subsample_sparse_outputs(c, out);
  in[0].ptr = nullptr;
  CHECK(!f64_shuffle_sparse_overlap(out, in, a, b));
}

// the regions of the workspace: each inside [0, total), pairwise disjoint, aligned, and as large as its user needs
int check_workspace() {
  int cases = 0;
  for (int n : {1, 7, 257, 70000}) {
    for (int ns : {1, 5, 256, 70000}) {
      if (ns > n) continue;
      for (int ms : {1, 3, 255, 256, 257, 1025, 65536}) {
        const F64SubsampleSparsePlan p = f64_subsample_sparse_plan(n, ns, ms);
        struct Region { size_t at, bytes, align; };
        const Region r[7] = {{p.counts, (size_t)ms * 8, 8}, {p.scan, ((size_t)ms + 1) * 8, 8}, {p.inv_row, (size_t)n * 4, 4},
                             {p.rows, (size_t)ns * 4, 4}, {p.cols, (size_t)ms * 4, 4}, {p.ints, 4 * sizeof(int), 4},
                             {p.mask, (size_t)ns + (size_t)ms, 1}};
        for (int x = 0; x < 7; ++x) {
          CHECK(r[x].at % r[x].align == 0 && r[x].at + r[x].bytes <= p.total);
          for (int y = x + 1; y < 7; ++y) CHECK(r[x].at + r[x].bytes <= r[y].at || r[y].at + r[y].bytes <= r[x].at);
        }
        CHECK(p.total % 8 == 0 && p.total < p.mask + (size_t)ns + (size_t)ms + 8);
        ++cases;
      }
    }
  }
  CHECK(F64_SUBSAMPLE_SPARSE_TRIP == 64 && F64_SUBSAMPLE_SPARSE_SCAN_BLOCK == 256 && F64_SUBSAMPLE_SPARSE_WAVES * 64 <= 1024);
  // the transient memory: per stored entry the source (4 + 8), 48 while a device source is built; per kept entry the
  // COO (4 + 4 + 8) and the canonicaliser's arrays (5 x 8 + 2 x 4)
  CHECK(F64_SUBSAMPLE_SPARSE_BYTES_PER_STORED == 4 + 8 && F64_SUBSAMPLE_SPARSE_BYTES_PER_STORED_BUILD == 5 * 8 + 2 * 4);
  CHECK(F64_SUBSAMPLE_SPARSE_BYTES_PER_KEPT == (4 + 4 + 8) + (5 * 8 + 2 * 4));
  CHECK(F64_SUBSAMPLE_SPARSE_BYTES_PER_STORED_BUILD + 20 == F64_SHUFFLE_SPARSE_BYTES_PER_ENTRY);       // (section 30 holds both at once)
  // a host source: 12 per stored entry and its pointers; nothing per kept entry in count mode (bound 0)
  CHECK(f64_subsample_sparse_transient_bytes(5, 3, 4, 2, 10, 0) == 10 * 12 + 4 * 8);
  CHECK(f64_subsample_sparse_transient_bytes(5, 3, 4, 2, 10, 8) == 10 * 12 + 4 * 8 + 8 * 64 + (3 + 5) * 8 + 24);
  // a device source: the larger of its build and of the sorted sub-sample beside the canonical source
  CHECK(f64_subsample_sparse_transient_bytes(5, 3, 4, 2, 10, 0, true) == 10 * 48 + 4 * 8 + 6 * 8 + 24);
  CHECK(f64_subsample_sparse_transient_bytes(5, 3, 4, 2, 10, 8, true) == 10 * 12 + 4 * 8 + 24 + 8 * 64 + (3 + 5) * 8 + 24);
  CHECK(f64_subsample_sparse_transient_bytes(200000, 20000, 180000, 18000, 40000000ull, 32400000ull) ==
        40000000ull * 12 + 20001ull * 8 + 32400000ull * 64 + (18001ull + 180001ull) * 8 + 24);
  return cases;
}
}  // namespace

int main() {
  const int cases = check_struct();
  const int lists = check_lists();
  check_extents();
  const int work = check_workspace();
  std::printf("fp64_subsample_sparse_check: %d refusals, %d list refusals, %d workspace cases, all checks passed\n", cases, lists, work);
  return 0;
}
