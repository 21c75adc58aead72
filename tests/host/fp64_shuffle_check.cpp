// Stand-alone host check of csrc/resnmtf_fp64_shuffle_job.h and csrc/resnmtf_feistel.h: the struct
// checks of resnmtf_fp64_shuffle that need no device, the extents and the overlap test, the workspace layout, and the
// permutation the device shuffles run -- a bijection on [0, count) for every count in 1 .. 4100 and three seeds, with
// inverse(forward(i)) = i.  No HIP call; built with a plain C++17 compiler by tests/test_fp64_shuffle_check_host.py (and
// under -fsanitize=address,undefined).  Exits non-zero at the first condition that does not hold.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "resnmtf_feistel.h"
#include "resnmtf_fp64_shuffle_job.h"

#define CHECK(cond)                                                                 \
  do {                                                                              \
    if (!(cond)) {                                                                  \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);                 \
      std::exit(1);                                                                 \
    }                                                                               \
  } while (0)

namespace {
double host_x[6], dev_out[6];          // (stand-ins: the struct checks compare pointers with NULL and read nothing)
float dev_x[6];
int counts[2];

resnmtf_fp64_shuffle_job sound_host_job() {
  resnmtf_fp64_shuffle_job j;
  std::memset(&j, 0, sizeof(j));
  j.struct_size = (int)sizeof(j);
  j.n = 3; j.m = 2; j.normalise = 1; j.seed = 7;
  j.x = host_x;
  j.out = dev_out;
  j.n_empty_rows = &counts[0]; j.n_empty_cols = &counts[1];
  return j;
}
resnmtf_fp64_shuffle_job sound_device_job() {
  resnmtf_fp64_shuffle_job j = sound_host_job();
  j.x = nullptr;
  j.x_dev.ptr = dev_x; j.x_dev.dtype = RESNMTF_DTYPE_F32; j.x_dev.row_stride = 2; j.x_dev.col_stride = 1;
  return j;
}
bool refused(const resnmtf_fp64_shuffle_job& j, const char* part) {
  const char* why = f64_shuffle_check_job(&j);
  return why && std::strstr(why, part);
}

int check_struct() {
  int cases = 0;
  resnmtf_fp64_shuffle_job j = sound_host_job();
  CHECK(f64_shuffle_check_job(&j) == nullptr);
  j = sound_device_job();
  CHECK(f64_shuffle_check_job(&j) == nullptr);
  CHECK(std::string(f64_shuffle_check_job(nullptr)) == "job is NULL"); ++cases;
  j = sound_host_job(); j.struct_size -= 1; CHECK(refused(j, "struct_size mismatch")); ++cases;
  j = sound_host_job(); j.struct_size = 0; CHECK(refused(j, "struct_size mismatch")); ++cases;
  j = sound_host_job(); j.n = 0; CHECK(refused(j, "dimensions must be positive")); ++cases;
  j = sound_host_job(); j.m = -4; CHECK(refused(j, "dimensions must be positive")); ++cases;
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
  j = sound_host_job(); j.x_dev.dtype = 9; j.x_dev.row_stride = -1; CHECK(f64_shuffle_check_job(&j) == nullptr);
  // masks, was_negative and the stream may be NULL; strides of 0 (an expanded tensor) are sound
  j = sound_device_job(); j.x_dev.row_stride = 0; j.x_dev.col_stride = 0; CHECK(f64_shuffle_check_job(&j) == nullptr);
  // n m never exceeds the Feistel domain for int extents: the largest is (2^31 - 1)^2 < 2^62
  j = sound_host_job(); j.n = 2147483647; j.m = 2147483647; CHECK(f64_shuffle_check_job(&j) == nullptr);
  CHECK((unsigned long long)j.n * (unsigned long long)j.m < F64_SHUFFLE_MAX_COUNT);
  CHECK(feistel_half_bits((unsigned long long)j.n * (unsigned long long)j.m) == 31);
  return cases;
}

void check_extents() {
  resnmtf_fp64_shuffle_job j = sound_device_job();          // 3 x 2 fp32 row-major: the last element is 2 * 2 + 1 = 5
  CHECK(f64_shuffle_source_bytes(j) == 6 * 4);
  CHECK(f64_shuffle_out_bytes(j) == 6 * 8);
  j.x_dev.row_stride = 0; j.x_dev.col_stride = 0; j.x_dev.dtype = RESNMTF_DTYPE_BF16;
  CHECK(f64_shuffle_source_bytes(j) == 2);                  // expanded: one element
  j.x_dev.row_stride = 5; j.x_dev.col_stride = 40; j.x_dev.dtype = RESNMTF_DTYPE_F64;
  CHECK(f64_shuffle_source_bytes(j) == (2 * 5 + 40 + 1) * 8);
  j.n = 50000; j.m = 8000;
  CHECK(f64_shuffle_out_bytes(j) == 3200000000ull);
  CHECK(!f64_shuffle_bytes_overflow(j));
  j.n = 2147483647; j.m = 2147483647;                      // 8 n m does not fit 64 bits: said so, never computed
  CHECK(f64_shuffle_bytes_overflow(j));
  j.n = 1 << 30; j.m = 1 << 30;
  CHECK(!f64_shuffle_bytes_overflow(j) && f64_shuffle_out_bytes(j) == (1ull << 63));
  j.m = (1 << 30) + 1;
  CHECK(f64_shuffle_bytes_overflow(j));

  char buf[64];
  CHECK(f64_shuffle_overlap(buf, 16, buf + 8, 16));
  CHECK(f64_shuffle_overlap(buf + 8, 16, buf, 16));
  CHECK(f64_shuffle_overlap(buf, 64, buf + 10, 1));
  CHECK(f64_shuffle_overlap(buf, 16, buf + 15, 1));
  CHECK(!f64_shuffle_overlap(buf, 16, buf + 16, 16));
  CHECK(!f64_shuffle_overlap(buf + 16, 16, buf, 16));

  for (int n : {1, 7, 255, 256, 257}) {
    for (int m : {1, 3, 8, 9}) {
      const F64ShufflePlan p = f64_shuffle_plan(n, m);
      CHECK(p.shift == 0 && p.colsum == (size_t)m * 8 && p.ints == (size_t)m * 16);
      CHECK(p.mask == p.ints + 16 && p.mask % 8 == 0);
      CHECK(p.total >= p.mask + (size_t)n + (size_t)m && p.total % 8 == 0 && p.total < p.mask + (size_t)n + (size_t)m + 8);
    }
  }
}

int check_feistel() {
  const unsigned long long seeds[3] = {0ull, 1ull, 0xFFFFFFFFFFFFFFFFull};
  std::vector<unsigned char> hit;
  int walked = 0;
  for (unsigned long long count = 1; count <= 4100; ++count) {
    const int hb = feistel_half_bits(count);
    CHECK(hb >= 1 && (1ull << (2 * hb)) >= count);
    CHECK(hb == 1 || (1ull << (2 * (hb - 1))) < count);       // the smallest domain that holds count
    if ((1ull << (2 * hb)) > count) ++walked;
    for (unsigned long long seed : seeds) {
      hit.assign((size_t)count, 0);
      for (unsigned long long i = 0; i < count; ++i) {
        const unsigned long long j = feistel_perm(i, count, hb, seed);
        CHECK(j < count);
        CHECK(!hit[(size_t)j]);
        hit[(size_t)j] = 1;
        CHECK(feistel_perm_inverse(j, count, hb, seed) == i);
      }
    }
  }
  // different seeds give different permutations of a domain that leaves room for it
  bool differ = false;
  for (unsigned long long i = 0; i < 1024 && !differ; ++i) differ = feistel_perm(i, 1024, 5, 0) != feistel_perm(i, 1024, 5, 1);
  CHECK(differ);
  return walked;
}
}  // namespace

int main() {
  const int cases = check_struct();
  check_extents();
  const int walked = check_feistel();
  std::printf("fp64_shuffle_check: %d refusals, 4100 counts (%d with a cycle walk) x 3 seeds, all checks passed\n", cases, walked);
  return 0;
}
