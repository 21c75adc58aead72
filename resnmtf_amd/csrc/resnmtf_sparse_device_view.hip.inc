// resnmtf_sparse_device_view.hip.inc -- a sparse view taken straight from device memory (resnmtf_set_view_sparse_device,
// DESIGN.md section 16).  Included by resnmtf_hip.hip after resnmtf_sparse_subsample.hip.inc (it uses load_wide of
// resnmtf_device_view.hip.inc; the build itself is finish_sparse_build, shared with the sparse shuffle and sub-sample).
//
// The caller's arrays -- CSC, CSR or COO, int32 or int64 indices, four value types, entries in any order -- are checked
// where they lie and turned into what finish_sparse_build takes: key[e] = c n + r (column-major position, distinct) and the
// value widened to fp64.  Sorted by that key the entries ARE the canonical CSC, so the view is bit for bit
// resnmtf_set_view_csc of it.
//   1. sparse_device_ptr_check_kernel   one thread per line pointer: ptr[0] = 0, monotone, ptr[lines] = nnz.  Its verdict
//                                       is read back before any kernel uses a pointer entry as a bound;
//   2. sparse_device_entries_kernel     one thread per stored entry: its line (COO: read; compressed: the last line whose
//                                       pointer is <= e, a binary search in the validated pointers), both indices against
//                                       [0, n) x [0, m), the value finite and >= 0, then key, value, the column's
//                                       "has an entry > 0" byte and (CSC) the "not strictly ascending" flag;
//   3. sparse_device_columns_kernel     one thread per column: a column without an entry > 0 (pre_processed = 0);
//   4. sparse_device_duplicates_kernel  one thread per sorted entry: key[q] == key[q - 1].
// No load's address derives from an unchecked index or pointer entry: idx / values are read at e < nnz only, the search
// reads ptr[1 .. lines - 1], and an index is used (as the column flag's address) only after its range check.
// A failure is ONE 64-bit word, kind << 56 | lowest offending entry or line, combined with an integer atomicMin from the
// initial ~0: the lowest kind wins, then the lowest number, so the message is the same on every run.

enum : unsigned long long {
  SPDV_PTR_FIRST = 1,      // ptr[0] != 0
  SPDV_PTR_MONOTONE = 2,   // ptr[line + 1] < ptr[line]
  SPDV_PTR_LAST = 3,       // ptr[lines] != nnz
  SPDV_ROW_RANGE = 4,      // entry e: row index outside [0, n)
  SPDV_COL_RANGE = 5,      // entry e: column index outside [0, m)
  SPDV_NON_FINITE = 6,     // entry e
  SPDV_NEGATIVE = 7,       // entry e
  SPDV_DUPLICATE = 8,      // sorted position q: the same (row, column) as q - 1
  SPDV_ZERO_COLUMN = 9,    // column j holds no entry > 0
};
constexpr unsigned long long kSpdvNone = ~0ull;
__device__ __forceinline__ void spdv_fail(unsigned long long* word, unsigned long long kind, long long where) {
  atomicMin(word, (kind << 56) | (unsigned long long)where);
}
template <bool I64>
__device__ __forceinline__ long long load_index(const void* __restrict__ a, long long i) {
  if constexpr (I64) return static_cast<const long long*>(a)[i];
  else return (long long)static_cast<const int*>(a)[i];
}

// one thread per pointer entry j = 0 .. lines
template <bool I64>
static __global__ __launch_bounds__(256) void sparse_device_ptr_check_kernel(const void* __restrict__ ptr, int lines, long long nnz,
                                                                             unsigned long long* __restrict__ word) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j > lines) return;
  const long long p = load_index<I64>(ptr, j);
  if (j == 0 && p != 0) spdv_fail(word, SPDV_PTR_FIRST, 0);
  if (j == lines) { if (p != nnz) spdv_fail(word, SPDV_PTR_LAST, lines); }
  else if (load_index<I64>(ptr, j + 1) < p) spdv_fail(word, SPDV_PTR_MONOTONE, j);
}

// LAYOUT: RESNMTF_SPARSE_CSC / _CSR / _COO.  a0 = the line pointers (COO: the row indices), a1 = the index of every entry
// in its line (COO: the column indices).  flags[0] = the failure word, flags[1] = 1 when a CSC column's rows do not ascend
// strictly (many threads may store the same 1); col_pos[c] = 1 when column c holds an entry > 0 (NULL: not asked for).
template <int LAYOUT, bool I64, int DT>
static __global__ __launch_bounds__(256) void sparse_device_entries_kernel(const void* __restrict__ a0, const void* __restrict__ a1,
                                                                           const void* __restrict__ values, long long nnz, int n, int m,
                                                                           unsigned long long* __restrict__ key, double* __restrict__ val,
                                                                           unsigned char* __restrict__ col_pos,
                                                                           unsigned long long* __restrict__ flags) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= nnz) return;
  long long r, c;
  if constexpr (LAYOUT == RESNMTF_SPARSE_COO) {
    r = load_index<I64>(a0, e);
    c = load_index<I64>(a1, e);
  } else {
    const int lines = LAYOUT == RESNMTF_SPARSE_CSC ? m : n;
    int lo = 0, hi = lines;                              // ptr[lo] <= e < ptr[hi] (validated: ptr[0] = 0, ptr[lines] = nnz)
    while (hi - lo > 1) {
      const int mid = lo + (hi - lo) / 2;
      if (load_index<I64>(a0, mid) <= e) lo = mid; else hi = mid;
    }
    const long long i = load_index<I64>(a1, e);
    if constexpr (LAYOUT == RESNMTF_SPARSE_CSC) {
      r = i; c = lo;
      // the keys ascend strictly iff the rows do within every column (the columns ascend with e by themselves)
      if (e > load_index<I64>(a0, lo) && load_index<I64>(a1, e - 1) >= i) flags[1] = 1ull;      // (ptr[lo] >= 0: e - 1 >= 0)
    } else { r = lo; c = i; }
  }
  const double x = load_wide<DT>(values, e);
  if (r < 0 || r >= n) { spdv_fail(flags, SPDV_ROW_RANGE, e); return; }
  if (c < 0 || c >= m) { spdv_fail(flags, SPDV_COL_RANGE, e); return; }
  if (!(fabs(x) <= 1.79769313486231570815e+308)) { spdv_fail(flags, SPDV_NON_FINITE, e); return; }   // NaN, +-inf
  if (x < 0.0) { spdv_fail(flags, SPDV_NEGATIVE, e); return; }
  key[e] = (unsigned long long)c * (unsigned long long)n + (unsigned long long)r;
  val[e] = x;
  if (col_pos && x > 0.0) col_pos[c] = 1;
}

static __global__ __launch_bounds__(256) void sparse_device_columns_kernel(const unsigned char* __restrict__ col_pos, int m,
                                                                           unsigned long long* __restrict__ word) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j < m && !col_pos[j]) spdv_fail(word, SPDV_ZERO_COLUMN, j);
}

// after the first sort: equal neighbours are one position stored twice
static __global__ __launch_bounds__(256) void sparse_device_duplicates_kernel(const unsigned long long* __restrict__ key, long long nnz,
                                                                              unsigned long long* __restrict__ word) {
  const long long q = (long long)blockIdx.x * 256 + threadIdx.x + 1;
  if (q < nnz && key[q] == key[q - 1]) spdv_fail(word, SPDV_DUPLICATE, q);
}
