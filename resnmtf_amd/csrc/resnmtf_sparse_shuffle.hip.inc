// resnmtf_sparse_shuffle.hip.inc -- shuffle_view (R/obtain_bicl.r:11-22) of a sparse view that stays sparse
// (resnmtf_shuffle_view_sparse, DESIGN.md section 10 "Sparse shuffles").  Included by resnmtf_hip.hip after
// resnmtf_sparse.hip.inc (it uses feistel_perm's constants and the upload kernels csc_normalise_kernel / csr_gather_kernel).
//
// The shuffle is the dense path's shuffle of the densified view: staging[i] = X[pi(i)], i column-major in the destination,
// pi(i) row-major in the source (shuffle_gather_kernel).  A stored source entry at (r, c) therefore lands at
// i = pi^-1(r m + c); only the nnz stored entries move, explicit zeros included, and no dense image exists at any point.
//   1. sparse_shuffle_keys_kernel: one thread per stored entry of the source CSC -> its destination position i (64-bit:
//      n m may exceed 2^32) and its value as fp64;
//   2. the entries sorted by i (rocprim::radix_sort_pairs, value = payload) ARE the CSC of the shuffle: column i / n, row
//      i % n, ascending rows within a column.  The keys are distinct (pi is a bijection), so the sorted order is unique
//      and every correct sort gives the same bits;
//   3. sparse_shuffle_csr_keys_kernel: the CSR key r' m + c' of every CSC position and the position itself as payload;
//      sorted by that key they are the CSR: column indices and the permutation csr_gather_kernel consumes;
//   4. sorted_lines_kernel: line pointers and line-local indices from sorted keys (boundary detection, no atomics);
//   5. sparse_empty_lines_kernel: the redraw condition of shuffle_view (:14-18).
// No float atomics anywhere; the two counts of empty lines are integer atomics, as in empty_lines_kernel.

// The inverse of feistel_perm, feistel_perm_inverse, is csrc/resnmtf_feistel.h, beside the permutation itself.

// one thread per stored entry e of the source CSC: its column from cp (the last column whose pointer is <= e), then
// key[e] = pi^-1(r m + c) and val[e] = (double)vcsc[e]
static __global__ __launch_bounds__(256) void sparse_shuffle_keys_kernel(const long long* __restrict__ cp, const int* __restrict__ ri,
                                                                         const float* __restrict__ vcsc, long long nnz, int n, int m,
                                                                         unsigned long long seed, unsigned long long* __restrict__ key,
                                                                         double* __restrict__ val) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= nnz) return;
  int lo = 0, hi = m;                                  // cp[lo] <= e < cp[hi] (cp[0] = 0, cp[m] = nnz)
  while (hi - lo > 1) {
    const int mid = lo + (hi - lo) / 2;
    if (cp[mid] <= e) lo = mid; else hi = mid;
  }
  const unsigned long long count = (unsigned long long)n * m;
  int half_bits = 1;
  while ((1ull << (2 * half_bits)) < count) ++half_bits;
  key[e] = feistel_perm_inverse((unsigned long long)ri[e] * m + lo, count, half_bits, seed);
  val[e] = (double)vcsc[e];
}

// CSC position q holds destination position i = key[q] (column-major): its CSR key r' m + c' and q itself as payload
static __global__ __launch_bounds__(256) void sparse_shuffle_csr_keys_kernel(const unsigned long long* __restrict__ key, long long nnz,
                                                                             int n, int m, unsigned long long* __restrict__ csr_key,
                                                                             long long* __restrict__ pos) {
  const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
  if (q >= nnz) return;
  const unsigned long long i = key[q];
  csr_key[q] = (i % (unsigned long long)n) * m + i / (unsigned long long)n;
  pos[q] = q;
}

// Sorted keys = line * div + idx (CSC: i = c' n + r', div = n; CSR: r' m + c', div = m): idx[q] and the line pointers
// ptr[0 .. lines].  A thread that sees the line change between its left neighbour and itself writes the pointers of every
// line in between (its own included, the first entry those of lines 0 .. its own); the last entry also those of the lines
// after its own and ptr[lines].  Every pointer is written exactly once.  nnz >= 1.
static __global__ __launch_bounds__(256) void sorted_lines_kernel(const unsigned long long* __restrict__ key, long long nnz,
                                                                  unsigned long long div, int lines, long long* __restrict__ ptr,
                                                                  int* __restrict__ idx) {
  const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
  if (q >= nnz) return;
  const unsigned long long k = key[q];
  const long long line = (long long)(k / div);
  idx[q] = (int)(k % div);
  const long long prev = q == 0 ? -1 : (long long)(key[q - 1] / div);
  for (long long j = prev + 1; j <= line; ++j) ptr[j] = q;
  if (q == nnz - 1)
    for (long long j = line + 1; j <= lines; ++j) ptr[j] = nnz;
}

// The redraw condition of shuffle_view (R/obtain_bicl.r:14-18) on the shuffled entries BEFORE normalisation: a line is
// empty when it holds no stored entry with a value > 0 (the values are non-negative: "sums to exactly zero", the dense
// path's test in empty_lines_kernel).  mask[0 .. n) rows (through the CSR permutation), mask[n .. n + m) columns; counts[0/1].
static __global__ __launch_bounds__(256) void sparse_empty_lines_kernel(const long long* __restrict__ cp, const long long* __restrict__ rp,
                                                                        const long long* __restrict__ perm, const double* __restrict__ val,
                                                                        int n, int m, unsigned char* __restrict__ mask,
                                                                        int* __restrict__ counts) {
  const int line = blockIdx.x * 256 + threadIdx.x;
  if (line >= n + m) return;
  bool empty = true;
  if (line < n) { for (long long p = rp[line]; p < rp[line + 1] && empty; ++p) empty = !(val[perm[p]] > 0.0); }
  else { for (long long e = cp[line - n]; e < cp[line - n + 1] && empty; ++e) empty = !(val[e] > 0.0); }
  mask[line] = empty ? 1 : 0;
  if (empty) atomicAdd(&counts[line < n ? 0 : 1], 1);
}
