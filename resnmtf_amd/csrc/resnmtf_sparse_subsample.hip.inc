// resnmtf_sparse_subsample.hip.inc -- data[[i]][row_samples[[i]], col_samples[[i]]] (R/stability_analysis.r:124, :184,
// :232, :238) of a sparse view that stays sparse (resnmtf_subsample_count_sparse / resnmtf_subsample_view_sparse,
// DESIGN.md section 10 "Device copies and sub-samples").  Included by resnmtf_hip.hip after
// resnmtf_sparse_shuffle.hip.inc: what these kernels emit is what sparse_shuffle_keys_kernel emits -- a 64-bit
// destination position per kept entry and its value as fp64 -- and the shuffle's tail (two sorts, line pointers, masks,
// values, data_norms, plan) turns it into the view.
//
// Destination row i is source row rows[i], destination column j is source column cols[j]; the lists are unsorted and
// free of repeats (checked on the host), so the rows have an inverse map:
//   1. sparse_subsample_inverse_kernel: inv_row[rows[i]] = i over a map preset to -1 (4 n_src bytes, transient);
//   2. sparse_subsample_count_kernel: one wave per destination column j walks source column cols[j] 64 entries per trip
//      and counts the entries whose row is kept (ballot + popcount); an exclusive scan of the counts is cp';
//   3. sparse_subsample_emit_kernel: the same walk; a kept entry goes to cp'[j] + (kept in earlier trips) + (its rank in
//      the trip's ballot) with the key j n' + inv_row[ri[e]] (n' m' may exceed 2^32).  Every slot is written exactly
//      once; no atomics.  Within a column the entries arrive in SOURCE row order, which the tail's first sort turns into
//      destination order.
// Latency-bound bookkeeping: a wave per column keeps the index loads of a trip coalesced; nothing here is worth LDS.

static __global__ __launch_bounds__(256) void sparse_subsample_inverse_kernel(const int* __restrict__ rows, int n_dst,
                                                                              int* __restrict__ inv_row) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n_dst) inv_row[rows[i]] = i;
}

// four waves per workgroup, wave w of block b takes destination column 4 b + w; counts[m_dst] = 0 closes the scan
static __global__ __launch_bounds__(256) void sparse_subsample_count_kernel(const long long* __restrict__ cp, const int* __restrict__ ri,
                                                                            const int* __restrict__ cols, int m_dst,
                                                                            const int* __restrict__ inv_row,
                                                                            long long* __restrict__ counts) {
  const int lane = threadIdx.x & 63;
  const int j = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (j > m_dst) return;                                  // (wave-uniform)
  if (j == m_dst) { if (lane == 0) counts[j] = 0; return; }
  const int c = cols[j];
  const long long e0 = cp[c], e1 = cp[c + 1];
  long long kept = 0;
  for (long long base = e0; base < e1; base += 64) {
    const long long e = base + lane;
    const bool keep = e < e1 && inv_row[ri[e]] >= 0;
    kept += __popcll(__ballot(keep));
  }
  if (lane == 0) counts[j] = kept;
}

static __global__ __launch_bounds__(256) void sparse_subsample_emit_kernel(const long long* __restrict__ cp, const int* __restrict__ ri,
                                                                           const float* __restrict__ vcsc, const int* __restrict__ cols,
                                                                           int n_dst, int m_dst, const int* __restrict__ inv_row,
                                                                           const long long* __restrict__ cp_dst,
                                                                           unsigned long long* __restrict__ key, double* __restrict__ val) {
  const int lane = threadIdx.x & 63;
  const int j = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (j >= m_dst) return;                                 // (wave-uniform)
  const int c = cols[j];
  const long long e0 = cp[c], e1 = cp[c + 1];
  long long out = cp_dst[j];
  for (long long base = e0; base < e1; base += 64) {
    const long long e = base + lane;
    const int r = e < e1 ? inv_row[ri[e]] : -1;
    const unsigned long long kept = __ballot(r >= 0);
    if (r >= 0) {
      const long long q = out + __popcll(kept & ((1ull << lane) - 1ull));
      key[q] = (unsigned long long)j * (unsigned long long)n_dst + (unsigned long long)r;
      val[q] = (double)vcsc[e];
    }
    out += __popcll(kept);
  }
}
