// The permutation of shuffle_view's draw (R/obtain_bicl.r:11-22 on the device, DESIGN.md sections 10 and 27) and its
// inverse, stated once.  No HIP dependency: under hipcc the functions are __host__ __device__, under a plain C++17
// compiler they are inline host functions, which is how tests/host/fp64_shuffle_check.cpp runs them.  Three users:
//   resnmtf_hip.hip   (through resnmtf_kernels.hip.inc: shuffle_gather_kernel; resnmtf_sparse_shuffle.hip.inc: the inverse)
//   resnmtf_fp64.hip  (through resnmtf_fp64_shuffle.hip.inc: fp64_shuffle_gather_kernel)
//   the host check.
// The bodies were moved here word for word from resnmtf_kernels.hip.inc and resnmtf_sparse_shuffle.hip.inc; the kernels
// of the main unit kept their instruction text (tools/kernel_fingerprint.py --diff: additions only).
#ifndef RESNMTF_FEISTEL_H
#define RESNMTF_FEISTEL_H

#if defined(__HIPCC__)
#define RESNMTF_FEISTEL_FN __host__ __device__ __forceinline__
#define RESNMTF_FEISTEL_UNROLL _Pragma("unroll")
#else
#define RESNMTF_FEISTEL_FN inline
#define RESNMTF_FEISTEL_UNROLL
#endif

// the domain of the network for `count` positions: 2^(2 half_bits) >= count, half_bits >= 1 (count <= 2^62)
RESNMTF_FEISTEL_FN int feistel_half_bits(unsigned long long count) {
  int half_bits = 1;
  while ((1ull << (2 * half_bits)) < count) ++half_bits;
  return half_bits;
}

// --------------------------------------------------------------------------------------
// shuffle_view (R/obtain_bicl.r:11-22) on the device: staging[i] = X[pi(i)] for a pseudo-random
// permutation pi of the n m entries -- a 4-round Feistel network on the next even power of two with
// cycle walking (a bijection on [0, n m), evaluated independently per element: no sort, no atomics).
// R draws the permutation from its Mersenne Twister (sample()); neither is reproducible by the other.
// --------------------------------------------------------------------------------------
RESNMTF_FEISTEL_FN unsigned long long feistel_perm(unsigned long long i, unsigned long long count, int half_bits,
                                                   unsigned long long seed) {
  const unsigned long long mask = (1ull << half_bits) - 1ull;
  do {
    unsigned long long l = i >> half_bits, r = i & mask;
    RESNMTF_FEISTEL_UNROLL
    for (int round = 0; round < 4; ++round) {
      unsigned long long f = (r + seed + 0x9E3779B97F4A7C15ull * (unsigned long long)(round + 1));
      f ^= f >> 31; f *= 0xBF58476D1CE4E5B9ull; f ^= f >> 29; f *= 0x94D049BB133111EBull; f ^= f >> 32;
      const unsigned long long nl = r, nr = (l ^ f) & mask;
      l = nl; r = nr;
    }
    i = (l << half_bits) | r;
  } while (i >= count);                              // cycle walking: < 4 expected trips
  return i;
}

// The inverse of feistel_perm (same round constants, same half_bits): the four rounds in reverse order -- a forward round
// maps (l, r) to (r, (l ^ f(r)) & mask), so r_old = l_new and l_old = (r_new ^ f(l_new)) & mask -- and cycle walking with
// the inverse until the value is < count (the inverse of a cycle-walked bijection walks the same cycle backwards).
RESNMTF_FEISTEL_FN unsigned long long feistel_perm_inverse(unsigned long long j, unsigned long long count, int half_bits,
                                                           unsigned long long seed) {
  const unsigned long long mask = (1ull << half_bits) - 1ull;
  do {
    unsigned long long l = j >> half_bits, r = j & mask;
    RESNMTF_FEISTEL_UNROLL
    for (int round = 3; round >= 0; --round) {
      unsigned long long f = (l + seed + 0x9E3779B97F4A7C15ull * (unsigned long long)(round + 1));
      f ^= f >> 31; f *= 0xBF58476D1CE4E5B9ull; f ^= f >> 29; f *= 0x94D049BB133111EBull; f ^= f >> 32;
      const unsigned long long ol = (r ^ f) & mask, orr = l;
      l = ol; r = orr;
    }
    j = (l << half_bits) | r;
  } while (j >= count);
  return j;
}

#endif  // RESNMTF_FEISTEL_H
