// resnmtf_fp64_bisil_sparse.hip.inc -- the restricted block of a SPARSE view in double precision
// (resnmtf_fp64_bisil_sparse, DESIGN.md section 29).  Included by resnmtf_fp64.hip only.
//
// A sparse view has no image to gather from.  Per side and active bicluster the block G (|J_l| x U_pad doubles) is
// zero-filled by a hipMemsetAsync and fp64_bisil_scatter_kernel writes the stored entries of the feature lines that fall
// in U to G[f][rank[idx]] -- the row side reads the CSC columns J_l, the column side the CSR rows I_l.  G then holds, bit
// for bit, what fp64_bisil_gather writes for the densified matrix of the same fp64 values (a position without a stored
// entry is +0.0 in both), so the norm, distance and epilogue kernels of resnmtf_fp64_bisil.hip.inc run on it unchanged and
// give the same bits.  The kernel is the fp64 twin of bisil_scatter_kernel (resnmtf_bisil.hip.inc), which stores floats.
//
// One wave64 owns one feature line and its lanes stride the line's entries: a dense line among sparse ones costs
// len / 64 steps of one wave, not len steps of one lane.  The indices of a line are distinct (the CSC check on the host
// route, the canonicaliser on the device route, both BEFORE the first launch: the kernel indexes rank[idx[e]] unchecked),
// so no two lanes write one element: no atomics, nothing waits on another workgroup, any execution order gives the
// same G.  The zero-fill stays a memset of its own, as in the twin: the fill is a dense stream over |J_l| x U_pad
// doubles, the scatter's work is proportional to the stored entries of the lines, and the stream orders the two.
//
// A template, as every kernel added to this code object (resnmtf_fp64_sparse.hip.inc says why: a template lands between
// the other kernels and displaces no section's last symbol).

constexpr int F64_BISIL_SCATTER_THREADS = 256;
constexpr int F64_BISIL_SCATTER_MAX_WGS = 65536;   // lines beyond 4 x this many are taken by a grid stride

// G[f * upad + rank[idx[e]]] = val[e] for every stored entry e of line feat[f] with rank[idx[e]] >= 0; G zeroed before.
// ptr / idx / val: the CSC (lines = columns, idx = rows) or the CSR (lines = rows, idx = columns); rank[p] = the position
// of point p in U or -1.
template <int THREADS>
__global__ __launch_bounds__(THREADS) void fp64_bisil_scatter_kernel(const long long* __restrict__ ptr, const int* __restrict__ idx,
                                                                     const double* __restrict__ val, const int* __restrict__ feat,
                                                                     int nf, const int* __restrict__ rank, int upad,
                                                                     double* __restrict__ G) {
  constexpr int WAVES = THREADS / 64;
  const int lane = threadIdx.x & 63;
  for (long long f = (long long)blockIdx.x * WAVES + (threadIdx.x >> 6); f < nf; f += (long long)gridDim.x * WAVES) {
    const int line = feat[f];
    const long long p1 = ptr[line + 1];
    double* __restrict__ g = G + (size_t)f * upad;
    for (long long e = ptr[line] + lane; e < p1; e += 64) {
      const int r = rank[idx[e]];
      if (r >= 0) g[r] = val[e];
    }
  }
}

// ---- launch ----  (nf >= 1: an active bicluster has members on both sides)
static hipError_t fp64_bisil_scatter(hipStream_t st, const long long* ptr, const int* idx, const double* val, const int* feat, int nf,
                                     const int* rank, int upad, double* G) {
  const hipError_t e = hipMemsetAsync(G, 0, (size_t)nf * upad * sizeof(double), st);
  if (e != hipSuccess) return e;
  constexpr int waves = F64_BISIL_SCATTER_THREADS / 64;
  const unsigned grid = (unsigned)std::min((nf + waves - 1) / waves, F64_BISIL_SCATTER_MAX_WGS);
  hipLaunchKernelGGL(fp64_bisil_scatter_kernel<F64_BISIL_SCATTER_THREADS>, dim3(grid), dim3(F64_BISIL_SCATTER_THREADS), 0, st, ptr, idx,
                     val, feat, nf, rank, upad, G);
  return hipGetLastError();
}
