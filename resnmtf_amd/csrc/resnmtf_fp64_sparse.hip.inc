// Sparse views in the device-wide fp64 path (resnmtf_fp64_run_sparse, DESIGN.md section 22).  A sparse view keeps no
// fp64 image: a CSC copy (for X^T F) and a CSR copy (for X G), pointers int64, indices int32, values fp64.  Its two
// products are SpMM passes that write what fp64_product_kernel writes -- slab[split][line][KP], leading dimension
// f64_ld(lines) -- so fp64_update_kernel consumes them unchanged; its error is the trace form, from the three k x k
// matrices its own sweep step produced (fp64_kk_sparse_kernel).  Determinism as in resnmtf_fp64.hip.inc: no atomics, no
// flags, nothing waits on another workgroup; every sum's order is fixed by the view's structure and k.

//
// Every kernel here is a template, instantiated by a launcher in this file.  That places them between the dense path's
// kernels in the code object without displacing the one that ends a section: tools/kernel_fingerprint.py hashes a kernel
// up to the next symbol, so the last kernel of a section carries the section's tail, and a new neighbour would show as a
// change of a kernel nobody touched.

#include "resnmtf_fp64_job.h"   // F64_SP_PIECE, F64_SP_MAX_SPLITS, f64_sp_group and f64_plan_sparse: host code, no HIP

#define F64_SP_T_ROWS 64        // rows per workgroup of the operand copy

// ---- the operand once per product as a row-major, KP-padded, zero-filled copy: OT[j][c] = O[j, c] (c < k), else 0 ----
// O (len x k) column-major.  64 rows per workgroup through LDS: coalesced on both sides.
template <int KP>
__global__ __launch_bounds__(F64_THREADS) void fp64_sp_operand_kernel(const double* __restrict__ O, int len, int k,
                                                                      double* __restrict__ OT) {
  constexpr int LD = KP + 1;
  __shared__ double tile[F64_SP_T_ROWS * LD];
  const size_t j0 = (size_t)blockIdx.x * F64_SP_T_ROWS, slen = (size_t)len;
  for (int e = threadIdx.x; e < F64_SP_T_ROWS * KP; e += F64_THREADS) {
    const int jj = e % F64_SP_T_ROWS, c = e / F64_SP_T_ROWS;
    tile[jj * LD + c] = (j0 + jj < slen && c < k) ? O[j0 + jj + (size_t)c * slen] : 0.0;
  }
  __syncthreads();
  for (int e = threadIdx.x; e < F64_SP_T_ROWS * KP; e += F64_THREADS) {
    const int c = e % KP, jj = e / KP;
    if (j0 + jj < slen) OT[(j0 + jj) * KP + c] = tile[jj * LD + c];
  }
}

// ---- SpMM: slab[split][line][c] = sum over the piece's stored entries e of val[e] OT[idx[e]][c], ascending e ----
// A group of f64_sp_group(KP) lanes owns one (line, split): lane c < KP owns column c, reads the entry (one address for
// the whole group) and one contiguous KP-double row of OT, and accumulates with fma in entry order.  Every (line, split)
// with line < lines is WRITTEN, zeros included: the slab is shared by all products of the sweep.  Rows from `lines` to
// the leading dimension are not written: fp64_update_kernel reads rows below n only.
template <int KP>
__global__ __launch_bounds__(F64_THREADS) void fp64_spmm_kernel(const long long* __restrict__ ptr, const int* __restrict__ idx,
                                                                const double* __restrict__ val, const double* __restrict__ OT,
                                                                int lines, long long piece, size_t ldx,
                                                                double* __restrict__ slab) {
  constexpr int GW = f64_sp_group(KP), GPB = F64_THREADS / GW;
  const int c = threadIdx.x % GW;
  const size_t line = (size_t)blockIdx.x * GPB + threadIdx.x / GW;
  if (line >= (size_t)lines || c >= KP) return;
  const long long b = ptr[line], len = ptr[line + 1] - b;
  const long long e0 = b + min((long long)blockIdx.y * piece, len), e1 = b + min(((long long)blockIdx.y + 1) * piece, len);
  double acc = 0.0;
  long long e = e0;
  for (; e + 4 <= e1; e += 4) {                   // four gathers in flight, summed in entry order
    const int i0 = idx[e], i1 = idx[e + 1], i2 = idx[e + 2], i3 = idx[e + 3];
    const double v0 = val[e], v1 = val[e + 1], v2 = val[e + 2], v3 = val[e + 3];
    const double o0 = OT[(size_t)i0 * KP + c], o1 = OT[(size_t)i1 * KP + c];
    const double o2 = OT[(size_t)i2 * KP + c], o3 = OT[(size_t)i3 * KP + c];
    acc = fma(v0, o0, acc);
    acc = fma(v1, o1, acc);
    acc = fma(v2, o2, acc);
    acc = fma(v3, o3, acc);
  }
  for (; e < e1; ++e) acc = fma(val[e], OT[(size_t)idx[e] * KP + c], acc);
  slab[((size_t)blockIdx.y * ldx + line) * KP + c] = acc;
}

// ---- the k x k side of a sparse view: a sibling of fp64_kk_kernel (which stays as it is) ----
// KEEP, between update_s's Gram launch and its k x k job: view v's three matrices into its slot -- F'^T F' (kkA, from
// the G side), (F'^T X) G' and G'^T G' (the Gram partials, reduced in workgroup order: the bits update_s gets).  The
// factors of view v do not change after its own step, so the slot holds until the error phase.
// TRACE, in the error phase (after all views' updates, in view order): calculate_error (R/utils.r:157-166) as
//   (||X||^2 - 2 <S', (F'^T X) G'> + <((F'^T F') S') (G'^T G'), S'>) / ||X||^2
// with the updated S'.  Each inner product: thread t sums its entries t, t + 256, ... in order, then the fixed tree.
struct F64KKSparseArgs {
  int k, V, v;
  int nblk_a, nblk_b;                     // KEEP: workgroups behind part_a / part_b
  const double* part_a;                   // KEEP: (F^T X) G
  const double* part_b;                   // KEEP: G^T G
  const double* kkA;                      // KEEP: F^T F
  double* slot;                           // this view's [F^T F | (F^T X) G | G^T G], k x k each
  double *t0, *t1;                        // TRACE: k x k temporaries
  const double* S;                        // TRACE: this view's S'
  double *norms, *errs;                   // per view
  double* err_out;                        // TRACE, last view: where the sweep's mean error goes
};
template <bool TRACE>
__global__ __launch_bounds__(F64_THREADS) void fp64_kk_sparse_kernel(F64KKSparseArgs a) {
  __shared__ double red[F64_THREADS];
  const int k = a.k, Q = k * k, t = threadIdx.x;
  double* A = a.slot;
  double* Cm = a.slot + Q;
  double* D = a.slot + 2 * (size_t)Q;
  if (!TRACE) {
    for (int q = t; q < Q; q += F64_THREADS) A[q] = a.kkA[q];
    f64_kk_reduce(Cm, a.part_a, a.nblk_a, Q);
    f64_kk_reduce(D, a.part_b, a.nblk_b, Q);
    return;
  }
  f64_kk_mul(A, a.S, false, k, a.t0);             // (F^T F) S'
  f64_kk_mul(a.t0, D, false, k, a.t1);            // ((F^T F) S') (G^T G)
  double cross = 0.0, quad = 0.0;
  for (int q = t; q < Q; q += F64_THREADS) {
    cross = fma(a.S[q], Cm[q], cross);
    quad = fma(a.t1[q], a.S[q], quad);
  }
  const double cr = f64_block_sum(cross, red);
  const double qd = f64_block_sum(quad, red);
  if (t == 0) {
    const double nrm = a.norms[a.v];
    a.errs[a.v] = ((nrm - 2.0 * cr) + qd) / nrm;
    if (a.v == a.V - 1) *a.err_out = f64_vec_sum(a.errs, a.V) / (double)a.V;      // (errs of the earlier views: earlier launches)
  }
}

// ---- launchers: the operand of one product row-major, then the SpMM over its lines; one instance per padded k ----
template <int KP>
static void fp64_spmm_kp(hipStream_t st, const F64SparsePlan& p, const long long* ptr, const int* idx, const double* val,
                         const double* O, int contr, int k, double* OT, int lines, size_t ldx, double* slab) {
  constexpr int GPB = F64_THREADS / f64_sp_group(KP);
  hipLaunchKernelGGL(fp64_sp_operand_kernel<KP>, dim3((contr + F64_SP_T_ROWS - 1) / F64_SP_T_ROWS), dim3(F64_THREADS), 0, st, O,
                     contr, k, OT);
  hipLaunchKernelGGL(fp64_spmm_kernel<KP>, dim3((lines + GPB - 1) / GPB, p.splits), dim3(F64_THREADS), 0, st, ptr, idx, val,
                     (const double*)OT, lines, p.piece, ldx, slab);
}
static void fp64_spmm(hipStream_t st, int KP, const F64SparsePlan& p, const long long* ptr, const int* idx, const double* val,
                      const double* O, int contr, int k, double* OT, int lines, size_t ldx, double* slab) {
  switch (KP) {
    case 16: fp64_spmm_kp<16>(st, p, ptr, idx, val, O, contr, k, OT, lines, ldx, slab); break;
    case 32: fp64_spmm_kp<32>(st, p, ptr, idx, val, O, contr, k, OT, lines, ldx, slab); break;
    case 48: fp64_spmm_kp<48>(st, p, ptr, idx, val, O, contr, k, OT, lines, ldx, slab); break;
    default: fp64_spmm_kp<64>(st, p, ptr, idx, val, O, contr, k, OT, lines, ldx, slab); break;
  }
}
static void fp64_kk_sparse(hipStream_t st, bool trace, const F64KKSparseArgs& a) {
  if (trace) hipLaunchKernelGGL(fp64_kk_sparse_kernel<true>, dim3(1), dim3(F64_THREADS), 0, st, a);
  else hipLaunchKernelGGL(fp64_kk_sparse_kernel<false>, dim3(1), dim3(F64_THREADS), 0, st, a);
}
