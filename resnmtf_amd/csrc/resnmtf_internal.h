// What the translation units of the library share besides the public header: not part of the C-ABI (hidden symbols).
#ifndef RESNMTF_INTERNAL_H
#define RESNMTF_INTERNAL_H
#include <string>

#include "resnmtf_hip.h"

#define RESNMTF_HIDDEN __attribute__((visibility("hidden")))

// resnmtf_group_run's host checks of one job with resnmtf_fp64_run's limits (k <= RESNMTF_MAX_K, no cap on n * m):
// a message on refusal, nullptr when the job is fine.  Defined in resnmtf_hip.hip next to check_group_job.
// x_elsewhere: bit v set = view v comes as CSC arrays (resnmtf_fp64_run_sparse) or from device memory
// (resnmtf_fp64_run_device) and job.x[v] must be NULL.  factors_elsewhere: bit v set = view v's initial factors come from
// device memory and job.f0 / s0 / g0 / lambda0 / mu0 [v] must be NULL.  outputs_elsewhere: the results are written to device
// memory and the job's per-view output pointers may be NULL.
RESNMTF_HIDDEN const char* resnmtf_check_fp64_job(const resnmtf_group_job& j, int max_iters, unsigned x_elsewhere = 0,
                                                  unsigned factors_elsewhere = 0, bool outputs_elsewhere = false);
// the text resnmtf_last_error(NULL) returns (entry points without a handle)
RESNMTF_HIDDEN void resnmtf_set_create_error(const std::string& text);

// One n x m sparse view in the CALLER's device memory (what resnmtf_set_view_sparse_device takes: CSC / CSR / COO, int32
// / int64 indices, four value types, entries in any order) as its canonical structure, for resnmtf_fp64_run_sparse_device
// (DESIGN.md section 24).  Defined in resnmtf_hip.hip: it launches the kernels of resnmtf_sparse_device_view.hip.inc and
// resnmtf_sparse_shuffle.hip.inc and rocPRIM's sort, so that translation unit holds their only copy.  The steps are
// resnmtf_set_view_sparse_device's own -- the pointer check and its verdict before any kernel bounds a search by a pointer
// entry, one thread per entry (checks, key c n + r, value widened to fp64), the sort by key unless a CSC input's keys
// already ascend strictly, the duplicates check, the CSR key r m + c of every CSC position and its sort --, on `stream`,
// and every failure word is read back before the call returns.  nnz = 0: the pointer check alone, no array but the flags
// is touched.
// The caller owns every array: five transient 8-byte arrays of nnz (key[0..1], pay[0..2]), the two flag words, and the
// four results cptr [m + 1], cidx [nnz], rptr [n + 1], ridx [nnz]; rocPRIM's temporary storage is asked from `alloc`
// (nullptr = refused, its text already set: RESNMTF_ERR_ALLOC is returned).  On RESNMTF_OK csc_values (the values in CSC
// order) and csr_perm (the CSC position of every CSR entry) point into pay[]: they hold until the caller frees those.
// RESNMTF_ERR_INVALID: a device check refused the view, `why` holds resnmtf_set_view_sparse_device's text for it (the
// lowest offender); RESNMTF_ERR_HIP: `why` holds the runtime's.
struct resnmtf_sparse_device_build {
  int layout, index_type, dtype, n, m;
  long long nnz;                                 // >= 0
  const void *ptr_or_rows, *idx_or_cols, *values;
  unsigned long long* key[2];
  long long* pay[3];
  unsigned long long* flags;                     // two words
  long long *cptr, *rptr;
  int *cidx, *ridx;
  const double* csc_values;                      // out
  const long long* csr_perm;                     // out
};
RESNMTF_HIDDEN int resnmtf_sparse_device_canonical(void* stream, resnmtf_sparse_device_build& b, void* (*alloc)(void* ctx, size_t bytes),
                                                   void* ctx, std::string& why);

#endif
