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

#endif
