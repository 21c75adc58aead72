// What the translation units of the library share besides the public header: not part of the C-ABI (hidden symbols).
#ifndef RESNMTF_INTERNAL_H
#define RESNMTF_INTERNAL_H
#include <string>

#include "resnmtf_hip.h"

#define RESNMTF_HIDDEN __attribute__((visibility("hidden")))

// resnmtf_group_run's host checks of one job with resnmtf_fp64_run's limits (k <= RESNMTF_MAX_K, no cap on n * m):
// a message on refusal, nullptr when the job is fine.  Defined in resnmtf_hip.hip next to check_group_job.
// sparse_views: bit v set = view v comes as CSC arrays (resnmtf_fp64_run_sparse) and job.x[v] must be NULL.
RESNMTF_HIDDEN const char* resnmtf_check_fp64_job(const resnmtf_group_job& j, int max_iters, unsigned sparse_views = 0);
// the text resnmtf_last_error(NULL) returns (entry points without a handle)
RESNMTF_HIDDEN void resnmtf_set_create_error(const std::string& text);

#endif
