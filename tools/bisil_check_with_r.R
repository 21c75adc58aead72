# Prints bisilhouette::bisilhouette for exported fixtures, for whoever has R (with the bisilhouette package from GitHub
# eso28599/bisilhouette installed) to compare against the project's definition (resnmtf_bisil / tests/bisil_ref.py,
# DESIGN.md section 13), whose parity with the R package is unpinned.
#
#   Rscript tools/bisil_check_with_r.R x.csv rows.csv cols.csv [euclidean|manhattan|cosine]
#
# x.csv: the view (n x m), rows.csv: its row clusters (n x k, 0 / 1), cols.csv: its column clusters (m x k, 0 / 1); no
# headers (e.g. written by numpy.savetxt(..., delimiter=",")).  Prints the view's score and, where the package returns
# them, its per-bicluster scores.  The project's number for the same files:
#   python -c "import numpy as np, sys; sys.path.insert(0, 'tests'); import bisil_ref as B; \
#     x, r, c = (np.loadtxt(f, delimiter=',', ndmin=2) for f in ('x.csv', 'rows.csv', 'cols.csv')); \
#     print(B.view_score(r, c, *B.silhouettes(x, r, c, 'euclidean')))"
# UNTESTED: there is no R interpreter where this project is built and tested.

args <- commandArgs(trailingOnly = TRUE)
x <- as.matrix(utils::read.csv(args[1], header = FALSE))
row_clusters <- as.matrix(utils::read.csv(args[2], header = FALSE))
col_clusters <- as.matrix(utils::read.csv(args[3], header = FALSE))
method <- if (length(args) >= 4) args[4] else "euclidean"
res <- bisilhouette::bisilhouette(x, row_clusters, col_clusters, method = method)   # as R/obtain_bicl.r:192-195 calls it
cat("bisil", sprintf("%.17g", res$bisil), "\n")
for (name in setdiff(names(res), "bisil")) {
  cat(name, sprintf("%.17g", unlist(res[[name]])), "\n")
}
