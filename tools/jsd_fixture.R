# Prints jsd_calc (R/utils.r:95-106) for the fixture columns of tests/test_gpu_spurious.py's pool, for whoever has R
# (with the resnmtf package and philentropy installed) to compare against resnmtf_jsd_pairs / tests/jsd_ref.py.
#
#   Rscript tools/jsd_fixture.R cols.csv
#
# cols.csv: one column per fixture column, no header (e.g. written by numpy.savetxt(..., delimiter=",")).  Prints one
# line "a b score" per ordered pair (1-based).  UNTESTED: there is no R interpreter where this project is built and tested.
# R >= 4.4 changed density()'s default coordinates (old.coords = FALSE); the restatement follows R <= 4.3, so run it
# under R <= 4.3 or expect differences of about 0.1 % in the densities.

jsd_calc <- resnmtf:::jsd_calc        # the installed package's own function (internal)

args <- commandArgs(trailingOnly = TRUE)
cols <- as.matrix(utils::read.csv(args[1], header = FALSE))
for (a in seq_len(ncol(cols))) {
  for (b in seq_len(ncol(cols))) {
    cat(a, b, sprintf("%.17g", jsd_calc(cols[, a], cols[, b])), "\n")
  }
}
