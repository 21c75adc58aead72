// The L x L linear algebra of the SVD initialisation (init_mats_inner, R/update_steps.r:78-125), on the host in fp64:
// the Cholesky factor with the rank cut, the inverse of the triangle, cyclic Jacobi.  L is at most 64.  Plain C++17, no
// HIP: the main unit (resnmtf_init_svd) and the fp64 unit (resnmtf_fp64_init_svd) include this one text, and
// tests/host/small_linalg_check.cpp compiles it alone.  Matrices are L x L, row-major.
#ifndef RESNMTF_SMALL_LINALG_H
#define RESNMTF_SMALL_LINALG_H

#include <cmath>
#include <cstddef>
#include <vector>

// C (L x L, row-major, symmetric positive semi-definite) = R^T R, R upper triangular.  A pivot that is not above `cut`
// marks a column that depends on the ones before it: its row of R stays zero (R[j][j] = 0) and the factorisation goes on
// without it.  Returns the number of columns kept, -1 for a pivot that is not a number.
static inline int cholesky_upper(const std::vector<double>& C, int L, double cut, std::vector<double>& R) {
  R.assign((size_t)L * L, 0.0);
  int kept = 0;
  for (int j = 0; j < L; ++j) {
    double d = C[(size_t)j * L + j];
    for (int t = 0; t < j; ++t) d -= R[(size_t)t * L + j] * R[(size_t)t * L + j];
    if (d != d) return -1;
    if (!(d > cut)) continue;
    ++kept;
    const double rjj = std::sqrt(d);
    R[(size_t)j * L + j] = rjj;
    for (int c = j + 1; c < L; ++c) {
      double v = C[(size_t)j * L + c];
      for (int t = 0; t < j; ++t) v -= R[(size_t)t * L + j] * R[(size_t)t * L + c];
      R[(size_t)j * L + c] = v / rjj;
    }
  }
  return kept;
}
// Ri = R^-1 on the columns cholesky_upper kept; row and column j of Ri are zero for a column j it cut (Y Ri is then zero there)
static inline void invert_upper(const std::vector<double>& R, int L, std::vector<double>& Ri) {
  Ri.assign((size_t)L * L, 0.0);
  for (int j = 0; j < L; ++j) {
    if (R[(size_t)j * L + j] == 0.0) continue;
    Ri[(size_t)j * L + j] = 1.0 / R[(size_t)j * L + j];
    for (int i = j - 1; i >= 0; --i) {
      if (R[(size_t)i * L + i] == 0.0) continue;
      double v = 0.0;
      for (int t = i + 1; t <= j; ++t) v += R[(size_t)i * L + t] * Ri[(size_t)t * L + j];
      Ri[(size_t)i * L + j] = -v / R[(size_t)i * L + i];
    }
  }
}
// cyclic Jacobi for a symmetric L x L matrix: A -> eigenvalues (diagonal), V columns = eigenvectors
static inline void jacobi_eigen(std::vector<double>& A, int L, std::vector<double>& V) {
  V.assign((size_t)L * L, 0.0);
  for (int i = 0; i < L; ++i) V[(size_t)i * L + i] = 1.0;
  for (int sweep = 0; sweep < 60; ++sweep) {
    double off = 0.0, diag = 0.0;
    for (int i = 0; i < L; ++i)
      for (int j = 0; j < L; ++j) (i == j ? diag : off) += A[(size_t)i * L + j] * A[(size_t)i * L + j];
    if (off <= 1e-30 * diag) break;
    for (int p = 0; p < L - 1; ++p)
      for (int q = p + 1; q < L; ++q) {
        const double apq = A[(size_t)p * L + q];
        if (apq == 0.0) continue;
        const double theta = (A[(size_t)q * L + q] - A[(size_t)p * L + p]) / (2.0 * apq);
        const double t = (theta >= 0.0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
        const double c = 1.0 / std::sqrt(t * t + 1.0), sn = t * c;
        for (int r = 0; r < L; ++r) {           // columns p, q
          const double arp = A[(size_t)r * L + p], arq = A[(size_t)r * L + q];
          A[(size_t)r * L + p] = c * arp - sn * arq;
          A[(size_t)r * L + q] = sn * arp + c * arq;
        }
        for (int r = 0; r < L; ++r) {           // rows p, q
          const double apr = A[(size_t)p * L + r], aqr = A[(size_t)q * L + r];
          A[(size_t)p * L + r] = c * apr - sn * aqr;
          A[(size_t)q * L + r] = sn * apr + c * aqr;
        }
        for (int r = 0; r < L; ++r) {
          const double vrp = V[(size_t)r * L + p], vrq = V[(size_t)r * L + q];
          V[(size_t)r * L + p] = c * vrp - sn * vrq;
          V[(size_t)r * L + q] = sn * vrp + c * vrq;
        }
      }
  }
}

#endif  // RESNMTF_SMALL_LINALG_H
