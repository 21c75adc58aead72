// The L x L linear algebra of the SVD initialisation (resnmtf_amd/csrc/resnmtf_small_linalg.h) against brute force, on the
// host alone: the header compiles with a plain C++17 compiler and nothing else of the project.  Built twice by
// tests/test_small_linalg_host.py -- plainly, and with -fsanitize=address,undefined -- and run here; never on a GPU.
//
//   cholesky_upper   R^T R = C on the columns kept, a dependent column cut (zero row, R[j][j] = 0), -1 for a NaN pivot
//   invert_upper     R Ri = I on the columns kept, zero rows and columns elsewhere
//   jacobi_eigen     A V = V diag, V orthogonal, the eigenvalues those of a matrix built from a known spectrum
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <limits>
#include <random>
#include <vector>

#include "resnmtf_small_linalg.h"

namespace {
int failures = 0;
void check(bool ok, const char* what, int L, double value) {
  if (ok) return;
  ++failures;
  std::printf("FAILED L = %d: %s (%.3e)\n", L, what, value);
}

// Y (rows x L, row-major) with standard normal entries; column `dep` (when >= 0) a combination of the two before it
std::vector<double> sketch(int rows, int L, unsigned seed, int dep) {
  std::mt19937_64 gen(seed);
  std::normal_distribution<double> normal(0.0, 1.0);
  std::vector<double> Y((size_t)rows * L);
  for (double& y : Y) y = normal(gen);
  if (dep >= 2)
    for (int i = 0; i < rows; ++i) Y[(size_t)i * L + dep] = 0.5 * Y[(size_t)i * L + dep - 1] - 2.0 * Y[(size_t)i * L + dep - 2];
  return Y;
}
std::vector<double> gram(const std::vector<double>& Y, int rows, int L) {
  std::vector<double> C((size_t)L * L, 0.0);
  for (int a = 0; a < L; ++a)
    for (int b = 0; b < L; ++b) {
      double s = 0.0;
      for (int i = 0; i < rows; ++i) s += Y[(size_t)i * L + a] * Y[(size_t)i * L + b];
      C[(size_t)a * L + b] = s;
    }
  return C;
}
double trace(const std::vector<double>& C, int L) {
  double t = 0.0;
  for (int i = 0; i < L; ++i) t += C[(size_t)i * L + i];
  return t;
}

void one_size(int L, unsigned seed, int dep) {
  const int rows = 4 * L + 3;
  const std::vector<double> Y = sketch(rows, L, seed, dep);
  const std::vector<double> C = gram(Y, rows, L);
  const double tr = trace(C, L), cut = 2e-14 * tr;
  std::vector<double> R, Ri;
  const int kept = cholesky_upper(C, L, cut, R);
  check(kept == (dep >= 2 ? L - 1 : L), "columns kept", L, kept);
  // R is upper triangular, its cut row zero, and R^T R is C on the columns kept
  double worst = 0.0, lower = 0.0;
  for (int a = 0; a < L; ++a)
    for (int b = 0; b < L; ++b) {
      if (b < a) lower = std::max(lower, std::fabs(R[(size_t)a * L + b]));
      if (a == dep || b == dep) continue;
      double s = 0.0;
      for (int t = 0; t < L; ++t) s += R[(size_t)t * L + a] * R[(size_t)t * L + b];
      worst = std::max(worst, std::fabs(s - C[(size_t)a * L + b]) / tr);
    }
  check(lower == 0.0, "R has entries below the diagonal", L, lower);
  check(worst <= 1e-14, "|R^T R - C| / trace", L, worst);
  if (dep >= 2) {
    double row = 0.0;
    for (int b = 0; b < L; ++b) row = std::max(row, std::fabs(R[(size_t)dep * L + b]));
    check(row == 0.0, "the cut column's row of R is not zero", L, row);
  }
  invert_upper(R, L, Ri);
  worst = 0.0;
  for (int a = 0; a < L; ++a)
    for (int b = 0; b < L; ++b) {
      double s = 0.0;
      for (int t = 0; t < L; ++t) s += R[(size_t)a * L + t] * Ri[(size_t)t * L + b];
      const double want = (a == b && a != dep) ? 1.0 : 0.0;      // (Ri's row `dep` is zero: R's column `dep` drops out)
      worst = std::max(worst, std::fabs(s - want));
    }
  check(worst <= 1e-10, "|R Ri - I| on the columns kept", L, worst);
  if (dep >= 2) {
    double line = 0.0;
    for (int t = 0; t < L; ++t) line = std::max(line, std::max(std::fabs(Ri[(size_t)dep * L + t]), std::fabs(Ri[(size_t)t * L + dep])));
    check(line == 0.0, "row / column of Ri of the cut column is not zero", L, line);
    // Q = Y Ri is orthonormal on the columns kept and zero in the cut one
    double orth = 0.0;
    for (int a = 0; a < L; ++a)
      for (int b = 0; b < L; ++b) {
        double s = 0.0;
        for (int i = 0; i < rows; ++i) {
          double qa = 0.0, qb = 0.0;
          for (int t = 0; t < L; ++t) { qa += Y[(size_t)i * L + t] * Ri[(size_t)t * L + a]; qb += Y[(size_t)i * L + t] * Ri[(size_t)t * L + b]; }
          s += qa * qb;
        }
        orth = std::max(orth, std::fabs(s - ((a == b && a != dep) ? 1.0 : 0.0)));
      }
    check(orth <= 1e-9, "|Q^T Q - I| of Q = Y Ri with a cut column", L, orth);
  }

  // Jacobi: A = C (symmetric positive semi-definite): A V = V diag, V^T V = I, trace and Frobenius norm kept
  std::vector<double> A = C, V;
  jacobi_eigen(A, L, V);
  double resid = 0.0, orth = 0.0, offd = 0.0, tr_after = 0.0;
  for (int a = 0; a < L; ++a) {
    tr_after += A[(size_t)a * L + a];
    for (int b = 0; b < L; ++b) {
      double cv = 0.0, vv = 0.0;
      for (int t = 0; t < L; ++t) { cv += C[(size_t)a * L + t] * V[(size_t)t * L + b]; vv += V[(size_t)t * L + a] * V[(size_t)t * L + b]; }
      resid = std::max(resid, std::fabs(cv - V[(size_t)a * L + b] * A[(size_t)b * L + b]) / tr);
      orth = std::max(orth, std::fabs(vv - (a == b ? 1.0 : 0.0)));
      if (a != b) offd = std::max(offd, std::fabs(A[(size_t)a * L + b]) / tr);
    }
  }
  check(resid <= 1e-13, "|C V - V diag| / trace", L, resid);
  check(orth <= 1e-13, "|V^T V - I|", L, orth);
  check(offd <= 1e-14, "off-diagonal left by Jacobi / trace", L, offd);
  check(std::fabs(tr_after - tr) <= 1e-12 * tr, "trace not kept", L, tr_after - tr);
  if (dep >= 2) {                                 // rank L - 1: the smallest eigenvalue is zero to rounding
    double smallest = tr;
    for (int a = 0; a < L; ++a) smallest = std::min(smallest, std::fabs(A[(size_t)a * L + a]));
    check(smallest <= 1e-13 * tr, "smallest eigenvalue of a rank-deficient Gram / trace", L, smallest / tr);
  }
}

void known_spectrum(int L) {                      // A = H diag(1 ... L) H with a Householder H: the eigenvalues are 1 ... L
  std::vector<double> u(L), A((size_t)L * L, 0.0), V;
  double nu = 0.0;
  for (int i = 0; i < L; ++i) { u[i] = std::sin(1.0 + i); nu += u[i] * u[i]; }
  auto h = [&](int a, int b) { return (a == b ? 1.0 : 0.0) - 2.0 * u[a] * u[b] / nu; };
  for (int a = 0; a < L; ++a)
    for (int b = 0; b < L; ++b)
      for (int t = 0; t < L; ++t) A[(size_t)a * L + b] += h(a, t) * (1.0 + t) * h(t, b);
  jacobi_eigen(A, L, V);
  std::vector<double> ev(L);
  for (int a = 0; a < L; ++a) ev[a] = A[(size_t)a * L + a];
  std::sort(ev.begin(), ev.end());
  double worst = 0.0;
  for (int a = 0; a < L; ++a) worst = std::max(worst, std::fabs(ev[a] - (1.0 + a)));
  check(worst <= 1e-12 * L, "eigenvalues of a matrix with the spectrum 1 ... L", L, worst);
}
}  // namespace

int main() {
  int cases = 0;
  for (int L : {16, 32, 48, 64}) { one_size(L, 7u + L, -1); known_spectrum(L); ++cases; }
  one_size(32, 5u, 9); ++cases;                   // rank-deficient: column 9 depends on columns 7 and 8
  one_size(64, 6u, 63); ++cases;                  // ... the last column
  {  // a pivot that is not a number: -1, whatever the cut
    std::vector<double> C = gram(sketch(70, 16, 3u, -1), 70, 16), R;
    C[5 * 16 + 5] = std::numeric_limits<double>::quiet_NaN();
    check(cholesky_upper(C, 16, 0.0, R) == -1, "a NaN pivot must return -1", 16, 0.0);
    std::vector<double> Z((size_t)16 * 16, 0.0), Ri;          // the all-zero Gram: nothing kept, nothing inverted
    check(cholesky_upper(Z, 16, 0.0, R) == 0, "the zero matrix keeps no column", 16, 0.0);
    invert_upper(R, 16, Ri);
    check(*std::max_element(Ri.begin(), Ri.end()) == 0.0, "the inverse of nothing is zero", 16, 0.0);
    ++cases;
  }
  if (failures) { std::printf("small_linalg_check: %d checks FAILED\n", failures); return 1; }
  std::printf("small_linalg_check: %d cases, all checks passed\n", cases);
  return 0;
}
