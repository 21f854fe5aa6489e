// The small real symmetric eigenproblem of the thick-restart Lanczos driver (eig.hip): the projected matrix, size <= 64, solved on
// the host by cyclic Jacobi rotations on the full matrix.  Plain C++: no HIP, no LAPACK, so that a host program can include it alone
// (tests/c_host/eig_small_main.cpp).  Jacobi is backward stable rotation by rotation and delivers eigenvectors orthonormal to a few
// epsilon whatever the spectrum looks like (repeated eigenvalues included), which is what the restart needs; at n = 64 a solve is
// some 10^6 flops, nothing beside one operator application.
#ifndef TMHIP_EIG_SMALL_H
#define TMHIP_EIG_SMALL_H
#include <cmath>
#include <vector>

#define TMHIP_EIG_SMALL_MAX_SWEEPS 64

// A: n*n doubles, row-major, symmetric on entry (only its upper triangle is read); on exit column j of A (A[i*n + j], i = 0..n-1) is
// the eigenvector of w[j], w ascending.  Returns 0, or 1 for n < 1 or when the sweeps run out (never seen: a sweep converges
// quadratically).
static inline int tmhip_eig_small_jacobi(int n, double *A, double *w) {
  if (n < 1 || !A || !w) return 1;
  std::vector<double> a((size_t)n * n), v((size_t)n * n, 0.0);
  for (int i = 0; i < n; i++)
    for (int j = 0; j < n; j++) a[(size_t)i * n + j] = j >= i ? A[(size_t)i * n + j] : A[(size_t)j * n + i];
  for (int i = 0; i < n; i++) v[(size_t)i * n + i] = 1.0;
  int sweep = 0;
  for (; sweep < TMHIP_EIG_SMALL_MAX_SWEEPS; sweep++) {
    double off = 0.0, diag = 0.0;
    for (int p = 0; p < n; p++) {
      diag += a[(size_t)p * n + p] * a[(size_t)p * n + p];
      for (int q = p + 1; q < n; q++) off += a[(size_t)p * n + q] * a[(size_t)p * n + q];
    }
    if (off == 0.0 || off <= 1e-36 * diag) break;
    for (int p = 0; p < n - 1; p++) {
      for (int q = p + 1; q < n; q++) {
        const double apq = a[(size_t)p * n + q];
        if (apq == 0.0) continue;
        const double app = a[(size_t)p * n + p], aqq = a[(size_t)q * n + q];
        // an element that no longer changes either diagonal entry is set to zero (Rutishauser's rule)
        if (std::fabs(app) + std::fabs(apq) == std::fabs(app) && std::fabs(aqq) + std::fabs(apq) == std::fabs(aqq)) {
          a[(size_t)p * n + q] = a[(size_t)q * n + p] = 0.0;
          continue;
        }
        const double theta = (aqq - app) / (2.0 * apq);
        const double t = (theta >= 0.0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
        const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
        for (int k = 0; k < n; k++) {   // columns p, q of a and of v
          const double akp = a[(size_t)k * n + p], akq = a[(size_t)k * n + q];
          a[(size_t)k * n + p] = c * akp - s * akq;
          a[(size_t)k * n + q] = s * akp + c * akq;
          const double vkp = v[(size_t)k * n + p], vkq = v[(size_t)k * n + q];
          v[(size_t)k * n + p] = c * vkp - s * vkq;
          v[(size_t)k * n + q] = s * vkp + c * vkq;
        }
        for (int k = 0; k < n; k++) {   // rows p, q of a
          const double apk = a[(size_t)p * n + k], aqk = a[(size_t)q * n + k];
          a[(size_t)p * n + k] = c * apk - s * aqk;
          a[(size_t)q * n + k] = s * apk + c * aqk;
        }
        a[(size_t)p * n + q] = a[(size_t)q * n + p] = 0.0;
      }
    }
  }
  if (sweep == TMHIP_EIG_SMALL_MAX_SWEEPS) return 1;
  // The product of some ten sweeps of rotations has drifted from orthonormal by their rounding, tens of epsilon at n = 64, and the
  // diagonal carries as much.  One first-order step V <- V (1 - E / 2), E = V^T V - 1, brings the columns back to a few epsilon (E is
  // tiny, so only the final subtraction rounds); the eigenvalues are then the Rayleigh quotients with the matrix as it was given.
  std::vector<double> e((size_t)n * n), d(n);
  for (int i = 0; i < n; i++)
    for (int j = i; j < n; j++) {
      double s = 0.0;
      for (int k = 0; k < n; k++) s += v[(size_t)k * n + i] * v[(size_t)k * n + j];
      e[(size_t)i * n + j] = e[(size_t)j * n + i] = s - (i == j ? 1.0 : 0.0);
    }
  for (int k = 0; k < n; k++) {
    for (int j = 0; j < n; j++) {
      double s = 0.0;
      for (int i = 0; i < n; i++) s += v[(size_t)k * n + i] * e[(size_t)i * n + j];
      d[j] = s;
    }
    for (int j = 0; j < n; j++) v[(size_t)k * n + j] -= 0.5 * d[j];
  }
  for (int i = 0; i < n; i++)   // a = the matrix as given, again
    for (int j = 0; j < n; j++) a[(size_t)i * n + j] = j >= i ? A[(size_t)i * n + j] : A[(size_t)j * n + i];
  for (int j = 0; j < n; j++) {
    double q = 0.0;
    for (int i = 0; i < n; i++) {
      double s = 0.0;
      for (int k = 0; k < n; k++) s += a[(size_t)i * n + k] * v[(size_t)k * n + j];
      q += v[(size_t)i * n + j] * s;
    }
    d[j] = q;
  }
  std::vector<int> order(n);
  for (int i = 0; i < n; i++) order[i] = i;
  for (int i = 1; i < n; i++) {   // insertion sort, ascending, stable
    const int o = order[i];
    int j = i - 1;
    for (; j >= 0 && d[order[j]] > d[o]; j--) order[j + 1] = order[j];
    order[j + 1] = o;
  }
  for (int j = 0; j < n; j++) {
    w[j] = d[order[j]];
    for (int i = 0; i < n; i++) A[(size_t)i * n + j] = v[(size_t)i * n + order[j]];
  }
  return 0;
}

#endif
