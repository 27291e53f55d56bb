// Host-side 1-D spectral bases for the device library: Gauss-Lobatto-Legendre
// (velocity mesh), Gauss-Legendre (pressure and dealiasing meshes), Lagrange
// derivative and interpolation matrices.  [UPSTREAM Nek5000 speclib: zwgll, zwgl,
// dgll, igllm] -- restated from the published formulas, not from Nek source.
#pragma once
#include <cmath>
#include <utility>
#include <vector>

namespace nsk {

inline void legendre(int n, double x, double& p, double& dp) {
  double p0 = 1.0, p1 = x;
  if (n == 0) { p = 1.0; dp = 0.0; return; }
  for (int k = 2; k <= n; ++k) {
    double p2 = ((2 * k - 1) * x * p1 - (k - 1) * p0) / k;
    p0 = p1; p1 = p2;
  }
  p = p1;
  dp = n * (x * p1 - p0) / (x * x - 1.0);
}

// n Gauss-Legendre nodes (ascending) and weights
inline void zwgl(int n, std::vector<double>& z, std::vector<double>& w) {
  z.resize(n); w.resize(n);
  for (int i = 0; i < n; ++i) {
    double x = -std::cos(M_PI * (i + 0.75) / (n + 0.5));
    double p, dp;
    for (int it = 0; it < 100; ++it) {
      legendre(n, x, p, dp);
      double dx = p / dp;
      x -= dx;
      if (std::fabs(dx) < 1e-16) break;
    }
    legendre(n, x, p, dp);
    z[i] = x;
    w[i] = 2.0 / ((1.0 - x * x) * dp * dp);
  }
  for (int i = 0; i < n / 2; ++i) {       // enforce exact symmetry
    double a = 0.5 * (z[n - 1 - i] - z[i]);
    z[i] = -a; z[n - 1 - i] = a;
    double b = 0.5 * (w[i] + w[n - 1 - i]);
    w[i] = w[n - 1 - i] = b;
  }
  if (n % 2) z[n / 2] = 0.0;
}

// n Gauss-Lobatto-Legendre nodes (ascending) and weights
inline void zwgll(int n, std::vector<double>& z, std::vector<double>& w) {
  const int N = n - 1;
  z.resize(n); w.resize(n);
  z[0] = -1.0; z[N] = 1.0;
  for (int i = 1; i < N; ++i) {
    double x = -std::cos(M_PI * i / N);
    for (int it = 0; it < 100; ++it) {
      double p, dp;
      legendre(N, x, p, dp);
      double d2p = (2 * x * dp - N * (N + 1) * p) / (1.0 - x * x);
      double dx = dp / d2p;
      x -= dx;
      if (std::fabs(dx) < 1e-16) break;
    }
    z[i] = x;
  }
  for (int i = 0; i < n / 2; ++i) {
    double a = 0.5 * (z[n - 1 - i] - z[i]);
    z[i] = -a; z[n - 1 - i] = a;
  }
  if (n % 2) z[n / 2] = 0.0;
  for (int i = 0; i < n; ++i) {
    double p, dp;
    if (i == 0 || i == N) { p = (i == 0 && (N % 2)) ? -1.0 : 1.0; }
    else legendre(N, z[i], p, dp);
    w[i] = 2.0 / (N * (N + 1) * p * p);
  }
}

// J[i*nf + j] = l_j(xt[i]) for the Lagrange basis on xf
inline std::vector<double> interp_matrix(const std::vector<double>& xf, const std::vector<double>& xt) {
  const int nf = (int)xf.size(), nt = (int)xt.size();
  std::vector<double> J((size_t)nt * nf);
  for (int i = 0; i < nt; ++i)
    for (int j = 0; j < nf; ++j) {
      double num = 1.0, den = 1.0;
      for (int k = 0; k < nf; ++k)
        if (k != j) { num *= (xt[i] - xf[k]); den *= (xf[j] - xf[k]); }
      J[(size_t)i * nf + j] = num / den;
    }
  return J;
}

// D[i*n + j] = l_j'(x[i])
inline std::vector<double> deriv_matrix(const std::vector<double>& x) {
  const int n = (int)x.size();
  std::vector<double> D((size_t)n * n, 0.0), c(n);
  for (int i = 0; i < n; ++i) {
    double p = 1.0;
    for (int k = 0; k < n; ++k) if (k != i) p *= (x[i] - x[k]);
    c[i] = p;
  }
  for (int i = 0; i < n; ++i) {
    double s = 0.0;
    for (int j = 0; j < n; ++j)
      if (i != j) { D[(size_t)i * n + j] = c[i] / (c[j] * (x[i] - x[j])); s += D[(size_t)i * n + j]; }
    D[(size_t)i * n + i] = -s;
  }
  return D;
}

// The 1-D matrix of Nek5000's filter_s0(f, wght, 1, .) on the n GLL points z, row-major: F = Phi diag(1, ..., 1, 1 - wght) Phi^-1,
// Phi[j][k] = phi_k(z_j), phi_0 = L_0, phi_1 = L_1, phi_k = L_k - L_{k-2} (L: Legendre).  Built in its rank-one form
// F = I - wght phi_{n-1} y^T, y^T the last row of Phi^-1 (Phi^T y = e_{n-1}, Gaussian elimination with partial pivoting).
inline std::vector<double> filter_matrix(const std::vector<double>& z, double wght) {
  const int n = (int)z.size();
  std::vector<double> phi((size_t)n * n), M((size_t)n * n), y(n, 0.0), F((size_t)n * n, 0.0);
  for (int j = 0; j < n; ++j) {
    std::vector<double> L(n);
    for (int k = 0; k < n; ++k) L[k] = k == 0 ? 1.0 : k == 1 ? z[j] : ((2 * k - 1) * z[j] * L[k - 1] - (k - 1) * L[k - 2]) / k;
    for (int k = 0; k < n; ++k) phi[(size_t)j * n + k] = k < 2 ? L[k] : L[k] - L[k - 2];
  }
  for (int j = 0; j < n; ++j)
    for (int k = 0; k < n; ++k) M[(size_t)k * n + j] = phi[(size_t)j * n + k];   // M = Phi^T
  y[n - 1] = 1.0;
  for (int c = 0; c < n; ++c) {
    int piv = c;
    for (int r = c + 1; r < n; ++r) if (std::fabs(M[(size_t)r * n + c]) > std::fabs(M[(size_t)piv * n + c])) piv = r;
    if (piv != c) {
      for (int k = 0; k < n; ++k) std::swap(M[(size_t)c * n + k], M[(size_t)piv * n + k]);
      std::swap(y[c], y[piv]);
    }
    for (int r = c + 1; r < n; ++r) {
      const double f = M[(size_t)r * n + c] / M[(size_t)c * n + c];
      for (int k = c; k < n; ++k) M[(size_t)r * n + k] -= f * M[(size_t)c * n + k];
      y[r] -= f * y[c];
    }
  }
  for (int r = n - 1; r >= 0; --r) {
    double s = y[r];
    for (int k = r + 1; k < n; ++k) s -= M[(size_t)r * n + k] * y[k];
    y[r] = s / M[(size_t)r * n + r];
  }
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < n; ++j) F[(size_t)i * n + j] = (i == j ? 1.0 : 0.0) - wght * phi[(size_t)i * n + n - 1] * y[j];
  return F;
}

inline std::vector<double> matmul(const std::vector<double>& A, const std::vector<double>& B, int m, int k, int n) {
  std::vector<double> C((size_t)m * n, 0.0);
  for (int i = 0; i < m; ++i)
    for (int l = 0; l < k; ++l) {
      double a = A[(size_t)i * k + l];
      for (int j = 0; j < n; ++j) C[(size_t)i * n + j] += a * B[(size_t)l * n + j];
    }
  return C;
}

}  // namespace nsk
