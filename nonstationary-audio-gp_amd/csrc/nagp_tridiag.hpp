// nagp_tridiag.hpp -- eigenvalues and (rows of the) eigenvectors of a symmetric tridiagonal matrix by the implicit QL iteration (the
// tql2 of EISPACK; the library links no LAPACK), and the Lanczos control of LanczosGPPAD.m that decides with it.  Plain C++ without the
// HIP runtime: tests/c/tridiag_check.cpp runs it under the host sanitizers.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <vector>

namespace nagp {

// d[0 .. n): the diagonal, e[1 .. n): the sub-diagonal (e[0] is not read).  Z (rows x n, row-major) holds on entry rows of an orthogonal
// matrix (the identity for the eigenvectors, its last row alone for the last components: the rotations act on every row by itself) and on
// exit the same rows of the eigenvector matrix.  Eigenvalues ascending in d, the columns of Z with them.  false: no convergence in 60
// iterations for one eigenvalue, or an entry that is not finite.
inline bool tridiag_ql(int n, double* d, double* e, double* Z, int rows) {
  for (int i = 0; i < n; ++i) if (!std::isfinite(d[i]) || (i && !std::isfinite(e[i]))) return false;
  for (int i = 1; i < n; ++i) e[i - 1] = e[i];
  e[n - 1] = 0.0;
  const double eps = 2.220446049250313e-16;
  double f = 0.0, tst1 = 0.0;
  for (int l = 0; l < n; ++l) {
    tst1 = std::max(tst1, std::fabs(d[l]) + std::fabs(e[l]));
    int m = l;
    while (m < n - 1 && std::fabs(e[m]) > eps * tst1) ++m;
    if (m > l) {
      int iter = 0;
      do {
        if (++iter > 60) return false;
        double g = d[l], p = (d[l + 1] - g) / (2.0 * e[l]), r = std::hypot(p, 1.0);
        if (p < 0) r = -r;
        d[l] = e[l] / (p + r);
        d[l + 1] = e[l] * (p + r);
        const double dl1 = d[l + 1];
        double h = g - d[l];
        for (int i = l + 2; i < n; ++i) d[i] -= h;
        f += h;
        p = d[m];
        double c = 1.0, c2 = c, c3 = c, s = 0.0, s2 = 0.0;
        const double el1 = e[l + 1];
        for (int i = m - 1; i >= l; --i) {
          c3 = c2; c2 = c; s2 = s;
          g = c * e[i];
          h = c * p;
          r = std::hypot(p, e[i]);
          e[i + 1] = s * r;
          s = e[i] / r;
          c = p / r;
          p = c * d[i] - s * g;
          d[i + 1] = h + s * (c * g + s * d[i]);
          for (int k = 0; k < rows; ++k) {
            double* z = Z + (size_t)k * n;
            h = z[i + 1];
            z[i + 1] = s * z[i] + c * h;
            z[i] = c * z[i] - s * h;
          }
        }
        p = -s * s2 * c3 * el1 * e[l] / dl1;
        e[l] = s * p;
        d[l] = c * p;
      } while (std::fabs(e[l]) > eps * tst1);
    }
    d[l] += f;
    e[l] = 0.0;
  }
  for (int i = 0; i + 1 < n; ++i) {                       // ascending, the columns with their values
    int k = i;
    for (int q = i + 1; q < n; ++q) if (d[q] < d[k]) k = q;
    if (k == i) continue;
    std::swap(d[i], d[k]);
    for (int r = 0; r < rows; ++r) std::swap(Z[(size_t)r * n + i], Z[(size_t)r * n + k]);
  }
  return true;
}

// spectral norm of the (m x 2) matrix h (rows a_i, b_i): the root of the larger eigenvalue of its 2 x 2 Gram matrix
inline double norm2_two_columns(const double* h, int m) {
  double p = 0.0, q = 0.0, c = 0.0;
  for (int i = 0; i < m; ++i) { p += h[2 * i] * h[2 * i]; q += h[2 * i + 1] * h[2 * i + 1]; c += h[2 * i] * h[2 * i + 1]; }
  const double hd = 0.5 * (p - q);
  return std::sqrt(0.5 * (p + q) + std::sqrt(hd * hd + c * c));
}

enum { LAP_OK = 0, LAP_NOT_FINITE = 1, LAP_NO_QL = 2 };

// The scalar side of one LanczosGPPAD.m run (:17-29 and :43-92), indices as in the .m (1-based).  The caller supplies alpha(j) and
// beta(j+1) of step j, asks whether v_j and r are to be reorthogonalised, and whether the run goes on.
struct LanczosControl {
  int nev = 0, jmax = 0, j = 0, nconv = 0, reorths = 0, status = LAP_OK;
  double tresh = 0, tolconv = 0, anorm = 0, epert = 0;
  bool flagreort = false, done = false;
  std::vector<double> al, be, wjm1, wj, wjp1, ev, last;    // ev, last: the Ritz values and the last row of s at the latest test
  std::vector<char> convd;
  void start(int nev_, int jmax_, double tresh_, double tolconv_, double beta1) {
    const double eps = 2.220446049250313e-16;
    nev = nev_; jmax = jmax_; tresh = tresh_; tolconv = tolconv_;
    j = 0; nconv = 0; reorths = 0; status = LAP_OK; anorm = 0; epert = 0; flagreort = false; done = false;
    const size_t n = (size_t)jmax + 4;
    al.assign(n, 0.0); be.assign(n, 0.0); wjm1.assign(n, 0.0); wj.assign(n, 0.0); wjp1.assign(n, 0.0);
    wj[2] = eps; wj[3] = eps;
    be[1] = beta1;
    ev.clear(); last.clear(); convd.clear();
  }
  // :43-63; true: it is time to reorthogonalise
  bool step(double alpha, double beta) {
    const double eps = 2.220446049250313e-16;
    ++j;
    al[j] = alpha; be[j + 1] = beta;
    anorm = j == 1 ? std::fabs(al[1] + be[2]) : std::max(anorm, be[j] + std::fabs(al[j]) + be[j + 1]);
    epert = anorm * eps;
    wjp1[1] = 0.0;
    for (int v = 2; v <= j; ++v) {
      const double w = be[v] * wj[v + 1] + (al[v - 1] - al[j]) * wj[v] + be[v - 1] * wj[v - 1] - be[j] * wjm1[v];
      const double sg = w > 0 ? 1.0 : (w < 0 ? -1.0 : 0.0);          // sign(0) = 0
      wjp1[v] = (w + sg * epert) / be[j + 1];
    }
    wjp1[j + 1] = epert / be[j + 1];
    wjp1[j + 2] = eps;
    double mx = 0.0;
    for (int v = 1; v <= j + 2; ++v) { const double a = std::fabs(wjp1[v]); if (a > mx) mx = a; }     // max() skips NaN
    if (mx > tresh) { flagreort = true; ++reorths; return true; }
    return false;
  }
  void after_reorth() {
    const double eps = 2.220446049250313e-16;
    for (int v = 2; v <= j + 1; ++v) wjp1[v] = eps;
    for (int v = 2; v <= j; ++v) wj[v] = eps;
  }
  // :72-92: the convergence test when it is due, and whether the run ends here
  void finish_step() {
    wjm1 = wj; wj = wjp1;
    if (flagreort || j == jmax || be[j + 1] < epert) {
      std::vector<double> d(al.begin() + 1, al.begin() + 1 + j), e(j, 0.0);
      for (int i = 1; i < j; ++i) e[i] = be[i + 1];
      last.assign(j, 0.0); last[j - 1] = 1.0;
      if (!tridiag_ql(j, d.data(), e.data(), last.data(), 1)) {
        bool fin = true;
        for (int i = 1; i <= j; ++i) fin = fin && std::isfinite(al[i]) && (i == 1 || std::isfinite(be[i]));
        status = fin ? LAP_NO_QL : LAP_NOT_FINITE; nconv = 0; convd.assign(j, 0); ev.assign(j, NAN); done = true;
        return;
      }
      ev = d; convd.assign(j, 0); nconv = 0;
      for (int i = 0; i < j; ++i) { convd[i] = std::fabs(be[j + 1] * last[i]) < tolconv * anorm; nconv += convd[i]; }
      flagreort = false;
    }
    if (be[j + 1] < epert || nconv >= nev || j == jmax) done = true;
  }
  // :93-96: the converged Ritz values in descending order (stable) and s(:, those) as the columns of S (j x jmax, row-major)
  bool ritz(std::vector<double>& lmb, double* S, int ld) const {
    lmb.clear();
    if (status != LAP_OK || nconv == 0) return true;
    std::vector<double> d(al.begin() + 1, al.begin() + 1 + j), e(j, 0.0), Z((size_t)j * j, 0.0);
    for (int i = 1; i < j; ++i) e[i] = be[i + 1];
    for (int i = 0; i < j; ++i) Z[(size_t)i * j + i] = 1.0;
    if (!tridiag_ql(j, d.data(), e.data(), Z.data(), j)) return false;
    std::vector<int> ix;
    for (int i = 0; i < j; ++i) if (convd[i]) ix.push_back(i);
    std::stable_sort(ix.begin(), ix.end(), [&](int a, int b) { return d[a] > d[b]; });
    for (size_t k = 0; k < ix.size(); ++k) {
      lmb.push_back(d[ix[k]]);
      for (int i = 0; i < j; ++i) S[(size_t)i * ld + k] = Z[(size_t)i * j + ix[k]];
    }
    return true;
  }
};

}  // namespace nagp
