// The host-side checks of nagp_sebf_conv, nagp_sebf_fit_create and nagp_tnmf_create (include/nagp.h), decided before any device call,
// the shape arithmetic they share with the launch code, and the taps of the squared-exponential basis (basis2SEGP.m:21-26), built on
// the host once per handle.  Plain C++ without the HIP runtime, so that tools/sebf_host_check.cpp can run all of it on exactly-sized
// heap blocks under the host sanitizers.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>

#include "nagp_nmf_temp_check.hpp"

namespace nagp {

constexpr int SEBF_NT = 256;                       // threads of a convolution workgroup
constexpr int SEBF_R = 8;                          // consecutive outputs of a thread
constexpr int SEBF_TT = SEBF_NT * SEBF_R;          // outputs of a workgroup (the tile length)
constexpr int SEBF_C = 512;                        // taps of a chunk
constexpr int64_t SEBF_TAU_MAX = ((int64_t)1 << 30) - 1;   // 2 tau + 1 taps are counted in an int32
constexpr int SEBF_OK = 0, SEBF_EINVAL = -1, SEBF_EUNSUPPORTED = -2;   // NAGP_OK, NAGP_EINVAL, NAGP_EUNSUPPORTED

struct SebfShape {
  int ntile = 1;             // workgroups of a convolution per column
  int learn = 0, nwg = 1;    // tnmf: the form and the workgroups of the row kernel per problem
  size_t nx = 0;             // entries of x per problem
  size_t n_taps = 0;         // taps of all tap columns together
  size_t per_problem = 0;    // bytes of the per-evaluation buffers per problem (column): the budget rule of include/nagp.h
};

#define SEBF_FAIL(code, ...) do { snprintf(msg, msg_len, __VA_ARGS__); return (code); } while (0)

// tau = ceil(lenx / sqrt(2) * tol), the operations in the order of basis2SEGP.m:21
inline int sebf_tau(double lenx, double tol, int64_t* tau, char* msg, size_t msg_len) {
  const double td = std::ceil(lenx / std::sqrt(2.0) * tol);
  if (!(td <= (double)SEBF_TAU_MAX)) SEBF_FAIL(SEBF_EUNSUPPORTED, "tau = ceil(lenx / sqrt(2) * tol) = %g: at most %lld (2 tau + 1 taps are counted in an int32)", td, (long long)SEBF_TAU_MAX);
  *tau = (int64_t)td;
  return SEBF_OK;
}

// lenx, varx (n each) and tol; tau[n] on return and the sum of the 2 tau + 1
inline int sebf_basis_check(size_t n, const double* lenx, const double* varx, double tol, int64_t* tau, size_t* n_taps, char* msg, size_t msg_len) {
  if (!std::isfinite(tol) || tol < 0.0) SEBF_FAIL(SEBF_EINVAL, "tol = %g: finite and >= 0", tol);
  for (size_t k = 0; k < n; ++k) {
    if (!std::isfinite(lenx[k]) || !(lenx[k] > 0.0)) SEBF_FAIL(SEBF_EINVAL, "lenx[%zu] = %g: finite and > 0", k, lenx[k]);
    if (!std::isfinite(varx[k]) || varx[k] < 0.0) SEBF_FAIL(SEBF_EINVAL, "varx[%zu] = %g: finite and >= 0", k, varx[k]);
  }
  *n_taps = 0;
  for (size_t k = 0; k < n; ++k) {
    const int st = sebf_tau(lenx[k], tol, &tau[k], msg, msg_len);
    if (st != SEBF_OK) return st;
    *n_taps += (size_t)(2 * tau[k] + 1);
  }
  return SEBF_OK;
}

// bas(s) = bh exp(-1 / lenx^2 * s^2), s = -tau .. tau, at out[s + tau]  (basis2SEGP.m:22-24: no tap is dropped, however small)
inline void sebf_build_taps(double lenx, double varx, int64_t tau, double* out) {
  const double bh = std::sqrt(varx * std::sqrt(2.0) / (lenx * std::sqrt(3.14159265358979323846)));
  const double c = -1.0 / (lenx * lenx);
  for (int64_t s = -tau; s <= tau; ++s) out[s + tau] = bh * std::exp(c * (double)(s * s));
}

inline int sebf_ntile(int64_t T) { return (int)((T + SEBF_TT - 1) / SEBF_TT); }

// nagp_sebf_conv: Z and Y per column
inline int sebf_conv_check(int32_t n_cols, int64_t T, const double* Z, const double* lenx, const double* varx, double tol, const double* Y, size_t budget,
                           SebfShape* sh, int64_t* tau, char* msg, size_t msg_len) {
  if (!Z || !lenx || !varx || !Y) SEBF_FAIL(SEBF_EINVAL, "null argument");
  if (n_cols < 1 || T < 1) SEBF_FAIL(SEBF_EINVAL, "bad sizes (n_cols=%d T=%lld)", n_cols, (long long)T);
  const int st = sebf_basis_check((size_t)n_cols, lenx, varx, tol, tau, &sh->n_taps, msg, msg_len);
  if (st != SEBF_OK) return st;
  sh->ntile = sebf_ntile(T); sh->nx = (size_t)T;
  sh->per_problem = 8 * 2 * (size_t)T;
  if (sh->per_problem > budget) SEBF_FAIL(SEBF_EUNSUPPORTED, "one column takes %zu B of device memory per evaluation (budget %zu B)", sh->per_problem, budget);
  return SEBF_OK;
}

// nagp_sebf_fit_create: z, dx, dObj and Obj per problem
inline int sebf_fit_check(int32_t n, int64_t T, const double* x, const double* lenx, const double* varx, double tol, size_t budget, SebfShape* sh, int64_t* tau,
                          char* msg, size_t msg_len) {
  if (!x || !lenx || !varx) SEBF_FAIL(SEBF_EINVAL, "null argument");
  if (n < 1 || T < 1) SEBF_FAIL(SEBF_EINVAL, "bad sizes (n_problems=%d T=%lld)", n, (long long)T);
  const int st = sebf_basis_check((size_t)n, lenx, varx, tol, tau, &sh->n_taps, msg, msg_len);
  if (st != SEBF_OK) return st;
  sh->ntile = sebf_ntile(T); sh->nx = (size_t)T;
  sh->per_problem = 8 * (3 * (size_t)T + 1);
  if (sh->per_problem > budget) SEBF_FAIL(SEBF_EUNSUPPORTED, "one problem takes %zu B of device memory per evaluation (budget %zu B)", sh->per_problem, budget);
  return SEBF_OK;
}

// nagp_tnmf_create: what nagp_nmf_temp_create checks of the sizes, A, vary and W (no prior), then the basis and the budget: x, logH (with
// log W), the row kernel's gradient and dObj, nx entries each, the row kernel's partial sums and Obj
inline int tnmf_host_check(int32_t n_problems, int64_t T, int32_t D, int32_t K, const double* A, const double* vary, const double* W, const double* lenx,
                           const double* mux, const double* varx, double tol, size_t budget, SebfShape* sh, int64_t* tau /* K, when K <= 16 */, char* msg, size_t msg_len) {
  if (!A || !lenx || !mux || !varx) SEBF_FAIL(SEBF_EINVAL, "null argument");
  NmftShape ns;
  const int st0 = nmft_host_check(n_problems, T, D, K, 0, A, vary, W, nullptr, nullptr, nullptr, ~(size_t)0, &ns, msg, msg_len);
  if (st0 != NMFT_OK) return st0;
  for (int k = 0; k < K; ++k)
    if (!std::isfinite(mux[k])) SEBF_FAIL(SEBF_EINVAL, "mux[%d] = %g: finite", k, mux[k]);
  const int st = sebf_basis_check((size_t)K, lenx, varx, tol, tau, &sh->n_taps, msg, msg_len);
  if (st != SEBF_OK) return st;
  sh->ntile = sebf_ntile(T); sh->learn = ns.learn; sh->nwg = ns.nwg; sh->nx = ns.nx;
  sh->per_problem = 8 * (4 * sh->nx + (size_t)sh->nwg * ((sh->learn ? (size_t)K * D : 0) + 1) + 1);
  if (sh->per_problem > budget) SEBF_FAIL(SEBF_EUNSUPPORTED, "one problem takes %zu B of device memory per evaluation (budget %zu B)", sh->per_problem, budget);
  return SEBF_OK;
}
#undef SEBF_FAIL

}  // namespace nagp
