// The host-side checks of nagp_nmf_temp_create (include/nagp.h), decided before any device call, and the shape arithmetic they share
// with the launch code.  Plain C++ without the HIP runtime, so that tools/nmf_temp_host_check.cpp can run them on exactly-sized heap
// blocks under the host sanitizers.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>

#if defined(__HIPCC__)
#define NMFT_HD __host__ __device__
#else
#define NMFT_HD
#endif

namespace nagp {

constexpr int NMFT_ROWS = 256;         // time rows of a pass workgroup (NMFT_NT of nagp_nmf_temp.hpp)
constexpr int NMFT_OK = 0, NMFT_EINVAL = -1, NMFT_EUNSUPPORTED = -2;   // NAGP_OK, NAGP_EINVAL, NAGP_EUNSUPPORTED

// per-component sums over t that obj2 is made of: none, TG (4), IG (5)
NMFT_HD inline int nmft_nq(int prior) { return prior == 1 ? 4 : (prior == 2 ? 5 : 0); }

struct NmftShape {
  int learn = 0, nwg = 1, n_po = 1;
  size_t nx = 0;             // entries of x per problem
  size_t per_problem = 0;    // bytes of the per-evaluation buffers per problem: the budget rule of include/nagp.h
};

#define NMFT_FAIL(code, ...) do { snprintf(msg, msg_len, __VA_ARGS__); return (code); } while (0)

inline int nmft_host_check(int32_t n_problems, int64_t T, int32_t D, int32_t K, int32_t prior, const double* A, const double* vary, const double* W,
                           const double* muinf, const double* varinf, const double* lam, size_t budget, NmftShape* sh, char* msg, size_t msg_len) {
  if (!A) NMFT_FAIL(NMFT_EINVAL, "null argument");
  if (n_problems < 1 || T < 1 || D < 1 || K < 1) NMFT_FAIL(NMFT_EINVAL, "bad sizes (n_problems=%d T=%lld D=%d K=%d)", n_problems, (long long)T, D, K);
  if (prior < 0 || prior > 2) NMFT_FAIL(NMFT_EINVAL, "prior=%d: NAGP_NMFT_NONE, _TG or _IG", prior);
  if (prior != 0 && T < 2) NMFT_FAIL(NMFT_EINVAL, "T=%lld: a temporal prior needs T >= 2", (long long)T);
  if (D > 64) NMFT_FAIL(NMFT_EUNSUPPORTED, "D=%d: at most 64 channels", D);
  if (K > 16) NMFT_FAIL(NMFT_EUNSUPPORTED, "K=%d: at most 16 components", K);
  if (prior != 0 && (!varinf || !lam)) NMFT_FAIL(NMFT_EINVAL, "varinf and lam are read by this prior");
  if (prior == 2 && !muinf) NMFT_FAIL(NMFT_EINVAL, "muinf is read by the inverse-gamma prior");
  const size_t TD = (size_t)T * D, TK = (size_t)T * K, KD = (size_t)K * D, nz = (size_t)n_problems;
  for (size_t e = 0; e < TD; ++e) {
    if (!std::isfinite(A[e]) || A[e] < 0.0) NMFT_FAIL(NMFT_EINVAL, "A[%zu] = %g: the data must be finite and >= 0", e, A[e]);
    if (vary && (!std::isfinite(vary[e]) || vary[e] < 0.0)) NMFT_FAIL(NMFT_EINVAL, "vary[%zu] = %g: the noise must be finite and >= 0", e, vary[e]);
  }
  if (W)
    for (size_t q = 0; q < nz; ++q) {
      const double* w = W + q * KD;
      for (int k = 0; k < K; ++k) {
        bool any = false;
        for (int d = 0; d < D; ++d) {
          const double x = w[k + (size_t)d * K];
          if (!std::isfinite(x) || x < 0.0) NMFT_FAIL(NMFT_EINVAL, "W(%d, %d) of problem %zu = %g: the weights must be finite and >= 0", k, d, q, x);
          any = any || x > 0.0;
        }
        if (!any) NMFT_FAIL(NMFT_EINVAL, "row %d of W of problem %zu is all zero", k, q);
      }
    }
  for (int k = 0; k < K && prior != 0; ++k) {
    if (!std::isfinite(varinf[k]) || !(varinf[k] > 0.0)) NMFT_FAIL(NMFT_EINVAL, "varinf[%d] = %g: finite and > 0", k, varinf[k]);
    if (!std::isfinite(lam[k])) NMFT_FAIL(NMFT_EINVAL, "lam[%d] = %g", k, lam[k]);
    if (prior == 2) {
      if (!std::isfinite(muinf[k]) || !(muinf[k] > 0.0)) NMFT_FAIL(NMFT_EINVAL, "muinf[%d] = %g: finite and > 0", k, muinf[k]);
      if (lam[k] < 0.0 || lam[k] > 1.0) NMFT_FAIL(NMFT_EINVAL, "lam[%d] = %g: the inverse-gamma chain needs 0 <= lam <= 1", k, lam[k]);
    }
  }
  sh->learn = W ? 0 : 1;
  sh->nwg = (int)((T + NMFT_ROWS - 1) / NMFT_ROWS);
  sh->n_po = 1 + nmft_nq(prior) * K;
  sh->nx = TK + (sh->learn ? KD : 0);
  sh->per_problem = 8 * (2 * sh->nx + (size_t)sh->nwg * ((sh->learn ? KD : 0) + (size_t)sh->n_po) + 1);
  if (sh->per_problem > budget)
    NMFT_FAIL(NMFT_EUNSUPPORTED, "one problem takes %zu B of device memory per evaluation (budget %zu B)", sh->per_problem, budget);
  return NMFT_OK;
}
#undef NMFT_FAIL

}  // namespace nagp
