// Objective and gradient of the filterbank spectrum fit, unifying_prob_tf/get_Obj_pSTFT_{exp,matern32,matern52,all}.m, FP64, a batch of
// independent problems.  See include/nagp.h (nagp_pstft_obj) for the boundary and DESIGN.md for the reasoning.
//
// With mVar = minVar + exp(theta_1..D), om and lam the sigmoids of :61-67 and the grid omegas of :72-74 the model spectrum is
//     spec_i = vary + sum_d (1 - lam_d^2) S_d(omega_i),     Obj = (sum_i log spec_i + sum_i specTar_i / spec_i + bet sum_d mVar_d) / N.
// All four files are one family.  The generic file's S_d = real(H ((F - i omega I) \ L) Qc (...)') of the Matern (x) rotation product
// model (_all.m:102-128) diagonalises over the rotation into two companion systems in omega -+ om, and a Matern companion system of
// order P has H1 (F1 - i w I)^-1 L1 = -(lm + i w)^-P, so
//     S_d(omega) = h_d (a1^-P + a2^-P),   a1,2 = lm_d^2 + (omega -+ om_d)^2,   h_d = (c_P / 2) mVar_d lm_d^(2P-1),   c_P = 2, 4, 16/3, 32/5,
// with lm = lam for exp / matern32 / matern52 -- which is the closed form of the three kernel-specific files -- and lm = sqrt(7/5) lam
// for matern72, the generic file's len = sqrt(5) / lam (_all.m:81-94) met by cf_matern72_to_ss's lambda = sqrt(7) / len.  The generic
// gradient (_all.m:194-209) is the exact derivative of that S_d in (mVar, len, om), so it collapses the same way; `form` therefore
// selects no second code path here: the kernel, its order P and lm / lam decide.  Per frequency, with g_i = 1/spec_i - specTar_i/spec_i^2:
//     G0_d = sum_i g_i (a1^-P + a2^-P)                                       (d spec / d mVar, up to constants)
//     G1_d = sum_i g_i (a1^-(P+1) (omega - om) - a2^-(P+1) (omega + om))     (d spec / d om)
//     G2_d = sum_i g_i (cA_d (a1^-P + a2^-P) - cB_d (a1^-(P+1) + a2^-(P+1)))  (d spec / d lam, up to h / lm: combined per frequency as the .m's do)
// These 3 D sums and the two of the objective are all that crosses threads.
//
// pstft_pass_kernel<P>: grid (ceil(N / 256), problems), 256 threads, a thread owns one frequency.  The per-component constants of the
// problem are formed from theta by the first D threads and sit in the LDS; specTar loads are coalesced.  The gradient pass keeps no
// S_d: it forms spec in a first loop over d and recomputes a1, a2 in a second (no O(N D) scratch).  Every sum is reduced by a fixed
// xor butterfly inside a wave, the four waves are added in wave order, and the workgroup writes its 3 D + 2 (objective only: 2)
// partial sums to part[problem][workgroup][].
// pstft_finish_kernel: grid (problems), 1024 threads.  Every output is the sum over the workgroups in a fixed two-level order that
// depends on (N, D) alone (an objective-only call gives the bits of the call with the gradient): contiguous runs of workgroups, each in ascending order, then the runs in ascending order;
// then the transforms' factors (cosh(theta/2)^-2 / 4, bet dVar on the variance part only, / N).  No atomics: a problem's bits depend
// neither on its batch mates nor on how the call was split into device batches.
#pragma once
#include "nagp_dev.hpp"

namespace nagp {

constexpr int PSTFT_NT = 256;          // threads (= frequencies) of a pass workgroup
constexpr int PSTFT_FIN_NT = 1024;     // threads of the finish kernel
constexpr int PSTFT_MAXD = 64;
constexpr int PSTFT_NC = 8;            // constants per component in the LDS

struct PstftPar {
  int64_t N;
  int D;
  int nwg;                 // workgroups of a pass per problem
  int grad;                // 1: objective and gradient (3 D + 2 sums), 0: objective only (2 sums)
  double kappa;            // lm / lam: 1, or sqrt(7/5) for matern72
  const double* theta;     // problems x 3 D
  const double* specTar;   // N (spec_stride = 0) or problems x N
  int64_t spec_stride;
  const double* vary;      // problems
  const double* bet;       // problems
  const double* minVar;    // D
  const double* limOm;     // D x 2 column-major
  const double* limLam;    // D x 2 column-major
  double* part;            // problems x nwg x n_out
  double* Obj;             // problems
  double* dObj;            // problems x 3 D (grad = 1)
};

// the transforms of :61-67 and what the two kernels need of them, for component d of problem `prob`; both kernels call this, so they
// see the same bits
struct PstftComp {
  double dVar, mVar, om, lam, lm, hv, h, hl, one_m_lam2, cA, cB;
};

template <int P>
__device__ inline PstftComp pstft_component(const PstftPar& p, int prob, int d) {
  const int D = p.D;
  const double* th = p.theta + (size_t)prob * 3 * D;
  PstftComp c;
  c.dVar = exp(th[d]);
  c.mVar = p.minVar[d] + c.dVar;
  c.om = p.limOm[d] + (p.limOm[D + d] - p.limOm[d]) / (1.0 + exp(-th[D + d]));
  c.lam = p.limLam[d] + (p.limLam[D + d] - p.limLam[d]) / (1.0 + exp(-th[2 * D + d]));
  c.lm = p.kappa * c.lam;
  constexpr double half_c = P == 1 ? 1.0 : P == 2 ? 2.0 : P == 3 ? 8.0 / 3.0 : 16.0 / 5.0;      // c_P / 2
  double pw = 1.0;                                    // lm^(2P-2)
#pragma unroll
  for (int k = 1; k < P; ++k) pw *= c.lm * c.lm;
  c.hv = half_c * (pw * c.lm);                        // S_d = mVar hv R_P,  R_q = a1^-q + a2^-q
  c.h = c.mVar * c.hv;
  c.hl = half_c * c.mVar * pw;                        // h / lm, without the division (lam = 0 stays finite)
  c.one_m_lam2 = 1.0 - c.lam * c.lam;
  // d spec_d / d lam = hl (cA R_P - cB R_(P+1)):  (1 - lam^2) dS/dlam - 2 lam S with dS/dlam = kappa dS/dlm
  c.cA = c.one_m_lam2 * p.kappa * (2 * P - 1) - 2.0 * c.lam * c.lm;
  c.cB = c.one_m_lam2 * p.kappa * (2 * P) * (c.lm * c.lm);
  return c;
}

// omegas(i) of :72-74 for the 0-based index i: [linspace(0, pi, ceil(N/2)), -omegas(floor(N/2):-1:1)]
__host__ __device__ inline double pstft_omega(int64_t i, int64_t N) {
  const int64_t half = (N + 1) / 2, n1 = half - 1;
  if (i < half) return ((double)i * 3.14159265358979323846) / (double)n1;
  const int64_t k = N / 2 - 1 - (i - half);
  return -(((double)k * 3.14159265358979323846) / (double)n1);
}

template <int P>
__device__ inline double pstft_ipow(double x) {       // x^P
  double r = x;
#pragma unroll
  for (int k = 1; k < P; ++k) r *= x;
  return r;
}

constexpr size_t pstft_pass_lds_doubles() { return (size_t)PSTFT_MAXD * PSTFT_NC + 4 * (3 * (size_t)PSTFT_MAXD + 2); }

template <int P>
__global__ void __launch_bounds__(PSTFT_NT) pstft_pass_kernel(PstftPar p) {
  __shared__ __attribute__((aligned(16))) double lds[pstft_pass_lds_doubles()];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int D = p.D, prob = blockIdx.y;
  const int64_t N = p.N;
  const int n_out = p.grad ? 3 * D + 2 : 2;
  double* cs = lds;                                   // [d][PSTFT_NC]: lm^2, om, (1 - lam^2) h, cA, cB
  double* red = lds + PSTFT_MAXD * PSTFT_NC;          // [wave][n_out]
  if (tid < D) {
    const PstftComp c = pstft_component<P>(p, prob, tid);
    double* q = cs + tid * PSTFT_NC;
    q[0] = c.lm * c.lm; q[1] = c.om; q[2] = c.one_m_lam2 * c.h; q[3] = c.cA; q[4] = c.cB;
  }
  __syncthreads();
  const int64_t i = (int64_t)blockIdx.x * PSTFT_NT + tid;
  const bool live = i < N;
  const int64_t ii = live ? i : 0;                    // a thread beyond N reads entry 0 and contributes zeros
  const double w = pstft_omega(ii, N);
  const double tar = p.specTar[(size_t)prob * p.spec_stride + ii];
  double spec = p.vary[prob];
  for (int d = 0; d < D; ++d) {
    const double* q = cs + d * PSTFT_NC;
    const double wm = w - q[1], wp = w + q[1];
    const double i1 = 1.0 / fma(wm, wm, q[0]), i2 = 1.0 / fma(wp, wp, q[0]);
    spec = fma(q[2], pstft_ipow<P>(i1) + pstft_ipow<P>(i2), spec);
  }
  const double inv = 1.0 / spec;
  double o_log = live ? log(spec) : 0.0, o_div = live ? tar * inv : 0.0;
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) { o_log += __shfl_xor(o_log, m); o_div += __shfl_xor(o_div, m); }
  if (lane == 0) { red[wave * n_out + n_out - 2] = o_log; red[wave * n_out + n_out - 1] = o_div; }
  if (p.grad) {
    const double g = live ? inv - tar * inv * inv : 0.0;                 // 1./spec - specTar./spec.^2
    for (int d = 0; d < D; ++d) {
      const double* q = cs + d * PSTFT_NC;
      const double wm = w - q[1], wp = w + q[1];
      const double i1 = 1.0 / fma(wm, wm, q[0]), i2 = 1.0 / fma(wp, wp, q[0]);
      const double p1 = pstft_ipow<P>(i1), p2 = pstft_ipow<P>(i2);
      const double r0 = p1 + p2, r1 = p1 * i1 + p2 * i2;
      double g0 = g * r0;
      double g1 = g * (p1 * i1 * wm - p2 * i2 * wp);
      double g2 = g * (q[3] * r0 - q[4] * r1);
#pragma unroll
      for (int m = 32; m >= 1; m >>= 1) { g0 += __shfl_xor(g0, m); g1 += __shfl_xor(g1, m); g2 += __shfl_xor(g2, m); }
      if (lane == 0) { red[wave * n_out + d] = g0; red[wave * n_out + D + d] = g1; red[wave * n_out + 2 * D + d] = g2; }
    }
  }
  __syncthreads();
  double* out = p.part + ((size_t)prob * p.nwg + blockIdx.x) * n_out;
  for (int o = tid; o < n_out; o += PSTFT_NT) out[o] = ((red[o] + red[n_out + o]) + red[2 * n_out + o]) + red[3 * n_out + o];
}

// runs of the finish kernel's two-level sum over the workgroups: a function of the shape alone
__host__ __device__ inline int pstft_finish_chunks(int n_out, int nwg) {
  int c = PSTFT_FIN_NT / n_out;
  if (c > nwg) c = nwg;
  return c < 1 ? 1 : c;
}

template <int P>
__global__ void __launch_bounds__(PSTFT_FIN_NT) pstft_finish_kernel(PstftPar p) {
  __shared__ double part[PSTFT_FIN_NT];               // [run][output] when there is more than one run
  __shared__ double tot[3 * PSTFT_MAXD + 2];
  const int tid = threadIdx.x, D = p.D, nwg = p.nwg, prob = blockIdx.x;
  const int n_out = p.grad ? 3 * D + 2 : 2;
  const int chunks = pstft_finish_chunks(3 * D + 2, nwg), per = (nwg + chunks - 1) / chunks;     // the same runs with and without the gradient
  const double* pp = p.part + (size_t)prob * nwg * n_out;
  auto run = [&](int o, int w0, int w1) {
    double s = 0.0;
    for (int w = w0; w < w1; ++w) s += pp[(size_t)w * n_out + o];
    return s;
  };
  if (chunks > 1) {                                   // chunks * n_out <= chunks * (3 D + 2) <= PSTFT_FIN_NT
    if (tid < chunks * n_out) {
      const int c = tid / n_out, o = tid % n_out, w0 = c * per, w1 = (w0 + per < nwg) ? w0 + per : nwg;
      part[c * n_out + o] = run(o, w0, w1);           // (an empty run at the end gives 0)
    }
    __syncthreads();
  }
  if (tid < n_out) {
    double s = 0.0;
    if (chunks > 1) { for (int c = 0; c < chunks; ++c) s += part[c * n_out + tid]; }
    else s = run(tid, 0, nwg);
    tot[tid] = s;
  }
  __syncthreads();
  const double Nd = (double)p.N, bet = p.bet[prob];
  if (tid == 0) {
    double sv = 0.0;                                  // sum(mVar), d ascending
    for (int d = 0; d < D; ++d) sv += pstft_component<P>(p, prob, d).mVar;
    p.Obj[prob] = ((tot[n_out - 2] + tot[n_out - 1]) + bet * sv) / Nd;
  }
  if (p.grad && tid < D) {
    const int d = tid;
    const PstftComp c = pstft_component<P>(p, prob, d);
    const double* th = p.theta + (size_t)prob * 3 * D;
    double* g = p.dObj + (size_t)prob * 3 * D;
    const double ch_om = cosh(0.5 * th[D + d]), ch_lam = cosh(0.5 * th[2 * D + d]);
    const double dom = (p.limOm[D + d] - p.limOm[d]) * 0.25 / (ch_om * ch_om);
    const double dlam = (p.limLam[D + d] - p.limLam[d]) * 0.25 / (ch_lam * ch_lam);
    // dspecdtransVar = dVar (1 - lam^2) S_d / mVar;  dspecdom = (1 - lam^2) h 2P (...);  dspecdlam = (h / lm) (cA R_P - cB R_(P+1))
    g[d] = (c.dVar * c.one_m_lam2 * c.hv * tot[d] + bet * c.dVar) / Nd;
    g[D + d] = (c.one_m_lam2 * c.h * (2 * P) * tot[D + d]) * dom / Nd;
    g[2 * D + d] = (c.hl * tot[2 * D + d]) * dlam / Nd;
  }
}

}  // namespace nagp

#define NAGP_LIST_PSTFT_P(X, P) X void nagp::pstft_pass_kernel<P>(nagp::PstftPar); X void nagp::pstft_finish_kernel<P>(nagp::PstftPar);
#define NAGP_LIST_PSTFT(X) NAGP_LIST_PSTFT_P(X, 1) NAGP_LIST_PSTFT_P(X, 2) NAGP_LIST_PSTFT_P(X, 3) NAGP_LIST_PSTFT_P(X, 4)
