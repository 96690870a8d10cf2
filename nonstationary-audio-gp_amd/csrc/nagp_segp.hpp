// Objective and gradient of the modulator prior fit, experiments/toolsGP/getObjSEGP.m on getGPSESpec.m (driven by trainSEGP_RS.m), FP64,
// a batch of independent problems.  See include/nagp.h (nagp_segp_obj) for the boundary and DESIGN.md for the reasoning.
//
// With len = exp(param[0]), varx and vary from param or given (the three nargin branches of getObjSEGP.m) and the frequency list of
// getGPSESpec.m:18, f_j = j for j <= ceil(T/2), else j - T (so for odd T entry (T+1)/2 is +(T+1)/2, as the .m writes it):
//     w_j = 2 pi f_j / T,   c_j = sqrt(2 pi len^2) exp(-w_j^2 len^2 / 2),   dc_j = c_j (1/len - w_j^2 len),   S_j = varx c_j + vary,
//     g_j = 1/(2 S_j) - specy_j / (2 T S_j^2),
//     Obj = (1/2 sum_j log S_j + 1/(2T) sum_j specy_j / S_j) / T,   dObj = [len varx sum g dc, varx sum g c, vary sum g] / T.
// These two sums and the n_param sums of the gradient are all that crosses threads.
//
// segp_pass_kernel<n_param>: grid (ceil(T / 256), problems), 256 threads, a thread owns one frequency (its index formed in 64-bit integers);
// specy loads are coalesced.  Every sum is reduced by a fixed xor butterfly inside a wave, the four waves are added in wave order, and
// the workgroup writes its 2 + n_param (objective only: 2) partial sums to part[problem][workgroup][].
// segp_finish_kernel<n_param>: grid (problems), 1024 threads.  Every output is the sum over the workgroups in a fixed two-level order that
// depends on T alone (neither on n_param nor on whether the gradient is asked for): contiguous runs of workgroups, each in ascending
// order, then the runs in ascending order; then the factors.  No atomics: a problem's bits depend neither on its batch mates nor on
// how the call was split into device batches, and an objective-only call gives the Obj bits of the call with the gradient.
#pragma once
#include "nagp_dev.hpp"

namespace nagp {

constexpr int SEGP_NT = 256;           // threads (= frequencies) of a pass workgroup
constexpr int SEGP_FIN_NT = 1024;      // threads of the finish kernel
constexpr int SEGP_MAXOUT = 5;         // two sums of the objective, at most three of the gradient

struct SegpPar {
  int64_t T;
  int nwg;                 // workgroups of a pass per problem
  int grad;                // 1: objective and gradient (2 + n_param sums), 0: objective only (2 sums)
  const double* param;     // problems x n_param
  const double* specy;     // T (spec_stride = 0) or problems x T
  int64_t spec_stride;
  const double* vary;      // problems (read when n_param <= 2)
  const double* varx;      // problems (read when n_param == 1)
  double* part;            // problems x nwg x n_out
  double* Obj;             // problems
  double* dObj;            // problems x n_param (grad = 1)
};

// len, varx, vary of problem `prob`; both kernels call this, so they see the same bits
struct SegpScal { double len, varx, vary; };

template <int NP>
__device__ inline SegpScal segp_scalars(const SegpPar& p, int prob) {
  const double* q = p.param + (size_t)prob * NP;
  SegpScal s;
  s.len = exp(q[0]);
  s.varx = NP >= 2 ? exp(q[1]) : p.varx[prob];
  s.vary = NP >= 3 ? exp(q[2]) : p.vary[prob];
  return s;
}

// f_j of getGPSESpec.m:18 for the 0-based index j: [0:ceil(T/2), -floor(T/2)+1:-1]
__host__ __device__ inline int64_t segp_freq(int64_t j, int64_t T) { return j <= (T + 1) / 2 ? j : j - T; }

template <int NP>
__global__ void __launch_bounds__(SEGP_NT) segp_pass_kernel(SegpPar p) {
  __shared__ double red[4 * SEGP_MAXOUT];             // [wave][n_out]
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int prob = blockIdx.y;
  constexpr int np = NP;
  const int64_t T = p.T;
  const int n_out = p.grad ? 2 + np : 2;
  const SegpScal s = segp_scalars<NP>(p, prob);
  const int64_t j = (int64_t)blockIdx.x * SEGP_NT + tid;
  const bool live = j < T;
  const int64_t jj = live ? j : 0;                    // a thread beyond T reads entry 0 and contributes zeros
  const double Td = (double)T;
  const double w = (2.0 * 3.14159265358979323846 * (double)segp_freq(jj, T)) / Td;
  const double sy = p.specy[(size_t)prob * p.spec_stride + jj];
  const double w2 = w * w;
  const double c = sqrt(2.0 * 3.14159265358979323846 * s.len * s.len) * exp(-w2 * s.len * s.len / 2.0);
  const double S = s.varx * c + s.vary;
  const double inv = 1.0 / S;
  double o_log = live ? log(S) : 0.0, o_div = live ? sy * inv : 0.0;
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) { o_log += __shfl_xor(o_log, m); o_div += __shfl_xor(o_div, m); }
  if (lane == 0) { red[wave * n_out] = o_log; red[wave * n_out + 1] = o_div; }
  if (p.grad) {
    const double g = live ? 0.5 * inv - (sy * inv * inv) / (2.0 * Td) : 0.0;       // 1./(2 S) - 1/(2T) specy./S.^2
    const double dc = c * (1.0 / s.len - w2 * s.len);
    double g0 = g * dc, g1 = g * c, g2 = g;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) { g0 += __shfl_xor(g0, m); g1 += __shfl_xor(g1, m); g2 += __shfl_xor(g2, m); }
    if (lane == 0) {
      red[wave * n_out + 2] = g0;
      if (np >= 2) red[wave * n_out + 3] = g1;
      if (np >= 3) red[wave * n_out + 4] = g2;
    }
  }
  __syncthreads();
  double* out = p.part + ((size_t)prob * p.nwg + blockIdx.x) * n_out;
  if (tid < n_out) out[tid] = ((red[tid] + red[n_out + tid]) + red[2 * n_out + tid]) + red[3 * n_out + tid];
}

// runs of the finish kernel's two-level sum over the workgroups: a function of T alone
__host__ __device__ inline int segp_finish_chunks(int nwg) {
  const int c = SEGP_FIN_NT / SEGP_MAXOUT;
  return c > nwg ? nwg : c;
}

template <int NP>
__global__ void __launch_bounds__(SEGP_FIN_NT) segp_finish_kernel(SegpPar p) {
  __shared__ double part[SEGP_FIN_NT];                // [run][output] when there is more than one run
  __shared__ double tot[SEGP_MAXOUT];
  const int tid = threadIdx.x, nwg = p.nwg, prob = blockIdx.x;
  constexpr int np = NP;
  const int n_out = p.grad ? 2 + np : 2;
  const int chunks = segp_finish_chunks(nwg), per = (nwg + chunks - 1) / chunks;     // the same runs for every n_param, with and without the gradient
  const double* pp = p.part + (size_t)prob * nwg * n_out;
  auto run = [&](int o, int w0, int w1) {
    double s = 0.0;
    for (int w = w0; w < w1; ++w) s += pp[(size_t)w * n_out + o];
    return s;
  };
  if (chunks > 1) {                                   // chunks * n_out <= chunks * SEGP_MAXOUT <= SEGP_FIN_NT
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
  const double Td = (double)p.T;
  if (tid == 0) p.Obj[prob] = (0.5 * tot[0] + (1.0 / (2.0 * Td)) * tot[1]) / Td;
  if (p.grad && tid < np) {
    const SegpScal s = segp_scalars<NP>(p, prob);
    const double f = tid == 0 ? s.len * s.varx : (tid == 1 ? s.varx : s.vary);
    p.dObj[(size_t)prob * np + tid] = (tot[2 + tid] * f) / Td;
  }
}

}  // namespace nagp

#define NAGP_LIST_SEGP_P(X, NP) X void nagp::segp_pass_kernel<NP>(nagp::SegpPar); X void nagp::segp_finish_kernel<NP>(nagp::SegpPar);
#define NAGP_LIST_SEGP(X) NAGP_LIST_SEGP_P(X, 1) NAGP_LIST_SEGP_P(X, 2) NAGP_LIST_SEGP_P(X, 3)
