// The squared-exponential basis-function primitive of experiments/toolsGP/basis2SEGP.m:21-28 -- the conv(., bas, 'same') that
// getObj_fitSE_basis_func.m, getObj_nmf_log_norm.m and getObj_nmf_log_norm_inf.m repeat -- as a direct convolution in FP64, batched over
// columns that each have their own taps.  See include/nagp.h (nagp_sebf_conv, nagp_tnmf_obj) for the boundary and DESIGN.md for the reasoning.
//
//     Y(t) = sum_{s = -tau .. tau} bas(s) Z(t - s),   Z = 0 outside 0 .. T-1,   bas(s) at taps[s + tau]  (built on the host, nagp_sebf_check.hpp)
//
// sebf_conv_kernel<MODE>: grid (columns x ceil(T / 2048)), 256 threads, a thread owns SEBF_R = 8 consecutive outputs in registers.  The
// taps are taken in chunks of SEBF_C = 512 in ascending s; a chunk and the window of Z it meets (2048 + 511 samples, zeros outside
// 0 .. T-1) are staged in the LDS.  Inside a chunk the taps go in blocks of 8: a thread reads the 15 window samples its 8 outputs meet
// in the block once and the 8 taps (the same address in every lane: a broadcast), then 64 fma().  Every output adds its taps in
// ascending s whatever the grid is: no atomics, no split of the tap range over workgroups.  A chunk whose whole window lies outside
// 0 .. T-1 is not run: it would add +-0 to a sum that starts at +0, which changes no bit.  A last chunk or block that is not full ends
// at tap 2 tau: nothing beyond the taps is multiplied (a padded tap would meet samples of Z the sum does not hold: Inf * 0).
// Window layout: sample i of the window lies at row i & 7, column i >> 3 of an 8 x 321 array.  The window index of (thread, output r,
// tap j) is 8 tid + r + 511 - j, so within a block of 8 taps a lane reads rows m & 7 at column tid + const: the 64 lanes of a read are
// 64 consecutive doubles (no two lanes of a ds_read_b64 group on one bank), and the address is one register plus a literal.
// MODE: what is stored -- the sum (CONV), + c[tap column] (ADDC: mux), - E(t) (SUBE: xHat - x), (. + E(t)) / T (ADDE_T: the gradient of
// the fit), . + E(t) / T (ADD_ET: the gradient of tnmf, whose input the row kernel has divided by T already).
// sebf_sumsq_kernel: grid (problems), 256 threads: sum of squares of n1 (and n2) entries per problem, thread tid adds entries tid,
// tid + 256, .. in ascending order, then a butterfly inside a wave and the waves in order: 1/2 sum z^2 + 1/2 sum dx^2 (FIT) or
// Obj + 1/2 sum X^2 / T (TNMF).  Products and sums are not contracted into fused multiply-adds except where fma() is written.
#pragma once
#include "nagp_dev.hpp"
#include "nagp_sebf_check.hpp"

namespace nagp {

constexpr int SEBF_U = 8;                                      // taps of a block
constexpr int SEBF_WIN = SEBF_TT + SEBF_C - 1;                 // samples of a staged window
constexpr int SEBF_P = 321;                                    // columns of the window array: >= ceil(SEBF_WIN / 8)
enum { SEBF_CONV = 0, SEBF_ADDC = 1, SEBF_SUBE = 2, SEBF_ADDE_T = 3, SEBF_ADD_ET = 4 };
static_assert(SEBF_R == 8 && SEBF_U == 8 && SEBF_C % 8 == 0, "the window layout keeps row = m & 7 only with 8 outputs per thread, blocks of 8 taps and whole blocks per chunk");
static_assert(SEBF_P * 8 >= SEBF_WIN, "the window array holds a window");

struct SebfPar {
  int64_t T;
  int ntile;             // workgroups per column
  int kc;                // columns per problem: column q is column q % kc of problem q / kc, at q / kc * ldp + q % kc * T of Z, E and Y
  int64_t ldp;
  int tmod;              // tap column of column q: q % tmod (the problems share their taps), or q with tmod = 0
  const int* tau;        // per tap column
  const int64_t* off;    // per tap column: its first tap in taps
  const double* taps;
  const double* c;       // ADDC: per tap column
  const double* Z;
  const double* E;       // SUBE, ADDE_T, ADD_ET
  double* Y;
};

template <int MODE>
__global__ void __launch_bounds__(SEBF_NT) sebf_conv_kernel(SebfPar p) {
#pragma clang fp contract(off)
  __shared__ __attribute__((aligned(16))) double win[8 * SEBF_P];
  __shared__ __attribute__((aligned(16))) double tp[SEBF_C];
  const int tid = threadIdx.x;
  const int64_t T = p.T;
  const int col = (int)(blockIdx.x / (unsigned)p.ntile), tile = (int)(blockIdx.x % (unsigned)p.ntile);
  const int tc = p.tmod ? col % p.tmod : col;
  const int64_t tau = p.tau[tc], n = 2 * tau + 1;
  const double* taps = p.taps + p.off[tc];
  const int64_t coff = (int64_t)(col / p.kc) * p.ldp + (int64_t)(col % p.kc) * T;
  const double* Z = p.Z + coff;
  const int64_t t0 = (int64_t)tile * SEBF_TT;
  double acc[SEBF_R];
#pragma unroll
  for (int r = 0; r < SEBF_R; ++r) acc[r] = 0.0;
  // chunk c holds the taps s0 .. s0 + C - 1, s0 = -tau + c C; its window starts at g0 = t0 - s0 - (C - 1) and meets 0 .. T-1 when
  // g0 <= T - 1 and g0 + SEBF_WIN - 1 >= 0
  const int64_t nchunk = (n + SEBF_C - 1) / SEBF_C;
  const int64_t lo = t0 - (SEBF_C - 1) - (T - 1) + tau;            // c C >= lo
  const int64_t hi = t0 + SEBF_TT - 1 + tau;                       // c C <= hi  (>= 0)
  const int64_t c_lo = lo <= 0 ? 0 : (lo + SEBF_C - 1) / SEBF_C;
  const int64_t c_hi = hi / SEBF_C < nchunk - 1 ? hi / SEBF_C : nchunk - 1;
  for (int64_t c = c_lo; c <= c_hi; ++c) {
    const int64_t j_first = c * SEBF_C;
    const int64_t g0 = t0 - (-tau + j_first) - (SEBF_C - 1);
    const int nC = (int)(n - j_first < SEBF_C ? n - j_first : SEBF_C);
    __syncthreads();                                               // the chunk before has been read
    for (int j = tid; j < SEBF_C; j += SEBF_NT) tp[j] = j < nC ? taps[j_first + j] : 0.0;
    for (int i = tid; i < SEBF_WIN; i += SEBF_NT) {
      const int64_t g = g0 + i;
      win[(i & 7) * SEBF_P + (i >> 3)] = (g >= 0 && g < T) ? Z[g] : 0.0;
    }
    __syncthreads();
    for (int jb = 0; jb * SEBF_U < nC; ++jb) {
      // block of the taps j = 8 jb + u: output r meets window sample 8 tid + (C - 8 - 8 jb) + m, m = r + 7 - u
      const double* wb = win + tid + (SEBF_C / 8 - 1 - jb);
      double w[SEBF_R + SEBF_U - 1], tv[SEBF_U];
#pragma unroll
      for (int m = 0; m < SEBF_R + SEBF_U - 1; ++m) w[m] = wb[(m & 7) * SEBF_P + (m >> 3)];
#pragma unroll
      for (int u = 0; u < SEBF_U; ++u) tv[u] = tp[jb * SEBF_U + u];
      const int nu = nC - jb * SEBF_U;
      if (nu >= SEBF_U) {
#pragma unroll
        for (int u = 0; u < SEBF_U; ++u)
#pragma unroll
          for (int r = 0; r < SEBF_R; ++r) acc[r] = fma(tv[u], w[r + SEBF_U - 1 - u], acc[r]);
      } else {
#pragma unroll
        for (int u = 0; u < SEBF_U - 1; ++u)
          if (u < nu) {
#pragma unroll
            for (int r = 0; r < SEBF_R; ++r) acc[r] = fma(tv[u], w[r + SEBF_U - 1 - u], acc[r]);
          }
      }
    }
  }
  const double Td = (double)T;
  double* Y = p.Y + coff;
  const double* E = (MODE == SEBF_CONV || MODE == SEBF_ADDC) ? nullptr : p.E + coff;
#pragma unroll
  for (int r = 0; r < SEBF_R; ++r) {
    const int64_t t = t0 + (int64_t)tid * SEBF_R + r;
    if (t < T) {
      double y = acc[r];
      if (MODE == SEBF_ADDC) y = y + p.c[tc];
      if (MODE == SEBF_SUBE) y = y - E[t];
      if (MODE == SEBF_ADDE_T) y = (y + E[t]) / Td;
      if (MODE == SEBF_ADD_ET) y = y + E[t] / Td;
      Y[t] = y;
    }
  }
}

enum { SEBF_SS_FIT = 0, SEBF_SS_TNMF = 1 };
struct SebfSumPar {
  int64_t T, n1, n2, ld1, ld2;   // n entries per problem from a + problem * ld
  const double* a1;
  const double* a2;              // FIT only
  double* Obj;
};

template <int MODE>
__global__ void __launch_bounds__(SEBF_NT) sebf_sumsq_kernel(SebfSumPar p) {
#pragma clang fp contract(off)
  __shared__ double red[2][4];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, prob = blockIdx.x;
  const double* a1 = p.a1 + (int64_t)prob * p.ld1;
  double s1 = 0.0, s2 = 0.0;
  for (int64_t i = tid; i < p.n1; i += SEBF_NT) { const double v = a1[i]; s1 += v * v; }
  if (MODE == SEBF_SS_FIT) {
    const double* a2 = p.a2 + (int64_t)prob * p.ld2;
    for (int64_t i = tid; i < p.n2; i += SEBF_NT) { const double v = a2[i]; s2 += v * v; }
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) { s1 += __shfl_xor(s1, m); s2 += __shfl_xor(s2, m); }
  if (lane == 0) { red[0][wave] = s1; red[1][wave] = s2; }
  __syncthreads();
  if (tid == 0) {
    const double t1 = ((red[0][0] + red[0][1]) + red[0][2]) + red[0][3], t2 = ((red[1][0] + red[1][1]) + red[1][2]) + red[1][3];
    const double Td = (double)p.T;
    if (MODE == SEBF_SS_FIT) p.Obj[prob] = (0.5 * t1 + 0.5 * t2) / Td;       // a1 = dx, a2 = z: getObj_fitSE_basis_func.m:36, :42
    else p.Obj[prob] = p.Obj[prob] + 0.5 * t1 / Td;                          // Obj holds obj1 / T
  }
}

}  // namespace nagp

#define NAGP_LIST_SEBF(P)                                                                                                          \
  P void nagp::sebf_conv_kernel<0>(nagp::SebfPar); P void nagp::sebf_conv_kernel<1>(nagp::SebfPar); P void nagp::sebf_conv_kernel<2>(nagp::SebfPar); \
  P void nagp::sebf_conv_kernel<3>(nagp::SebfPar); P void nagp::sebf_conv_kernel<4>(nagp::SebfPar);                                  \
  P void nagp::sebf_sumsq_kernel<0>(nagp::SebfSumPar); P void nagp::sebf_sumsq_kernel<1>(nagp::SebfSumPar);
