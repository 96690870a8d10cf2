// nagp_slowfb.hpp -- the exact filterbank smoother with per-step observation noise (nagp_slowfb_run, include/nagp.h):
// the Kalman filter and RTS smoother of unifying_prob_tf/kernel_ss_kalmanSlowFB_rewrite.m:55-84, :100-134 for a scalar
// observation y_k = H x_k + e_k, e_k ~ N(0, vary_k), and a block-diagonal transition (blocks of B <= 8 states).
//
// The RTS recursion of the .m factorises an S x S matrix and forms two S^3 products per step inside a sequential chain.
// With a scalar observation the same smoothed moments follow without a factorisation from the adjoint recursion
// (de Jong 1989; the "modified Bryson-Frazier" form).  Write m-_k, P-_k for the predicted pair of step k (before its update),
// v_k = y_k - H m-_k, s_k = H P-_k H' + vary_k, K_k = P-_k H' / s_k, C_k = I - K_k H.  Backward from r = 0, N = 0:
//     r_k = H' v_k / s_k + C_k' A' r_{k+1}          N_k = H' H / s_k + C_k' A' N_{k+1} A C_k
//     MS_k = m-_k + P-_k r_k                        PS_k = P-_k - P-_k N_k P-_k
// A missing step (NaN) has v = 0, 1/s = 0, K = 0.  Three kernels:
//   sfb_forward_kernel<B>   one workgroup per series, sequential in k.  P lives in the LDS (S = 128: 128 KiB); A P A' + Q is a
//                           congruence tile by tile (tile (I,J) of b x b states maps to itself: in place, lower tiles computed, upper
//                           mirrored, so P stays symmetric to the bit); the update is rank one.  Stores m-_k, P-_k, v_k, 1/s_k, K_k
//                           (filter_only: the updated pair m_k, P_k instead) and accumulates lik.
//   sfb_backward_kernel<B>  one workgroup per series, sequential in k = T-1 .. 0, N in the LDS.  C' N C is N with rank-one
//                           corrections built from u = N K: N - H'u' - u H + H'H (K'u); A' N A is the tile congruence again.
//                           Publishes (r_k, N_k).  Sequential work per step: O(S^2) for u and the stores, O(S^2 B) for the congruence.
//   sfb_combine_kernel<NTL> one workgroup per (series, k): MS_k, and the requested part of PS_k.  W = N P- runs on the matrix
//                           cores (v_mfma_f64_16x16x4_f64), N padded to Sp = 16 NTL in the LDS, a 16-column panel of P- per wave read
//                           through its guards (rows and columns >= S are zeros, never addresses).  diag(P N P)_i = sum_j P_ji W_ji
//                           needs only the same panel.  Psub: Y = N P-(:, sub) the same way, then PS(a,b) = P(a,b) - P(:,a)' Y(:,b)
//                           for a >= b, written to (a,b) and (b,a): symmetric to the bit.
// Nothing here factorises, so there is no jitter retry.  No workgroup waits for another.
#pragma once
#include "nagp_dev.hpp"

namespace nagp {

struct SfbPar {
  int S, nblk;
  int64_t T;
  int filter_only;
  const double* Ab;     // [nblk][B*B] diagonal blocks of A, column-major
  const double* Qb;     // [nblk][B*B]
  const double* H;      // [S]
  const double* P0;     // [S][S]
  const double* y;      // [nb][T]
  const double* vary;   // [nb][T]
  double* pm;           // [nb][T][S]      m-_k   (filter_only: m_k)
  double* pP;           // [nb][T][S*S]    P-_k   (filter_only: P_k)
  double* vv;           // [nb][T]         v_k
  double* sinv;         // [nb][T]         1 / s_k   (0: missing step)
  double* K;            // [nb][T][S]
  double* r;            // [nb][T][S]
  double* N;            // [nb][T][S*S]
  double* lik;          // [nb]
  int* flag;            // [nb]  1: an innovation variance s <= 0
  int n_sub;
  const int* sub;       // [n_sub]
  double* MS;           // [nb][S*T]
  double* Pdiag;        // [nb][S*T]            (nullptr: not wanted)
  double* Psub;         // [nb][n_sub*n_sub*T]  (nullptr: not wanted)
};

__host__ __device__ inline size_t sfb_seq_lds_doubles(int S, int B) { return (size_t)S * S + 2 * (size_t)S * B + 6 * (size_t)S + 8; }
__host__ __device__ inline size_t sfb_combine_lds_doubles(int Sp) { return (size_t)Sp * (Sp + 1) + Sp; }

// index t of a lower tile (I >= J) in row order -> (I, J)
__device__ __forceinline__ void sfb_tile_ij(int t, int& I, int& J) {
  int i = (int)((sqrtf(8.0f * (float)t + 1.0f) - 1.0f) * 0.5f);
  while (i * (i + 1) / 2 > t) --i;
  while ((i + 1) * (i + 2) / 2 <= t) ++i;
  I = i; J = t - i * (i + 1) / 2;
}

// every lower tile of the symmetric S x S matrix M (LDS, column-major): TR = false: A_I M_IJ A_J' (+ Q_I on the diagonal),
// TR = true: A_I' M_IJ A_J.  In place: a tile maps to itself; the upper tiles are written as mirrors and never read.
template <int B, bool TR>
__device__ __forceinline__ void sfb_congruence(double* M, const double* Ab, const double* Qb, int S, int nblk, int tid, int NT) {
  const int ntl = nblk * (nblk + 1) / 2;
  for (int t = tid; t < ntl; t += NT) {
    int I, J;
    sfb_tile_ij(t, I, J);
    const double* AI = Ab + (size_t)I * B * B;
    const double* AJ = Ab + (size_t)J * B * B;
    double* Mt = M + (size_t)I * B + (size_t)J * B * S;
    double tl[B][B];
#pragma unroll
    for (int j = 0; j < B; ++j)
#pragma unroll
      for (int i = 0; i < B; ++i) tl[i][j] = Mt[i + (size_t)j * S];
    double* Mu = M + (size_t)J * B + (size_t)I * B * S;       // the mirror tile (J, I); the tile itself on the diagonal
#pragma unroll
    for (int i = 0; i < B; ++i) {
      double x[B];                                  // row i of A_I M (A_I' M)
#pragma unroll
      for (int j = 0; j < B; ++j) {
        double a = 0.0;
#pragma unroll
        for (int l = 0; l < B; ++l) a = fma(TR ? AI[l + i * B] : AI[i + l * B], tl[l][j], a);
        x[j] = a;
      }
#pragma unroll
      for (int j = 0; j < B; ++j) {
        if (I == J && j > i) continue;              // diagonal tile: the lower half, mirrored
        double a = 0.0;
#pragma unroll
        for (int l = 0; l < B; ++l) a = fma(x[l], TR ? AJ[l + j * B] : AJ[j + l * B], a);
        if (!TR && I == J) a += Qb[(size_t)I * B * B + i + j * B];
        Mt[i + (size_t)j * S] = a;
        Mu[j + (size_t)i * S] = a;
      }
    }
  }
}

// x . z over S entries of two LDS vectors, the same bits in every lane of every wave
__device__ __forceinline__ double sfb_dot(const double* x, const double* z, int S) {
  const int lane = threadIdx.x & 63;
  double a = 0.0;
  for (int j = lane; j < S; j += 64) a = fma(x[j], z[j], a);
  return wave_sum(a);
}

// LDS of the two sequential kernels: M[S*S] | Ab[S*B] | Qb[S*B] | v0 | v1 | h | w0 | w1 | (spare S)
template <int B>
__global__ void __launch_bounds__(512) sfb_forward_kernel(SfbPar p) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int tid = threadIdx.x, NT = blockDim.x, S = p.S, nblk = p.nblk;
  const int wave = tid >> 6, lane = tid & 63, nw = NT >> 6;
  double* P = lds;
  double* Ab = P + (size_t)S * S;
  double* Qb = Ab + (size_t)S * B;
  double* m0 = Qb + (size_t)S * B;
  double* m1 = m0 + S;
  double* hh = m1 + S;
  double* ph = hh + S;
  const int bd = blockIdx.x;
  const int64_t T = p.T;
  const bool fo = p.filter_only != 0;
  for (int e = tid; e < S * S; e += NT) P[e] = p.P0[e];
  for (int e = tid; e < S * B; e += NT) { Ab[e] = p.Ab[e]; Qb[e] = p.Qb[e]; }
  for (int i = tid; i < S; i += NT) { m0[i] = 0.0; hh[i] = p.H[i]; }
  const double* yy = p.y + (size_t)bd * T;
  const double* vr = p.vary + (size_t)bd * T;
  double* pm = p.pm + (size_t)bd * T * S;
  double* pP = p.pP + (size_t)bd * T * S * S;
  double* mc = m0;
  double* mn = m1;
  double lik = 0.0;
  int bad = 0;
  double yk = yy[0], rk = vr[0];
  __syncthreads();
  for (int64_t k = 0; k < T; ++k) {
    const double yn = (k + 1 < T) ? yy[k + 1] : 0.0, rn = (k + 1 < T) ? vr[k + 1] : 0.0;    // the next step's, in flight during this one
    if (k > 0) {                                                // m = A m;  P = A P A' + Q
      if (tid < S) {
        const int I = tid / B, il = tid - I * B;
        double a = 0.0;
#pragma unroll
        for (int l = 0; l < B; ++l) a = fma(Ab[(size_t)I * B * B + il + l * B], mc[I * B + l], a);
        mn[tid] = a;
      }
      sfb_congruence<B, false>(P, Ab, Qb, S, nblk, tid, NT);
      double* t_ = mc; mc = mn; mn = t_;
      lds_barrier();
    }
    if (!fo) {                                                  // the predicted pair of step k
      if (tid < S) pm[(size_t)k * S + tid] = mc[tid];
      double* Pk = pP + (size_t)k * S * S;
      for (int e = tid; e < S * S; e += NT) Pk[e] = P[e];
    }
    const bool obs = !(yk != yk);
    if (obs) {
      if (tid < S) {                                            // P H'
        double a0 = 0.0, a1 = 0.0;
        int j = 0;
        for (; j + 2 <= S; j += 2) { a0 = fma(P[tid + (size_t)j * S], hh[j], a0); a1 = fma(P[tid + (size_t)(j + 1) * S], hh[j + 1], a1); }
        if (j < S) a0 = fma(P[tid + (size_t)j * S], hh[j], a0);
        ph[tid] = a0 + a1;
      }
      lds_barrier();
      const double s = sfb_dot(hh, ph, S) + rk;
      const double v = yk - sfb_dot(hh, mc, S);
      const double si = 1.0 / s;
      if (!(s > 0.0)) bad = 1;
      lik -= 0.9189385332046727 + 0.5 * log(s) + 0.5 * v / s * v;
      if (tid < S) {
        const double Kt = ph[tid] / s;
        mn[tid] = mc[tid] + Kt * v;
        if (!fo) p.K[((size_t)bd * T + k) * S + tid] = Kt;
      }
      if (tid == 0 && !fo) { p.vv[(size_t)bd * T + k] = v; p.sinv[(size_t)bd * T + k] = si; }
      for (int j = wave; j < S; j += nw) {                      // P - K H P, as P_ij - (ph_i ph_j) / s: symmetric to the bit
        const double pj = ph[j];
        for (int i = lane; i < S; i += 64) P[i + (size_t)j * S] = fma(-__dmul_rn(ph[i], pj), si, P[i + (size_t)j * S]);
      }
      double* t_ = mc; mc = mn; mn = t_;
    } else if (!fo) {
      if (tid < S) p.K[((size_t)bd * T + k) * S + tid] = 0.0;
      if (tid == 0) { p.vv[(size_t)bd * T + k] = 0.0; p.sinv[(size_t)bd * T + k] = 0.0; }
    }
    lds_barrier();
    if (fo) {                                                   // the updated pair of step k
      if (tid < S) pm[(size_t)k * S + tid] = mc[tid];
      double* Pk = pP + (size_t)k * S * S;
      for (int e = tid; e < S * S; e += NT) Pk[e] = P[e];
      lds_barrier();
    }
    yk = yn; rk = rn;
  }
  if (tid == 0) { p.lik[bd] = bad ? __builtin_nan("") : lik; p.flag[bd] = bad; }
}

template <int B>
__global__ void __launch_bounds__(512) sfb_backward_kernel(SfbPar p) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int tid = threadIdx.x, NT = blockDim.x, S = p.S, nblk = p.nblk;
  const int wave = tid >> 6, lane = tid & 63, nw = NT >> 6;
  double* N = lds;
  double* Ab = N + (size_t)S * S;
  double* r0 = Ab + 2 * (size_t)S * B;
  double* r1 = r0 + S;
  double* hh = r1 + S;
  double* kk = hh + S;
  double* uu = kk + S;
  const int bd = blockIdx.x;
  const int64_t T = p.T;
  for (int e = tid; e < S * S; e += NT) N[e] = 0.0;
  for (int e = tid; e < S * B; e += NT) Ab[e] = p.Ab[e];
  for (int i = tid; i < S; i += NT) { r0[i] = 0.0; hh[i] = p.H[i]; }
  const double* Kg = p.K + (size_t)bd * T * S;
  const double* vg = p.vv + (size_t)bd * T;
  const double* sg = p.sinv + (size_t)bd * T;
  double* rg = p.r + (size_t)bd * T * S;
  double* Ng = p.N + (size_t)bd * T * S * S;
  double* rc = r0;
  double* rn = r1;
  double Kc = (tid < S) ? Kg[(size_t)(T - 1) * S + tid] : 0.0, vk = vg[T - 1], sk = sg[T - 1];
  __syncthreads();
  for (int64_t k = T - 1; k >= 0; --k) {
    double Kn = 0.0, vn = 0.0, sn = 0.0;                        // the next step's, in flight during this one
    if (k > 0) { Kn = (tid < S) ? Kg[(size_t)(k - 1) * S + tid] : 0.0; vn = vg[k - 1]; sn = sg[k - 1]; }
    double* Nk = Ng + (size_t)k * S * S;
    if (sk != 0.0) {                                            // an observed step
      if (tid < S) kk[tid] = Kc;
      lds_barrier();
      if (tid < S) {                                            // u = N K
        double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
        int j = 0;
        for (; j + 4 <= S; j += 4) {
          a0 = fma(N[tid + (size_t)j * S], kk[j], a0); a1 = fma(N[tid + (size_t)(j + 1) * S], kk[j + 1], a1);
          a2 = fma(N[tid + (size_t)(j + 2) * S], kk[j + 2], a2); a3 = fma(N[tid + (size_t)(j + 3) * S], kk[j + 3], a3);
        }
        for (; j < S; ++j) a0 = fma(N[tid + (size_t)j * S], kk[j], a0);
        uu[tid] = (a0 + a1) + (a2 + a3);
      }
      lds_barrier();
      const double c = sfb_dot(kk, uu, S) + sk;                 // K' N K + 1/s
      const double g = vk * sk - sfb_dot(kk, rc, S);            // v/s - K' r
      if (tid < S) {
        const double rv = fma(hh[tid], g, rc[tid]);             // r = H' v/s + (I - K H)' r
        rn[tid] = rv;
        rg[(size_t)k * S + tid] = rv;
      }
      for (int j = wave; j < S; j += nw) {                      // N = H'H/s + C' N C, every term symmetric to the bit
        const double hj = hh[j], uj = uu[j];
        for (int i = lane; i < S; i += 64) {
          double nv = N[i + (size_t)j * S];
          const double hi = hh[i];
          if (hi != 0.0 || hj != 0.0) {
            const double t = __dadd_rn(__dmul_rn(hi, uj), __dmul_rn(uu[i], hj));
            nv = __dadd_rn(__dsub_rn(nv, t), __dmul_rn(__dmul_rn(hi, hj), c));
            N[i + (size_t)j * S] = nv;
          }
          Nk[i + (size_t)j * S] = nv;
        }
      }
      double* t_ = rc; rc = rn; rn = t_;
    } else {
      if (tid < S) rg[(size_t)k * S + tid] = rc[tid];
      for (int e = tid; e < S * S; e += NT) Nk[e] = N[e];
    }
    lds_barrier();
    if (k > 0) {                                                // r = A' r;  N = A' N A
      if (tid < S) {
        const int I = tid / B, il = tid - I * B;
        double a = 0.0;
#pragma unroll
        for (int l = 0; l < B; ++l) a = fma(Ab[(size_t)I * B * B + l + il * B], rc[I * B + l], a);
        rn[tid] = a;
      }
      sfb_congruence<B, true>(N, Ab, nullptr, S, nblk, tid, NT);
      double* t_ = rc; rc = rn; rn = t_;
      lds_barrier();
    }
    Kc = Kn; vk = vn; sk = sn;
  }
}

// acc[ti] += N[rows of tile ti, :] * X[:, 16 columns]: lane (lr, lk) supplies N(16 ti + lr, 4 ks + lk) from the LDS and
// X(4 ks + lk, column lr of the panel) from global memory; xcol = nullptr: a padding column (zeros)
template <int NTL>
__device__ __forceinline__ void sfb_panel(const double* Ns, int LD, const double* xcol, int S, v4d (&acc)[NTL]) {
  const int lane = threadIdx.x & 63, lr = lane & 15, lk = lane >> 4;
#pragma unroll
  for (int ti = 0; ti < NTL; ++ti) acc[ti] = v4d{0.0, 0.0, 0.0, 0.0};
#pragma unroll 2
  for (int ks = 0; ks < 4 * NTL; ++ks) {
    const int row = 4 * ks + lk;
    const double b = (xcol && row < S) ? xcol[row] : 0.0;
#pragma unroll
    for (int ti = 0; ti < NTL; ++ti) {
      const double a = Ns[(size_t)(16 * ti + lr) * LD + row];
      acc[ti] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[ti], 0, 0, 0);
    }
  }
}

// sum over the rows of  acc(row, column lr) * z(row): every lane of column lr gets the sum  (acc element r of tile ti: row 16 ti + lk + 4 r)
template <int NTL>
__device__ __forceinline__ double sfb_coldot(const v4d (&acc)[NTL], const double* z, int S) {
  const int lk = (threadIdx.x & 63) >> 4;
  double a = 0.0;
#pragma unroll
  for (int ti = 0; ti < NTL; ++ti)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = 16 * ti + lk + 4 * r;
      if (row < S) a = fma(acc[ti][r], z[row], a);
    }
  a += __shfl_xor(a, 16);
  a += __shfl_xor(a, 32);
  return a;
}

template <int NTL>
__global__ void __launch_bounds__(256) sfb_combine_kernel(SfbPar p) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  constexpr int Sp = 16 * NTL, LD = Sp + 1;
  const int tid = threadIdx.x, S = p.S;
  const int wave = tid >> 6, lane = tid & 63, lr = lane & 15, lk = lane >> 4;
  double* Ns = lds;                         // Ns[j * LD + i] = N(i, j), zero beyond S
  double* rv = Ns + (size_t)Sp * LD;
  const int64_t k = blockIdx.x, T = p.T;
  const int bd = blockIdx.y;
  const bool smooth = p.filter_only == 0;
  const double* Pk = p.pP + ((size_t)bd * T + k) * S * S;
  const double* pmk = p.pm + ((size_t)bd * T + k) * S;
  if (smooth) {
    const double* Nk = p.N + ((size_t)bd * T + k) * S * S;
    for (int e = tid; e < Sp * Sp; e += 256) {
      const int i = e % Sp, j = e / Sp;
      Ns[(size_t)j * LD + i] = (i < S && j < S) ? Nk[i + (size_t)j * S] : 0.0;
    }
    if (tid < S) rv[tid] = p.r[((size_t)bd * T + k) * S + tid];
  }
  __syncthreads();
  if (tid < S) {                            // MS_k = m- + P- r
    double a0 = pmk[tid], a1 = 0.0;
    if (smooth) {
      int j = 0;
      for (; j + 2 <= S; j += 2) { a0 = fma(Pk[tid + (size_t)j * S], rv[j], a0); a1 = fma(Pk[tid + (size_t)(j + 1) * S], rv[j + 1], a1); }
      if (j < S) a0 = fma(Pk[tid + (size_t)j * S], rv[j], a0);
    }
    if (p.MS) p.MS[(size_t)bd * S * T + (size_t)k * S + tid] = a0 + a1;
  }
  if (p.Pdiag) {
    double* out = p.Pdiag + (size_t)bd * S * T + (size_t)k * S;
    if (!smooth) {
      if (tid < S) out[tid] = Pk[tid + (size_t)tid * S];
    } else {
      for (int c = wave; c < NTL; c += 4) {
        const int col = 16 * c + lr;
        const double* xc = (col < S) ? Pk + (size_t)col * S : nullptr;
        v4d acc[NTL];
        sfb_panel<NTL>(Ns, LD, xc, S, acc);
        const double d = sfb_coldot<NTL>(acc, xc ? xc : Pk, xc ? S : 0);
        if (xc && lk == 0) out[col] = xc[col] - d;
      }
    }
  }
  if (p.Psub) {
    const int ns = p.n_sub;
    double* out = p.Psub + ((size_t)bd * T + k) * ns * ns;
    if (!smooth) {
      for (int e = tid; e < ns * ns; e += 256) {
        const int a = e % ns, b = e / ns;
        out[e] = Pk[p.sub[a] + (size_t)p.sub[b] * S];
      }
    } else {
      const int npan = (ns + 15) / 16;
      for (int c = wave; c < npan; c += 4) {
        const int b = 16 * c + lr;
        const int sb = (b < ns) ? p.sub[b] : -1;
        const double* xc = (sb >= 0) ? Pk + (size_t)sb * S : nullptr;
        v4d acc[NTL];
        sfb_panel<NTL>(Ns, LD, xc, S, acc);
        for (int a = 16 * c; a < ns; ++a) {                     // PS(a, b) for a >= b, mirrored
          const int sa = p.sub[a];
          const double d = sfb_coldot<NTL>(acc, Pk + (size_t)sa * S, S);
          if (xc && lk == 0 && a >= b) {
            const double val = xc[sa] - d;
            out[a + (size_t)b * ns] = val;
            out[b + (size_t)a * ns] = val;
          }
        }
      }
    }
  }
}

}  // namespace nagp

#define NAGP_LIST_SLOWFB_B(P, B)                                                                                           \
  P void nagp::sfb_forward_kernel<B>(nagp::SfbPar); P void nagp::sfb_backward_kernel<B>(nagp::SfbPar);                     \
  P void nagp::sfb_combine_kernel<B>(nagp::SfbPar);
#define NAGP_LIST_SLOWFB(P)                                                                                                \
  NAGP_LIST_SLOWFB_B(P, 1) NAGP_LIST_SLOWFB_B(P, 2) NAGP_LIST_SLOWFB_B(P, 3) NAGP_LIST_SLOWFB_B(P, 4)                      \
  NAGP_LIST_SLOWFB_B(P, 5) NAGP_LIST_SLOWFB_B(P, 6) NAGP_LIST_SLOWFB_B(P, 7) NAGP_LIST_SLOWFB_B(P, 8)
