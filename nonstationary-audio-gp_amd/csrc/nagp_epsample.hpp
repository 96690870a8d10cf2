// nagp_epsample.hpp -- joint posterior draws of a full-covariance EP run (nagp_ep_sample, include/nagp.h) by forward filtering
// with the sites the run returned and backward sampling (Fruehwirth-Schnatter 1994, Carter & Kohn 1994).
//
// The last forward pass of gf_ep_modulator*.m is a linear recursion in the returned sites (ttau, tnu); with the RTS smoother on
// top of it, it defines one Gaussian over the whole state path, whose backward chain is
//     x_{T-1} ~ N(MF_{T-1}, PF_{T-1}),      x_k | x_{k+1} ~ N( MF_k + G_k (x_{k+1} - A MF_k),  C_k ),
//     G_k = PF_k A' / PSkp_k,   PSkp_k = A PF_k A' + Q,   C_k = PF_k - G_k PSkp_k G_k' = (I - G_k A) PF_k (I - G_k A)' + G_k Q G_k'.
// Its marginals are the MS_k, PS_k of the run.  Three kernels, none of which waits for another workgroup:
//   eps_filter_kernel      one workgroup per call, sequential in k, P in the LDS.  A and Q are block diagonal, so A P A' + Q is two
//                          passes over (block, column) / (row, block) items, in place, O(S^2 b).  H has one non-zero per row: W = P H'
//                          is a gather of M columns, and the update of the reference (gf_ep_modulator_nmf.m:159-176) is a rank-M
//                          correction from M staged rows of P, an S x M x S product on the matrix cores.  Stores MF_k and PF_k.
//   eps_factor_kernel<NTL> one workgroup per step, all steps in flight: PSkp (lower triangle), its Cholesky factor with the
//                          reference's jitter retry, G by the two triangular solves (a thread per row of G), then C_k in the Joseph
//                          form above: the three S^3 products M1 PF, (M1 PF) M1' and (G Q) G' run on v_mfma_f64_16x16x4_f64 with the
//                          operands in the LDS, padded to Sp = 16 NTL through guards (an index >= S reads as zero and is never an
//                          address); results stay in the accumulators until every wave has read the operand they replace, so three
//                          S x S buffers are all the LDS holds.  Lc_k = chol(C_k): a pivot <= 0 zeroes its column and is counted.
//                          G_k takes the place of PF_k in global memory.  Step T-1 factorises PF_{T-1}.
//   eps_draw_kernel<NTL>   one workgroup per 16 draws, sequential in k = T-1 .. 0:  X = MF_k + [G_k | Lc_k] [X - A MF_k ; Z_k], an
//                          Sp x 2Sp x 16 product on the matrix cores, G_k and Lc_k streamed from global memory (every element is used
//                          once) and requested before Z_k is formed, the right-hand side in the LDS.  A column's result depends on nothing but its own
//                          draw.  One more workgroup runs the chain with z = 0, the RTS means, beside the draws.
//   eps_signal_kernel      a thread per (draw, step): Sdraw = sum_d a_d z_d from Fdraw.
#pragma once
#include "nagp_dev.hpp"

namespace nagp {

constexpr int EPS_MAXS = 80;            // ceiling on S: three S x S operands of the factor kernel in 160 KiB of LDS
constexpr int EPS_MAXB = 8;             // states per block
constexpr double EPS_JITTER = 0.005;    // sqrt(1e-4) * 0.5: the reference's retry (gf_ep_modulator_nmf.m:219-222) with rand -> 0.5

struct EpsPar {
  int S, M, D, N;
  int64_t T;
  int predict_at_k1;
  const double* A;      // [S][S] column-major, zero outside the blocks
  const double* Q;      // [S][S]
  const double* P0;     // [S][S]
  const double* Ab;     // packed diagonal blocks of A: block n at boff[n], b x b column-major
  const double* Qb;     // ... of Q
  const double* hval;   // [M]
  const int* off;       // [M+1] first state of a block
  const int* boff;      // [M+1] first double of a packed block
  const int* blk;       // [S]   block of a state
  const double* ttau;   // [T][M]
  const double* tnu;    // [T][M]
  const double* y;      // [T]   NaN = missing
  double* MF;           // [T][S]
  double* PG;           // [T][S*S]  PF_k from the filter; G_k from the factor kernel (k < T-1)
  double* Lc;           // [T][S*S]  lower factors of C_k (of PF_{T-1} at k = T-1), zero above the diagonal
  unsigned long long* cnt;   // [3] jitter retries of PSkp, clamped pivots of C_k, PSkp not positive definite with the jitter
  // the draws of one launch
  int n;                // draws of this launch
  int draw0;            // index of its first draw in the whole call (the generator counts draws of the call)
  unsigned long long seed;
  const double* z;      // [n][T][S] the caller's normals, or nullptr: the generator
  double* MSout;        // [T][S] or nullptr: one more workgroup runs the chain with z = 0 (the RTS means)
  double* X;            // [n][T][S] or nullptr
  double* F;            // [n][T][M] or nullptr
  // the signal
  const double* W;      // [D][N] column-major
  int link_kind; double link_shift;
  double* Sd;           // [n][T]
};

__host__ __device__ inline size_t eps_filter_lds_bytes(int S, int M, int nb2) {
  return ((size_t)S * S + 2 * (size_t)S * M + 2 * (size_t)S + 3 * (size_t)M + 2 * (size_t)nb2) * sizeof(double) + (2 * (size_t)M + 2 + S) * sizeof(int);
}
__host__ __device__ inline size_t eps_factor_lds_bytes(int S) { return 3 * (size_t)S * S * sizeof(double); }
__host__ __device__ inline size_t eps_draw_lds_bytes(int Sp) { return (3 * (size_t)Sp * 16 + 2 * (size_t)Sp) * sizeof(double); }

// ---------------------------------------------------------------------------------------------
// one (block, column) / (row, block) item of the congruence with the block size known at compile time: no predicate in the loops
template <int B>
__device__ __forceinline__ void eps_rows(double* col, const double* a) {                      // col[0 .. B) <- A_I col
  double v[B], r[B];
#pragma unroll
  for (int l = 0; l < B; ++l) v[l] = col[l];
#pragma unroll
  for (int q = 0; q < B; ++q) {
    double s = 0.0;
#pragma unroll
    for (int l = 0; l < B; ++l) s = fma(a[q + l * B], v[l], s);
    r[q] = s;
  }
#pragma unroll
  for (int q = 0; q < B; ++q) col[q] = r[q];
}
template <int B>
__device__ __forceinline__ void eps_cols(double* row, int S, const double* a, const double* qrow) {   // row[0 .. B) (stride S) <- row A_J' (+ Q)
  double v[B], r[B];
#pragma unroll
  for (int l = 0; l < B; ++l) v[l] = row[(size_t)l * S];
#pragma unroll
  for (int q = 0; q < B; ++q) {
    double s = 0.0;
#pragma unroll
    for (int l = 0; l < B; ++l) s = fma(v[l], a[q + l * B], s);
    if (qrow) s += qrow[q * B];
    r[q] = s;
  }
#pragma unroll
  for (int q = 0; q < B; ++q) row[(size_t)q * S] = r[q];
}
#define EPS_BY_BLOCK(b, CALL)                                                                                          \
  switch (b) { case 1: { constexpr int B = 1; CALL; } break; case 2: { constexpr int B = 2; CALL; } break; case 3: { constexpr int B = 3; CALL; } break; \
               case 4: { constexpr int B = 4; CALL; } break; case 5: { constexpr int B = 5; CALL; } break; case 6: { constexpr int B = 6; CALL; } break; \
               case 7: { constexpr int B = 7; CALL; } break; default: { constexpr int B = 8; CALL; } break; }

// the fixed-site filter (LB threads: 256 up to S = 32, 512 above)
template <int LB>
__global__ void __launch_bounds__(LB) eps_filter_kernel(EpsPar p) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int tid = threadIdx.x, NT = blockDim.x, S = p.S, M = p.M;
  const int nb2 = p.boff[M];
  double* P = lds;
  double* Kh = P + (size_t)S * S;          // [M][S]  (K H)(:, c_n) = K(:, n) h_n
  double* Rw = Kh + (size_t)S * M;         // [M][S]  row c_n of P
  double* m0 = Rw + (size_t)S * M;
  double* m1 = m0 + S;
  double* hv = m1 + S;
  double* cm = hv + M;                     // [M] m += W cm
  double* dd = cm + M;                     // [M] HPH + 1/ttau; 0: a site with ttau = 0
  double* Ab = dd + M;
  double* Qb = Ab + nb2;
  int* off = reinterpret_cast<int*>(Qb + nb2);
  int* boff = off + M + 1;
  int* blk = boff + M + 1;
  const int64_t T = p.T;
  for (int e = tid; e < S * S; e += NT) P[e] = p.P0[e];
  for (int e = tid; e < nb2; e += NT) { Ab[e] = p.Ab[e]; Qb[e] = p.Qb[e]; }
  for (int i = tid; i < S; i += NT) { m0[i] = 0.0; blk[i] = p.blk[i]; }
  for (int i = tid; i < M; i += NT) hv[i] = p.hval[i];
  for (int i = tid; i <= M; i += NT) { off[i] = p.off[i]; boff[i] = p.boff[i]; }
  double* mc = m0;
  double* mn = m1;
  double yk = p.y[0];
  double ttk = (tid < M) ? p.ttau[tid] : 0.0, tnk = (tid < M) ? p.tnu[tid] : 0.0;
  __syncthreads();
  for (int64_t k = 0; k < T; ++k) {
    double yn = 0.0, ttn = 0.0, tnn = 0.0;       // the next step's, in flight during this one
    if (k + 1 < T) {
      yn = p.y[k + 1];
      if (tid < M) { ttn = p.ttau[(size_t)(k + 1) * M + tid]; tnn = p.tnu[(size_t)(k + 1) * M + tid]; }
    }
    if (k > 0 || p.predict_at_k1) {              // m = A m;  P = (A P) A' + Q
      if (tid < S) {
        const int I = blk[tid], o = off[I], b = off[I + 1] - o;
        const double* a = Ab + boff[I] + (tid - o);
        double s = 0.0;
        for (int l = 0; l < b; ++l) s = fma(a[l * b], mc[o + l], s);
        mn[tid] = s;
      }
      for (int it = tid; it < M * S; it += NT) {           // rows of block I in column j
        const int j = it % S, I = it / S, o = off[I], b = off[I + 1] - o;      // a wave shares the block: its A entries are one LDS broadcast
        EPS_BY_BLOCK(b, eps_rows<B>(P + (size_t)j * S + o, Ab + boff[I]))
      }
      { double* t_ = mc; mc = mn; mn = t_; }
      lds_barrier();
      for (int it = tid; it < M * S; it += NT) {           // columns of block J in row i
        const int i = it % S, J = it / S, o = off[J], b = off[J + 1] - o;
        const double* qrow = (blk[i] == J) ? Qb + boff[J] + (i - o) : nullptr;
        EPS_BY_BLOCK(b, eps_cols<B>(P + i + (size_t)o * S, S, Ab + boff[J], qrow))
      }
      lds_barrier();
    }
    if (!(yk != yk)) {                           // an observed step: the update with the sites of step k
      if (tid < M) {
        const int c = off[tid];
        const double h = hv[tid];
        const double fm = h * mc[c], hp = h * P[c + (size_t)c * S] * h;
        if (ttk == 0.0) {                        // K = W ttau / (ttau HPH + 1) = 0: P - K W' is P
          cm[tid] = -(ttk * fm - tnk) / (ttk * hp + 1.0);
          dd[tid] = 0.0;
        } else {
          const double d = hp + 1.0 / ttk;
          cm[tid] = (tnk / ttk - fm) / d;
          dd[tid] = d;
        }
      }
      lds_barrier();
      for (int e = tid; e < S * M; e += NT) {
        const int i = e % S, n = e / S, c = off[n];
        const double d = dd[n], w = P[i + (size_t)c * S] * hv[n];
        Kh[e] = (d != 0.0) ? (w / d) * hv[n] : 0.0;
        Rw[e] = P[c + (size_t)i * S];
      }
      if (tid < S) {
        double s = 0.0;
        for (int n = 0; n < M; ++n) s = fma(P[tid + (size_t)off[n] * S] * hv[n], cm[n], s);
        mn[tid] = mc[tid] + s;
      }
      lds_barrier();
      {                                          // P - (K H) P: an S x M x S product, a 16 x 16 tile of P per wave and trip
        const int lane = tid & 63, lr = lane & 15, lk = lane >> 4, nw = NT >> 6, ntl = (S + 15) >> 4;
        for (int t = __builtin_amdgcn_readfirstlane(tid >> 6); t < ntl * ntl; t += nw) {
          const int ti = t % ntl, tj = t / ntl, ra = 16 * ti + lr, cb = 16 * tj + lr;
          v4d acc = v4d{0.0, 0.0, 0.0, 0.0};
          for (int n0 = 0; n0 < M; n0 += 4) {
            const int n = n0 + lk;
            const double ka = (ra < S && n < M) ? Kh[ra + (size_t)n * S] : 0.0;
            const double rb = (cb < S && n < M) ? Rw[cb + (size_t)n * S] : 0.0;
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(ka, rb, acc, 0, 0, 0);
          }
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int row = 16 * ti + lk + 4 * r;
            if (row < S && cb < S) P[row + (size_t)cb * S] -= acc[r];
          }
        }
      }
      { double* t_ = mc; mc = mn; mn = t_; }
      lds_barrier();
    }
    if (tid < S) p.MF[(size_t)k * S + tid] = mc[tid];
    double* Pk = p.PG + (size_t)k * S * S;
    for (int e = tid; e < S * S; e += NT) Pk[e] = P[e];
    lds_barrier();                               // P has been read before the next step rewrites it
    yk = yn; ttk = ttn; tnk = tnn;
  }
}

// ---------------------------------------------------------------------------------------------
// Cholesky factor of the lower triangle of V (LDS, column-major, leading dimension S), in place, by the whole workgroup; the
// caller has synchronised.  CLAMP: a pivot that is not > 0 zeroes its column; returns how many.  !CLAMP: returns 1 at the first
// such pivot (V is then half done).  Ends with a barrier.
template <bool CLAMP>
__device__ __forceinline__ int eps_chol(double* V, int S, int tid, int NT) {
  int bad = 0;
  for (int j = 0; j < S; ++j) {
    const double d = V[j + (size_t)j * S];
    if (!(d > 0.0)) {
      if (!CLAMP) return 1;
      ++bad;
      __syncthreads();
      for (int i = j + tid; i < S; i += NT) V[i + (size_t)j * S] = 0.0;
      __syncthreads();
      continue;
    }
    const double r = sqrt(d);
    for (int i = j + 1 + tid; i < S; i += NT) V[i + (size_t)j * S] /= r;
    __syncthreads();                             // every thread has read the pivot
    if (tid == 0) V[j + (size_t)j * S] = r;
    const int n = S - j - 1;
    for (int e = tid; e < n * n; e += NT) {
      const int i = j + 1 + e % n, c = j + 1 + e / n;
      if (i >= c) V[i + (size_t)c * S] = fma(-V[i + (size_t)j * S], V[c + (size_t)j * S], V[i + (size_t)c * S]);
    }
    __syncthreads();
  }
  return bad;
}

// acc += X(rows of tile ti, :) Y(:, columns of tile tj) over k < 16 NTL; xa(i, k), yb(k, j) return the operand or zero beyond S
template <int NTL, class FX, class FY>
__device__ __forceinline__ void eps_tile_mma(v4d& acc, int ti, int tj, FX xa, FY yb) {
  const int lane = threadIdx.x & 63, lr = lane & 15, lk = lane >> 4;
#pragma unroll 4
  for (int ks = 0; ks < 4 * NTL; ++ks) {
    const int kk = 4 * ks + lk;
    const double a = xa(16 * ti + lr, kk), b = yb(kk, 16 * tj + lr);
    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
  }
}

// lower tile t (row order) -> (ti >= tj)
__device__ __forceinline__ void eps_lower_tile(int t, int& ti, int& tj) {
  int i = 0;
  while ((i + 1) * (i + 2) / 2 <= t) ++i;
  ti = i; tj = t - i * (i + 1) / 2;
}

template <int NTL>
__global__ void __launch_bounds__(256) eps_factor_kernel(EpsPar p) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  constexpr int NT = 256, NFT = NTL * NTL, QT = (NFT + 3) / 4, NLT = NTL * (NTL + 1) / 2, QL = (NLT + 3) / 4;
  const int tid = threadIdx.x, S = p.S;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, lr = lane & 15, lk = lane >> 4;
  double* U = lds;                          // PF_k, then M1 PF_k, then C_k and its factor
  double* V = U + (size_t)S * S;            // PSkp and its factor L, then M1 = I - G A, then G Q
  double* W = V + (size_t)S * S;            // PF_k A', then G_k
  const int64_t k = blockIdx.x, T = p.T;
  const int SS = S * S;
  double* PGk = p.PG + (size_t)k * SS;
  double* Lck = p.Lc + (size_t)k * SS;
  const double* A = p.A;
  const double* Q = p.Q;
  const int* off = p.off;
  const int* blk = p.blk;
  if (k == T - 1) {                         // x_{T-1} ~ N(MF_{T-1}, PF_{T-1})
    for (int e = tid; e < SS; e += NT) U[e] = PGk[e];
    __syncthreads();
    const int bad = eps_chol<true>(U, S, tid, NT);
    if (tid == 0 && bad) atomicAdd(p.cnt + 1, (unsigned long long)bad);
    for (int e = tid; e < SS; e += NT) Lck[e] = (e % S >= e / S) ? U[e] : 0.0;
    return;
  }
  for (int e = tid; e < SS; e += NT) U[e] = PGk[e];
  __syncthreads();
  for (int attempt = 0; attempt < 2; ++attempt) {          // PSkp = (A PF) A' + Q, lower triangle; L = chol(PSkp)
    for (int e = tid; e < SS; e += NT) {
      const int i = e % S, j = e / S;
      if (i < j) continue;
      const int I = blk[i], J = blk[j], oi = off[I], ei = off[I + 1], oj = off[J], ej = off[J + 1];
      double s = 0.0;
      for (int m = oj; m < ej; ++m) {
        double t = 0.0;
        for (int l = oi; l < ei; ++l) t = fma(A[i + (size_t)l * S], U[l + (size_t)m * S], t);
        s = fma(t, A[j + (size_t)m * S], s);
      }
      if (I == J) s += Q[e];
      if (attempt == 1 && i == j) s += EPS_JITTER;
      V[e] = s;
    }
    __syncthreads();
    int bad;
    if (attempt == 0) bad = eps_chol<false>(V, S, tid, NT); else bad = eps_chol<true>(V, S, tid, NT);
    if (!bad) break;
    if (tid == 0) atomicAdd(p.cnt + (attempt == 0 ? 0 : 2), 1ull);
    __syncthreads();
  }
  for (int e = tid; e < SS; e += NT) {      // W = PF A'
    const int i = e % S, j = e / S, J = blk[j];
    double s = 0.0;
    for (int m = off[J]; m < off[J + 1]; ++m) s = fma(U[i + (size_t)m * S], A[j + (size_t)m * S], s);
    W[e] = s;
  }
  __syncthreads();
  if (tid < S) {                            // G = W / L' / L, row tid
    double* g = W + tid;
    for (int j = 0; j < S; ++j) {           // x L' = b
      double s = g[(size_t)j * S];
      for (int l = 0; l < j; ++l) s = fma(-g[(size_t)l * S], V[j + (size_t)l * S], s);
      g[(size_t)j * S] = s / V[j + (size_t)j * S];
    }
    for (int j = S - 1; j >= 0; --j) {      // g L = x
      double s = g[(size_t)j * S];
      for (int l = j + 1; l < S; ++l) s = fma(-g[(size_t)l * S], V[l + (size_t)j * S], s);
      g[(size_t)j * S] = s / V[j + (size_t)j * S];
    }
  }
  __syncthreads();
  for (int e = tid; e < SS; e += NT) {      // G out; V = M1 = I - G A
    const int i = e % S, j = e / S, J = blk[j];
    PGk[e] = W[e];
    double s = 0.0;
    for (int l = off[J]; l < off[J + 1]; ++l) s = fma(W[i + (size_t)l * S], A[l + (size_t)j * S], s);
    V[e] = ((i == j) ? 1.0 : 0.0) - s;
  }
  __syncthreads();
  auto ldU = [&](int i, int j) { return (i < S && j < S) ? U[i + (size_t)j * S] : 0.0; };
  auto ldV = [&](int i, int j) { return (i < S && j < S) ? V[i + (size_t)j * S] : 0.0; };
  auto ldVt = [&](int i, int j) { return (i < S && j < S) ? V[j + (size_t)i * S] : 0.0; };
  auto ldWt = [&](int i, int j) { return (i < S && j < S) ? W[j + (size_t)i * S] : 0.0; };
  {                                         // U = M1 PF
    v4d acc[QT];
#pragma unroll
    for (int q = 0; q < QT; ++q) {
      acc[q] = v4d{0.0, 0.0, 0.0, 0.0};
      const int t = wave + 4 * q;
      if (t < NFT) eps_tile_mma<NTL>(acc[q], t % NTL, t / NTL, ldV, ldU);
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < QT; ++q) {
      const int t = wave + 4 * q;
      if (t < NFT) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = 16 * (t % NTL) + lk + 4 * r, col = 16 * (t / NTL) + lr;
          if (row < S && col < S) U[row + (size_t)col * S] = acc[q][r];
        }
      }
    }
    __syncthreads();
  }
  v4d acc[QL];                              // C = (M1 PF) M1' + (G Q) G', lower tiles
#pragma unroll
  for (int q = 0; q < QL; ++q) {
    acc[q] = v4d{0.0, 0.0, 0.0, 0.0};
    const int t = wave + 4 * q;
    if (t < NLT) { int ti, tj; eps_lower_tile(t, ti, tj); eps_tile_mma<NTL>(acc[q], ti, tj, ldU, ldVt); }
  }
  __syncthreads();
  for (int e = tid; e < SS; e += NT) {      // V = G Q
    const int i = e % S, j = e / S, J = blk[j];
    double s = 0.0;
    for (int l = off[J]; l < off[J + 1]; ++l) s = fma(W[i + (size_t)l * S], Q[l + (size_t)j * S], s);
    V[e] = s;
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < QL; ++q) {
    const int t = wave + 4 * q;
    if (t < NLT) { int ti, tj; eps_lower_tile(t, ti, tj); eps_tile_mma<NTL>(acc[q], ti, tj, ldV, ldWt); }
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < QL; ++q) {
    const int t = wave + 4 * q;
    if (t < NLT) {
      int ti, tj; eps_lower_tile(t, ti, tj);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = 16 * ti + lk + 4 * r, col = 16 * tj + lr;
        if (row < S && col <= row) U[row + (size_t)col * S] = acc[q][r];
      }
    }
  }
  __syncthreads();
  const int bad = eps_chol<true>(U, S, tid, NT);
  if (tid == 0 && bad) atomicAdd(p.cnt + 1, (unsigned long long)bad);
  for (int e = tid; e < SS; e += NT) Lck[e] = (e % S >= e / S) ? U[e] : 0.0;
}

// ---------------------------------------------------------------------------------------------
// four standard normals of sample block q at (t, site): the generator of nagp_reconstruct (normal4, nagp_dev.hpp)
__device__ __forceinline__ void eps_normal4(int64_t t, int q, int site, unsigned k0, unsigned k1, double* z) {
  normal4((unsigned)t, (unsigned)((unsigned long long)t >> 32), (unsigned)q, (unsigned)site, k0, k1, z);
}

// NTL waves, wave ti owns rows 16 ti .. 16 ti + 15.  The operands of step k from G_k and Lc_k do not depend on the state: they are
// requested at the top of the step and arrive while Z_k and X - A MF_k are formed.  With p.MSout the last workgroup of the grid runs the
// chain with z = 0 (the RTS means) beside the draws.
template <int NTL>
__global__ void __launch_bounds__(64 * NTL) eps_draw_kernel(EpsPar p) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  constexpr int NT = 64 * NTL, Sp = 16 * NTL, NK = 4 * NTL;
  const int tid = threadIdx.x, S = p.S, M = p.M;
  const int ti = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, lr = lane & 15, lk = lane >> 4;
  double* xs = lds;                         // [Sp][16] the state of the 16 draws
  double* dv = xs + Sp * 16;                // [Sp][16] X - A MF_k
  double* zv = dv + Sp * 16;                // [Sp][16] Z_k
  double* mf = zv + Sp * 16;                // [Sp] MF_k
  double* am = mf + Sp;                     // [Sp] A MF_k
  const int64_t T = p.T;
  const int SS = S * S;
  const bool mean = p.MSout != nullptr && blockIdx.x == gridDim.x - 1;
  const int c0 = mean ? 0 : 16 * blockIdx.x;         // first draw of the block inside the launch
  const int nc = mean ? 1 : ((p.n - c0 < 16) ? p.n - c0 : 16);
  const int g0 = p.draw0 + c0;              // ... in the call
  double* const Xo = mean ? p.MSout : p.X;
  double* const Fo = mean ? nullptr : p.F;
  const bool zero_z = mean;
  const unsigned k0s = (unsigned)p.seed, k1s = (unsigned)(p.seed >> 32);
  const int* off = p.off;
  for (int e = tid; e < 3 * Sp * 16 + 2 * Sp; e += NT) lds[e] = 0.0;
  double mfn = (tid < S) ? p.MF[(size_t)(T - 1) * S + tid] : 0.0;
  double arow[EPS_MAXB];                    // row tid of A inside its block
  int ao = 0, ab = 0;
  if (tid < S) { const int I = p.blk[tid]; ao = off[I]; ab = off[I + 1] - ao; }
#pragma unroll
  for (int l = 0; l < EPS_MAXB; ++l) arow[l] = (l < ab) ? p.A[tid + (size_t)(ao + l) * S] : 0.0;
  const int row = 16 * ti + lr;
  __syncthreads();
  for (int64_t k = T - 1; k >= 0; --k) {
    const bool last = k == T - 1;
    const double* Gk = p.PG + (size_t)k * SS;
    const double* Lk = p.Lc + (size_t)k * SS;
    double aG[NK], aL[NK];
#pragma unroll
    for (int ks = 0; ks < NK; ++ks) {
      const int kk = 4 * ks + lk;
      aG[ks] = (!last && row < S && kk < S) ? Gk[row + (size_t)kk * S] : 0.0;
      aL[ks] = (row < S && kk <= row) ? Lk[row + (size_t)kk * S] : 0.0;
    }
    if (tid < S) mf[tid] = mfn;
    if (k > 0 && tid < S) mfn = p.MF[(size_t)(k - 1) * S + tid];      // in flight during this step
    // Z_k
    if (zero_z) {
      // (zv stays zero)
    } else if (p.z) {
      for (int e = tid; e < nc * S; e += NT) {
        const int col = e / S, j = e % S;
        zv[j * 16 + col] = p.z[((size_t)(c0 + col) * T + k) * S + j];
      }
    } else {
      const int q0 = g0 >> 2;
      for (int e = tid; e < 5 * S; e += NT) {
        const int j = e % S, q = q0 + e / S;
        if (4 * q < g0 + nc) {
          double z4[4];
          eps_normal4(k, q, j, k0s, k1s, z4);
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const int col = 4 * q + u - g0;
            if (col >= 0 && col < nc) zv[j * 16 + col] = z4[u];
          }
        }
      }
    }
    lds_barrier();
    if (!last) {
      if (tid < S) {                        // A MF_k
        double s = 0.0;
#pragma unroll
        for (int l = 0; l < EPS_MAXB; ++l) if (l < ab) s = fma(arow[l], mf[ao + l], s);
        am[tid] = s;
      }
      lds_barrier();
      for (int e = tid; e < 16 * S; e += NT) { const int j = e / 16; dv[e] = xs[e] - am[j]; }
      lds_barrier();
    }
    v4d acc = v4d{0.0, 0.0, 0.0, 0.0};
    if (!last) {
#pragma unroll
      for (int ks = 0; ks < NK; ++ks) {
        const int kk = 4 * ks + lk;
        const double b = (kk < S) ? dv[kk * 16 + lr] : 0.0;
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(aG[ks], b, acc, 0, 0, 0);
      }
    }
#pragma unroll
    for (int ks = 0; ks < NK; ++ks) {
      const int kk = 4 * ks + lk;
      const double b = (kk < S) ? zv[kk * 16 + lr] : 0.0;
      acc = __builtin_amdgcn_mfma_f64_16x16x4f64(aL[ks], b, acc, 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int rw = 16 * ti + lk + 4 * r;
      if (rw < S) xs[rw * 16 + lr] = mf[rw] + acc[r];
    }
    lds_barrier();
    if (Xo) for (int e = tid; e < nc * S; e += NT) { const int col = e / S, j = e % S; Xo[((size_t)(c0 + col) * T + k) * S + j] = xs[j * 16 + col]; }
    if (Fo) for (int e = tid; e < nc * M; e += NT) { const int col = e / M, n = e % M; Fo[((size_t)(c0 + col) * T + k) * M + n] = p.hval[n] * xs[off[n] * 16 + col]; }
  }
}

// Sdraw = sum_d a_d z_d,  a_d = W_d . link(g) or its square root, on the draw's own z_d, g_n (the amplitudes and links of
// nagp_reconstruct_sources)
template <bool AMP_SQRT>
__global__ void __launch_bounds__(256) eps_signal_kernel(EpsPar p) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (size_t)p.n * p.T) return;
  const int D = p.D, N = p.N;
  const double* f = p.F + e * p.M;
  double sig = 0.0;
  for (int d = 0; d < D; ++d) {
    double a = 0.0;
    for (int n = 0; n < N; ++n) a = fma(p.W[d + (size_t)D * n], link_eval(p.link_kind, p.link_shift, f[D + n]), a);
    if (AMP_SQRT) a = sqrt(a);
    sig = fma(a, f[d], sig);
  }
  p.Sd[e] = sig;
}

}  // namespace nagp

#define NAGP_LIST_EPSAMPLE_N(P, N) P void nagp::eps_factor_kernel<N>(nagp::EpsPar); P void nagp::eps_draw_kernel<N>(nagp::EpsPar);
#define NAGP_LIST_EPSAMPLE(P)                                                                                              \
  P void nagp::eps_filter_kernel<256>(nagp::EpsPar); P void nagp::eps_filter_kernel<512>(nagp::EpsPar);                    \
  P void nagp::eps_signal_kernel<false>(nagp::EpsPar); P void nagp::eps_signal_kernel<true>(nagp::EpsPar);                 \
  NAGP_LIST_EPSAMPLE_N(P, 1) NAGP_LIST_EPSAMPLE_N(P, 2) NAGP_LIST_EPSAMPLE_N(P, 3) NAGP_LIST_EPSAMPLE_N(P, 4) NAGP_LIST_EPSAMPLE_N(P, 5)
