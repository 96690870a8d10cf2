// Fixed-point NMF of experiments/nmf/nmf_fp.m and nmf_inf_fp.m (objective: getObj_nmf_temp.m:48-54, :134), FP64, a batch of
// independent problems (restarts) on one data matrix.  See include/nagp.h (nagp_nmf_fp) for the boundary and DESIGN.md for the reasoning.
//
// One iteration of nmf_fp.m:65-87 is
//     AHat = H W + vary;  H <- ((A .* AHat^-2) W') ./ (AHat^-1 W') .* H          (:74-75)
//     Obj  <- sum(A ./ (H W + vary) + log(H W + vary)) / T                        (:77-79)
//     AHat = H W;         W <- (H' (A .* AHat^-2)) ./ (H' AHat^-1) .* W           (:81-82: vary is NOT added -- kept)
//     W <- diag(1 ./ sum(W,2)) W                                                  (:83)
//     Obj  <- the same expression with the new W                                  (:85-87)
// The second Obj of iteration l is a sum over the AHat = H W_new + vary that the H update of iteration l + 1 forms anyway, so an
// iteration is ONE pass over A, vary and H (nmf_pass_kernel) followed by a small kernel on the partial sums (nmf_finish_kernel), and
// a call ends with one closing pass that forms only that objective.  The phases are ordered by the kernel boundary on one stream.
//
// nmf_pass_kernel<K>: grid (ceil(T / 256), problems), 256 threads, a thread owns one time row and keeps H(t, :) in registers; W sits
// in the LDS; the loads of A(:, d), vary(:, d), H(:, k) are coalesced over t.  The sums over t of the W update, H' G1 and H' G2 with
// G1 = A .* AHat^-2, G2 = AHat^-1, are products over t: per tile of 16 columns d every wave multiplies its 64 rows with
// v_mfma_f64_16x16x4_f64 (K padded to 16, operands staged through the LDS), the four waves' tiles are added in wave order, and the
// workgroup writes its partial sums to pw[problem][workgroup][g][k + d K].  The objective terms are reduced by a fixed butterfly
// inside a wave and in wave order across waves, to po[problem][workgroup][2].
// nmf_finish_kernel: grid (problems), 1024 threads.  Every output (2 K D sums, 2 objective sums) is the sum over the workgroups in
// a fixed two-level order that depends on (T, K, D) alone: `chunks` contiguous runs of workgroups, each summed in ascending order,
// then the runs in ascending order.  It updates and normalises W and stores the objective entries.  No atomics anywhere: a
// problem's result depends neither on its batch mates nor on how the call was split into device batches.
#pragma once
#include "nagp_dev.hpp"

namespace nagp {

constexpr int NMF_NT = 256;            // threads (= time rows) of a pass workgroup
constexpr int NMF_LD = 17;             // row stride of the MFMA staging tiles: 16 + 1
constexpr int NMF_FIN_NT = 1024;       // threads of the finish kernel

struct NmfPar {
  int64_t T;
  int D, K;
  int nwg;               // workgroups of a pass per problem
  const double* A;       // T x D column-major, shared by the problems
  const double* vary;    // T x D, or nullptr = zeros
  double* W;             // problems x (K x D)
  double* H;             // problems x (T x K)
  double* pw;            // problems x nwg x 2 x (K D): partial sums of H' G1, H' G2
  double* po;            // problems x nwg x 2: partial sums of the two objectives of a pass
  double* Obj;           // problems x n_obj
  int n_obj;
  int obj_prev;          // index of the objective with the H of the pass's input (the second Obj of the iteration before), -1: not formed
  int obj_new;           // index of the objective with the updated H, -1: not formed (the closing pass)
  int update_h;          // 0: the closing pass
  int update_w;          // the pass forms the sums of the W update and the finish kernel applies it
};

constexpr size_t nmf_pass_lds_doubles(int K, int D) { return (size_t)K * D + 3 * (size_t)NMF_NT * NMF_LD + 2 * 4 * 256 + 8; }

template <int K>
__global__ void __launch_bounds__(NMF_NT) nmf_pass_kernel(NmfPar p) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, lr = lane & 15, lk = lane >> 4;
  const int D = p.D;
  const int64_t T = p.T;
  const int prob = blockIdx.y;
  double* Ws = lds;                                   // W(k, d) at k + d K
  double* Hs = Ws + (size_t)K * D;                    // [row][NMF_LD]: the updated H of the workgroup's rows, zero beyond K and beyond T
  double* G1 = Hs + (size_t)NMF_NT * NMF_LD;          // [row][NMF_LD]: G1 of the current tile of 16 columns
  double* G2 = G1 + (size_t)NMF_NT * NMF_LD;
  double* red = G2 + (size_t)NMF_NT * NMF_LD;         // [wave][g][k][16]
  double* ored = red + 2 * 4 * 256;                   // [2][wave]
  const double* Wg = p.W + (size_t)prob * K * D;
  for (int e = tid; e < K * D; e += NMF_NT) Ws[e] = Wg[e];
  const int64_t t = (int64_t)blockIdx.x * NMF_NT + tid;
  const bool live = t < T;
  const int64_t tt = live ? t : 0;                    // a row beyond T reads row 0 and contributes zeros
  double* Hg = p.H + (size_t)prob * T * K;
  double h[K];
#pragma unroll
  for (int k = 0; k < K; ++k) h[k] = Hg[tt + (size_t)k * T];
  __syncthreads();
  double o_prev = 0.0, o_new = 0.0;
  if (p.update_h || p.obj_prev >= 0) {
    double num[K], den[K];
#pragma unroll
    for (int k = 0; k < K; ++k) { num[k] = 0.0; den[k] = 0.0; }
    for (int d = 0; d < D; ++d) {
      const double a = p.A[tt + (size_t)d * T];
      const double v = p.vary ? p.vary[tt + (size_t)d * T] : 0.0;
      double s = 0.0;
#pragma unroll
      for (int k = 0; k < K; ++k) s = fma(h[k], Ws[k + d * K], s);
      const double ah = s + v;                        // :74
      const double inv = 1.0 / ah, q = a * inv * inv;
      if (p.obj_prev >= 0) o_prev += a * inv + log(ah);
#pragma unroll
      for (int k = 0; k < K; ++k) { num[k] = fma(q, Ws[k + d * K], num[k]); den[k] = fma(inv, Ws[k + d * K], den[k]); }
    }
    if (p.update_h) {
#pragma unroll
      for (int k = 0; k < K; ++k) h[k] = num[k] / den[k] * h[k];       // :75
      if (live) {
#pragma unroll
        for (int k = 0; k < K; ++k) Hg[t + (size_t)k * T] = h[k];
      }
    }
  }
  if (p.update_h) {
    if (p.update_w) {
#pragma unroll
      for (int k = 0; k < 16; ++k) Hs[tid * NMF_LD + k] = (k < K && live) ? h[k < K ? k : 0] : 0.0;
    }
    const int ntile = p.update_w ? (D + 15) / 16 : 0;
    if (!p.update_w) {                                // nmf_inf_fp.m: the objective alone
      for (int d = 0; d < D; ++d) {
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < K; ++k) s = fma(h[k], Ws[k + d * K], s);
        const double ah = s + (p.vary ? p.vary[tt + (size_t)d * T] : 0.0);
        o_new += p.A[tt + (size_t)d * T] / ah + log(ah);
      }
    }
    double* pwg = p.pw + ((size_t)prob * p.nwg + blockIdx.x) * 2 * K * D;
    for (int dt = 0; dt < ntile; ++dt) {
#pragma unroll 4
      for (int j = 0; j < 16; ++j) {
        const int d = 16 * dt + j;
        double g1 = 0.0, g2 = 0.0;
        if (d < D) {
          const double a = p.A[tt + (size_t)d * T];
          double s = 0.0;
#pragma unroll
          for (int k = 0; k < K; ++k) s = fma(h[k], Ws[k + d * K], s);
          const double ah = s + (p.vary ? p.vary[tt + (size_t)d * T] : 0.0);
          o_new += a / ah + log(ah);                  // :77-79
          const double inv = 1.0 / s;                 // :81: without vary
          if (live) { g2 = inv; g1 = a * inv * inv; }
        }
        G1[tid * NMF_LD + j] = g1; G2[tid * NMF_LD + j] = g2;
      }
      __syncthreads();
      v4d c1 = {0.0, 0.0, 0.0, 0.0}, c2 = {0.0, 0.0, 0.0, 0.0};
#pragma unroll 4
      for (int ks = 0; ks < 16; ++ks) {               // the wave's 64 rows, 4 at a time: C(k, d) += H(row, k) G(row, d)
        const int row = 64 * wave + 4 * ks + lk;
        const double a = Hs[row * NMF_LD + lr];
        c1 = __builtin_amdgcn_mfma_f64_16x16x4f64(a, G1[row * NMF_LD + lr], c1, 0, 0, 0);
        c2 = __builtin_amdgcn_mfma_f64_16x16x4f64(a, G2[row * NMF_LD + lr], c2, 0, 0, 0);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {                   // accumulator element r of lane (lr, lk): C(lk + 4 r, lr)
        red[((wave * 2 + 0) * 16 + lk + 4 * r) * 16 + lr] = c1[r];
        red[((wave * 2 + 1) * 16 + lk + 4 * r) * 16 + lr] = c2[r];
      }
      __syncthreads();
      for (int e = tid; e < 512; e += NMF_NT) {
        const int g = e >> 8, k = (e >> 4) & 15, j = e & 15, d = 16 * dt + j;
        if (k < K && d < D) {
          double s = red[((0 * 2 + g) * 16 + k) * 16 + j];
          s += red[((1 * 2 + g) * 16 + k) * 16 + j];
          s += red[((2 * 2 + g) * 16 + k) * 16 + j];
          s += red[((3 * 2 + g) * 16 + k) * 16 + j];
          pwg[(size_t)g * K * D + k + (size_t)d * K] = s;
        }
      }
      __syncthreads();
    }
  }
  // the two objective sums of the workgroup: a fixed butterfly inside each wave, then the waves in order
  if (!live) { o_prev = 0.0; o_new = 0.0; }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) { o_prev += __shfl_xor(o_prev, m); o_new += __shfl_xor(o_new, m); }
  if (lane == 0) { ored[wave] = o_prev; ored[4 + wave] = o_new; }
  __syncthreads();
  if (tid < 2) {
    const double s = ((ored[4 * tid] + ored[4 * tid + 1]) + ored[4 * tid + 2]) + ored[4 * tid + 3];
    p.po[((size_t)prob * p.nwg + blockIdx.x) * 2 + tid] = s;
  }
}

// chunks of the finish kernel's two-level sum over the workgroups: a function of the shape alone
__host__ __device__ inline int nmf_finish_chunks(int n_out, int nwg) {
  int c = NMF_FIN_NT / n_out;
  if (c > nwg) c = nwg;
  return c < 1 ? 1 : c;
}
constexpr size_t nmf_finish_lds_doubles(int K, int D) { return (size_t)NMF_FIN_NT + 2 * (size_t)K * D + 16; }

// UW: the call updates W (nmf_fp.m); false: the objective sums alone (nmf_inf_fp.m)
template <bool UW>
__global__ void __launch_bounds__(NMF_FIN_NT) nmf_finish_kernel(NmfPar p) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int tid = threadIdx.x, K = p.K, D = p.D, KD = K * D, nwg = p.nwg, prob = blockIdx.x;
  double* part = lds;                                 // [chunk][output] when chunks > 1
  double* num = lds + NMF_FIN_NT;                     // H' G1, then the updated W
  double* den = num + KD;                             // H' G2
  double* rs = den + KD;                              // 1 / row sums
  const int nw = (UW && p.update_w) ? 2 * KD : 0, n_out = nw + 2;      // (the closing pass of a UW call has update_w = 0)
  const int chunks = nmf_finish_chunks(n_out, nwg), per = (nwg + chunks - 1) / chunks;
  const double* pw = p.pw + (size_t)prob * nwg * 2 * KD;
  const double* po = p.po + (size_t)prob * nwg * 2;
  double* Wg = p.W + (size_t)prob * KD;
  double* Og = p.Obj + (size_t)prob * p.n_obj;
  // output o < nw: element o of a workgroup's (2 x K D) block of partial sums; o = nw, nw + 1: its two objective sums
  auto run = [&](int o, int w0, int w1) {
    double s = 0.0;
    if (o < nw) for (int w = w0; w < w1; ++w) s += pw[(size_t)w * 2 * KD + o];
    else        for (int w = w0; w < w1; ++w) s += po[(size_t)w * 2 + (o - nw)];
    return s;
  };
  if (chunks > 1) {                                   // chunks * n_out <= NMF_FIN_NT
    if (tid < chunks * n_out) {
      const int c = tid / n_out, o = tid % n_out, w0 = c * per, w1 = (w0 + per < nwg) ? w0 + per : nwg;
      part[c * n_out + o] = run(o, w0, w1);           // (an empty run at the end gives 0)
    }
    __syncthreads();
  }
  for (int o = tid; o < n_out; o += NMF_FIN_NT) {
    double s = 0.0;
    if (chunks > 1) { for (int c = 0; c < chunks; ++c) s += part[c * n_out + o]; }
    else s = run(o, 0, nwg);
    if (o < nw) { if (o < KD) num[o] = s; else den[o - KD] = s; }
    else {
      const int idx = (o == nw) ? p.obj_prev : p.obj_new;
      if (idx >= 0) Og[idx] = s / (double)p.T;        // getObj_nmf_temp.m:134
    }
  }
  if (nw == 0) return;
  __syncthreads();
  for (int o = tid; o < KD; o += NMF_FIN_NT) num[o] = num[o] / den[o] * Wg[o];      // :82
  __syncthreads();
  if (tid < K) {                                      // :83  diag(1 ./ sum(W,2)) W
    double s = 0.0;
    for (int d = 0; d < D; ++d) s += num[tid + d * K];
    rs[tid] = 1.0 / s;
  }
  __syncthreads();
  for (int o = tid; o < KD; o += NMF_FIN_NT) Wg[o] = rs[o % K] * num[o];
}

}  // namespace nagp

#define NAGP_LIST_NMF_K(P, K) P void nagp::nmf_pass_kernel<K>(nagp::NmfPar);
#define NAGP_LIST_NMF(P)                                                                                                      \
  P void nagp::nmf_finish_kernel<false>(nagp::NmfPar); P void nagp::nmf_finish_kernel<true>(nagp::NmfPar);                   \
  NAGP_LIST_NMF_K(P, 1) NAGP_LIST_NMF_K(P, 2) NAGP_LIST_NMF_K(P, 3) NAGP_LIST_NMF_K(P, 4) NAGP_LIST_NMF_K(P, 5) NAGP_LIST_NMF_K(P, 6)   \
  NAGP_LIST_NMF_K(P, 7) NAGP_LIST_NMF_K(P, 8) NAGP_LIST_NMF_K(P, 9) NAGP_LIST_NMF_K(P, 10) NAGP_LIST_NMF_K(P, 11) NAGP_LIST_NMF_K(P, 12) \
  NAGP_LIST_NMF_K(P, 13) NAGP_LIST_NMF_K(P, 14) NAGP_LIST_NMF_K(P, 15) NAGP_LIST_NMF_K(P, 16)
