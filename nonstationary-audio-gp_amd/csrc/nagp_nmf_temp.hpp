// Conjugate-gradient NMF with temporal priors: objective and gradient of experiments/nmf/getObj_nmf_temp.m (learning form, variables
// [log H(:); log W(:)]) and getObj_nmf_temp_inf.m (inference form, variables log H(:), W given), FP64, a batch of independent problems
// (restarts) on one data matrix.  See include/nagp.h (nagp_nmf_temp_obj) for the boundary and DESIGN.md for the reasoning.
//
//     H = exp(logH);  W = exp(logW), W = diag(1 ./ sum(W,2)) W  (learning form; a given W is used as it is);  Ahat = H W + vary
//     obj1 = sum(A ./ Ahat + log(Ahat));  dA = (Ahat - A) ./ Ahat.^2;  dlogh = (dA W') .* H
//     dW = H' dA;  dWW = dW .* W;  dlogw = dWW - diag(sum(dWW,2)) W                                   (learning form)
//     prior (none / truncated-Gaussian chain / inverse-gamma chain): obj2 and dobj2dH of getObj_nmf_temp.m:69-131, three row forms each
//     obj = (obj1 + obj2) / T,  dobj = [dlogh + dobj2dH .* H; dlogw] / T
//
// nmft_pass_kernel<K, LEARN, MFMA>: grid (ceil(T / 256), problems), 256 threads, a thread owns one time row: H(t, :) in registers, W
// (normalised by every workgroup in the same order) and the per-component prior constants in the LDS, H of the workgroup's rows with
// one halo row on each side in the LDS for the neighbour terms.  It writes dlogh and, per workgroup, po[problem][workgroup][1 + nq K]:
// the sum of obj1 and the nq per-component sums over t that obj2 is made of (a fixed butterfly inside a wave, the waves in order), and
// in the learning form pw[problem][workgroup][k + d K], the workgroup's part of H' dA: per tile of 16 columns every wave multiplies its
// 64 rows with v_mfma_f64_16x16x4_f64 (K padded to 16, operands staged through the LDS) and the four waves are added in order; with
// MFMA = false one thread per (k, d) adds the 256 rows in ascending order on the VALU (the measured alternative, a developer switch).
// nmft_finish_kernel<LEARN>: grid (problems), 1024 threads: every output is the sum over the workgroups in a two-level order that
// depends on the shape alone (as nmf_finish_kernel), then obj2 from the per-component sums as the .m writes it, the / T, and the
// normalisation correction of dlogw.  No atomics anywhere: a problem's result depends neither on its batch mates, nor on whether the
// gradient was asked for, nor on how the call was cut into device batches.  Products and sums are not contracted into fused
// multiply-adds except where fma() is written: the H W dot product and dA W'.
#pragma once
#include "nagp_dev.hpp"
#include "nagp_nmf_temp_check.hpp"

namespace nagp {

constexpr int NMFT_NT = 256;          // threads (= time rows) of a pass workgroup
constexpr int NMFT_LD = 17;            // row stride of the staging tile of dA: 16 + 1
constexpr int NMFT_FIN_NT = 1024;      // threads of the finish kernel
constexpr int NMFT_NC = 6;             // prior constants per component
constexpr int NMFT_HS = NMFT_NT + 2;   // a component's row of the halo stage
enum { NMFT_NONE = 0, NMFT_TG = 1, NMFT_IG = 2 };

struct NmftPar {
  int64_t T;
  int D, K;
  int nwg;               // workgroups of a pass per problem
  int prior;             // NMFT_*
  int grad;              // 0: the objective alone
  int64_t nx;            // entries of x / dObj per problem: T K (+ K D in the learning form)
  const double* A;       // T x D column-major, shared by the problems
  const double* vary;    // T x D, or nullptr = zeros
  const double* x;       // problems x nx
  const double* Wg;      // inference form: problems x (K x D)
  const double* prm;     // muinf | varinf | lam, K each (read as the prior says)
  double* dObj;          // problems x nx
  double* pw;            // learning form: problems x nwg x (K D), partial sums of H' dA
  double* po;            // problems x nwg x (1 + nq K)
  double* Obj;           // problems
};

static_assert(NMFT_NT == NMFT_ROWS, "the shape arithmetic of nagp_nmf_temp_check.hpp counts workgroups of NMFT_NT rows");

constexpr size_t nmft_pass_lds_doubles(int K, int D, bool stage) {
  return (size_t)K * D + 16 + (size_t)NMFT_NC * 16 + 4 * 88 + (size_t)K * NMFT_HS + (stage ? (size_t)NMFT_NT * (K | 1) + (size_t)NMFT_NT * NMFT_LD + 4 * 256 : 0);
}

// W(k, d) at Ws[k + d K]: the given one, or exp(logW) with its rows scaled by 1 / (their sum over ascending d)
template <bool LEARN>
__device__ inline void nmft_load_w(const NmftPar& p, int prob, double* Ws, double* rs, int tid, int nt) {
#pragma clang fp contract(off)
  const int K = p.K, KD = p.K * p.D;
  if (LEARN) {
    const double* lw = p.x + (size_t)prob * p.nx + (size_t)p.T * K;
    for (int e = tid; e < KD; e += nt) Ws[e] = exp(lw[e]);
    __syncthreads();
    if (tid < K) {
      double s = 0.0;
      for (int d = 0; d < p.D; ++d) s += Ws[tid + d * K];
      rs[tid] = 1.0 / s;
    }
    __syncthreads();
    for (int e = tid; e < KD; e += nt) Ws[e] = rs[e % K] * Ws[e];
  } else {
    const double* w = p.Wg + (size_t)prob * KD;
    for (int e = tid; e < KD; e += nt) Ws[e] = w[e];
  }
  __syncthreads();
}

// the constants of component k.  TG: c[0] = lam^2 / varinf, c[1] = (1 + lam^2) / varinf, c[2] = 1 / varinf, c[3] = lam / varinf.
// IG (getObj_nmf_temp.m:75-84): c[0] = alp1, c[1] = bet1, c[2] = alp, c[3] = a, c[4] = b, c[5] = alp a.
__device__ inline void nmft_consts(const NmftPar& p, int k, double* c) {
#pragma clang fp contract(off)
  const double varinf = p.prm[p.K + k], lam = p.prm[2 * p.K + k];
  if (p.prior == NMFT_TG) {
    c[0] = lam * lam / varinf; c[1] = (1.0 + lam * lam) / varinf; c[2] = 1.0 / varinf; c[3] = lam / varinf; c[4] = 0.0; c[5] = 0.0;
  } else {
    const double muinf = p.prm[k];
    const double alp1 = muinf * muinf / varinf + 2.0;
    const double alp = 2.0 + lam * lam + muinf * muinf / varinf;
    c[0] = alp1; c[1] = (alp1 - 1.0) * muinf; c[2] = alp; c[3] = (alp - 1.0) * lam; c[4] = (alp - 1.0) * (1.0 - lam) * muinf; c[5] = alp * c[3];
  }
}

template <int K, bool LEARN, bool MFMA>
__global__ void __launch_bounds__(NMFT_NT) nmft_pass_kernel(NmftPar p) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, lr = lane & 15, lk = lane >> 4;
  const int D = p.D, prior = p.prior, nq = nmft_nq(prior), n_po = 1 + nq * K;
  const int64_t T = p.T;
  const int prob = blockIdx.y;
  double* Ws = lds;                                   // W(k, d) at k + d K
  double* rs = Ws + (size_t)K * D;                    // [16]
  double* pc = rs + 16;                               // [k][NMFT_NC]
  double* ored = pc + NMFT_NC * 16;                   // [wave][88]
  double* Hh = ored + 4 * 88;                         // [k][NMFT_HS]: H of rows t0 - 1 .. t0 + 256
  constexpr int HSD = K | 1;                          // odd row stride of Hs (a staging tile of 16 columns would leave one workgroup per CU)
  double* Hs = Hh + (size_t)K * NMFT_HS;              // [row][HSD]: H of the workgroup's rows, zero beyond T
  double* G = Hs + (size_t)NMFT_NT * HSD;             // [row][NMFT_LD]: dA of the current tile of 16 columns
  double* red = G + (size_t)NMFT_NT * NMFT_LD;        // [wave][k][16]
  nmft_load_w<LEARN>(p, prob, Ws, rs, tid, NMFT_NT);
  if (prior != NMFT_NONE && tid < K) nmft_consts(p, tid, pc + tid * NMFT_NC);
  const int64_t t = (int64_t)blockIdx.x * NMFT_NT + tid;
  const bool live = t < T;
  const int64_t tt = live ? t : 0;                    // a row beyond T reads row 0 and contributes zeros
  const double* xg = p.x + (size_t)prob * p.nx;
  double lh[K], h[K];
#pragma unroll
  for (int k = 0; k < K; ++k) { lh[k] = xg[tt + (size_t)k * T]; h[k] = exp(lh[k]); }
  if (prior != NMFT_NONE) {
#pragma unroll
    for (int k = 0; k < K; ++k) {
      Hh[k * NMFT_HS + tid + 1] = h[k];
      if (tid == 0) Hh[k * NMFT_HS] = (t > 0 && live) ? exp(xg[t - 1 + (size_t)k * T]) : 0.0;
      if (tid == NMFT_NT - 1) Hh[k * NMFT_HS + NMFT_NT + 1] = (t + 1 < T) ? exp(xg[t + 1 + (size_t)k * T]) : 0.0;
    }
  }
  const bool stage = LEARN && p.grad;
  if (stage) {
#pragma unroll
    for (int k = 0; k < K; ++k) Hs[tid * HSD + k] = live ? h[k] : 0.0;
  }
  __syncthreads();
  double o1 = 0.0, dh[K];
#pragma unroll
  for (int k = 0; k < K; ++k) dh[k] = 0.0;
  double* pwg = p.pw + ((size_t)prob * p.nwg + blockIdx.x) * K * D;
  const int ntile = (D + 15) / 16;
  for (int dt = 0; dt < ntile; ++dt) {
#pragma unroll 4
    for (int j = 0; j < 16; ++j) {
      const int d = 16 * dt + j;
      double g = 0.0;
      if (d < D) {
        const double a = p.A[tt + (size_t)d * T];
        const double v = p.vary ? p.vary[tt + (size_t)d * T] : 0.0;
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < K; ++k) s = fma(h[k], Ws[k + d * K], s);
        const double ah = s + v;
        o1 += a / ah + log(ah);
        const double da = (ah - a) / (ah * ah);
#pragma unroll
        for (int k = 0; k < K; ++k) dh[k] = fma(da, Ws[k + d * K], dh[k]);
        if (live) g = da;
      }
      if (stage) G[tid * NMFT_LD + j] = g;
    }
    if (stage) {
      __syncthreads();
      if (MFMA) {
        v4d c = {0.0, 0.0, 0.0, 0.0};
#pragma unroll 4
        for (int ks = 0; ks < 16; ++ks) {             // the wave's 64 rows, 4 at a time: C(k, d) += H(row, k) dA(row, d)
          const int row = 64 * wave + 4 * ks + lk;
          c = __builtin_amdgcn_mfma_f64_16x16x4f64(lr < K ? Hs[row * HSD + lr] : 0.0, G[row * NMFT_LD + lr], c, 0, 0, 0);   // K padded to 16 with zeros
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) red[(wave * 16 + lk + 4 * r) * 16 + lr] = c[r];      // accumulator element r of lane (lr, lk): C(lk + 4 r, lr)
        __syncthreads();
        {
          const int k = tid >> 4, j = tid & 15, d = 16 * dt + j;
          if (k < K && d < D)
            pwg[k + (size_t)d * K] = ((red[(0 * 16 + k) * 16 + j] + red[(1 * 16 + k) * 16 + j]) + red[(2 * 16 + k) * 16 + j]) + red[(3 * 16 + k) * 16 + j];
        }
      } else {
        const int k = tid >> 4, j = tid & 15, d = 16 * dt + j;
        if (k < K && d < D) {
          double s = 0.0;
          for (int row = 0; row < NMFT_NT; ++row) s = fma(Hs[row * HSD + k], G[row * NMFT_LD + j], s);
          pwg[k + (size_t)d * K] = s;
        }
      }
      __syncthreads();
    }
  }
  // the sums of the workgroup: a fixed butterfly inside each wave, then the waves in order
  auto wsum = [&](double v, int slot) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    if (lane == 0) ored[wave * 88 + slot] = v;
  };
  wsum(live ? o1 : 0.0, 0);
  const double Td = (double)T;
  double* dg = p.dObj + (size_t)prob * p.nx;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    double d2 = 0.0;
    if (prior != NMFT_NONE) {
      const double* c = pc + k * NMFT_NC;
      const double hk = h[k], hm = Hh[k * NMFT_HS + tid], hp = Hh[k * NMFT_HS + tid + 2];
      const bool first = t == 0, last = t == T - 1, inner = live && !first && !last;
      if (prior == NMFT_TG) {                         // getObj_nmf_temp.m:114-125
        wsum(inner ? hk * hk : 0.0, 1 + 0 * K + k);
        wsum((live && !first) ? hk * hm : 0.0, 1 + 1 * K + k);
        wsum(first ? hk * hk : 0.0, 1 + 2 * K + k);
        wsum(last ? hk * hk : 0.0, 1 + 3 * K + k);
        if (first) d2 = c[0] * hk - c[3] * hp;
        else if (last) d2 = c[2] * hk - c[3] * hm;
        else d2 = c[1] * hk - c[3] * (hp + hm);
      } else {                                        // :85-101
        const double ab = c[3] * hk + c[4];           // ahtpb(t), t < T
        const double abm = c[3] * hm + c[4];          // ahtpb(t - 1), t > 1
        wsum((live && !last) ? log(ab) : 0.0, 1 + 0 * K + k);
        wsum((live && !first) ? lh[k] : 0.0, 1 + 1 * K + k);
        wsum((live && !first) ? abm / hk : 0.0, 1 + 2 * K + k);
        wsum(first ? hk : 0.0, 1 + 3 * K + k);
        wsum(first ? lh[k] : 0.0, 1 + 4 * K + k);
        if (first) d2 = c[3] / hp - c[1] / (hk * hk) + (c[0] + 1.0) / hk - c[5] / ab;
        else if (last) d2 = -abm / (hk * hk) + (1.0 + c[2]) / hk;
        else d2 = c[3] / hp - abm / (hk * hk) + (c[2] + 1.0) / hk - c[5] / ab;
      }
    }
    if (p.grad && live) dg[t + (size_t)k * T] = (prior != NMFT_NONE) ? (dh[k] * h[k] + d2 * h[k]) / Td : dh[k] * h[k] / Td;
  }
  __syncthreads();
  if (tid < n_po) p.po[((size_t)prob * p.nwg + blockIdx.x) * n_po + tid] = ((ored[tid] + ored[88 + tid]) + ored[2 * 88 + tid]) + ored[3 * 88 + tid];
}

// chunks of the finish kernel's two-level sum over the workgroups: a function of the shape alone (not of p.grad)
__host__ __device__ inline int nmft_finish_chunks(int n_out, int nwg) {
  int c = NMFT_FIN_NT / n_out;
  if (c > nwg) c = nwg;
  return c < 1 ? 1 : c;
}
constexpr size_t nmft_finish_lds_doubles(int K, int D) { return (size_t)NMFT_FIN_NT + 2 * (size_t)K * D + 16 + 88 + 16; }

template <bool LEARN>
__global__ void __launch_bounds__(NMFT_FIN_NT) nmft_finish_kernel(NmftPar p) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int tid = threadIdx.x, K = p.K, D = p.D, KD = K * D, nwg = p.nwg, prob = blockIdx.x;
  const int nq = nmft_nq(p.prior), n_po = 1 + nq * K;
  double* part = lds;                                 // [chunk][output] when chunks > 1
  double* num = lds + NMFT_FIN_NT;                    // H' dA, then dWW
  double* Ws = num + KD;
  double* rs = Ws + KD;                               // [16]
  double* os = rs + 16;                               // [88]: the sums of po
  double* rw = os + 88;                               // [16]: sum(dWW, 2)
  const int nw_shape = LEARN ? KD : 0, nw = (LEARN && p.grad) ? KD : 0, n_out = nw + n_po;
  const int chunks = nmft_finish_chunks(nw_shape + n_po, nwg), per = (nwg + chunks - 1) / chunks;
  const double* pw = p.pw + (size_t)prob * nwg * KD;
  const double* po = p.po + (size_t)prob * nwg * n_po;
  // output o < nw: element o of a workgroup's K D block; beyond: entry o - nw of its po record
  auto run = [&](int o, int w0, int w1) {
    double s = 0.0;
    if (o < nw) for (int w = w0; w < w1; ++w) s += pw[(size_t)w * KD + o];
    else        for (int w = w0; w < w1; ++w) s += po[(size_t)w * n_po + (o - nw)];
    return s;
  };
  if (chunks > 1) {                                   // chunks * n_out <= NMFT_FIN_NT
    if (tid < chunks * n_out) {
      const int c = tid / n_out, o = tid % n_out, w0 = c * per, w1 = (w0 + per < nwg) ? w0 + per : nwg;
      part[c * n_out + o] = run(o, w0, w1);           // (an empty run at the end gives 0)
    }
    __syncthreads();
  }
  for (int o = tid; o < n_out; o += NMFT_FIN_NT) {
    double s = 0.0;
    if (chunks > 1) { for (int c = 0; c < chunks; ++c) s += part[c * n_out + o]; }
    else s = run(o, 0, nwg);
    if (o < nw) num[o] = s; else os[o - nw] = s;
  }
  __syncthreads();
  const double Td = (double)p.T;
  if (tid == 0) {
    double obj = os[0];
    if (p.prior == NMFT_TG) {                         // getObj_nmf_temp.m:114-116
      double t1 = 0.0, t2 = 0.0, t3 = 0.0, t4 = 0.0;
      for (int k = 0; k < K; ++k) {
        const double varinf = p.prm[K + k], lam = p.prm[2 * K + k];
        t1 += (1.0 + lam * lam) / (2.0 * varinf) * os[1 + 0 * K + k];
        t2 += 1.0 / (2.0 * varinf) * os[1 + 3 * K + k];
        t3 += lam * lam / (2.0 * varinf) * os[1 + 2 * K + k];
        t4 += lam / varinf * os[1 + 1 * K + k];
      }
      obj = obj + (t1 + t2 + t3 - t4);
    } else if (p.prior == NMFT_IG) {                  // :87-90
      double s1 = 0.0, s2 = 0.0, s3 = 0.0, s4 = 0.0, s5 = 0.0;
      for (int k = 0; k < K; ++k) {
        double c[NMFT_NC];
        nmft_consts(p, k, c);
        s1 += c[1] / os[1 + 3 * K + k];
        s2 += (c[0] + 1.0) * os[1 + 4 * K + k];
        s3 += c[2] * os[1 + 0 * K + k];
        s4 += (c[2] + 1.0) * os[1 + 1 * K + k];
        s5 += os[1 + 2 * K + k];
      }
      obj = obj + (s1 + s2 - s3 + s4 + s5);
    }
    p.Obj[prob] = obj / Td;
  }
  if (nw == 0) return;
  nmft_load_w<LEARN>(p, prob, Ws, rs, tid, NMFT_FIN_NT);
  for (int o = tid; o < KD; o += NMFT_FIN_NT) num[o] = num[o] * Ws[o];                 // dWW = dW .* W
  __syncthreads();
  if (tid < K) {
    double s = 0.0;
    for (int d = 0; d < D; ++d) s += num[tid + d * K];
    rw[tid] = s;
  }
  __syncthreads();
  double* dw = p.dObj + (size_t)prob * p.nx + (size_t)p.T * K;
  for (int o = tid; o < KD; o += NMFT_FIN_NT) dw[o] = (num[o] - rw[o % K] * Ws[o]) / Td;
}

}  // namespace nagp

#define NAGP_LIST_NMFT_K(P, K)                                                                                               \
  P void nagp::nmft_pass_kernel<K, false, true>(nagp::NmftPar); P void nagp::nmft_pass_kernel<K, true, true>(nagp::NmftPar); \
  P void nagp::nmft_pass_kernel<K, true, false>(nagp::NmftPar);
#define NAGP_LIST_NMFT(P)                                                                                                     \
  P void nagp::nmft_finish_kernel<false>(nagp::NmftPar); P void nagp::nmft_finish_kernel<true>(nagp::NmftPar);               \
  NAGP_LIST_NMFT_K(P, 1) NAGP_LIST_NMFT_K(P, 2) NAGP_LIST_NMFT_K(P, 3) NAGP_LIST_NMFT_K(P, 4) NAGP_LIST_NMFT_K(P, 5) NAGP_LIST_NMFT_K(P, 6)   \
  NAGP_LIST_NMFT_K(P, 7) NAGP_LIST_NMFT_K(P, 8) NAGP_LIST_NMFT_K(P, 9) NAGP_LIST_NMFT_K(P, 10) NAGP_LIST_NMFT_K(P, 11) NAGP_LIST_NMFT_K(P, 12) \
  NAGP_LIST_NMFT_K(P, 13) NAGP_LIST_NMFT_K(P, 14) NAGP_LIST_NMFT_K(P, 15) NAGP_LIST_NMFT_K(P, 16)
