// nagp_fbsample.hpp -- joint posterior draws of the stationary filterbank (nagp_fastfb_sample, include/nagp.h) by the
// simulation smoother (Durbin & Koopman 2002): draw a trajectory x* and data y* from the prior, smooth y - y* with the
// steady-state filter / smoother of nagp_fastfb_run, add x*.
//
// A draw (i = 0 .. n_draws-1, t = 0 .. T-1; `normals` = the generator of nagp_dev.hpp, restated on the host by the tests):
//     z[t][j] = normals(T, j, n_draws, seed)[t, i]   j = 0..S-1        e[t] = normals(T, S, n_draws, seed)[t, i]
//     x*_0 = Lp z[0];   x*_t = A x*_{t-1} + Lq z[t]                    (Lp Lp' = Pinf, Lq Lq' = Q)
//     y*_t = H x*_t + sqrt(R) e[t]  where y_t is observed, NaN where y_t is NaN
//     X_i  = x* + S_y(y - y*)                                          Ydraw_i[t] = H X_i[:, t]
// with S_y(.) the smoothed means nagp_fastfb_run returns (filter from m = 0, smoother with G, NaN = missing).  The mean over
// draws is S_y(y) in expectation; the covariance is the error covariance of that steady-state smoother under the model:
// Psm away from the ends and from gaps, larger inside gaps.
//
// The three recursions -- prior x*, filter, smoother -- are affine with time-constant matrices, and the draws are
// independent: the grid is (spans, draws).  Per scan: an OFFSET pass runs every span from a zero entry value (c_j), a
// boundary pass per draw walks  s_next = Phi_j s + c_j  over the spans, and the replay pass runs every span from its exact
// entry value and writes.  Only c_j depends on the draw: Phi_j is A^L (prior), G^len_j (smoother) or the product of the span's
// filter matrices, which depends on the NaN pattern of y alone (fastfb_compose_kernel<false> on y, once for all draws).
// With one span per draw (short series, or enough draws to fill the chip) only the replay pass runs.
// Matrix layouts are those of fastfb_filter_kernel: transposed in the LDS up to S = 96, read from global memory (L2) above,
// a thread per state.
#pragma once
#include "nagp_kernels.hpp"

namespace nagp {

struct FbsPar {
  int S;
  int64_t T;
  int64_t L;            // span length; span j = steps [j L, min((j+1) L, n)) of n = T (prior, filter) or T-1 (smoother) steps
  int ns;               // spans of the scan at hand
  int draw0;            // index of the first draw of this device batch (the generator counts draws of the whole call)
  unsigned long long seed;
  double sqrtR;
  const double* A;      // [S][S] column-major
  const double* B;      // prior: Lq ; filter: AKHA ; smoother: G      [S][S] column-major
  const double* Lp;     // [S][S] column-major                          (prior, step 0)
  const double* H;      // [S]
  const double* K;      // [S] gain                                      (filter)
  const double* y;      // [T]
  double* xs;           // [nb][T][S]  prior: x* out ; smoother: x* in, X out when want_x
  double* d;            // [nb][T]     prior: y - y* out ; filter: in
  double* ms;           // [nb][T][S]  filter: out ; smoother: in
  double* yd;           // [nb][T]     H X
  int want_x;
  double* c;            // [nb][ns][S] OFFSET pass out
  double* starts;       // [nb][ns][S] boundary pass out: value entering span j (nullptr: one span)
  const double* Phi;    // boundary: Phi_j = Phi + j * phi_stride for j < ns-1, PhiLast for j = ns-1; [S][S+4] row-major
  size_t phi_stride;
  const double* PhiLast;
  int mat_global;       // the two S x S matrices of a pass stay in global memory (S > 96)
};

// one standard normal: element (draw & 3) of normal4 at the counter (t, draw >> 2, site), bit for bit
__device__ __forceinline__ double fbs_normal(int64_t t, int draw, int site, unsigned k0, unsigned k1) {
  unsigned u[4];
  philox4x32_10((unsigned)t, (unsigned)((unsigned long long)t >> 32), (unsigned)(draw >> 2), (unsigned)site, k0, k1, u);
  const double s = 2.3283064365386963e-10;   // 2^-32
  const int h = (draw >> 1) & 1;
  const double u1 = ((double)(h ? u[2] : u[0]) + 0.5) * s, u2 = ((double)(h ? u[3] : u[1]) + 0.5) * s;
  const double r = sqrt(-2.0 * log(u1)), a = 6.283185307179586 * u2;
  return (draw & 1) ? r * sin(a) : r * cos(a);
}

// LDS of the three scan kernels: the sizes of fb_lds_doubles (two matrices, 5 S vectors, FB_CHK staged steps)
//   prior:  A | Lq | m0 | m1 | z0 | z1 | h | yc[FB_CHK] | msc[FB_CHK][S]

// prior scan: x*_0 = Lp z_0, x*_t = A x*_{t-1} + Lq z_t; replay writes x* and d = y - (H x* + sqrt(R) e)
template <bool OFFSET>
__global__ void __launch_bounds__(256) fbs_prior_kernel(FbsPar fp) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int tid = threadIdx.x, NT = blockDim.x, S = fp.S;
  const bool mg = fp.mat_global != 0;
  const double* At = mg ? fp.A : lds;
  const double* Bt = mg ? fp.B : lds + (size_t)S * S;
  double* m0 = lds + (mg ? 0 : 2 * (size_t)S * S);
  double* m1 = m0 + S;
  double* z0 = m1 + S;
  double* z1 = z0 + S;
  double* hh = z1 + S;
  double* yc = hh + S;                    // [FB_CHK]
  double* msc = yc + FB_CHK;              // [FB_CHK][S]
  const int bd = blockIdx.y, draw = fp.draw0 + bd;
  const unsigned k0s = (unsigned)fp.seed, k1s = (unsigned)(fp.seed >> 32);
  const int64_t ka = (int64_t)blockIdx.x * fp.L, kb = (ka + fp.L < fp.T) ? ka + fp.L : fp.T;
  if (!mg) for (int e = tid; e < S * S; e += NT) { lds[e] = fp.A[e]; lds[(size_t)S * S + e] = fp.B[e]; }
  for (int i = tid; i < S; i += NT) {
    hh[i] = fp.H[i];
    m0[i] = (!OFFSET && fp.starts) ? fp.starts[((size_t)bd * fp.ns + blockIdx.x) * S + i] : 0.0;
  }
  double* xs = fp.xs + (size_t)bd * fp.T * S;
  double* dd = fp.d + (size_t)bd * fp.T;
  __syncthreads();
  double* mc = m0;
  double* mn = m1;
  for (int64_t kq = ka; kq < kb; kq += FB_CHK) {
    const int nb = (kb - kq < FB_CHK) ? (int)(kb - kq) : FB_CHK;
    double zr[FB_CHK];
#pragma unroll
    for (int kk = 0; kk < FB_CHK; ++kk) zr[kk] = (tid < S && kk < nb) ? fbs_normal(kq + kk, draw, tid, k0s, k1s) : 0.0;
    if (tid < S) z0[tid] = zr[0];
    if (!OFFSET) for (int i = tid; i < nb; i += NT) yc[i] = fp.y[kq + i];
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < FB_CHK; ++kk) {
      if (kk < nb) {                                   // uniform over the block
        const double* zc = (kk & 1) ? z1 : z0;         // z of step kk; the other slot takes the next step's
        if (tid < S) {
          double a0 = 0.0, a1 = 0.0;
          if (kq + kk == 0) {                 // x*_0 = Lp z_0
            for (int j = 0; j < S; ++j) a0 = fma(fp.Lp[(size_t)j * S + tid], zc[j], a0);
          } else {
            int j = 0;
            for (; j + 2 <= S; j += 2) {
              a0 = fma(At[(size_t)j * S + tid], mc[j], a0); a1 = fma(At[(size_t)(j + 1) * S + tid], mc[j + 1], a1);
              a0 = fma(Bt[(size_t)j * S + tid], zc[j], a0); a1 = fma(Bt[(size_t)(j + 1) * S + tid], zc[j + 1], a1);
            }
            if (j < S) { a0 = fma(At[(size_t)j * S + tid], mc[j], a0); a0 = fma(Bt[(size_t)j * S + tid], zc[j], a0); }
          }
          const double mi = a0 + a1;
          mn[tid] = mi;
          if (!OFFSET) msc[(size_t)kk * S + tid] = mi;
          if (kk + 1 < FB_CHK) ((kk & 1) ? z0 : z1)[tid] = zr[(kk + 1 < FB_CHK) ? kk + 1 : kk];
        }
        lds_barrier();
        double* t_ = mc; mc = mn; mn = t_;
      }
    }
    if (!OFFSET) {
      for (int e = tid; e < nb * S; e += NT) xs[(size_t)kq * S + e] = msc[e];
      if (tid < nb) {                        // d_t = y_t - (H x*_t + sqrt(R) e_t); NaN stays NaN
        const double* xr = msc + (size_t)tid * S;
        double h0 = 0.0;
        for (int j = 0; j < S; ++j) h0 = fma(hh[j], xr[j], h0);
        const double yk = yc[tid];
        const double ys = h0 + fp.sqrtR * fbs_normal(kq + tid, draw, S, k0s, k1s);
        dd[kq + tid] = (yk != yk) ? yk : yk - ys;
      }
    }
    __syncthreads();
  }
  if (OFFSET) for (int i = tid; i < S; i += NT) fp.c[((size_t)bd * fp.ns + blockIdx.x) * S + i] = mc[i];
}

// filter of draw blockIdx.y on d:  if ~isnan(d): m = AKHA*m + K*d; else m = A*m   (fastfb_filter_kernel without the innovations)
template <bool OFFSET>
__global__ void __launch_bounds__(256) fbs_filter_kernel(FbsPar fp) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int tid = threadIdx.x, NT = blockDim.x, S = fp.S;
  const bool mg = fp.mat_global != 0;
  const double* At = mg ? fp.A : lds;
  const double* Bt = mg ? fp.B : lds + (size_t)S * S;
  double* kg = lds + (mg ? 0 : 2 * (size_t)S * S);
  double* m0 = kg + S;
  double* m1 = m0 + S;
  double* yc = m1 + S;                    // [FB_CHK]
  double* msc = yc + FB_CHK;              // [FB_CHK][S]
  const int bd = blockIdx.y;
  const int64_t ka = (int64_t)blockIdx.x * fp.L, kb = (ka + fp.L < fp.T) ? ka + fp.L : fp.T;
  if (!mg) for (int e = tid; e < S * S; e += NT) { lds[e] = fp.A[e]; lds[(size_t)S * S + e] = fp.B[e]; }
  for (int i = tid; i < S; i += NT) {
    kg[i] = fp.K[i];
    m0[i] = (!OFFSET && fp.starts) ? fp.starts[((size_t)bd * fp.ns + blockIdx.x) * S + i] : 0.0;
  }
  const double* dd = fp.d + (size_t)bd * fp.T;
  double* ms = fp.ms + (size_t)bd * fp.T * S;
  __syncthreads();
  double* mc = m0;
  double* mn = m1;
  for (int64_t kq = ka; kq < kb; kq += FB_CHK) {
    const int nb = (kb - kq < FB_CHK) ? (int)(kb - kq) : FB_CHK;
    for (int i = tid; i < nb; i += NT) yc[i] = dd[kq + i];
    __syncthreads();
    for (int kk = 0; kk < nb; ++kk) {
      const double yk = yc[kk];
      const bool obs = !(yk != yk);
      if (tid < S) {
        const double* Mt = obs ? Bt : At;
        double a0 = 0.0, a1 = 0.0;
        int j = 0;
        for (; j + 2 <= S; j += 2) { a0 = fma(Mt[(size_t)j * S + tid], mc[j], a0); a1 = fma(Mt[(size_t)(j + 1) * S + tid], mc[j + 1], a1); }
        if (j < S) a0 = fma(Mt[(size_t)j * S + tid], mc[j], a0);
        double mi = a0 + a1;
        if (obs) mi = mi + kg[tid] * yk;
        mn[tid] = mi;
        if (!OFFSET) msc[(size_t)kk * S + tid] = mi;
      }
      lds_barrier();
      double* t_ = mc; mc = mn; mn = t_;
    }
    if (!OFFSET) for (int e = tid; e < nb * S; e += NT) ms[(size_t)kq * S + e] = msc[e];
    __syncthreads();
  }
  if (OFFSET) for (int i = tid; i < S; i += NT) fp.c[((size_t)bd * fp.ns + blockIdx.x) * S + i] = mc[i];
}

// smoother of draw blockIdx.y:  m = MS_k + G*(m - A*MS_k), k descending inside span j of the n = T-1 smoothing steps.
// The replay adds x*_k and takes the product with H: X goes to xs when the caller wants states, H X to yd.
template <bool OFFSET>
__global__ void __launch_bounds__(256) fbs_smoother_kernel(FbsPar fp) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int tid = threadIdx.x, NT = blockDim.x, S = fp.S;
  const bool mg = fp.mat_global != 0;
  const double* At = mg ? fp.A : lds;
  const double* Gt = mg ? fp.B : lds + (size_t)S * S;
  double* hh = lds + (mg ? 0 : 2 * (size_t)S * S);
  double* m = hh + S;                     // [S] current smoothed mean
  double* dv = m + S;                     // [S] m - A*MS_k
  double* msc = dv + S;                   // [FB_CHK][S]
  const int bd = blockIdx.y;
  const int64_t n = fp.T - 1;
  const int64_t ka = (int64_t)blockIdx.x * fp.L, kb = (ka + fp.L < n) ? ka + fp.L : n;   // steps ka .. kb-1
  const double* ms = fp.ms + (size_t)bd * fp.T * S;
  double* xs = fp.xs + (size_t)bd * fp.T * S;
  double* yd = fp.yd + (size_t)bd * fp.T;
  if (!mg) for (int e = tid; e < S * S; e += NT) { lds[e] = fp.A[e]; lds[(size_t)S * S + e] = fp.B[e]; }
  for (int i = tid; i < S; i += NT) {
    hh[i] = fp.H[i];
    m[i] = OFFSET ? 0.0 : (fp.starts ? fp.starts[((size_t)bd * fp.ns + blockIdx.x) * S + i] : ms[(size_t)(fp.T - 1) * S + i]);
  }
  __syncthreads();
  for (int64_t k1 = kb; k1 > ka; k1 -= FB_CHK) {            // steps k1-1 ... k1-nb, descending
    const int nb = (k1 - ka < FB_CHK) ? (int)(k1 - ka) : FB_CHK;
    const int64_t kl = k1 - nb;
    for (int e = tid; e < nb * S; e += NT) msc[e] = ms[(size_t)kl * S + e];
    __syncthreads();
    for (int kk = nb - 1; kk >= 0; --kk) {
      const double* mk = msc + (size_t)kk * S;
      if (tid < S) {
        double a0 = 0.0, a1 = 0.0;
        int j = 0;
        for (; j + 2 <= S; j += 2) { a0 = fma(At[(size_t)j * S + tid], mk[j], a0); a1 = fma(At[(size_t)(j + 1) * S + tid], mk[j + 1], a1); }
        if (j < S) a0 = fma(At[(size_t)j * S + tid], mk[j], a0);
        dv[tid] = m[tid] - (a0 + a1);
      }
      lds_barrier();
      double mi = 0.0;
      if (tid < S) {
        double g0 = 0.0, g1 = 0.0;
        int j = 0;
        for (; j + 2 <= S; j += 2) { g0 = fma(Gt[(size_t)j * S + tid], dv[j], g0); g1 = fma(Gt[(size_t)(j + 1) * S + tid], dv[j + 1], g1); }
        if (j < S) g0 = fma(Gt[(size_t)j * S + tid], dv[j], g0);
        mi = mk[tid] + (g0 + g1);
      }
      lds_barrier();     // all reads of m / mk of this step are done
      if (tid < S) { m[tid] = mi; msc[(size_t)kk * S + tid] = mi; }
      lds_barrier();
    }
    if (!OFFSET) {
      for (int e = tid; e < nb * S; e += NT) {
        const double x = msc[e] + xs[(size_t)kl * S + e];
        msc[e] = x;
        if (fp.want_x) xs[(size_t)kl * S + e] = x;
      }
      __syncthreads();
      if (tid < nb) {
        const double* xr = msc + (size_t)tid * S;
        double h0 = 0.0;
        for (int j = 0; j < S; ++j) h0 = fma(hh[j], xr[j], h0);
        yd[kl + tid] = h0;
      }
    }
    __syncthreads();
  }
  if (OFFSET) for (int i = tid; i < S; i += NT) fp.c[((size_t)bd * fp.ns + blockIdx.x) * S + i] = m[i];
}

// boundary values of draw blockIdx.x.  Forward (prior, filter): s_0 = 0, s_{j+1} = Phi_j s_j + c_j.
// Backward (smoother): s_{ns-1} = MS_{T-1}, s_{j-1} = Phi_j s_j + c_j.
template <bool BACKWARD>
__global__ void __launch_bounds__(256) fbs_boundary_kernel(FbsPar fp) {
  __shared__ double sv[256];
  const int tid = threadIdx.x, S = fp.S, SP = S + 4, bd = blockIdx.x;
  if (tid < S) sv[tid] = BACKWARD ? fp.ms[((size_t)bd * fp.T + (fp.T - 1)) * S + tid] : 0.0;
  __syncthreads();
  const double* cc = fp.c + (size_t)bd * fp.ns * S;
  double* st = fp.starts + (size_t)bd * fp.ns * S;
  for (int q = 0; q < fp.ns; ++q) {
    const int j = BACKWARD ? (fp.ns - 1 - q) : q;
    if (tid < S) st[(size_t)j * S + tid] = sv[tid];
    if (q + 1 == fp.ns) break;                       // the last value leaves the scan: not needed
    double nv = 0.0;
    if (tid < S) {
      const double* ph = ((j == fp.ns - 1) ? fp.PhiLast : fp.Phi + (size_t)j * fp.phi_stride) + (size_t)tid * SP;
      double a0 = 0.0, a1 = 0.0;
      int l = 0;
      for (; l + 2 <= S; l += 2) { a0 = fma(ph[l], sv[l], a0); a1 = fma(ph[l + 1], sv[l + 1], a1); }
      if (l < S) a0 = fma(ph[l], sv[l], a0);
      nv = (a0 + a1) + cc[(size_t)j * S + tid];
    }
    __syncthreads();
    if (tid < S) sv[tid] = nv;
    __syncthreads();
  }
}

// the last step has no smoothing step: X_{T-1} = MS_{T-1} + x*_{T-1}
template <bool WANT_X>
__global__ void __launch_bounds__(256) fbs_last_kernel(FbsPar fp) {
  __shared__ double xv[256];
  const int tid = threadIdx.x, S = fp.S, bd = blockIdx.x;
  const size_t o = ((size_t)bd * fp.T + (fp.T - 1)) * S;
  if (tid < S) {
    const double x = fp.ms[o + tid] + fp.xs[o + tid];
    xv[tid] = x;
    if (WANT_X) fp.xs[o + tid] = x;
  }
  __syncthreads();
  if (tid == 0) {
    double h0 = 0.0;
    for (int j = 0; j < S; ++j) h0 = fma(fp.H[j], xv[j], h0);
    fp.yd[(size_t)bd * fp.T + (fp.T - 1)] = h0;
  }
}

}  // namespace nagp

#define NAGP_LIST_FBSAMPLE(P)                                                                                              \
  P void nagp::fbs_prior_kernel<false>(nagp::FbsPar); P void nagp::fbs_prior_kernel<true>(nagp::FbsPar);                   \
  P void nagp::fbs_filter_kernel<false>(nagp::FbsPar); P void nagp::fbs_filter_kernel<true>(nagp::FbsPar);                 \
  P void nagp::fbs_smoother_kernel<false>(nagp::FbsPar); P void nagp::fbs_smoother_kernel<true>(nagp::FbsPar);             \
  P void nagp::fbs_boundary_kernel<false>(nagp::FbsPar); P void nagp::fbs_boundary_kernel<true>(nagp::FbsPar);             \
  P void nagp::fbs_last_kernel<false>(nagp::FbsPar); P void nagp::fbs_last_kernel<true>(nagp::FbsPar);
