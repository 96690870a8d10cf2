// The Laplace step of GPPAD, experiments/gppad/GPModelFast/Laplace (GetHessian.m, SigDSigTimesV.m, LanczosGPPAD.m, GetErrorBarGPPAD.m,
// GetLaplaceObjGPPADOneChunk.m), FP64, a device batch of independent problems in lock-step.  See include/nagp.h (nagp_gppad_lap_create)
// for the boundary and DESIGN.md for the reasoning.  The transforms, the twiddle table, the LDS layout and the block sums are those of
// nagp_gppad.hpp; the forward column kernel and the row kernel of the four-step form are its V = 0 instantiations, run on a vector with
// mux = 0 and the spectrum g in the place of 1 / (c Tx).
//
//   g = sqrt(c varx) / Tx in the transform's position order (lap_spec_kernel), d the per-sample Hessian of the likelihood (lap_hess_kernel).
//   A "sandwich" is u = real(ifft(g Tx .* fft(v))) (the 1 / Tx of the inverse sits in g); the operator A = Sigma^1/2 D Sigma^1/2 of
//   SigDSigTimesV.m is two of them with an epilogue each (E):
//     E = 0  out_n = u_n                                              (the second half of nagp_gppad_lap_apply)
//     E = 1  out_n = d_n u_n for n < T, 0 beyond                      (the first half)
//     E = 2  r_n = u_n - beta_j v_{j-1,n} (j > 0), the workgroup's partial of r . v_j          (the Lanczos residual)
//     E = 3  Varx_n -= u_n^2 lambda / (lambda + 1)                    (GetErrorBarGPPAD.m, one launch per Ritz vector, k ascending)
//   Tx <= 4096: lap_lds_kernel<E>, grid (problems).  Tx >= 8192: gppad_colf_kernel<0>, gppad_row_kernel<0>, lap_coli_kernel<E>, grid (N1, problems).
//   The vectors are real: the imaginary rounding noise that the .m carries along (and drops with real(lmb)) is dropped after every sandwich.
//
// Every vector of a device batch of nb problems lies slot-major, slot s of problem q at (s nb + q) Tx: a slot of all problems is one
// contiguous (nb x Tx) block the transform kernels take as their input, and a thread that walks the basis reads coalesced.
// A problem is masked by flag[q] < lev (E = 3: by a NaN lambda): its workgroups return before they touch its state.  Sums: a thread adds
// its samples in ascending order, gp_block_sums_to adds the wave and the waves in a fixed order, lap_finish_kernel adds the workgroups in
// ascending order.  No atomics; thread counts and tiles are functions of Tx alone: a problem's bits depend neither on its batch mates
// nor on the cut into device batches.
#pragma once
#include "nagp_gppad.hpp"

namespace nagp {

constexpr int LAP_NT = 256;          // threads, and samples per workgroup, of the per-sample kernels
constexpr int LAP_KT = 4;            // Ritz vectors per thread of lap_ritz_kernel

struct LapPar {
  int64_t T, Tx;
  int N1, N2, lcb;
  int nb;                  // problems of the device batch: the stride between slots is nb Tx
  int j;                   // E = 2: the step (0: no v_{j-1}); lap_update: < 0 = no subtraction; lap_h1 / lap_sub: the basis vectors
  int jmax;                // row stride of h1 (2 jmax per problem) and of S (jmax x jmax per problem)
  int np;                  // lap_finish: the partial sums per problem
  int root;                // lap_finish: 1 = the square root of the sum
  int ss;                  // lap_update: the stride of sc
  double lev;              // a problem takes part when flag >= lev
  int64_t vary_stride;
  const double* flag;      // nb
  const double* g;         // nb x Tx
  const double2* tw;
  double2* work;           // nb x Tx (four-step)
  const double* in;        // nb x Tx
  double* out;             // nb x Tx
  double* va;              // nb x Tx: v_j
  const double* vb;        // nb x Tx: v_{j-1}
  const double* q;         // the basis, slot-major
  const double* d;         // nb x T
  const double* sc;        // nb: beta_j (E = 2), lambda_k (E = 3), alpha (lap_update), the divisor (lap_scale), the steps (lap_ritz)
  const double* h1;        // nb x jmax x 2
  const double* S;         // nb x jmax x jmax
  double* part;            // nb x np x 2
  double* res;             // nb (lap_finish), nb x jmax x 2 (lap_h1), nb x 3 (lap_obj)
  const double* x; const double* y; const double* vary; const double* len;
  const double* varx; const double* varc;
};

__host__ __device__ inline int lap_nwe(int64_t Tx) { return (int)((Tx + LAP_NT - 1) / LAP_NT); }

template <int E>
__host__ __device__ inline bool lap_on(const LapPar& p, int prob) {
  if (E == 3) { const double l = p.sc[prob]; return l == l; }
  return p.flag[prob] >= p.lev;
}

// g = sqrt(c varx) / Tx of GetHessian.m's h = GetFFTCovFast(len, Tx) varx, in position order
__host__ __device__ inline void lap_spec_item(const LapPar& p, int prob, int64_t q) {
  const int64_t k = gppad_freq_at(q, p.N1, p.N2), f = k <= p.Tx / 2 ? k : k - p.Tx;
  const double len = p.len[prob], Txd = (double)p.Tx;
  const double omega = 2.0 * 3.14159265358979323846 * (double)f / Txd;
  const double c = sqrt(2.0 * 3.14159265358979323846 * len * len) * exp(-(omega * omega) * (len * len) / 2.0) + 1e-6;
  p.out[(size_t)prob * (size_t)p.Tx + (size_t)q] = sqrt(c * p.varx[prob]) * (1.0 / Txd);
}

// d_t of GetHessian.m:28-40, the three branches of GetAmp as gp_amp has them
__host__ __device__ inline void lap_hess_item(const LapPar& p, int prob, int64_t t) {
  const double x = p.x[(size_t)prob * (size_t)p.Tx + (size_t)t];
  double a, s;
  gp_amp(x, a, s);
  const double ch = cosh(x / 2.0), c2 = 0.25 / (ch * ch);
  const size_t it = (size_t)prob * (size_t)p.T + (size_t)t;
  const double vy = p.vary[p.vary_stride ? it : (size_t)prob] + 1e-5, y = p.y[it], varc = p.varc[prob];
  const double v = a * a * varc + vy, dv = 2.0 * varc * a * s, yy = y * y, w = 1.0 - yy / v;
  p.out[it] = (c2 * a + s * s) / v * w * varc - s * a / (v * v) * w * varc * dv + s * a / v * yy / (v * v) * varc * dv;
}

// sample n of problem prob behind a sandwich
template <int E>
__host__ __device__ inline void lap_point(const LapPar& p, int prob, int64_t n, double u, double& acc) {
  const size_t ix = (size_t)prob * (size_t)p.Tx + (size_t)n;
  if (E == 0) p.out[ix] = u;
  if (E == 1) p.out[ix] = n < p.T ? p.d[(size_t)prob * (size_t)p.T + (size_t)n] * u : 0.0;
  if (E == 2) {
    double r = u;
    if (p.j > 0) r -= p.vb[ix] * p.sc[prob];
    p.out[ix] = r;
    acc += r * p.va[ix];
  }
  if (E == 3) { const double l = p.sc[prob]; p.out[ix] -= u * u * l / (l + 1.0); }
}

// Tx <= 4096: one workgroup per problem
template <int E>
__host__ __device__ inline void lap_lds_body(const LapPar& p, int prob, int tid, int nt, double2* lds, double* red) {
  if (!lap_on<E>(p, prob)) return;
  const int n = (int)p.Tx, ln = gp_log2(n);
  double2* src = lds; double2* dst = lds + gp_pad(n - 1) + 1;
  const double* v = p.in + (size_t)prob * (size_t)p.Tx;
  for (int e = tid; e < n; e += nt) src[gp_pad(e)] = make_double2(v[e], 0.0);
  gp_sync();
  gp_fft<1>(src, dst, ln, 0, p.tw, 1, tid, nt);
  const double* g = p.g + (size_t)prob * (size_t)p.Tx;
  for (int e = tid; e < n; e += nt) { const double f = g[e]; double2 w = src[gp_pad(e)]; w.x *= f; w.y *= f; src[gp_pad(e)] = w; }
  gp_sync();
  gp_fft<-1>(src, dst, ln, 0, p.tw, 1, tid, nt);
  double acc = 0.0;
  for (int e = tid; e < n; e += nt) lap_point<E>(p, prob, e, src[gp_pad(e)].x, acc);
  if (E == 2) gp_block_sums_to(p.part + (size_t)prob * 2, acc, 0.0, red, tid, nt);
}

// four-step, third kernel: column tile blk, inverse along k1, the epilogue (gppad_coli_body with lap_point)
template <int E>
__host__ __device__ inline void lap_coli_body(const LapPar& p, int prob, int blk, int tid, int nt, double2* lds, double* red) {
  if (!lap_on<E>(p, prob)) return;
  const int lcb = p.lcb, cb = 1 << lcb, pts = p.N1 << lcb, c0 = blk << lcb, ln = gp_log2(p.N1);
  double2* src = lds; double2* dst = lds + gp_pad(pts - 1) + 1;
  const double2* work = p.work + (size_t)prob * (size_t)p.Tx;
  for (int e = tid; e < pts; e += nt) src[gp_pad(e)] = work[(int64_t)(e >> lcb) * p.N2 + c0 + (e & (cb - 1))];
  gp_sync();
  gp_fft<-1>(src, dst, ln, lcb, p.tw, p.N2, tid, nt);
  double acc = 0.0;
  for (int e = tid; e < pts; e += nt) {
    const int64_t n = (int64_t)(e >> lcb) * p.N2 + c0 + (e & (cb - 1));
    lap_point<E>(p, prob, n, src[gp_pad(e)].x, acc);
  }
  if (E == 2) gp_block_sums_to(p.part + ((size_t)prob * p.N1 + blk) * 2, acc, 0.0, red, tid, nt);
}

// r -= alpha v_j (j >= 0) and the workgroup's partial of |r|^2; workgroup blk owns samples [blk LAP_NT, (blk + 1) LAP_NT)
__host__ __device__ inline void lap_update_body(const LapPar& p, int prob, int blk, int tid, int nt, double* red) {
  if (p.flag[prob] < p.lev) return;
  const int64_t n0 = (int64_t)blk * LAP_NT, n1 = n0 + LAP_NT < p.Tx ? n0 + LAP_NT : p.Tx;
  double acc = 0.0;
  for (int64_t n = n0 + tid; n < n1; n += nt) {
    const size_t ix = (size_t)prob * (size_t)p.Tx + (size_t)n;
    double r = p.out[ix];
    if (p.j >= 0) { r -= p.va[ix] * p.sc[(size_t)prob * p.ss]; p.out[ix] = r; }
    acc += r * r;
  }
  gp_block_sums_to(p.part + ((size_t)prob * p.np + blk) * 2, acc, 0.0, red, tid, nt);
}

// the workgroups' partial sums in ascending order (root: the square root of the sum)
__host__ __device__ inline void lap_finish_item(const LapPar& p, int prob) {
  if (p.flag[prob] < p.lev) return;
  const double* pp = p.part + (size_t)prob * p.np * 2;
  double s = 0.0;
  for (int w = 0; w < p.np; ++w) s += pp[2 * w];
  p.res[prob] = p.root ? sqrt(s) : s;
}

// out = in / sc: v_j = r / beta_j
__host__ __device__ inline void lap_scale_item(const LapPar& p, int prob, int64_t n) {
  if (p.flag[prob] < p.lev) return;
  const size_t ix = (size_t)prob * (size_t)p.Tx + (size_t)n;
  p.out[ix] = p.in[ix] / p.sc[prob];
}

// h1 = Q' [v_j r]: workgroup (i, prob), the two dot products of basis vector i in a fixed order
__host__ __device__ inline void lap_h1_body(const LapPar& p, int prob, int i, int tid, int nt, double* red) {
  if (p.flag[prob] < p.lev) return;
  const size_t ix = (size_t)prob * (size_t)p.Tx;
  const double* q = p.q + ((size_t)i * p.nb + prob) * (size_t)p.Tx;
  double a = 0.0, b = 0.0;
  for (int64_t n = tid; n < p.Tx; n += nt) { const double qq = q[n]; a += qq * p.va[ix + n]; b += qq * p.in[ix + n]; }
  gp_block_sums_to(p.res + ((size_t)prob * p.jmax + i) * 2, a, b, red, tid, nt);
}

// [v_j r] -= Q h1, one thread per sample, the basis vectors in ascending order
__host__ __device__ inline void lap_sub_item(const LapPar& p, int prob, int64_t n) {
  if (p.flag[prob] < p.lev) return;
  const size_t ix = (size_t)prob * (size_t)p.Tx + (size_t)n;
  const double* h = p.h1 + (size_t)prob * p.jmax * 2;
  double a = p.va[ix], b = p.out[ix];
  for (int i = 0; i < p.j; ++i) {
    const double qq = p.q[((size_t)i * p.nb + prob) * (size_t)p.Tx + (size_t)n];
    a -= qq * h[2 * i]; b -= qq * h[2 * i + 1];
  }
  p.va[ix] = a; p.out[ix] = b;
}

// xv = V s: thread (n, tile of LAP_KT Ritz vectors), the basis vectors in ascending order; flag = the Ritz vectors, sc = the steps of the problem
__host__ __device__ inline void lap_ritz_item(const LapPar& p, int prob, int kt, int64_t n) {
  const int K = (int)p.flag[prob], js = (int)p.sc[prob], k0 = kt * LAP_KT;
  if (k0 >= K) return;
  const double* S = p.S + (size_t)prob * p.jmax * p.jmax;
  double acc[LAP_KT];
  for (int c = 0; c < LAP_KT; ++c) acc[c] = 0.0;
  for (int i = 0; i < js; ++i) {
    const double v = p.q[((size_t)i * p.nb + prob) * (size_t)p.Tx + (size_t)n];
    for (int c = 0; c < LAP_KT; ++c) acc[c] += v * (k0 + c < K ? S[(size_t)i * p.jmax + k0 + c] : 0.0);
  }
  for (int c = 0; c < LAP_KT; ++c)
    if (k0 + c < K) p.out[((size_t)(k0 + c) * p.nb + prob) * (size_t)p.Tx + (size_t)n] = acc[c];
}

// Obj1 = -sum_t (1/2 log v + 1/2 y^2 / v), Obj2 = -(u' xe) / (2 varx) from the partial sums the kernels of nagp_gppad.hpp leave (gp: their part, nwg per problem)
__host__ __device__ inline void lap_obj_item(const LapPar& p, int prob) {
  const double* pp = p.part + (size_t)prob * p.np * 2;
  double sa = 0.0, sb = 0.0;
  for (int w = 0; w < p.np; ++w) { sa += pp[2 * w]; sb += pp[2 * w + 1]; }
  p.res[(size_t)prob * 3 + 1] = -sa;
  p.res[(size_t)prob * 3 + 2] = -(1.0 / (2.0 * p.varx[prob]) * sb);
}

template <int E> __global__ void __launch_bounds__(GPPAD_MAX_NT) lap_lds_kernel(LapPar p) {
  extern __shared__ double2 gp_lds[];
  lap_lds_body<E>(p, blockIdx.x, threadIdx.x, blockDim.x, gp_lds, reinterpret_cast<double*>(gp_lds + gppad_lds_points(p.Tx)));
}
template <int E> __global__ void __launch_bounds__(GPPAD_MAX_NT) lap_coli_kernel(LapPar p) {
  extern __shared__ double2 gp_lds[];
  lap_coli_body<E>(p, blockIdx.y, blockIdx.x, threadIdx.x, blockDim.x, gp_lds, reinterpret_cast<double*>(gp_lds + gppad_lds_points(p.Tx)));
}
// W: 0 spectrum, 1 Hessian, 2 scale, 3 [v_j r] -= Q h1 -- one thread per sample, grid (ceil(n / LAP_NT), problems)
template <int W> __global__ void __launch_bounds__(LAP_NT) lap_sample_kernel(LapPar p) {
  const int64_t n = (int64_t)blockIdx.x * LAP_NT + threadIdx.x;
  if (n >= (W == 1 ? p.T : p.Tx)) return;
  if (W == 0) lap_spec_item(p, blockIdx.y, n);
  if (W == 1) lap_hess_item(p, blockIdx.y, n);
  if (W == 2) lap_scale_item(p, blockIdx.y, n);
  if (W == 3) lap_sub_item(p, blockIdx.y, n);
}
template <int W> __global__ void __launch_bounds__(LAP_NT) lap_update_kernel(LapPar p) {
  __shared__ double red[16];
  lap_update_body(p, blockIdx.y, blockIdx.x, threadIdx.x, blockDim.x, red);
}
template <int W> __global__ void __launch_bounds__(LAP_NT) lap_h1_kernel(LapPar p) {
  __shared__ double red[16];
  lap_h1_body(p, blockIdx.y, blockIdx.x, threadIdx.x, blockDim.x, red);
}
template <int W> __global__ void __launch_bounds__(LAP_NT) lap_ritz_kernel(LapPar p) {
  const int64_t n = (int64_t)blockIdx.x * LAP_NT + threadIdx.x;
  if (n < p.Tx) lap_ritz_item(p, blockIdx.z, blockIdx.y, n);
}
// W: 0 lap_finish_item, 1 lap_obj_item -- one thread per problem
template <int W> __global__ void __launch_bounds__(64) lap_finish_kernel(LapPar p, int n) {
  const int prob = blockIdx.x * 64 + threadIdx.x;
  if (prob >= n) return;
  if (W == 0) lap_finish_item(p, prob); else lap_obj_item(p, prob);
}

}  // namespace nagp

#define NAGP_LIST_GPPAD_LAP(X) X void nagp::lap_lds_kernel<0>(nagp::LapPar); X void nagp::lap_lds_kernel<1>(nagp::LapPar); \
  X void nagp::lap_lds_kernel<2>(nagp::LapPar); X void nagp::lap_lds_kernel<3>(nagp::LapPar); \
  X void nagp::lap_coli_kernel<0>(nagp::LapPar); X void nagp::lap_coli_kernel<1>(nagp::LapPar); \
  X void nagp::lap_coli_kernel<2>(nagp::LapPar); X void nagp::lap_coli_kernel<3>(nagp::LapPar); \
  X void nagp::lap_sample_kernel<0>(nagp::LapPar); X void nagp::lap_sample_kernel<1>(nagp::LapPar); \
  X void nagp::lap_sample_kernel<2>(nagp::LapPar); X void nagp::lap_sample_kernel<3>(nagp::LapPar); \
  X void nagp::lap_update_kernel<0>(nagp::LapPar); X void nagp::lap_h1_kernel<0>(nagp::LapPar); X void nagp::lap_ritz_kernel<0>(nagp::LapPar); \
  X void nagp::lap_finish_kernel<0>(nagp::LapPar, int); X void nagp::lap_finish_kernel<1>(nagp::LapPar, int);
