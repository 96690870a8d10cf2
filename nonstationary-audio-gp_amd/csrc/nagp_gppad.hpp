// Objective and gradient of the GPPAD envelope inference, experiments/gppad/GPModelFast/GetGPObjFast.m (driven by MAPGPFast.m and
// InferAmplitudeGPMAP.m), FP64, a batch of independent problems (one channel at one resolution each).  See include/nagp.h
// (nagp_gppad_obj) for the boundary and DESIGN.md for the reasoning.
//
// With a = GetAmp(x_t), s = 1/(1+exp(-x_t)), v_t = a^2 varc + (vary_t + 1e-5) for t < T, xe = x - mux (length Tx), c = fftCov:
//     ObjA = sum_t 1/2 log v_t + 1/2 y_t^2 / v_t,          dA_t = s a / v_t (1 - y_t^2 / v_t) varc,
//     u = real(ifft(fft(xe) ./ c)),  ObjB = (u' xe) / (2 varx),  dObj = u / varx (+ dA on the first T entries),  Obj = ObjA + ObjB.
//
// The transform is a complex Stockham FFT on the whole sequence (imaginary part zero: two problems are never packed into one transform),
// radix 4 with one leading radix-2 pass when log2 of the length is odd, ping-pong between two LDS buffers, twiddles from a table of
// Tx entries exp(-2 pi i m / Tx) built on the host in extended precision (the inverse conjugates them).  ic = 1 / (c Tx) is resident, so
// the inverse needs no normalisation (Tx is a power of two: the factor is exact).
//   Tx <= 4096 (N1 = 1):  gppad_lds_kernel, grid (problems): load, forward, times ic, inverse, the per-sample pass.
//   Tx >= 8192:           Tx = N1 x 4096 (four-step, N2 = 4096), n = n1 N2 + n2, k = k1 + N1 k2:
//     gppad_colf_kernel   grid (N1, problems): a tile of CB = 4096 / N1 adjacent columns n2, forward transforms of length N1 along n1, times
//                         exp(-2 pi i n2 k1 / Tx), stored to work[k1][n2];
//     gppad_row_kernel    grid (N1, problems): row k1: forward of length N2 along n2 -> k2, times ic (held in this permuted order, position
//                         k1 N2 + k2 for frequency k1 + N1 k2: no transposition anywhere), inverse along k2 -> n2, times the conjugate
//                         twiddle, stored in place;
//     gppad_coli_kernel   grid (N1, problems): the column tile again, inverse transforms along k1 -> n1, then the per-sample pass.
// The per-sample pass (gp_point) owns u_n: it adds u_n xe_n to the ObjB sum, the likelihood term to the ObjA sum for n < T, and writes
// dObj_n.  A thread adds its samples in ascending order, a wave is reduced by a fixed xor butterfly, the waves are added in wave
// order, the workgroup writes its two partial sums to part[problem][workgroup][2] and gppad_finish_kernel adds the workgroups in ascending order.
// Thread count, tile and split are functions of Tx alone; no atomics: a problem's bits depend neither on its batch mates nor on how the
// call was split into device batches, and a call without the gradient runs the same instructions but for the store of dObj.
//
// Every kernel body is a __host__ __device__ function of (workgroup, thread, thread count): a host program can run the bodies with one
// "thread" per workgroup (barriers and the butterfly fall away) to check the index arithmetic without a device.
// LDS index i is stored at i + (i >> 4): the first radix-4 pass stores with a stride of four 16 B slots, a 4-way conflict for a 16 B store
// (groups of 8 lanes over 32 banks); the extra slot per 256 B makes it 2-way (DESIGN.md says why no more was done).
#pragma once
#include "nagp_dev.hpp"

namespace nagp {

constexpr int GPPAD_LOG_TILE = 12;                 // a workgroup transforms at most 4096 complex points: 2 x 4352 x 16 B = 136 KiB of LDS
constexpr int GPPAD_TILE = 1 << GPPAD_LOG_TILE;
constexpr int GPPAD_MAX_NT = 512;
constexpr int GPPAD_LOG_MAX = 20;                  // Tx <= 2^20

struct GppadPar {
  int64_t T, Tx;
  int N1, N2;              // Tx = N1 x N2; N1 = 1: the whole sequence in one workgroup
  int lcb;                 // log2 of the columns of a column tile (four-step)
  int grad;                // 1: dObj is written
  int nwg;                 // workgroups of the per-sample pass per problem
  const double* x;         // problems x Tx
  const double* y;         // problems x T
  const double* vary;      // problems (vary_stride = 0) or problems x T
  int64_t vary_stride;
  const double* ic;        // Tx (ic_stride = 0) or problems x Tx: 1 / (c Tx) in the order the forward transform leaves
  int64_t ic_stride;
  const double* varx; const double* mux; const double* varc;     // problems each
  const double2* tw;       // Tx: exp(-2 pi i m / Tx)
  double2* work;           // problems x Tx (four-step)
  double* part;            // problems x nwg x 2
  double* Obj;             // problems
  double* dObj;            // problems x Tx
  const double* len;       // problems (gppad_cov_kernel)
  double* ic_out;          // problems x Tx (gppad_cov_kernel)
  // the cascade form (V = 1, see below): a "problem" is column m of cascade prob / M
  int M;                   // columns of a cascade
  int nwgA;                // workgroups of the pre-pass per cascade
  double* D;               // cascades x T: D_t = 1 - y_t^2 / (varc P_t^2) (written by the pre-pass, read by the per-sample pass)
  double* partA;           // cascades x nwgA x 2: the pre-pass's sums of log A and of 1/2 (y / P)^2
};

__host__ __device__ inline int gp_pad(int i) { return i + (i >> 4); }
__host__ __device__ inline int gppad_points(int64_t Tx) { return Tx < GPPAD_TILE ? (int)Tx : GPPAD_TILE; }
__host__ __device__ inline int gppad_threads(int64_t Tx) {
  const int q = gppad_points(Tx) / 4;
  return q < 64 ? 64 : (q > GPPAD_MAX_NT ? GPPAD_MAX_NT : q);
}
// the two buffers, then the 16 doubles of the wave sums (all of it dynamic: a kernel whose dynamic limit is raised to 160 KiB may hold no static LDS)
__host__ __device__ inline size_t gppad_lds_points(int64_t Tx) { return 2 * (size_t)(gp_pad(gppad_points(Tx) - 1) + 1); }
__host__ __device__ inline size_t gppad_lds_bytes(int64_t Tx) { return gppad_lds_points(Tx) * sizeof(double2) + 16 * sizeof(double); }

__host__ __device__ inline void gp_sync() {
#if defined(__HIP_DEVICE_COMPILE__)
  __syncthreads();
#endif
}

__host__ __device__ inline double2 gp_cmul(double2 a, double2 b) { return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
template <int DIR>
__host__ __device__ inline double2 gp_tw(const double2* tw, int64_t m) { const double2 w = tw[m]; return DIR > 0 ? w : make_double2(w.x, -w.y); }

// one item of a Stockham pass of radix R over 2^lcb interleaved sequences of n points each (point i of sequence c at i 2^lcb + c):
// item w owns butterfly j = w >> lcb of sequence c; Ns: the product of the radices of the passes before; tws = Tx / n
template <int DIR, int R>
__host__ __device__ inline void gp_pass(const double2* src, double2* dst, int n, int lcb, int Ns, int w, const double2* tw, int64_t tws) {
  const int c = w & ((1 << lcb) - 1), j = w >> lcb, k = j & (Ns - 1);
  if (R == 2) {
    const int h = n >> 1;
    const double2 a = src[gp_pad((j << lcb) + c)];
    double2 b = src[gp_pad(((j + h) << lcb) + c)];
    if (Ns > 1) b = gp_cmul(b, gp_tw<DIR>(tw, (int64_t)k * (h / Ns) * tws));
    const int j0 = ((j - k) << 1) + k;
    dst[gp_pad((j0 << lcb) + c)] = make_double2(a.x + b.x, a.y + b.y);
    dst[gp_pad(((j0 + Ns) << lcb) + c)] = make_double2(a.x - b.x, a.y - b.y);
  } else {
    const int q = n >> 2;
    const double2 a0 = src[gp_pad((j << lcb) + c)];
    double2 a1 = src[gp_pad(((j + q) << lcb) + c)], a2 = src[gp_pad(((j + 2 * q) << lcb) + c)], a3 = src[gp_pad(((j + 3 * q) << lcb) + c)];
    if (Ns > 1) {
      const int64_t m = (int64_t)k * (q / Ns) * tws;            // 3 m < Tx
      a1 = gp_cmul(a1, gp_tw<DIR>(tw, m)); a2 = gp_cmul(a2, gp_tw<DIR>(tw, 2 * m)); a3 = gp_cmul(a3, gp_tw<DIR>(tw, 3 * m));
    }
    const double2 t0 = make_double2(a0.x + a2.x, a0.y + a2.y), t1 = make_double2(a0.x - a2.x, a0.y - a2.y);
    const double2 t2 = make_double2(a1.x + a3.x, a1.y + a3.y), t3 = make_double2(a1.x - a3.x, a1.y - a3.y);
    const double2 m3 = DIR > 0 ? make_double2(t3.y, -t3.x) : make_double2(-t3.y, t3.x);      // -i t3 (forward), +i t3 (inverse)
    const int j0 = ((j - k) << 2) + k;
    dst[gp_pad((j0 << lcb) + c)] = make_double2(t0.x + t2.x, t0.y + t2.y);
    dst[gp_pad(((j0 + Ns) << lcb) + c)] = make_double2(t1.x + m3.x, t1.y + m3.y);
    dst[gp_pad(((j0 + 2 * Ns) << lcb) + c)] = make_double2(t0.x - t2.x, t0.y - t2.y);
    dst[gp_pad(((j0 + 3 * Ns) << lcb) + c)] = make_double2(t1.x - m3.x, t1.y - m3.y);
  }
}

// all passes of the transforms of length n = 2^ln; the result is in `src` afterwards (the two pointers are swapped after every pass).
// Entered with the input complete in src (a barrier behind the loads), left with a barrier behind the last pass.
template <int DIR>
__host__ __device__ inline void gp_fft(double2*& src, double2*& dst, int ln, int lcb, const double2* tw, int64_t tws, int tid, int nt) {
  const int n = 1 << ln;
  int Ns = 1;
  if (ln & 1) {
    for (int w = tid; w < ((n >> 1) << lcb); w += nt) gp_pass<DIR, 2>(src, dst, n, lcb, Ns, w, tw, tws);
    gp_sync();
    double2* t = src; src = dst; dst = t; Ns = 2;
  }
  while (Ns < n) {
    for (int w = tid; w < ((n >> 2) << lcb); w += nt) gp_pass<DIR, 4>(src, dst, n, lcb, Ns, w, tw, tws);
    gp_sync();
    double2* t = src; src = dst; dst = t; Ns <<= 2;
  }
}

__host__ __device__ inline int gp_log2(int64_t n) { int l = 0; while (((int64_t)1 << l) < n) ++l; return l; }

// the three branches of GetAmp.m and the logistic next to it
__host__ __device__ inline void gp_amp(double x, double& a, double& s) {
  a = x > 500.0 ? x : (x < -30.0 ? exp(x) : log(1.0 + exp(x)));
  s = 1.0 / (1.0 + exp(-x));
}

struct GpScal { double varx, mux, varc; };

// sample n of problem prob with u_n = real(ifft(fft(xe) ./ c))_n: the two sums and dObj_n
__host__ __device__ inline void gp_point(const GppadPar& p, int prob, const GpScal& sc, int64_t n, double u, double& oa, double& ob) {
  const size_t ix = (size_t)prob * (size_t)p.Tx + (size_t)n;
  const double x = p.x[ix];
  ob += u * (x - sc.mux);
  double g = u / sc.varx;
  if (n < p.T) {
    double a, s;
    gp_amp(x, a, s);
    const double vy = p.vary[p.vary_stride ? (size_t)prob * (size_t)p.T + (size_t)n : (size_t)prob];
    const double y = p.y[(size_t)prob * (size_t)p.T + (size_t)n];
    const double v = a * a * sc.varc + (vy + 1e-5);
    const double r = y * y / v;
    oa += 0.5 * log(v) + 0.5 * r;
    g += s * a / v * (1.0 - r) * sc.varc;
  }
  if (p.grad) p.dObj[ix] = g;
}

// sample n of column prob of a cascade (V = 1) with u_n as above and D_n from the pre-pass: the ObjB sum and dObj_n
__host__ __device__ inline void gp_point_cas(const GppadPar& p, int prob, const GpScal& sc, int64_t n, double u, double& ob) {
  const size_t ix = (size_t)prob * (size_t)p.Tx + (size_t)n;
  const double x = p.x[ix];
  ob += u * (x - sc.mux);
  double g = u / sc.varx;
  if (n < p.T) {
    double a, s;
    gp_amp(x, a, s);
    g += s / a * p.D[(size_t)(prob / p.M) * (size_t)p.T + (size_t)n];
  }
  if (p.grad) p.dObj[ix] = g;
}

// the workgroup's two sums to out[2]: xor butterfly in a wave, waves in wave order (red: 2 x 8 doubles of LDS)
__host__ __device__ inline void gp_block_sums_to(double* out, double oa, double ob, double* red, int tid, int nt) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) { oa += __shfl_xor(oa, m); ob += __shfl_xor(ob, m); }
  if ((tid & 63) == 0) { red[2 * (tid >> 6)] = oa; red[2 * (tid >> 6) + 1] = ob; }
  __syncthreads();
  if (tid < 2) {
    double s = 0.0;
    for (int w = 0; w < (nt >> 6); ++w) s += red[2 * w + tid];
    out[tid] = s;
  }
#else
  (void)red; (void)tid; (void)nt;
  out[0] = oa; out[1] = ob;
#endif
}
__host__ __device__ inline void gp_block_sums(const GppadPar& p, int prob, int blk, double oa, double ob, double* red, int tid, int nt) {
  gp_block_sums_to(p.part + ((size_t)prob * p.nwg + blk) * 2, oa, ob, red, tid, nt);
}

// V = 0: GetGPObjFast.m, one problem per transform.  V = 1: the cascade (GetObjCasGPFAST.m, header below): varx, mux, 1 / c per column,
// varc per cascade (read by the pre-pass and the finish only)
template <int V>
__host__ __device__ inline GpScal gp_scalars(const GppadPar& p, int prob) { return GpScal{p.varx[prob], p.mux[prob], V ? 0.0 : p.varc[prob]}; }
// 1 / (c Tx) of a problem; a spectrum shared by the cascades (ic_stride = 0) is M x Tx
template <int V>
__host__ __device__ inline const double* gp_ic(const GppadPar& p, int prob) {
  return p.ic + (V && !p.ic_stride ? (size_t)(prob % p.M) * (size_t)p.Tx : (size_t)prob * (size_t)p.ic_stride);
}
template <int V>
__host__ __device__ inline void gp_sample(const GppadPar& p, int prob, const GpScal& sc, int64_t n, double u, double& oa, double& ob) {
  if (V) gp_point_cas(p, prob, sc, n, u, ob); else gp_point(p, prob, sc, n, u, oa, ob);
}

// Tx <= 4096: one workgroup per problem
template <int V = 0>
__host__ __device__ inline void gppad_lds_body(const GppadPar& p, int prob, int tid, int nt, double2* lds, double* red) {
  const int n = (int)p.Tx, ln = gp_log2(n);
  double2* src = lds; double2* dst = lds + gp_pad(n - 1) + 1;
  const GpScal sc = gp_scalars<V>(p, prob);
  const double* x = p.x + (size_t)prob * (size_t)p.Tx;
  for (int e = tid; e < n; e += nt) src[gp_pad(e)] = make_double2(x[e] - sc.mux, 0.0);
  gp_sync();
  gp_fft<1>(src, dst, ln, 0, p.tw, 1, tid, nt);
  const double* ic = gp_ic<V>(p, prob);
  for (int e = tid; e < n; e += nt) { const double f = ic[e]; double2 v = src[gp_pad(e)]; v.x *= f; v.y *= f; src[gp_pad(e)] = v; }
  gp_sync();
  gp_fft<-1>(src, dst, ln, 0, p.tw, 1, tid, nt);
  double oa = 0.0, ob = 0.0;
  for (int e = tid; e < n; e += nt) gp_sample<V>(p, prob, sc, e, src[gp_pad(e)].x, oa, ob);
  gp_block_sums(p, prob, 0, oa, ob, red, tid, nt);
}

// four-step, first kernel: column tile blk, forward along n1, twiddle, store to work[k1][n2]
__host__ __device__ inline void gppad_colf_body(const GppadPar& p, int prob, int blk, int tid, int nt, double2* lds) {
  const int lcb = p.lcb, cb = 1 << lcb, pts = p.N1 << lcb, c0 = blk << lcb, ln = gp_log2(p.N1);
  double2* src = lds; double2* dst = lds + gp_pad(pts - 1) + 1;
  const double mux = p.mux[prob];
  const double* x = p.x + (size_t)prob * (size_t)p.Tx;
  for (int e = tid; e < pts; e += nt) {
    const int64_t n = (int64_t)(e >> lcb) * p.N2 + c0 + (e & (cb - 1));
    src[gp_pad(e)] = make_double2(x[n] - mux, 0.0);
  }
  gp_sync();
  gp_fft<1>(src, dst, ln, lcb, p.tw, p.N2, tid, nt);
  double2* work = p.work + (size_t)prob * (size_t)p.Tx;
  for (int e = tid; e < pts; e += nt) {
    const int k1 = e >> lcb, n2 = c0 + (e & (cb - 1));
    work[(int64_t)k1 * p.N2 + n2] = gp_cmul(src[gp_pad(e)], gp_tw<1>(p.tw, (int64_t)n2 * k1));
  }
}

// four-step, second kernel: row k1 = blk, forward along n2, times ic, inverse, conjugate twiddle, in place
template <int V = 0>
__host__ __device__ inline void gppad_row_body(const GppadPar& p, int prob, int blk, int tid, int nt, double2* lds) {
  const int n = p.N2, ln = gp_log2(n);
  double2* src = lds; double2* dst = lds + gp_pad(n - 1) + 1;
  double2* row = p.work + (size_t)prob * (size_t)p.Tx + (size_t)blk * (size_t)n;
  for (int e = tid; e < n; e += nt) src[gp_pad(e)] = row[e];
  gp_sync();
  gp_fft<1>(src, dst, ln, 0, p.tw, p.N1, tid, nt);
  const double* ic = gp_ic<V>(p, prob) + (size_t)blk * (size_t)n;
  for (int e = tid; e < n; e += nt) { const double f = ic[e]; double2 v = src[gp_pad(e)]; v.x *= f; v.y *= f; src[gp_pad(e)] = v; }
  gp_sync();
  gp_fft<-1>(src, dst, ln, 0, p.tw, p.N1, tid, nt);
  for (int e = tid; e < n; e += nt) row[e] = gp_cmul(src[gp_pad(e)], gp_tw<-1>(p.tw, (int64_t)e * blk));
}

// four-step, third kernel: column tile blk, inverse along k1, the per-sample pass
template <int V = 0>
__host__ __device__ inline void gppad_coli_body(const GppadPar& p, int prob, int blk, int tid, int nt, double2* lds, double* red) {
  const int lcb = p.lcb, cb = 1 << lcb, pts = p.N1 << lcb, c0 = blk << lcb, ln = gp_log2(p.N1);
  double2* src = lds; double2* dst = lds + gp_pad(pts - 1) + 1;
  const GpScal sc = gp_scalars<V>(p, prob);
  const double2* work = p.work + (size_t)prob * (size_t)p.Tx;
  for (int e = tid; e < pts; e += nt) src[gp_pad(e)] = work[(int64_t)(e >> lcb) * p.N2 + c0 + (e & (cb - 1))];
  gp_sync();
  gp_fft<-1>(src, dst, ln, lcb, p.tw, p.N2, tid, nt);
  double oa = 0.0, ob = 0.0;
  for (int e = tid; e < pts; e += nt) {
    const int64_t n = (int64_t)(e >> lcb) * p.N2 + c0 + (e & (cb - 1));
    gp_sample<V>(p, prob, sc, n, src[gp_pad(e)].x, oa, ob);
  }
  gp_block_sums(p, prob, blk, oa, ob, red, tid, nt);
}

// frequency held at position q of the transform's output: k1 + N1 k2 for q = k1 N2 + k2
__host__ __device__ inline int64_t gppad_freq_at(int64_t q, int N1, int N2) { return q / N2 + (int64_t)N1 * (q % N2); }

// ic = 1 / (c Tx) of GetFFTCovFast.m:10-16 from len, in position order
__host__ __device__ inline void gppad_cov_item(const GppadPar& p, int prob, int64_t q) {
  const int64_t k = gppad_freq_at(q, p.N1, p.N2), f = k <= p.Tx / 2 ? k : k - p.Tx;      // [0:floor(Tx/2), -floor(Tx/2)+1:-1]
  const double len = p.len[prob], Txd = (double)p.Tx;
  const double omega = 2.0 * 3.14159265358979323846 * (double)f / Txd;
  const double c = sqrt(2.0 * 3.14159265358979323846 * len * len) * exp(-(omega * omega) * (len * len) / 2.0) + 1e-6;
  p.ic_out[(size_t)prob * (size_t)p.Tx + (size_t)q] = (1.0 / c) * (1.0 / Txd);
}

__host__ __device__ inline void gppad_finish_item(const GppadPar& p, int prob) {
  const double* pp = p.part + (size_t)prob * p.nwg * 2;
  double sa = 0.0, sb = 0.0;
  for (int w = 0; w < p.nwg; ++w) { sa += pp[2 * w]; sb += pp[2 * w + 1]; }
  p.Obj[prob] = sa + 1.0 / (2.0 * p.varx[prob]) * sb;
}

// ---- the cascade, Cascade/GetObjCasGPFAST.m:19-50: X (Tx x M, column m = "problem" cas M + m of the kernels above), one y and one varc,
// per column a spectrum, varx and mux:
//     A_tm = amp(X_tm) (t < T),  P_t = prod_m A_tm (m ascending),  ObjA = sum_t sum_m log A_tm + (sum_t 1/2 (y_t / P_t)^2) / varc,
//     D_t = 1 - y_t^2 / (varc P_t^2),  u_m = real(ifft(fft(X_:m - mux_m) ./ c_m)),  ObjB = sum_m (u_m' (X_:m - mux_m)) / (2 varx_m),
//     dObj_tm = u_tm / varx_m + (t < T ? s_tm / A_tm D_t : 0),  Obj = ObjA + ObjB      (no vary, no 1/2 log v, no 1e-5 in this objective).
// amp is gp_amp: wherever the .m's plain log(1 + exp(x)) is finite it equals it to rounding, and it stays finite beyond (x up to 700 and
// past it: a = x); entries outside +-700 give Inf or NaN (A = 0 below -745: log A = -Inf, s / A = 0 / 0) as the .m does, never a fault.
//   gppad_cas_pre_kernel     grid (ceil(T / 256), cascades), 256 threads, one per sample: the M amp calls, the product, D_t to the
//                            workspace, the workgroup's sums of sum_m log A_tm and of 1/2 (y_t / P_t)^2 to partA;
//   the transform kernels    in their V = 1 instantiation on cascades x M "problems" (the forward column kernel and the spectrum kernel do
//                            not differ: V = 0 serves): the per-sample pass of a column is one amp, D_t and u (gp_point_cas), ObjA's slot of part is 0;
//   gppad_cas_finish_kernel  one thread per cascade: the pre-pass's workgroups in ascending order, / varc, then the columns in ascending order,
//                            each the sum of its workgroups in ascending order / (2 varx_m).  No atomics.
// The bits of a cascade are a function of (M, T, Tx) and its own data.
constexpr int GPPAD_CAS_NT = 256;
constexpr int GPPAD_CAS_MAX_M = 8;
__host__ __device__ inline int gppad_cas_nwg(int64_t T) { return (int)((T + GPPAD_CAS_NT - 1) / GPPAD_CAS_NT); }

__host__ __device__ inline void gppad_cas_pre_body(const GppadPar& p, int cas, int blk, int tid, int nt, double* red) {
  const int64_t t0 = (int64_t)blk * GPPAD_CAS_NT, t1 = t0 + GPPAD_CAS_NT < p.T ? t0 + GPPAD_CAS_NT : p.T;
  const double* x = p.x + (size_t)cas * (size_t)p.M * (size_t)p.Tx;
  const double varc = p.varc[cas];
  double ol = 0.0, oq = 0.0;
  for (int64_t t = t0 + tid; t < t1; t += nt) {
    double P = 1.0, l = 0.0;
    for (int m = 0; m < p.M; ++m) {
      double a, s;
      gp_amp(x[(size_t)m * (size_t)p.Tx + (size_t)t], a, s);
      l += log(a); P *= a;
    }
    const double y = p.y[(size_t)cas * (size_t)p.T + (size_t)t], r = y / P;
    ol += l; oq += 0.5 * (r * r);
    p.D[(size_t)cas * (size_t)p.T + (size_t)t] = 1.0 - y * y / (varc * (P * P));
  }
  gp_block_sums_to(p.partA + ((size_t)cas * p.nwgA + blk) * 2, ol, oq, red, tid, nt);
}

__host__ __device__ inline void gppad_cas_finish_item(const GppadPar& p, int cas) {
  const double* pa = p.partA + (size_t)cas * p.nwgA * 2;
  double sl = 0.0, sq = 0.0;
  for (int w = 0; w < p.nwgA; ++w) { sl += pa[2 * w]; sq += pa[2 * w + 1]; }
  double ob = 0.0;
  for (int m = 0; m < p.M; ++m) {
    const size_t q = (size_t)cas * p.M + m;
    const double* pp = p.part + q * p.nwg * 2;
    double sb = 0.0;
    for (int w = 0; w < p.nwg; ++w) sb += pp[2 * w + 1];
    ob += sb / (2.0 * p.varx[q]);
  }
  p.Obj[cas] = (sl + sq / p.varc[cas]) + ob;
}

// (templates so that the instantiations live in inst_gppad.hip and inst_gppad_cas.hip)
template <int V> __global__ void __launch_bounds__(GPPAD_MAX_NT) gppad_lds_kernel(GppadPar p) {
  extern __shared__ double2 gp_lds[];
  gppad_lds_body<V>(p, blockIdx.x, threadIdx.x, blockDim.x, gp_lds, reinterpret_cast<double*>(gp_lds + gppad_lds_points(p.Tx)));
}
template <int V> __global__ void __launch_bounds__(GPPAD_MAX_NT) gppad_colf_kernel(GppadPar p) {
  extern __shared__ double2 gp_lds[];
  gppad_colf_body(p, blockIdx.y, blockIdx.x, threadIdx.x, blockDim.x, gp_lds);
}
template <int V> __global__ void __launch_bounds__(GPPAD_MAX_NT) gppad_row_kernel(GppadPar p) {
  extern __shared__ double2 gp_lds[];
  gppad_row_body<V>(p, blockIdx.y, blockIdx.x, threadIdx.x, blockDim.x, gp_lds);
}
template <int V> __global__ void __launch_bounds__(GPPAD_MAX_NT) gppad_coli_kernel(GppadPar p) {
  extern __shared__ double2 gp_lds[];
  gppad_coli_body<V>(p, blockIdx.y, blockIdx.x, threadIdx.x, blockDim.x, gp_lds, reinterpret_cast<double*>(gp_lds + gppad_lds_points(p.Tx)));
}
template <int V> __global__ void __launch_bounds__(256) gppad_cov_kernel(GppadPar p) {
  const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (q < p.Tx) gppad_cov_item(p, blockIdx.y, q);
}
template <int V> __global__ void __launch_bounds__(64) gppad_finish_kernel(GppadPar p, int n) {
  const int prob = blockIdx.x * 64 + threadIdx.x;
  if (prob < n) gppad_finish_item(p, prob);
}

template <int V> __global__ void __launch_bounds__(GPPAD_CAS_NT) gppad_cas_pre_kernel(GppadPar p) {
  __shared__ double red[16];
  gppad_cas_pre_body(p, blockIdx.y, blockIdx.x, threadIdx.x, blockDim.x, red);
}
template <int V> __global__ void __launch_bounds__(64) gppad_cas_finish_kernel(GppadPar p, int n) {
  const int cas = blockIdx.x * 64 + threadIdx.x;
  if (cas < n) gppad_cas_finish_item(p, cas);
}

}  // namespace nagp

#define NAGP_LIST_GPPAD(X) X void nagp::gppad_lds_kernel<0>(nagp::GppadPar); X void nagp::gppad_colf_kernel<0>(nagp::GppadPar); \
  X void nagp::gppad_row_kernel<0>(nagp::GppadPar); X void nagp::gppad_coli_kernel<0>(nagp::GppadPar); \
  X void nagp::gppad_cov_kernel<0>(nagp::GppadPar); X void nagp::gppad_finish_kernel<0>(nagp::GppadPar, int);
#define NAGP_LIST_GPPAD_CAS(X) X void nagp::gppad_lds_kernel<1>(nagp::GppadPar); X void nagp::gppad_row_kernel<1>(nagp::GppadPar); \
  X void nagp::gppad_coli_kernel<1>(nagp::GppadPar); X void nagp::gppad_cas_pre_kernel<1>(nagp::GppadPar); \
  X void nagp::gppad_cas_finish_kernel<1>(nagp::GppadPar, int);
