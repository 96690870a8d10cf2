// nagp_recon.hpp -- what the drivers do with the outputs of the hot path (matlab/demo_toy_modulators_nmf.m:119-158):
// the reconstructed signal  sig = sum_d (W link(g))_d z_d  and the modulator amplitudes link(g_n) under the INDEPENDENT posterior
// marginals z_d ~ N(Eft_d, Varft_d), g_n ~ N(Eft_{D+n}, Varft_{D+n}) of one time step:
//   Eft_mod = mean link(g_n), Varft_mod = var link(g_n), Esig = mean sig, Vsig = var sig.
// Embarrassingly parallel over t.  Two forms:
//   moments   the population values of those means / variances: one-dimensional Gauss-Hermite quadrature of link and link^2 per
//             modulator (exp link: closed form), then
//               Esig = sum_d a_d m_d,  a = W mu_lk
//               Vsig = sum_d a_d^2 v_d + sum_n var_lk,n [ (sum_d W_dn m_d)^2 + sum_d W_dn^2 v_d ]
//   sampling  the reference's own estimator (s = 250 draws per marginal, :123, sample variance with s-1), draws from a
//             counter-based generator (Philox4x32-10, key = seed, counter = (t, sample block, site)) + Box-Muller, so that a host
//             restatement reproduces them.  One wave per time step, four samples per lane and trip.
#pragma once
#include "nagp_dev.hpp"

namespace nagp {

struct ReconPar {
  int D, N, M;
  int64_t T;
  int link_kind; double link_shift;
  const double* W;       // [D][N] row-major
  const double* Eft;     // [T][M]
  const double* Varft;   // [T][M]
  int n_gh; const double* gh_x; const double* gh_w;   // moments form (standard-normal weight)
  int n_samp; unsigned long long seed;                 // sampling form
  double* Esig; double* Vsig;                          // [T]
  double* Emod; double* Vmod;                          // [T][N]
};

// (the generator -- philox4x32_10, normal4 -- is in nagp_dev.hpp: the joint draws of nagp_fbsample.hpp use the same one)

// moments form: one thread per time step
__global__ void __launch_bounds__(256) recon_moments_kernel(ReconPar rp) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  double* sW = lds;                       // [D][N]
  double* gx = sW + rp.D * rp.N;          // [n_gh]
  double* gw = gx + rp.n_gh;
  for (int i = threadIdx.x; i < rp.D * rp.N; i += blockDim.x) sW[i] = rp.W[i];
  for (int i = threadIdx.x; i < rp.n_gh; i += blockDim.x) { gx[i] = rp.gh_x[i]; gw[i] = rp.gh_w[i]; }
  __syncthreads();
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= rp.T) return;
  const int D = rp.D, N = rp.N, M = rp.M;
  const double* m = rp.Eft + (size_t)t * M;
  const double* v = rp.Varft + (size_t)t * M;
  double vs = 0.0, es = 0.0;
  double mu[MOM_MAXCD], va[MOM_MAXCD];
  for (int n = 0; n < N; ++n) {
    const double mg = m[D + n], vg = v[D + n];
    double e1, e2;
    if (rp.link_kind == 1) {              // exp link: E exp(g) = exp(m + v/2), E exp(2g) = exp(2m + 2v)
      e1 = exp(mg + 0.5 * vg); e2 = exp(2.0 * mg + 2.0 * vg);
    } else {
      const double sg = sqrt(vg);
      e1 = 0.0; e2 = 0.0;
      for (int q = 0; q < rp.n_gh; ++q) {
        const double l = link_eval(0, rp.link_shift, mg + sg * gx[q]);
        e1 = fma(gw[q], l, e1); e2 = fma(gw[q] * l, l, e2);
      }
    }
    mu[n] = e1; va[n] = e2 - e1 * e1;
    rp.Emod[(size_t)t * N + n] = e1; rp.Vmod[(size_t)t * N + n] = va[n];
  }
  for (int d = 0; d < D; ++d) {
    double a = 0.0;
    for (int n = 0; n < N; ++n) a = fma(sW[d * N + n], mu[n], a);
    es = fma(a, m[d], es);
    vs = fma(a * a, v[d], vs);
  }
  for (int n = 0; n < N; ++n) {
    double wm = 0.0, wv = 0.0;
    for (int d = 0; d < D; ++d) { const double w = sW[d * N + n]; wm = fma(w, m[d], wm); wv = fma(w * w, v[d], wv); }
    vs = fma(va[n], fma(wm, wm, wv), vs);
  }
  rp.Esig[t] = es; rp.Vsig[t] = vs;
}

// sampling form: one wave per time step
__global__ void __launch_bounds__(64) recon_sample_kernel(ReconPar rp) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  double* sW = lds;
  for (int i = threadIdx.x; i < rp.D * rp.N; i += 64) sW[i] = rp.W[i];
  __syncthreads();
  const int lane = threadIdx.x, D = rp.D, N = rp.N, M = rp.M, S = rp.n_samp;
  const unsigned k0 = (unsigned)rp.seed, k1 = (unsigned)(rp.seed >> 32);
  for (int64_t t = blockIdx.x; t < rp.T; t += gridDim.x) {
    const double* m = rp.Eft + (size_t)t * M;
    const double* v = rp.Varft + (size_t)t * M;
    // sums of (x - c) and (x - c)^2 with the shift c = value at the marginal mean (keeps the variance formula well conditioned)
    double cl[MOM_MAXCD], s1[MOM_MAXCD], s2[MOM_MAXCD];
    for (int n = 0; n < N; ++n) { cl[n] = link_eval(rp.link_kind, rp.link_shift, m[D + n]); s1[n] = 0.0; s2[n] = 0.0; }
    double csig = 0.0;
    for (int d = 0; d < D; ++d) { double a = 0.0; for (int n = 0; n < N; ++n) a = fma(sW[d * N + n], cl[n], a); csig = fma(a, m[d], csig); }
    double g1 = 0.0, g2 = 0.0;
    for (int q0 = 0; q0 * 4 < S; q0 += 64) {
      const int q = q0 + lane;                       // sample block: samples 4q .. 4q+3
      double lk[MOM_MAXCD][4], sig[4] = {0, 0, 0, 0};
      for (int n = 0; n < N; ++n) {
        double z[4];
        normal4((unsigned)t, (unsigned)((unsigned long long)t >> 32), (unsigned)q, (unsigned)(D + n), k0, k1, z);
        const double sg = sqrt(v[D + n]);
#pragma unroll
        for (int e = 0; e < 4; ++e) lk[n][e] = link_eval(rp.link_kind, rp.link_shift, fma(sg, z[e], m[D + n]));
      }
      for (int d = 0; d < D; ++d) {
        double z[4];
        normal4((unsigned)t, (unsigned)((unsigned long long)t >> 32), (unsigned)q, (unsigned)d, k0, k1, z);
        const double sd = sqrt(v[d]);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          double a = 0.0;
          for (int n = 0; n < N; ++n) a = fma(sW[d * N + n], lk[n][e], a);
          sig[e] = fma(a, fma(sd, z[e], m[d]), sig[e]);
        }
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if (4 * q + e < S) {
          for (int n = 0; n < N; ++n) { const double x = lk[n][e] - cl[n]; s1[n] += x; s2[n] = fma(x, x, s2[n]); }
          const double x = sig[e] - csig; g1 += x; g2 = fma(x, x, g2);
        }
      }
    }
    g1 = wave_sum(g1); g2 = wave_sum(g2);
    for (int n = 0; n < N; ++n) { s1[n] = wave_sum(s1[n]); s2[n] = wave_sum(s2[n]); }
    if (lane == 0) {
      const double inv = 1.0 / S, inv1 = 1.0 / (S - 1);
      rp.Esig[t] = csig + g1 * inv; rp.Vsig[t] = (g2 - g1 * g1 * inv) * inv1;
      for (int n = 0; n < N; ++n) { rp.Emod[(size_t)t * N + n] = cl[n] + s1[n] * inv; rp.Vmod[(size_t)t * N + n] = (s2[n] - s1[n] * s1[n] * inv) * inv1; }
    }
  }
}

// ---------------------------------------------------------------------------------------------
// The post-processing as the experiment scripts write it (nagp_reconstruct_sources; experiments/source_sep_piano.m:165-244,
// noise_reduction_speech.m:142): amplitude a_d = W_d.lk or sqrt(W_d.lk), J sources = contiguous ranges of sub-bands, envelopes.
//   sig = sum_d a_d z_d,  sig_j = sum_{d in j} a_d z_d,  env_d = a_d
// The kernels keep W in the LDS with rows padded to MOM_MAXCD (zeros), so that the per-modulator register arrays are indexed by
// unrolled loops only; the sources are walked in order (an outer loop unrolled over RECON_MAXSRC), a sub-band's source being the
// range of the LDS offset table that holds it.
constexpr int RECON_MAXSRC = 8;

struct ReconSrcPar {
  int D, N, M, J;
  int64_t T;
  int amp_sqrt, link_kind; double link_shift;
  const double* W;       // [D][N] row-major
  const double* Eft;     // [T][M]
  const double* Varft;   // [T][M]
  const int* off;        // [J+1]
  int n_gh; const double* gh_x; const double* gh_w;   // 1-D rule (population forms)
  int n_pts; const double* wn; const double* xn;      // N-dimensional rule, xn [n_pts][N] (population form of the sqrt kind)
  int n_samp; unsigned long long seed;                // sampling form
  double* Esig; double* Vsig;                          // [T]
  double* Esrc; double* Vsrc;                          // [T][J]
  double* Eenv;                                        // [T][D]
  double* Emod; double* Vmod;                          // [T][N]
};

// W -> LDS rows of MOM_MAXCD entries (zero beyond N), the source offsets -> LDS (entries beyond J repeat D: empty ranges)
__device__ __forceinline__ void recon_src_stage(const ReconSrcPar& rp, double* sW, int* soff, int nthreads) {
  for (int i = threadIdx.x; i < rp.D * MOM_MAXCD; i += nthreads) { const int d = i / MOM_MAXCD, n = i - d * MOM_MAXCD; sW[i] = n < rp.N ? rp.W[d * rp.N + n] : 0.0; }
  for (int i = threadIdx.x; i <= RECON_MAXSRC; i += nthreads) soff[i] = i <= rp.J ? rp.off[i] : rp.D;
}
__device__ __forceinline__ double recon_amp(int amp_sqrt, double a) { return amp_sqrt ? sqrt(a) : a; }   // sqrt of a negative number: NaN

// sampling form: one wave per time step, four samples per lane and trip; the draws of recon_sample_kernel
__global__ void __launch_bounds__(64) recon_src_sample_kernel(ReconSrcPar rp) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  __shared__ int soff[RECON_MAXSRC + 1];
  double* sW = lds;                              // [D][MOM_MAXCD]
  double* senv = sW + rp.D * MOM_MAXCD;          // [D]  sum over the draws of a_d
  double* scl = senv + rp.D;                     // [MOM_MAXCD]  link at the marginal mean
  double* scs = scl + MOM_MAXCD;                 // [RECON_MAXSRC]  sig_j at the marginal means
  recon_src_stage(rp, sW, soff, 64);
  __syncthreads();
  const int lane = threadIdx.x, D = rp.D, N = rp.N, M = rp.M, S = rp.n_samp, J = rp.J, asq = rp.amp_sqrt;
  const unsigned k0 = (unsigned)rp.seed, k1 = (unsigned)(rp.seed >> 32);
  for (int64_t t = blockIdx.x; t < rp.T; t += gridDim.x) {
    const double* m = rp.Eft + (size_t)t * M;
    const double* v = rp.Varft + (size_t)t * M;
    // sums of (x - c) and (x - c)^2 with the shift c = value at the marginal mean (keeps the variance formula well conditioned)
    double cl[MOM_MAXCD], s1[MOM_MAXCD], s2[MOM_MAXCD], r1[RECON_MAXSRC], r2[RECON_MAXSRC];
#pragma unroll
    for (int n = 0; n < MOM_MAXCD; ++n) { cl[n] = n < N ? link_eval(rp.link_kind, rp.link_shift, m[D + n]) : 0.0; s1[n] = 0.0; s2[n] = 0.0; }
    double csig = 0.0;
#pragma unroll
    for (int j = 0; j < RECON_MAXSRC; ++j) {
      r1[j] = 0.0; r2[j] = 0.0;
      if (j < J) {
        double cj = 0.0;
        for (int d = __builtin_amdgcn_readfirstlane(soff[j]), d1 = __builtin_amdgcn_readfirstlane(soff[j + 1]); d < d1; ++d) {
          double a = 0.0;
#pragma unroll
          for (int n = 0; n < MOM_MAXCD; ++n) a = fma(sW[d * MOM_MAXCD + n], cl[n], a);
          a = recon_amp(asq, a);
          cj = fma(a, m[d], cj); csig = fma(a, m[d], csig);
        }
        if (lane == 0) scs[j] = cj;
      }
    }
    if (lane == 0) {
#pragma unroll
      for (int n = 0; n < MOM_MAXCD; ++n) scl[n] = cl[n];
    }
    for (int i = lane; i < D; i += 64) senv[i] = 0.0;
    __syncthreads();
    double g1 = 0.0, g2 = 0.0;
    for (int q0 = 0; q0 * 4 < S; q0 += 64) {
      const int q = q0 + lane;                       // sample block: samples 4q .. 4q+3
      double lk[MOM_MAXCD][4], sig[4] = {0, 0, 0, 0};
#pragma unroll
      for (int n = 0; n < MOM_MAXCD; ++n) {
        if (n < N) {
          double z[4];
          normal4((unsigned)t, (unsigned)((unsigned long long)t >> 32), (unsigned)q, (unsigned)(D + n), k0, k1, z);
          const double sg = sqrt(v[D + n]), c = scl[n];
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            lk[n][e] = link_eval(rp.link_kind, rp.link_shift, fma(sg, z[e], m[D + n]));
            if (4 * q + e < S) { const double x = lk[n][e] - c; s1[n] += x; s2[n] = fma(x, x, s2[n]); }
          }
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) lk[n][e] = 0.0;
        }
      }
#pragma unroll
      for (int j = 0; j < RECON_MAXSRC; ++j) {
        if (j < J) {
          double sj[4] = {0, 0, 0, 0};
          for (int d = __builtin_amdgcn_readfirstlane(soff[j]), d1 = __builtin_amdgcn_readfirstlane(soff[j + 1]); d < d1; ++d) {
            double z[4];
            normal4((unsigned)t, (unsigned)((unsigned long long)t >> 32), (unsigned)q, (unsigned)d, k0, k1, z);
            const double sd = sqrt(v[d]);
            double ea = 0.0;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              double a = 0.0;
#pragma unroll
              for (int n = 0; n < MOM_MAXCD; ++n) a = fma(sW[d * MOM_MAXCD + n], lk[n][e], a);
              a = recon_amp(asq, a);
              const double zd = fma(sd, z[e], m[d]);
              sig[e] = fma(a, zd, sig[e]); sj[e] = fma(a, zd, sj[e]);
              ea += (4 * q + e < S) ? a : 0.0;
            }
            if (rp.Eenv) {                           // the envelope sum of a sub-band is reduced as it is produced
              ea = wave_sum(ea);
              if (lane == 0) senv[d] += ea;
            }
          }
          const double c = scs[j];
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (4 * q + e < S) { const double x = sj[e] - c; r1[j] += x; r2[j] = fma(x, x, r2[j]); }
        }
      }
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (4 * q + e < S) { const double x = sig[e] - csig; g1 += x; g2 = fma(x, x, g2); }
    }
    const double inv = 1.0 / S, inv1 = 1.0 / (S - 1);
    g1 = wave_sum(g1); g2 = wave_sum(g2);
    if (lane == 0) {
      if (rp.Esig) rp.Esig[t] = csig + g1 * inv;
      if (rp.Vsig) rp.Vsig[t] = (g2 - g1 * g1 * inv) * inv1;
    }
#pragma unroll
    for (int n = 0; n < MOM_MAXCD; ++n) {
      if (n < N) {
        const double a = wave_sum(s1[n]), b = wave_sum(s2[n]);
        if (lane == 0) {
          if (rp.Emod) rp.Emod[(size_t)t * N + n] = scl[n] + a * inv;
          if (rp.Vmod) rp.Vmod[(size_t)t * N + n] = (b - a * a * inv) * inv1;
        }
      }
    }
#pragma unroll
    for (int j = 0; j < RECON_MAXSRC; ++j) {
      if (j < J) {
        const double a = wave_sum(r1[j]), b = wave_sum(r2[j]);
        if (lane == 0) {
          if (rp.Esrc) rp.Esrc[(size_t)t * J + j] = scs[j] + a * inv;
          if (rp.Vsrc) rp.Vsrc[(size_t)t * J + j] = (b - a * a * inv) * inv1;
        }
      }
    }
    __syncthreads();
    if (rp.Eenv) for (int i = lane; i < D; i += 64) rp.Eenv[(size_t)t * D + i] = senv[i] * inv;
    __syncthreads();
  }
}

// E link(g), E link(g)^2 of one modulator by the 1-D rule, the points spread over the lanes of the wave (exp link: closed form)
__device__ __forceinline__ void recon_link_moments(const ReconSrcPar& rp, const double* gx, const double* gw, double mg, double vg, double& e1, double& e2) {
  if (rp.link_kind == 1) { e1 = exp(mg + 0.5 * vg); e2 = exp(2.0 * mg + 2.0 * vg); return; }
  const double sg = sqrt(vg);
  e1 = 0.0; e2 = 0.0;
  for (int q = threadIdx.x; q < rp.n_gh; q += 64) {
    const double l = link_eval(0, rp.link_shift, mg + sg * gx[q]);
    e1 = fma(gw[q], l, e1); e2 = fma(gw[q] * l, l, e2);
  }
  e1 = wave_sum(e1); e2 = wave_sum(e2);
}

// population form of the sqrt kind: one wave per time step, lanes over the points of the N-dimensional rule in trips of 64.
//   E a_d = sum_p w_p a_d(g_p),  u_j(g) = sum_{d in j} a_d(g) m_d,  c_j = u_j(m_g),  S1 = sum_p w_p (u_j - c_j),  S2 = sum_p w_p (u_j - c_j)^2
//   E u_j = c_j sw + S1,  E u_j^2 - (E u_j)^2 = S2 - S1^2 + (1 - sw) (c_j^2 sw + 2 c_j S1),  sw = sum_p w_p
// and the total (all sub-bands) as one more "source".  The per-lane envelope sums live in the LDS ([D][65]: conflict-free both ways).
__global__ void __launch_bounds__(64) recon_src_pop_sqrt_kernel(ReconSrcPar rp) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  __shared__ int soff[RECON_MAXSRC + 1];
  double* sW = lds;                              // [D][MOM_MAXCD]
  double* gx = sW + rp.D * MOM_MAXCD;            // [n_gh]
  double* gw = gx + rp.n_gh;
  double* sacc = gw + rp.n_gh;                   // [D][65]
  recon_src_stage(rp, sW, soff, 64);
  for (int i = threadIdx.x; i < rp.n_gh; i += 64) { gx[i] = rp.gh_x[i]; gw[i] = rp.gh_w[i]; }
  __syncthreads();
  const int lane = threadIdx.x, D = rp.D, N = rp.N, M = rp.M, J = rp.J;
  for (int64_t t = blockIdx.x; t < rp.T; t += gridDim.x) {
    const double* m = rp.Eft + (size_t)t * M;
    const double* v = rp.Varft + (size_t)t * M;
    double el[MOM_MAXCD], cl[MOM_MAXCD], mg[MOM_MAXCD], sg[MOM_MAXCD];
#pragma unroll
    for (int n = 0; n < MOM_MAXCD; ++n) {
      el[n] = 0.0; cl[n] = 0.0; mg[n] = 0.0; sg[n] = 0.0;
      if (n < N) {
        double e1, e2;
        mg[n] = m[D + n]; sg[n] = sqrt(v[D + n]);
        recon_link_moments(rp, gx, gw, mg[n], v[D + n], e1, e2);
        el[n] = e1; cl[n] = link_eval(rp.link_kind, rp.link_shift, mg[n]);
        if (lane == 0) {
          if (rp.Emod) rp.Emod[(size_t)t * N + n] = e1;
          if (rp.Vmod) rp.Vmod[(size_t)t * N + n] = e2 - e1 * e1;
        }
      }
    }
    // centre values u_j(m_g), and sum_{d in j} (W_d . E lk) v_d
    double cj[RECON_MAXSRC], vj[RECON_MAXSRC], S1[RECON_MAXSRC], S2[RECON_MAXSRC], ct = 0.0, vt = 0.0, T1 = 0.0, T2 = 0.0, sw = 0.0;
#pragma unroll
    for (int j = 0; j < RECON_MAXSRC; ++j) {
      cj[j] = 0.0; vj[j] = 0.0; S1[j] = 0.0; S2[j] = 0.0;
      if (j < J) {
        for (int d = __builtin_amdgcn_readfirstlane(soff[j]), d1 = __builtin_amdgcn_readfirstlane(soff[j + 1]); d < d1; ++d) {
          double a = 0.0, a2 = 0.0;
#pragma unroll
          for (int n = 0; n < MOM_MAXCD; ++n) { a = fma(sW[d * MOM_MAXCD + n], cl[n], a); a2 = fma(sW[d * MOM_MAXCD + n], el[n], a2); }
          a = sqrt(a);
          cj[j] = fma(a, m[d], cj[j]); ct = fma(a, m[d], ct);
          vj[j] = fma(a2, v[d], vj[j]); vt = fma(a2, v[d], vt);
        }
      }
    }
    for (int d = 0; d < D; ++d) sacc[d * 65 + lane] = 0.0;
    for (int p0 = 0; p0 < rp.n_pts; p0 += 64) {
      const int pt = p0 + lane;
      const bool ok = pt < rp.n_pts;
      const double w = ok ? rp.wn[pt] : 0.0;
      const double* x = rp.xn + (size_t)(ok ? pt : 0) * N;
      double lk[MOM_MAXCD];
#pragma unroll
      for (int n = 0; n < MOM_MAXCD; ++n) lk[n] = n < N ? link_eval(rp.link_kind, rp.link_shift, fma(sg[n], x[n], mg[n])) : 0.0;
      sw += w;
      double ut = 0.0;
#pragma unroll
      for (int j = 0; j < RECON_MAXSRC; ++j) {
        if (j < J) {
          double uj = 0.0;
          for (int d = __builtin_amdgcn_readfirstlane(soff[j]), d1 = __builtin_amdgcn_readfirstlane(soff[j + 1]); d < d1; ++d) {
            double a = 0.0;
#pragma unroll
            for (int n = 0; n < MOM_MAXCD; ++n) a = fma(sW[d * MOM_MAXCD + n], lk[n], a);
            a = sqrt(a);
            if (ok) sacc[d * 65 + lane] = fma(w, a, sacc[d * 65 + lane]);
            uj = fma(a, m[d], uj); ut = fma(a, m[d], ut);
          }
          if (ok) { const double xj = uj - cj[j]; S1[j] = fma(w, xj, S1[j]); S2[j] = fma(w * xj, xj, S2[j]); }
        }
      }
      if (ok) { const double xt = ut - ct; T1 = fma(w, xt, T1); T2 = fma(w * xt, xt, T2); }
    }
    sw = wave_sum(sw); T1 = wave_sum(T1); T2 = wave_sum(T2);
    if (lane == 0) {
      if (rp.Esig) rp.Esig[t] = fma(ct, sw, T1);
      if (rp.Vsig) rp.Vsig[t] = vt + ((T2 - T1 * T1) + (1.0 - sw) * (ct * ct * sw + 2.0 * ct * T1));
    }
#pragma unroll
    for (int j = 0; j < RECON_MAXSRC; ++j) {
      if (j < J) {
        const double a = wave_sum(S1[j]), b = wave_sum(S2[j]);
        if (lane == 0) {
          if (rp.Esrc) rp.Esrc[(size_t)t * J + j] = fma(cj[j], sw, a);
          if (rp.Vsrc) rp.Vsrc[(size_t)t * J + j] = vj[j] + ((b - a * a) + (1.0 - sw) * (cj[j] * cj[j] * sw + 2.0 * cj[j] * a));
        }
      }
    }
    __syncthreads();
    if (rp.Eenv) {
      for (int d = lane; d < D; d += 64) {
        double e = 0.0;
        for (int l = 0; l < 64; ++l) e += sacc[d * 65 + l];
        rp.Eenv[(size_t)t * D + d] = e;
      }
    }
    __syncthreads();
  }
}

// population form of the linear kind: one thread per time step; the closed forms of recon_moments_kernel per source
//   Esig_j = sum_{d in j} a_d m_d,  a = W mu_lk = Eenv
//   Vsig_j = sum_{d in j} a_d^2 v_d + sum_n var_lk,n [ (sum_{d in j} W_dn m_d)^2 + sum_{d in j} W_dn^2 v_d ]
// and the total over all sub-bands in the summation order of recon_moments_kernel.
__global__ void __launch_bounds__(256) recon_src_moments_kernel(ReconSrcPar rp) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  __shared__ int soff[RECON_MAXSRC + 1];
  double* sW = lds;                              // [D][MOM_MAXCD]
  double* gx = sW + rp.D * MOM_MAXCD;            // [n_gh]
  double* gw = gx + rp.n_gh;
  recon_src_stage(rp, sW, soff, blockDim.x);
  for (int i = threadIdx.x; i < rp.n_gh; i += blockDim.x) { gx[i] = rp.gh_x[i]; gw[i] = rp.gh_w[i]; }
  __syncthreads();
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= rp.T) return;
  const int D = rp.D, N = rp.N, M = rp.M, J = rp.J;
  const double* m = rp.Eft + (size_t)t * M;
  const double* v = rp.Varft + (size_t)t * M;
  double mu[MOM_MAXCD], va[MOM_MAXCD], twm[MOM_MAXCD], twv[MOM_MAXCD];
#pragma unroll
  for (int n = 0; n < MOM_MAXCD; ++n) {
    mu[n] = 0.0; va[n] = 0.0; twm[n] = 0.0; twv[n] = 0.0;
    if (n < N) {
      const double mg = m[D + n], vg = v[D + n];
      double e1, e2;
      if (rp.link_kind == 1) {
        e1 = exp(mg + 0.5 * vg); e2 = exp(2.0 * mg + 2.0 * vg);
      } else {
        const double sg = sqrt(vg);
        e1 = 0.0; e2 = 0.0;
        for (int q = 0; q < rp.n_gh; ++q) {
          const double l = link_eval(0, rp.link_shift, mg + sg * gx[q]);
          e1 = fma(gw[q], l, e1); e2 = fma(gw[q] * l, l, e2);
        }
      }
      mu[n] = e1; va[n] = e2 - e1 * e1;
      if (rp.Emod) rp.Emod[(size_t)t * N + n] = e1;
      if (rp.Vmod) rp.Vmod[(size_t)t * N + n] = va[n];
    }
  }
  double est = 0.0, vst = 0.0;
  for (int j = 0; j < J; ++j) {
    double es = 0.0, vs = 0.0, wm[MOM_MAXCD], wv[MOM_MAXCD];
#pragma unroll
    for (int n = 0; n < MOM_MAXCD; ++n) { wm[n] = 0.0; wv[n] = 0.0; }
    for (int d = __builtin_amdgcn_readfirstlane(soff[j]), d1 = __builtin_amdgcn_readfirstlane(soff[j + 1]); d < d1; ++d) {
      const double md = m[d], vd = v[d];
      double a = 0.0;
#pragma unroll
      for (int n = 0; n < MOM_MAXCD; ++n) {
        const double w = sW[d * MOM_MAXCD + n];
        a = fma(w, mu[n], a);
        wm[n] = fma(w, md, wm[n]); wv[n] = fma(w * w, vd, wv[n]);
        twm[n] = fma(w, md, twm[n]); twv[n] = fma(w * w, vd, twv[n]);
      }
      es = fma(a, md, es); vs = fma(a * a, vd, vs);
      est = fma(a, md, est); vst = fma(a * a, vd, vst);
      if (rp.Eenv) rp.Eenv[(size_t)t * D + d] = a;
    }
#pragma unroll
    for (int n = 0; n < MOM_MAXCD; ++n) vs = fma(va[n], fma(wm[n], wm[n], wv[n]), vs);
    if (rp.Esrc) rp.Esrc[(size_t)t * J + j] = es;
    if (rp.Vsrc) rp.Vsrc[(size_t)t * J + j] = vs;
  }
#pragma unroll
  for (int n = 0; n < MOM_MAXCD; ++n) vst = fma(va[n], fma(twm[n], twm[n], twv[n]), vst);
  if (rp.Esig) rp.Esig[t] = est;
  if (rp.Vsig) rp.Vsig[t] = vst;
}

}  // namespace nagp
