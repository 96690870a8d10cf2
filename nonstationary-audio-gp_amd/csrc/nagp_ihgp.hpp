// nagp_ihgp.hpp -- HIP kernels of the infinite-horizon (steady-state) path.
//   ihgp_filter_kernel  forward filter with per-channel DARE table look-ups, mean-only recursion
//                       (matlab/ihgp_ep_modulator_nmf.m:233-310); one workgroup per problem; block n's
//                       state lives in the registers of thread n, the workgroup cooperates on `mom`.
//   ihgp_adf_kernel, ihgp_adf8_kernel, ihgp_adf8b_kernel, ihgp_adf8sq_kernel   the ADF sweep of that filter organised around one
//                       sequential chain: four waves; role-specialised waves in the three-barrier schedule (the product) and in the
//                       schedule with barrier B1; the same for likModulatorPreCalcwn.  What they share is written once (IhLds .. ih_site_update)
//   ihgp_scan_kernel    backward mean recursion with looked-up steady-state smoother gains (:373-394)
// The EP refresh (:397-436) reuses ep_site_kernel (parallel over steps).
#pragma once
#include <type_traits>
#include "nagp_kernels.hpp"
#include "nagp_momsq.hpp"
#include "nagp_lookup.hpp"

namespace nagp {

// Device look-up tables of ONE problem (all doubles), derived on the host from PPlist / PGlist:
//   hph[M][NG]      h_n^2 * PP(1,1)             (diag(H*PP*H'))
//   wcol[M][NG][BS] h_n * PP(:,1)               (W(ii,n) = PP(ii,ii) * H(n,ii)')          BS = Shape::BS: 4, or 8 when a block has 5 .. 8 states
//   hph0[M], wcol0[M][BS] the same from Pinf (k = 1 of the reference uses PP = Pinf)
//   gtab[M][NG][BS*BS] smoother gain block G (row-major, zero padded)
//   vtab[M][NG]     h_n^2 * PS2(1,1)            (diag(H*P*H') of the looked-up smoother covariance)
struct IhgpTabs {
  int NG;
  const double* r;     // [NG] shared grid
  double lr0;          // log10(r[0])
  double inv_dlr;      // (NG-1)/(log10(r[NG-1])-log10(r[0]))
  const double* base;  // [B][ihgp_tab_size]
};
__host__ __device__ inline size_t itab_hph(const Shape&, int) { return 0; }
__host__ __device__ inline size_t itab_wcol(const Shape& s, int NG) { return (size_t)s.M * NG; }
__host__ __device__ inline size_t itab_hph0(const Shape& s, int NG) { return (size_t)s.M * NG * (1 + s.BS); }
__host__ __device__ inline size_t itab_wcol0(const Shape& s, int NG) { return (size_t)s.M * NG * (1 + s.BS) + s.M; }
__host__ __device__ inline size_t itab_g(const Shape& s, int NG) { return (size_t)s.M * NG * (1 + s.BS) + (1 + s.BS) * (size_t)s.M; }
__host__ __device__ inline size_t itab_v(const Shape& s, int NG) { return itab_g(s, NG) + (size_t)s.M * NG * s.BS * s.BS; }
__host__ __device__ inline size_t itab_size(const Shape& s, int NG) { return itab_v(s, NG) + (size_t)s.M * NG; }

// [~,ind] = min(abs(r-R)): first minimiser; NaN / +-Inf distances everywhere -> index 0 (SURVEY C-4)
__device__ __forceinline__ int nearest_idx(const IhgpTabs& tb, double R) {
  if (!(R == R) || isinf(R)) return 0;
  int est = 0;
  if (R > 0.0) {
    const double f = (log10(R) - tb.lr0) * tb.inv_dlr;
    est = (f <= 0.0) ? 0 : ((f >= (double)(tb.NG - 1)) ? tb.NG - 1 : (int)(f + 0.5));
  }
  if (R > tb.r[tb.NG - 1]) {
    // beyond the grid |r_i - R| is non-increasing in i and may ROUND to the same value for several -- for
    // R > ~1e20 all -- grid points: MATLAB's min returns the first of them (e.g. index 0 for R = 1/ttau = 1e100)
    const double dmin = fabs(tb.r[tb.NG - 1] - R);
    if (fabs(tb.r[0] - R) == dmin) return 0;
    int i = tb.NG - 1;
    while (i > 0 && fabs(tb.r[i - 1] - R) == dmin) --i;
    return i;
  }
  const int lo = (est - 2 < 0) ? 0 : est - 2;
  const int hi = (est + 2 > tb.NG - 1) ? tb.NG - 1 : est + 2;
  int best = lo;
  double bd = fabs(tb.r[lo] - R);
  for (int i = lo + 1; i <= hi; ++i) {
    const double d = fabs(tb.r[i] - R);
    if (d < bd) { bd = d; best = i; }
  }
  return best;
}

struct IhgpPar {
  int itt;
  double ep_damp;
  int mom_all;       // sweep 1: mom at every step; later only at k == T-1
  int64_t k_start;   // first step to process (sweeps >= 2 run only k = T-1 here; the rest is ihgp_aff_*)
  double R_init;     // exp(lik) (or 0 for the constraints variant): initial content of R(:,k)
  int hph_lds;       // filter: keep the H PP H' look-up table [M][NG] in LDS
  int kb;            // steps per I/O block of the filter (LDS ring), <= IH_KB
  int dbg_wave;      // developer diagnostics (NAGP_STAMP_WORKER, default 0): & 7 which worker's time line goes to stamps[8..15] (NAGP_STAMPS);
                     // & 32 the serial time line is wave 1's; & 64 the wrong product table of msp_wproducts (a test shows it to fail)
  double w_old, w_new, mom_alpha;   // as FilterPar: (1-d, d, 1) ihgp_ep_modulator_nmf.m:210-211 ; (1-d, d/alpha, alpha) experiments/ihgp_ep_mods_nmf_mixture.m:291-297
};

constexpr int IH_KB = 16;   // steps per I/O block of the filter (LDS ring); fewer when the LDS is needed elsewhere

__host__ __device__ inline size_t ihgp_ring_doubles(const Shape& s, int kb) { return (size_t)kb * (4 * s.M + s.S + 3); }
__host__ __device__ inline size_t ihgp_filter_lds_doubles(const Shape& s, const MomCfg& mc, int NG, int hph_lds, int kb = IH_KB) {
  return LDS_INT_DOUBLES + (size_t)s.D * s.N + 6 * (size_t)s.M + 8 + NG + (hph_lds ? (size_t)s.M * NG : 0) +
         ihgp_ring_doubles(s, kb) + mom_lds_doubles(mc);
}

// log10 to ~0.003 absolute (exponent + quadratic in the mantissa): only seeds the +-2 window below
__device__ __forceinline__ double coarse_log10(double R) {
  const int hi = __double2hiint(R);
  const int e = ((hi >> 20) & 0x7ff) - 1023;
  const double t = __hiloint2double((hi & 0x000fffff) | 0x3ff00000, __double2loint(R)) - 1.0;
  return ((double)e + t + 0.3466 * t * (1.0 - t)) * 0.30102999566398120;
}

// first minimiser of |r_i - R| with the grid in LDS (same semantics as nearest_idx)
__device__ __forceinline__ int nearest_idx_lds(const double* r, int NG, double lr0, double inv_dlr, double R) {
  if (!(R == R) || isinf(R)) return 0;
  int est = 0;
  if (R > 0.0) {
    const double f = (coarse_log10(R) - lr0) * inv_dlr;
    est = (f <= 0.0) ? 0 : ((f >= (double)(NG - 1)) ? NG - 1 : (int)(f + 0.5));
  }
  if (R > r[NG - 1]) {   // rounding ties beyond the grid: first minimiser (see nearest_idx)
    const double dmin = fabs(r[NG - 1] - R);
    if (fabs(r[0] - R) == dmin) return 0;
    int i = NG - 1;
    while (i > 0 && fabs(r[i - 1] - R) == dmin) --i;
    return i;
  }
  const int lo = (est - 2 < 0) ? 0 : est - 2;
  const int hi = (est + 2 > NG - 1) ? NG - 1 : est + 2;
  int best = lo;
  double bd = fabs(r[lo] - R);
  for (int i = lo + 1; i <= hi; ++i) {
    const double d = fabs(r[i] - R);
    if (d < bd) { bd = d; best = i; }
  }
  return best;
}

// All per-step global traffic goes through an LDS ring of IH_KB steps that is filled / flushed with
// coalesced transfers once per block, so the sequential loop body contains no global-memory waits
// except the (L2-resident) table gather.
// SRC: the block-structured mom path (source-separation mixtures) and a run-time ring depth; compiled out otherwise
// BS: doubles per block row in the packed model and the tables (4; 8 for plans with a block of 5 .. 8 states)
template <int MV, bool SRC, int BS = 4>
__global__ void __launch_bounds__(MV >= 9 ? 512 : 256) ihgp_filter_kernel(Shape sh, Bufs b, MomCfg mc, IhgpTabs tb, IhgpPar ip) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int tid = threadIdx.x, NT = blockDim.x;
  const int S = sh.S, M = sh.M, NG = tb.NG;
  const int64_t T = sh.T;
  const int pb = blockIdx.x;
  const double* mdl = b.model + (size_t)pb * mdl_size(sh);
  const double* tab = tb.base + (size_t)pb * itab_size(sh, NG);

  int* ioff = reinterpret_cast<int*>(lds);
  int* ibsz = ioff + (MAXM + 1);
  double* sW = lds + LDS_INT_DOUBLES;
  double* fmu = sW + (size_t)sh.D * sh.N;
  double* HPH = fmu + M;
  double* dl = HPH + M;
  double* d2l = dl + M;
  double* misc = d2l + M;
  double* rg = misc + 8 + 2 * M;          // [NG] look-up grid
  double* thph = rg + NG;                  // [M][NG] H PP H' table (ip.hph_lds)
  const int KB = SRC ? ip.kb : IH_KB;
  double* ry = thph + (ip.hph_lds ? (size_t)M * NG : 0);   // ring: y[KB]
  double* rlZ = ry + KB;                //       lZ[KB]
  double* rZ = rlZ + KB;                //       Z of the steps that called mom (< 0: none); log taken at the flush
  double* rtt = rZ + KB;                //       ttau[KB][M]
  double* rtn = rtt + (size_t)KB * M;   //       tnu
  double* rR = rtn + (size_t)KB * M;    //       R
  double* rfm = rR + (size_t)KB * M;    //       H*m (filtered)
  double* rMF = rfm + (size_t)KB * M;   //       m (filtered) [KB][S]
  double* ws = rMF + (size_t)KB * S;
  for (int i = tid; i <= M; i += NT) ioff[i] = sh.off[i];
  for (int i = tid; i < M; i += NT) ibsz[i] = sh.bsz[i];
  for (int i = tid; i < sh.D * sh.N; i += NT) sW[i] = mdl[mdl_W(sh) + i];
  for (int i = tid; i < NG; i += NT) rg[i] = tb.r[i];
  if (ip.hph_lds)
    for (int i = tid; i < M * NG; i += NT) thph[i] = tab[itab_hph(sh, NG) + i];
  const double sn2 = mdl[mdl_sn2(sh)];
  mom_cache_tables(mc, ws);
  const double pEP1 = mom_pEP(mc, sn2, ip.mom_alpha);
  __syncthreads();

  // thread n < M owns block n
  const int n = tid;
  const bool act = n < M;
  double A4[BS * BS], mreg[BS];
#pragma unroll
  for (int i = 0; i < BS; ++i) mreg[i] = 0.0;
  double hn = 0.0;
  int o = 0, bs = 0;
  if (act) {
    if constexpr (BS == 4) tile_load(A4, mdl + mdl_A(sh) + (size_t)n * 16);
    else {
#pragma unroll
      for (int e = 0; e < BS * BS; ++e) A4[e] = mdl[mdl_A(sh) + (size_t)n * BS * BS + e];
    }
    hn = mdl[mdl_h(sh) + n];
    o = ioff[n]; bs = ibsz[n];
    if (ip.k_start > 0) {      // continue from the filtered mean of the previous step
      const double* mp = b.MF + ((size_t)pb * T + (ip.k_start - 1)) * S;
#pragma unroll
      for (int i = 0; i < BS; ++i)
        if (i < bs) mreg[i] = mp[o + i];
    } else if (ip.itt > 1) {   // m is NOT reset between sweeps (SURVEY C-22): smoothed mean at k=0
      const double* ms0 = b.MS + (size_t)pb * T * S;
#pragma unroll
      for (int i = 0; i < BS; ++i)
        if (i < bs) mreg[i] = ms0[o + i];
    }
  }
  const double* yv = b.y + (size_t)pb * T;
  double* g_tt = b.ttau + (size_t)pb * T * M;
  double* g_tn = b.tnu + (size_t)pb * T * M;
  double* g_R = b.R + (size_t)pb * T * M;
  double* g_lZ = b.lZ + (size_t)pb * T;
  double* g_MF = b.MF + (size_t)pb * T * S;
  double* g_fm = b.fm + (size_t)pb * T * M;
  double Rprev = (act && ip.k_start > 0) ? b.R[((size_t)pb * T + (ip.k_start - 1)) * M + n] : 0.0;
  unsigned long long n_clamped = 0;
  unsigned long long st_a = 0, st_b = 0, st[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (mc.stamps && tid == 0) st_a = __builtin_readcyclecounter();

  for (int64_t k0 = ip.k_start; k0 < T; k0 += KB) {
    const int nb = (T - k0 < KB) ? (int)(T - k0) : KB;
    // ---- fill the ring for steps k0 .. k0+nb-1
    for (int i = tid; i < nb; i += NT) { ry[i] = yv[k0 + i]; rlZ[i] = g_lZ[k0 + i]; rZ[i] = -1.0; }
    for (int i = tid; i < nb * M; i += NT) {
      rtt[i] = g_tt[(size_t)k0 * M + i]; rtn[i] = g_tn[(size_t)k0 * M + i]; rR[i] = g_R[(size_t)k0 * M + i];
    }
    __syncthreads();
    for (int kk = 0; kk < nb; ++kk) {
      const int64_t k = k0 + kk;
      const double yk = ry[kk];
      double hph = 0.0, wc[BS], Am[BS], fmun = 0.0;
#pragma unroll
      for (int i = 0; i < BS; ++i) { wc[i] = 0.0; Am[i] = 0.0; }
      if (act) {
        if (k > 0) {
          const int idx = nearest_idx_lds(rg, NG, tb.lr0, tb.inv_dlr, Rprev);
          hph = ip.hph_lds ? thph[n * NG + idx] : tab[itab_hph(sh, NG) + (size_t)n * NG + idx];
          const double* w = tab + itab_wcol(sh, NG) + ((size_t)n * NG + idx) * BS;
#pragma unroll
          for (int i = 0; i < BS; ++i) wc[i] = w[i];
        } else {
          hph = tab[itab_hph0(sh, NG) + n];
          const double* w = tab + itab_wcol0(sh, NG) + (size_t)n * BS;
#pragma unroll
          for (int i = 0; i < BS; ++i) wc[i] = w[i];
        }
#pragma unroll
        for (int i = 0; i < BS; ++i) {
          double a = 0.0;
#pragma unroll
          for (int l = 0; l < BS; ++l) a = fma(A4[BS * i + l], mreg[l], a);
          Am[i] = a;
        }
        fmun = hn * Am[0];
        fmu[n] = fmun; HPH[n] = hph;
      }
      const bool do_mom = ip.mom_all || (k == T - 1);
      double tnew = 0.0, nnew = 0.0, Rn = 0.0;
      if (do_mom) {
        lds_barrier();
        if (mc.stamps && tid == 0) { st_b = __builtin_readcyclecounter(); st[4] += st_b - st_a; }
        mom_eval<MV, false, SRC>(mc, sW, pEP1, sn2, ip.mom_alpha, yk, fmu, HPH, ws, &misc[0], dl, d2l, st);
        if (act) {
          const double d1 = dl[n], d2 = d2l[n];
          const double t_old = rtt[kk * M + n], n_old = rtn[kk * M + n];
          tnew = ip.w_old * t_old + ip.w_new * (-d2 / (1.0 + d2 * hph));
          nnew = ip.w_old * n_old + ip.w_new * ((d1 - fmun * d2) / (1.0 + d2 * hph));
          Rn = 1.0 / tnew;                      // before the clamp (:269)
        }
        if (tid == 0) rZ[kk] = misc[0];
        if (mc.stamps && tid == 0) st_a = __builtin_readcyclecounter();
      } else if (act) {
        tnew = rtt[kk * M + n]; nnew = rtn[kk * M + n];
        Rn = rR[kk * M + n];
      }
      if (act) {
        if (!(tnew > 0.0)) ++n_clamped;
        tnew = max0(tnew);                       // :274 (NaN -> 0, C-3)
        const double ys = nnew / tnew;
        if (tnew == 0.0) {
          Rn = INFINITY;
#pragma unroll
          for (int i = 0; i < BS; ++i) mreg[i] = Am[i];
        } else {
          const double den = hph + Rn;
#pragma unroll
          for (int i = 0; i < BS; ++i) mreg[i] = Am[i] + (wc[i] / den) * (ys - fmun);
        }
        rtt[kk * M + n] = tnew; rtn[kk * M + n] = nnew; rR[kk * M + n] = Rn;
#pragma unroll
        for (int i = 0; i < BS; ++i)
          if (i < bs) rMF[(size_t)kk * S + o + i] = mreg[i];
        rfm[kk * M + n] = hn * mreg[0];
        Rprev = Rn;
      }
      if (do_mom) lds_barrier();   // fmu/HPH/dl reuse
      if (mc.stamps && tid == 0) { st_b = __builtin_readcyclecounter(); st[5] += st_b - st_a; st_a = st_b; }
    }
    // ---- flush the ring
    __syncthreads();
    for (int i = tid; i < nb; i += NT) g_lZ[k0 + i] = (rZ[i] < 0.0) ? rlZ[i] : log(rZ[i]);
    for (int i = tid; i < nb * M; i += NT) {
      g_tt[(size_t)k0 * M + i] = rtt[i]; g_tn[(size_t)k0 * M + i] = rtn[i]; g_R[(size_t)k0 * M + i] = rR[i];
      g_fm[(size_t)k0 * M + i] = rfm[i];
    }
    for (int i = tid; i < nb * S; i += NT) g_MF[(size_t)k0 * S + i] = rMF[i];
    __syncthreads();
  }
  if (act && n_clamped) atomicAdd(&b.counters[(size_t)pb * 4 + 1], n_clamped);
  if (mc.stamps && tid == 0)
    for (int i = 0; i < 8; ++i) mc.stamps[i] += st[i];
}

// ---------------------------------------------------------------------------------------------
// ADF sweep of the infinite-horizon filter for likModulatorNMFPower on fully symmetric sigma-point sets
// (ihgp_ep_modulator_nmf.m:233-310 with the mom of likModulatorNMFPower.m:28-87): the same step as ihgp_filter_kernel,
// organised around the latency of ONE sequential chain.  Wave 0 owns the sub-band sites (lane d = block d), wave 1 the modulator
// sites (lane j = block D+j); each runs, without any workgroup barrier, everything from the reduced cubature sums of step k to the
// inputs of the cubature of step k+1:
//   sums -> d lZ, d2 lZ -> site update, clamp, R -> gain, mean update, ring -> table look-up for k+1 -> A m, fmu, H PP H'
// The modulator sites have the short tail (their sums come ready-made out of the cubature), so wave 1 goes straight on to the
// link tables of step k+1 -- the exp / log chain of the step -- while wave 0 still forms W_d'RW_d for the sub-bands.
// The four waves then share the remaining cubature stages of nagp_momsp.hpp (five barriers per step).  Every processed step calls
// mom (sweep 1: all steps; later sweeps: launched for k = T-1 only).
// Ring of the filtered means: [KB][M][4], block padded (two 16-byte stores per lane and step); the flush strips the padding.
__host__ __device__ inline size_t ihgp_adf_ring_doubles(const Shape& s, int kb) { return (size_t)kb * (8 * s.M + 3); }
__host__ __device__ inline size_t ihgp_adf_lds_doubles(const Shape& s, int CD, int NG, int hph_lds, int kb) {
  return (size_t)s.D * s.N + 2 * 68 + NG + (hph_lds ? (size_t)s.M * NG : 0) + ihgp_adf_ring_doubles(s, kb) + (s.S + 1) / 2 + 2 +
         msp_lds_doubles(CD, s.D);
}
// (ih_thr_tail: the steps of the look-up from ttau, NG - 1 doubles behind the state map of ihgp_adf8_kernel; an even count keeps the
// workspace behind it 16-byte aligned)
__host__ __device__ inline int ih_thr_tail(int NG) { return NG + (NG & 1); }
__host__ __device__ inline size_t ihgp_adf8_lds_doubles(const Shape& s, int CD, int NG, int hph_lds, int kb) {
  return ihgp_adf_lds_doubles(s, CD, NG, hph_lds, kb) - msp_lds_doubles(CD, s.D) + msp_lds_doubles(CD, s.D, 1) + ih_thr_tail(NG);
}

// [~,ind] = min(abs(r-R)) as nearest_idx_lds, with a three-point window around the seed: the seed's error (0.003 in log10,
// a tenth of a grid step, plus 0.02 steps between the linear and the logarithmic mid-point) keeps the minimiser inside it.
// Grids that are not the reference's logspace(-2,4,200) (ihgp_ep_modulator_nmf.m:131) take the five-point form.
__device__ __forceinline__ int nearest_idx3(msp_rp r, int NG, double lr0, double inv_dlr, double rmax, double R) {
  if (!(R == R) || isinf(R)) return 0;
  if (R > rmax) {   // rounding ties beyond the grid: first minimiser (see nearest_idx)
    const double dmin = fabs(r[NG - 1] - R);
    if (fabs(r[0] - R) == dmin) return 0;
    int i = NG - 1;
    while (i > 0 && fabs(r[i - 1] - R) == dmin) --i;
    return i;
  }
  int est = 0;
  if (R > 0.0) {
    const double f = (coarse_log10(R) - lr0) * inv_dlr;
    est = (f <= 0.0) ? 0 : ((f >= (double)(NG - 1)) ? NG - 1 : (int)(f + 0.5));
  }
  const int mid = (est < 1) ? 1 : ((est > NG - 2) ? NG - 2 : est);
  const double d0 = fabs(r[mid - 1] - R), d1 = fabs(r[mid] - R), d2 = fabs(r[mid + 1] - R);
  int best = mid - 1; double bd = d0;
  if (d1 < bd) { bd = d1; best = mid; }
  if (d2 < bd) best = mid + 1;
  return best;
}

// ---- What the ADF kernels below have in common, written once: ihgp_adf_kernel, ihgp_adf8b_kernel and ihgp_adf8sq_kernel use all of it;
// the three-barrier ihgp_adf8_kernel the LDS set-up and the lane set-up only (its head, its site update and its ring are its own).
// Functions of small structs of scalars and pointers, as MsrS / ih_window_pick: a lambda capturing by reference put its state into scratch.

// LDS of one launch, and the scalars every role reads.  tail: doubles between the state map and the cubature's workspace (the square-root
// kernel's W transposed)
struct IhLds {
  double *rMF, *rtt, *rtn, *rR, *rfm, *ry, *rlZ, *rZ;      // the I/O ring
  double *sW, *fmu, *HPH, *rg, *thph; int* smap; double *tail, *ws;
  const double *mdl, *tab; double sn2a, pEP1, rmax;
};
__device__ __forceinline__ void ih_lds_setup(IhLds& L, double* lds, const Shape& sh, const Bufs& b, const MomCfg& mc, const IhgpTabs& tb, const IhgpPar& ip,
                                             int CD, int tail, int tid, int NT) {
  const int S = sh.S, M = sh.M, D = sh.D, NG = tb.NG, KB = ip.kb;
  L.mdl = b.model + (size_t)blockIdx.x * mdl_size(sh);
  L.tab = tb.base + (size_t)blockIdx.x * itab_size(sh, NG);
  L.rMF = lds;                                   // ring: m (filtered) [KB][M][4]   (16-byte aligned)
  L.rtt = L.rMF + (size_t)KB * M * 4;            //       ttau[KB][M]
  L.rtn = L.rtt + (size_t)KB * M;                //       tnu
  L.rR = L.rtn + (size_t)KB * M;                 //       R
  L.rfm = L.rR + (size_t)KB * M;                 //       H*m (filtered)
  L.ry = L.rfm + (size_t)KB * M;                 //       y[KB]
  L.rlZ = L.ry + KB;                             //       lZ[KB]
  L.rZ = L.rlZ + KB;                             //       Z of the step; log taken at the flush
  L.sW = L.rZ + KB;                              // [D][CD]
  L.fmu = L.sW + (size_t)D * CD;                 // [68]: M sites, zero padded (stage A of the cubature reads 4*K entries)
  L.HPH = L.fmu + 68;
  L.rg = L.HPH + 68;                             // [NG] look-up grid
  L.thph = L.rg + NG;                            // [M][NG] H PP H' table (ip.hph_lds)
  L.smap = reinterpret_cast<int*>(L.thph + (ip.hph_lds ? (size_t)M * NG : 0));   // [S] state -> padded ring slot 4*block + row
  L.tail = reinterpret_cast<double*>(L.smap) + (S + 1) / 2;
  L.ws = L.tail + tail;
  for (int i = tid; i < D * CD; i += NT) L.sW[i] = L.mdl[mdl_W(sh) + i];
  for (int i = tid; i < NG; i += NT) L.rg[i] = tb.r[i];
  if (ip.hph_lds)
    for (int i = tid; i < M * NG; i += NT) L.thph[i] = L.tab[itab_hph(sh, NG) + i];
  for (int i = tid; i < 68; i += NT) { L.fmu[i] = 0.0; L.HPH[i] = 0.0; }
  for (int i = tid; i < M; i += NT)
    for (int r = 0; r < sh.bsz[i]; ++r) L.smap[sh.off[i] + r] = 4 * i + r;
  const double sn2 = L.mdl[mdl_sn2(sh)];
  L.sn2a = sn2 / ip.mom_alpha;
  L.pEP1 = mom_pEP(mc, sn2, ip.mom_alpha);
  L.rmax = tb.r[NG - 1];
  __syncthreads();
}

// global rows of this problem
struct IhRows { const double* yv; double *g_tt, *g_tn, *g_R, *g_lZ, *g_MF, *g_fm; };
__device__ __forceinline__ void ih_rows(IhRows& G, const Shape& sh, const Bufs& b) {
  const size_t pT = (size_t)blockIdx.x * sh.T;
  G.yv = b.y + pT; G.g_lZ = b.lZ + pT;
  G.g_tt = b.ttau + pT * sh.M; G.g_tn = b.tnu + pT * sh.M; G.g_R = b.R + pT * sh.M; G.g_fm = b.fm + pT * sh.M;
  G.g_MF = b.MF + pT * sh.S;
}

// the block ring: steps k0 .. k0+nb-1 in, by the whole workgroup ...
__device__ __forceinline__ void ih_ring_fill(const IhLds& L, const IhRows& G, int64_t k0, int nb, int M, int tid, int NT) {
  for (int i = tid; i < nb; i += NT) { L.ry[i] = G.yv[k0 + i]; L.rlZ[i] = G.g_lZ[k0 + i]; L.rZ[i] = -1.0; }
  for (int i = tid; i < nb * M; i += NT) { L.rtt[i] = G.g_tt[(size_t)k0 * M + i]; L.rtn[i] = G.g_tn[(size_t)k0 * M + i]; }
  __syncthreads();
}
// ... and out (the filtered means through the state map: the flush strips the padding).  The lane index is opaque here: the flush's
// per-lane addresses are formed where they are used and not carried, as loop invariants, in vector registers across the serial chain
__device__ __forceinline__ void ih_ring_flush(const IhLds& L, const IhRows& G, int64_t k0, int nb, int M, int S, int lane0, int NT) {
  const int tid = lane0 + opaque_zero();
  __syncthreads();
  for (int i = tid; i < nb; i += NT) G.g_lZ[k0 + i] = (L.rZ[i] < 0.0) ? L.rlZ[i] : log(L.rZ[i]);
  for (int i = tid; i < nb * M; i += NT) {
    G.g_tt[(size_t)k0 * M + i] = L.rtt[i]; G.g_tn[(size_t)k0 * M + i] = L.rtn[i]; G.g_R[(size_t)k0 * M + i] = L.rR[i];
    G.g_fm[(size_t)k0 * M + i] = L.rfm[i];
  }
  for (int i = tid; i < nb * S; i += NT) { const int q = i / S, e = i - q * S; G.g_MF[(size_t)k0 * S + i] = L.rMF[(size_t)q * M * 4 + L.smap[e]]; }
  __syncthreads();
}

// developer diagnostics (NAGP_STAMPS): one time line, eight slots
struct IhSt { bool on; unsigned long long a, t[8]; };
__device__ __forceinline__ void ih_st_start(IhSt& s, bool on) {
  s.on = on; s.a = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) s.t[i] = 0;
  if (on) s.a = __builtin_readcyclecounter();
}
__device__ __forceinline__ void ih_stamp(IhSt& s, int slot) {
  if (s.on) { const unsigned long long c = __builtin_readcyclecounter(); s.t[slot] += c - s.a; s.a = c; }
}
__device__ __forceinline__ void ih_st_store(const IhSt& s, unsigned long long* stamps) {
  if (s.on)
    for (int i = 0; i < 8; ++i) stamps[i] += s.t[i];
}

// The serial lane: wave 0, lane d < D owns sub-band block d; wave 1, lane j < N owns modulator block D + j.  Its state -- the block of A,
// h, the filtered mean, R of the step before -- and its per-lane ring / table addresses (vector registers; the step index adds an
// immediate-free scalar offset; the addresses of idle lanes are those of site 0).  wrow[NW]: a sub-band lane's row of W, zero on the
// other lanes (NW = 0: the kernel has no use for it)
struct IhLane {
  bool sub, act; int n;
  double A4[16], mreg[4], hn, Rprev;
  msp_wp p_tt, p_tn, p_R, p_fm, p_MF, p_fmu, p_HPH; msp_rp p_hph, p_rg;
  const double *g_wcol, *g_hph;
  unsigned int n_clamped;
};
template <int NW>
__device__ __forceinline__ void ih_lane_setup(IhLane& ln, const IhLds& L, const Shape& sh, const Bufs& b, const IhgpPar& ip, int NG, int wave, int lane, double* wrow) {
  const int S = sh.S, M = sh.M, D = sh.D, pb = blockIdx.x;
  const int64_t T = sh.T;
  ln.sub = (wave == 0) && lane < D;
  ln.act = ln.sub || ((wave == 1) && lane < sh.N);
  const int n = (wave == 0) ? lane : D + lane;
  const int nn = ln.act ? n : 0;
  ln.n = n;
#pragma unroll
  for (int i = 0; i < 4; ++i) ln.mreg[i] = 0.0;
  ln.hn = 0.0;
#pragma unroll
  for (int j = 0; j < NW; ++j) wrow[j] = 0.0;
  tile_zero(ln.A4);
  if (ln.act) {
    tile_load(ln.A4, L.mdl + mdl_A(sh) + (size_t)n * 16);
    ln.hn = L.mdl[mdl_h(sh) + n];
    const int o = sh.off[n], bs = sh.bsz[n];
    if (ln.sub) {
#pragma unroll
      for (int j = 0; j < NW; ++j) wrow[j] = L.sW[n * NW + j];
    }
    if (ip.k_start > 0) {      // continue from the filtered mean of the previous step
      const double* mp = b.MF + ((size_t)pb * T + (ip.k_start - 1)) * S;
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (i < bs) ln.mreg[i] = mp[o + i];
    } else if (ip.itt > 1) {   // m is NOT reset between sweeps (SURVEY C-22): smoothed mean at k=0
      const double* ms0 = b.MS + (size_t)pb * T * S;
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (i < bs) ln.mreg[i] = ms0[o + i];
    }
  }
  ln.p_tt = (msp_wp)(L.rtt + nn); ln.p_tn = (msp_wp)(L.rtn + nn); ln.p_R = (msp_wp)(L.rR + nn); ln.p_fm = (msp_wp)(L.rfm + nn);
  ln.p_MF = (msp_wp)(L.rMF + 4 * nn);
  ln.p_fmu = (msp_wp)(L.fmu + nn); ln.p_HPH = (msp_wp)(L.HPH + nn);
  ln.p_hph = (msp_rp)(L.thph + (size_t)nn * NG);
  ln.p_rg = (msp_rp)L.rg + opaque_zero();
  ln.g_wcol = L.tab + itab_wcol(sh, NG) + (size_t)nn * NG * 4;
  ln.g_hph = L.tab + itab_hph(sh, NG) + (size_t)nn * NG;
  ln.Rprev = (ln.act && ip.k_start > 0) ? b.R[((size_t)pb * T + (ip.k_start - 1)) * M + n] : 0.0;
  ln.n_clamped = 0;
}
__device__ __forceinline__ void ih_lane_end(const IhLane& ln, const Bufs& b) {
  if (ln.act && ln.n_clamped) atomicAdd(&b.counters[(size_t)blockIdx.x * 4 + 1], (unsigned long long)ln.n_clamped);
}

// Head of step k in the block-ring kernels: table look-up from R of step k-1 (k_pos: k > 0; the tables of k = 0 otherwise), A m, the
// cubature's inputs fmu and H PP H' (no barrier: the lane's own entries)
struct IhHead { double hph, wc[4], Am[4], fmun; };
__device__ __forceinline__ void ih_head(IhLane& ln, IhHead& h, bool k_pos, const Shape& sh, const IhgpTabs& tb, const IhLds& L, const IhgpPar& ip, IhSt& st) {
  if (!ln.act) return;
  const int NG = tb.NG;
  if (k_pos) {
    const int idx = nearest_idx3(ln.p_rg, NG, tb.lr0, tb.inv_dlr, L.rmax, ln.Rprev);
    if (st.on) { asm volatile("" :: "v"(idx)); ih_stamp(st, 6); }
    h.hph = ip.hph_lds ? ln.p_hph[idx] : ln.g_hph[idx];
    const double2* w = reinterpret_cast<const double2*>(ln.g_wcol + (size_t)idx * 4);
    const double2 w0 = w[0], w1 = w[1];
    h.wc[0] = w0.x; h.wc[1] = w0.y; h.wc[2] = w1.x; h.wc[3] = w1.y;
  } else {
    h.hph = L.tab[itab_hph0(sh, NG) + ln.n];
    const double* w = L.tab + itab_wcol0(sh, NG) + (size_t)ln.n * 4;
#pragma unroll
    for (int i = 0; i < 4; ++i) h.wc[i] = w[i];
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    double a0 = ln.A4[4 * i] * ln.mreg[0], a1 = ln.A4[4 * i + 1] * ln.mreg[1];
    a0 = fma(ln.A4[4 * i + 2], ln.mreg[2], a0); a1 = fma(ln.A4[4 * i + 3], ln.mreg[3], a1);
    h.Am[i] = a0 + a1;
  }
  h.fmun = ln.hn * h.Am[0];
  *ln.p_fmu = h.fmun; *ln.p_HPH = h.hph;
  ih_stamp(st, 7);
}

// Site update of step k in the block-ring kernels, from the cubature's outputs Z, d1, d2 of this lane's site (msp_outputs, msq_outputs)
// to the ring stores (slot kk) and R for the look-up of step k+1.  Active lanes only.
__device__ __forceinline__ void ih_site_update(IhLane& ln, const IhHead& h, const IhgpPar& ip, const IhLds& L, int kk, int M, double Z, double d1, double d2, IhSt& st) {
  const int ko = kk * M;
  if (st.on) { asm volatile("" :: "v"(d2)); ih_stamp(st, 4); }
  const double t_old = ln.p_tt[ko], n_old = ln.p_tn[ko];
  // site update (:265-266): -d2/(1+d2 HPH), (d1 - fmu d2)/(1+d2 HPH) through one reciprocal
  const double r1 = rcp_nr(fma(d2, h.hph, 1.0));
  double tnew = fma(ip.w_new, -d2 * r1, ip.w_old * t_old);
  const double nnew = fma(ip.w_new, fma(-h.fmun, d2, d1) * r1, ip.w_old * n_old);
  if (!(tnew > 0.0)) ++ln.n_clamped;
  tnew = max0(tnew);                                               // :274 (NaN -> 0, C-3)
  const double Rn = 1.0 / tnew;                                    // R = 1/ttau: the look-up key and an output, exact division
  // (for tnew > 0 the reference's R(:,k) = 1./ttau before the clamp is this value; otherwise :287 overwrites it with Inf)
  // R = inf: ttau = 0, or ttau of underflow size (1/ttau overflows while ys = tnu/ttau stays finite): the reference's
  // (ys - fmu)/(HPH + R) is 0 there; the reciprocal form below would multiply inf by 0
  double g = 0.0;
  if (Rn < INFINITY) g = fma(nnew, Rn, -h.fmun) * rcp_nr(h.hph + Rn);  // (ys - fmu)/(HPH + R), ys = tnu/ttau (:277, :289-292)
  typedef double d2v __attribute__((ext_vector_type(2)));
  d2v m01, m23;
  ln.mreg[0] = fma(h.wc[0], g, h.Am[0]); ln.mreg[1] = fma(h.wc[1], g, h.Am[1]); ln.mreg[2] = fma(h.wc[2], g, h.Am[2]); ln.mreg[3] = fma(h.wc[3], g, h.Am[3]);
  m01.x = ln.mreg[0]; m01.y = ln.mreg[1]; m23.x = ln.mreg[2]; m23.y = ln.mreg[3];
  ln.p_tt[ko] = tnew; ln.p_tn[ko] = nnew; ln.p_R[ko] = Rn;
  typedef d2v __attribute__((address_space(3))) * lds_d2p;
  lds_d2p mf = (lds_d2p)(ln.p_MF + 4 * ko);
  mf[0] = m01; mf[1] = m23;
  ln.p_fm[ko] = ln.hn * ln.mreg[0];
  ln.Rprev = Rn;
  if (ln.n == 0) L.rZ[kk] = Z;
  if (st.on) { asm volatile("" :: "v"(ln.Rprev)); ih_stamp(st, 5); }
}

template <int CD>
__global__ void __launch_bounds__(MSP_NT) ihgp_adf_kernel(Shape sh, Bufs b, MomCfg mc, MomSp sp, IhgpTabs tb, IhgpPar ip) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  constexpr int NT = MSP_NT;
  const int S = sh.S, M = sh.M, D = sh.D, KB = ip.kb;
  const int64_t T = sh.T;
  IhLds L;
  ih_lds_setup(L, lds, sh, b, mc, tb, ip, CD, 0, tid, NT);
  IhRows G;
  ih_rows(G, sh, b);
  MspCtx<CD> x;
  msp_setup<CD>(x, mc, sp, L.sW, L.fmu, L.HPH, L.ws, 1);

  IhLane ln;
  double wrow[CD];
  ih_lane_setup<CD>(ln, L, sh, b, ip, tb.NG, wave, tid & 63, wrow);
  IhSt st;                                           // wave 0's time line
  ih_st_start(st, mc.stamps && tid == 0);
  IhHead h = {0.0, {0, 0, 0, 0}, {0, 0, 0, 0}, 0.0};
  if (wave <= 1) ih_head(ln, h, ip.k_start > 0, sh, tb, L, ip, st);
  if (wave == 1) { msp_wave_fence(); msp_link<CD>(x, mc); }      // link tables of the first step
  if (st.on) st.a = __builtin_readcyclecounter();

  for (int64_t k0 = ip.k_start; k0 < T; k0 += KB) {
    const int nb = (T - k0 < KB) ? (int)(T - k0) : KB;
    ih_ring_fill(L, G, k0, nb, M, tid, NT);
    for (int kk = 0; kk < nb; ++kk) {
      const int64_t k = k0 + kk;
      lds_barrier();                 // B1: fmu, HPH of step k; its link tables (written by wave 1 on its way here)
      ih_stamp(st, 3);
      msp_qv<CD>(x, mc);             // waves 0, 2, 3
      lds_barrier();                 // B2
      ih_stamp(st, 0);
      msp_stageB<CD>(x, mc, L.ws);
      lds_barrier();                 // B3
      msp_stage1b<CD>(x, mc, sp, L.sn2a, L.ry[kk], L.ws);
      lds_barrier();                 // B4
      ih_stamp(st, 1);
      msp_stage2<CD>(x, mc, L.ws);
      lds_barrier();                 // B5
      ih_stamp(st, 2);
      if (wave <= 1) {
        msp_reduce<CD>(x);
        msp_wave_fence();
        if (ln.act) {
          double Z, d1, d2;
          msp_outputs<CD>(x.accp, ln.sub, ln.n - D, wrow, L.pEP1, mc.jitter, Z, d1, d2);
          ih_site_update(ln, h, ip, L, kk, M, Z, d1, d2, st);
        }
        if (k + 1 < T) {
          ih_head(ln, h, true, sh, tb, L, ip, st);
          if (wave == 1) { msp_wave_fence(); msp_link<CD>(x, mc); }     // fmu / HPH of the modulators just written by this wave
        }
      }
    }
    ih_ring_flush(L, G, k0, nb, M, S, tid, NT);
  }
  ih_lane_end(ln, b);
  ih_st_store(st, mc.stamps);
}

// The look-up of the three-barrier schedule of ihgp_adf8_kernel in its two halves (nagp_lookup.hpp).  ih_window_reads: the three grid
// words and three H PP H' entries round the seed mid = 1 .. NG - 2 (entries 0 .. NG - 1), one batch of LDS reads (the table's only
// when it is in LDS).  Both halves are functions of scalars: as lambdas capturing by reference they put the captured state into scratch.
// ih_window_pick, behind R: the index of the step's table entries and H PP H'; the two side paths -- finite R beyond the grid, the
// table in global memory -- overwrite what the straight line selected.
__device__ __forceinline__ void ih_window_reads(msp_rp p_rg, msp_rp p_hph, bool hph_in_lds, int mid, double& r0, double& r1, double& r2, double& h0, double& h1,
                                                double& h2) {
  r0 = p_rg[mid - 1]; r1 = p_rg[mid]; r2 = p_rg[mid + 1];
  if (hph_in_lds) { h0 = p_hph[mid - 1]; h1 = p_hph[mid]; h2 = p_hph[mid + 1]; }      // (table in global memory: the grid words only)
}
__device__ __forceinline__ void ih_window_pick(int mid, double r0, double r1, double r2, double h0, double h1, double h2, msp_rp p_rg, msp_rp p_hph,
                                               const double* g_hph, bool hph_in_lds, double rmax, int NG, double R, int& idx, double& hph) {
  const int sel = lookup_pick3(r0, r1, r2, R);
  idx = mid - 1 + sel;
  hph = (sel == 0) ? h0 : ((sel == 1) ? h1 : h2);
  if (lookup_beyond(rmax, R)) {
    idx = lookup_tail(p_rg, NG, R);
    hph = hph_in_lds ? p_hph[idx] : g_hph[idx];
  } else if (!hph_in_lds) hph = g_hph[idx];      // (issued ahead of the ring stores; first used, and so waited for, where the head stores HPH)
}

// The look-up inside the loop, from ttau alone (nagp_lookup.hpp: lookup_mid_bits, lookup_pick_thr): the two steps tau[mid - 1], tau[mid]
// in place of the three grid words, and a pick that waits for no division.  ttau <= t_inf (R = Inf): index 0 and its H PP H' (h_first, a
// register of the launch).  R itself is read only on the side path t_inf < ttau <= t_beyond (finite R beyond the grid, lookup_tail).
__device__ __forceinline__ void ih_thr_reads(msp_rp p_thr, msp_rp p_hph, bool hph_in_lds, int mid, double& ta, double& tb, double& h0, double& h1, double& h2) {
  ta = p_thr[mid - 1]; tb = p_thr[mid];
  if (hph_in_lds) { h0 = p_hph[mid - 1]; h1 = p_hph[mid]; h2 = p_hph[mid + 1]; }
}
__device__ __forceinline__ void ih_thr_pick(int mid, double ta, double tb, double h0, double h1, double h2, double h_first, msp_rp p_rg, msp_rp p_hph,
                                            const double* g_hph, bool hph_in_lds, double t_beyond, double t_inf, int NG, double ttau, double R, int& idx,
                                            double& hph) {
  const int sel = lookup_pick_thr(ta, tb, ttau);
  const bool at_inf = ttau <= t_inf;
  idx = at_inf ? 0 : mid - 1 + sel;
  hph = (sel == 0) ? h0 : ((sel == 1) ? h1 : h2);
  hph = at_inf ? h_first : hph;
  if (ttau <= t_beyond && !at_inf) {
    idx = lookup_tail(p_rg, NG, R);
    hph = hph_in_lds ? p_hph[idx] : g_hph[idx];
  } else if (!hph_in_lds && !at_inf) hph = g_hph[idx];      // (issued ahead of the ring stores; first used, and so waited for, where the head stores HPH)
}

// y = A x for the lane's 4 x 4 block, two chains of two terms per row (the order of additions of the head of ihgp_adf8_kernel)
__device__ __forceinline__ void ih_a4_times(const double* A4, const double* x, double* y) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    double a0 = A4[4 * i] * x[0], a1 = A4[4 * i + 1] * x[1];
    a0 = fma(A4[4 * i + 2], x[2], a0); a1 = fma(A4[4 * i + 3], x[3], a1);
    y[i] = a0 + a1;
  }
}

// The same sweep with role-specialised waves (nagp_momsp.hpp, role layout): 512 threads, waves 0 / 1 as above, waves 2..7 run the
// parallel stages of the cubature in their own loop.  A wave holds the registers of its role only, which is what lets two
// waves share a SIMD.
// ihgp_adf8_kernel is the product: the direct form of stage 1b at CD <= 6.  CD = 7 and the table form run ihgp_adf8b_kernel (below).
// Barriers of a step: THREE.  B2 | Gaussian weights straight from Q, v and the link tables
// (msr_stage1b_direct); e table (wave 1) | B4 | bin sums; table words of the reduction (serial waves) | B5 | serial tail, head of step
// k+1, then Q / 2Q / v on wave 0 (msr_qv_serial) and the link tables on wave 1 (msp_link), each from the wave's own fmu / HPH stores.
// The two serial chains run side by side from B5 to B2; no barrier puts one behind the other.  Without a barrier between the tail of
// step k and the cubature inputs of step k+1, every LDS region is ordered by construction:
//   region                     writer (step k+1)                    last reader (step k)                         ordered by
//   fmu, sub-bands             wave 0, tail, behind the gain        wave 0, msr_qv_serial                        same wave
//   HPH, sub-bands             wave 0, head                         wave 0, msr_qv_serial                        same wave
//   fmu, modulators            wave 1, tail, behind the gain        wave 1, msp_link                             same wave
//   HPH, modulators            wave 1, head                         wave 1, msp_link                             same wave
//     (fmu of step k+1 is stored behind B5(k); its readers of step k ran ahead of B2(k).  The tail of the last step stores an fmu that
//      nothing reads: the word is the lane's own.  The prologue's head stores both fmu and HPH of the first step.)
//     (msr_qv_serial never uses an entry beyond the sub-bands: with D = 4K it reads none, otherwise it discards what it read)
//   Q / 2Q / v                 wave 0, B5(k) .. B2(k+1)             workers' weights, B2(k) .. B4(k)             B4, B5
//   link tables lk / xg / xg2  wave 1, B5(k) .. B2(k+1)             workers' weights and level 2 of msr_sums, both ahead of B5(k);    B5
//                                                                   msr_reduce_tab on the serial waves, B4(k) .. B5(k)
//   e table                    wave 1, B2 .. B4                     level 2 of msr_sums, B4 .. B5                B5, B2
//   level-2 results (part)     workers, B4 .. B5                    msr_reduce_bins, behind B5                   B2, B4 of step k+1
//   c0 / c1 / c2, acc          as in ihgp_adf8b_kernel              (weights B2 .. B4, level 1 B4 .. B5; acc: one wave)
//   wwt (static products)      wave 0, once                         wave 0                                       same lane
//   W rows, look-up grid and its threshold table, H PP H' table: written ahead of the loop (one __syncthreads), read-only in it -- wave 0
//     reads its row of W between B4 and B5, both serial waves two thresholds and three table entries round the seed in the site update
//     (one batch of reads; the grid words only on the side path beyond the grid)
// The look-up of step k+1 comes from ttau alone (nagp_lookup.hpp), straight behind the clamp of the site update: the window's centre from
// the bit pattern of ttau by integer operations (lookup_mid_bits), two steps of the grid's threshold table and three table entries in one
// batch of reads, the index as the count of steps at or above ttau.  The gain is (tnu - fmu ttau) / (1 + HPH ttau).  The exact division
// R = 1 / ttau stands ahead of the ring stores in program order and feeds them, Rprev and the side branch beyond the grid (finite
// R > rmax, entered by t_inf < ttau <= t_beyond: lookup_tail); nothing on the straight path waits for it.
// The prediction stands one fma behind the gain g.  With m_k = Am_k + wc_k g the next prediction is A m_k = A Am_k + (A wc_k) g, and both
// products are known from the head of step k on: the serial waves form P1 = A Am_k, P2 = A wc_k, pa = h P1[0], pb = h P2[0] between B4 and
// B5, where they wait for the bin sums (beside msr_reduce_tab; 42 f64 operations off the chain B5 -> B2).  Behind the gain's select:
// fmu_{k+1} = fma(pb, g, pa), its store, then Am_{k+1} = fma(P2, g, P1) and m_k = fma(wc_k, g, Am_k) for the ring (MF, fm).  The head
// inside the loop keeps the index, the load of wc and H PP H'; the prologue's head (k_start > 0 included) forms A m from the stored mean
// as before, and the first step's window takes its operands from that.  A (Am + wc g) and A Am + (A wc) g round differently: the sweep
// is held by the oracle and the multi-precision fixture (tests/test_ihgp_adf_early_inputs.py), not by the bits of the commit before.
// The serial tail waits for none of its ring stores: no LDS read of the straight path is issued behind them, and the loop reads
// no kernel argument in the head or the site update (a scalar load there would bring an lgkmcnt(0) for the stores with it): the look-up's
// constants are copied into vector registers ahead of the loop.
// The I/O ring of this schedule is circular and streamed: slot k mod KB serves step k (KB = 16, 8 or 4), and four worker waves (2, 3, 6, 7:
// the SIMDs without a serial wave) move one step's worth per step inside their idle window W(k) = B5(k) .. B2(k+1): they store the inputs
// of step k+1 (loaded in W(k-1), carried in a register), load those of step k+2 and flush the outputs of step k-1.  The first step is
// filled ahead of the loop, the last one flushed behind it, one __syncthreads each; no block-level section is left inside the loop.
//   region                     writer                               last reader                                  ordered by
//   ring inputs, slot of k+1   I/O lanes, W(k)                      workers' weights (ry), B2(k+1) .. B4(k+1);   B2(k+1)
//     (y, lZ, ttau, tnu, Z=-1)                                      serial waves (ttau, tnu), B4(k+1) .. B5(k+1), beside msr_reduce_tab
//     ttau, tnu of the slot are next written by the lane that read them (its tail of step k+1, behind B5(k+1))    same lane
//     the slot's previous step k+1-KB: flushed in W(k+2-KB), at least two windows earlier (KB >= 4)              B2 .. B5 of the steps between
//   ring outputs, slot of k    serial tail of step k,               flush by the I/O lanes, W(k+1)               B2(k+1) (.. B5(k+1))
//     (ttau, tnu, R, fm, MF, Z)  B5(k) .. B2(k+1)
//     the slot's next writers: the fill of step k+KB in W(k+KB-1) >= W(k+3), the tail of step k+KB                B2 .. B5 of the steps between
//   one window touches three different slots: k+1 (fill), k (serial tail), k-1 (flush): KB >= 3
// The global loads of a window are issued ahead of its stores and are not waited for before the next window; the flush's stores are
// never waited for (nothing in this launch reads them back).  lds_barrier() waits for LDS traffic only, so both stay in flight across
// the step's barriers.
// msr_reduce as a whole behind B5 would read l0_j and xg2_j(centre) while wave 1 -- whose tail is the shorter one -- may already be
// writing the tables of step k+1; hence its split (msr_reduce_tab / msr_reduce_bins).
// QF (nagp_qform.hpp): the form of Q / 2Q / v on wave 0 -- K and PAD fixed in the instantiation the plan
// picks by its D (qform_pick), or QF_RUNTIME, which serves every D (the remaining padded shapes; every shape under NAGP_IH_QFORM=0).
// The serial loop of wave 1 exists once per link kind, picked ahead of it.  The weights, the exp link and Q / 2Q / v of this schedule are
// bit-equal to the forms the other schedules run (gauss_terms, msp_link, msp_qv).  The softplus link (softplus_short, nagp_explog.hpp) and
// the sub-bands' second moment w'Rw (static products, msp_outputs_b) are not: they round differently from link_eval and msp_outputs, and
// the schedule's results are held by the multi-precision fixture and the oracle instead (tests/test_ep_fixture.py,
// tests/test_ihgp_adf_lean_tail.py).
// STAMPS: the stamps are a build of their own, IH_STAMP / WK_STAMP expand to nothing otherwise.
template <int CD, bool STAMPS = false, int QF = QF_RUNTIME>
__global__ void __launch_bounds__(MSR_NT) ihgp_adf8_kernel(Shape sh, Bufs b, MomCfg mc, MomSp sp, IhgpTabs tb, IhgpPar ip) {
  static_assert(CD >= 1 && CD <= 6, "the 2 x 35 outputs of Q / 2Q / v at CD = 7 do not fit the lanes of wave 0: ihgp_adf8b_kernel");
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  constexpr int NT = MSR_NT;
  const int S = sh.S, M = sh.M, D = sh.D, NG = tb.NG, KB = ip.kb;
  const int64_t T = sh.T;
  IhLds ld;
  ih_lds_setup(ld, lds, sh, b, mc, tb, ip, CD, ih_thr_tail(NG), tid, NT);
  IhRows gr;                                         // (the streamed ring: the I/O lanes of the worker role fill and flush it)
  ih_rows(gr, sh, b);
  msr_init(CD, D, ld.ws);
  // the steps tau[NG - 1] of the look-up from ttau (lookup_thresholds: the plan uploads them behind the grid), read-only in the loop
  for (int i = tid; i < NG - 1; i += NT) ld.tail[i] = tb.r[NG + i];
  __syncthreads();
  if (wave >= MSR_W0) {
    // ================= worker role: the parallel stages of the cubature; the same barriers as the serial role below
    // the placed copy of the lists and its position tables: the point's three weights each where the bin sums' reads collide least (with
    // NAGP_IH_PLACE=0 the plan hands in the second copy and identity positions there)
    MsrW<CD, true> xw;
    msr_setup_W<CD>(xw, mc, sp, ld.sW, ld.fmu, ld.HPH, ld.ws, false, msr_desc_p_base(), sp.bdesc + msr_desc_pos_base());
    // Q | 2Q | v of the weights behind ONE address register: every word of the region is then read through an instruction offset, where
    // the compiler otherwise rebuilds an address per pair of reads every step
    asm volatile("" : "+v"(xw.d_qv));
    asm volatile("" : "+v"(xw.p_c[0]), "+v"(xw.p_c1[0]), "+v"(xw.p_c2[0]));      // (three stores through three registers, no address rebuilt per step)
    // developer diagnostics (NAGP_STAMPS): time lines of worker (NAGP_STAMP_WORKER & 7) in stamps[8..15] and of the last worker in
    // stamps[16..23]
    const int wk_slot = (wave == MSR_W0 + (ip.dbg_wave & 7)) ? 8 : ((wave == MSR_W0 + MSR_NWK - 1) ? 16 : -1);
    const bool wk_stamp = STAMPS && mc.stamps && wk_slot >= 0 && (tid & 63) == 0;
    unsigned long long wk_a = 0, wk_b = 0, wk[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (wk_stamp) wk_a = __builtin_readcyclecounter();
#define WK_STAMP(slot) do { if constexpr (STAMPS) if (wk_stamp) { wk_b = __builtin_readcyclecounter(); wk[slot] += wk_b - wk_a; wk_a = wk_b; } } while (0)
    // one step between its barriers; kk = the step's ring slot
    auto wstep = [&](int kk) __attribute__((always_inline)) {
      lds_barrier();                 // B2
      WK_STAMP(2);                   // (wait at B2: the serial waves' tail, head, Q / v and link tables)
      msr_stage1b_direct<CD, true>(xw, ld.sn2a, ld.ry[kk]);
      WK_STAMP(3);
      lds_barrier();                 // B4
      WK_STAMP(4);
      msr_sums(xw);                  // bin sums, then this wave's share of the 40 sums
      WK_STAMP(5);
      lds_barrier();                 // B5
      WK_STAMP(7);
    };
    {
      // ---- the streamed ring (see the table above): the I/O lanes are the 256 lanes of waves 2, 3, 6, 7 -- the SIMDs that hold no serial
      // wave.  The lane -> item mapping is static: an LDS address, its stride per slot, a global pointer that advances by one step's row.
      // Outputs of a step: ttau | tnu | R | fm (M each) | MF (S, through smap), at most two per lane; lZ with its log on lane 0 of wave 7.
      // Inputs: ttau | tnu | y | lZ, one per lane, carried in a register from the window that loads it to the next one, which stores it.
      static_assert((IH_KB & (IH_KB - 1)) == 0 && IH_KB >= 4, "the streamed ring masks the step index: the plan's depths are IH_KB, 8 and 4");
      const int KM = KB - 1;                               // (KB is 4, 8 or 16: at least 3 slots, a power of two)
      const bool io = (wave & 2) != 0;
      const int L = io ? ((((wave >> 2) << 1) | (wave & 1)) * 64 + (tid & 63)) : (1 << 20);
      const int n4 = 4 * M, nout = n4 + S;
      msp_rp o_l[2]; double* o_g[2]; int o_ls[2], o_gs[2]; bool o_on[2];
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const int j = L + 256 * t;
        o_on[t] = j < nout;
        const int jj = o_on[t] ? j : 0;
        if (jj < n4) {
          const int a = jj / M, i = jj - a * M;
          o_l[t] = (msp_rp)((a == 0 ? ld.rtt : a == 1 ? ld.rtn : a == 2 ? ld.rR : ld.rfm) + i);
          o_g[t] = (a == 0 ? gr.g_tt : a == 1 ? gr.g_tn : a == 2 ? gr.g_R : gr.g_fm) + (size_t)ip.k_start * M + i;
          o_ls[t] = M; o_gs[t] = M;
        } else {
          const int e = jj - n4;
          o_l[t] = (msp_rp)(ld.rMF + ld.smap[e]);
          o_g[t] = gr.g_MF + (size_t)ip.k_start * S + e;
          o_ls[t] = n4; o_gs[t] = S;
        }
      }
      const bool z_on = io && L == 192;
      double* z_g = gr.g_lZ + ip.k_start;
      const msp_rp z_r = (msp_rp)ld.rZ, z_l = (msp_rp)ld.rlZ;
      const bool i_on = L < 2 * M + 2, i_z = L == 2 * M + 1;
      msp_wp i_l = (msp_wp)ld.rtt; const double* i_g = gr.g_tt; int i_ls = M, i_gs = M;
      if (i_on) {
        if (L < M) { i_l = (msp_wp)(ld.rtt + L); i_g = gr.g_tt + (size_t)ip.k_start * M + L; }
        else if (L < 2 * M) { i_l = (msp_wp)(ld.rtn + (L - M)); i_g = gr.g_tn + (size_t)ip.k_start * M + (L - M); }
        else { i_l = (msp_wp)(L == 2 * M ? ld.ry : ld.rlZ); i_g = (L == 2 * M ? gr.yv : gr.g_lZ) + ip.k_start; i_ls = 1; i_gs = 1; }
      }
      const msp_wp i_rz = (msp_wp)ld.rZ;
      auto flush = [&](int s) __attribute__((always_inline)) {
#pragma unroll
        for (int t = 0; t < 2; ++t)
          if (o_on[t]) { *o_g[t] = o_l[t][s * o_ls[t]]; o_g[t] += o_gs[t]; }
        if (z_on) { const double z = z_r[s]; *z_g = (z < 0.0) ? z_l[s] : log(z); ++z_g; }
      };
      int64_t k = ip.k_start;
      double carry = 0.0;
      // prologue: the first step straight into its slot, the second into the register
      if (i_on && k < T) {
        const int s0 = (int)(k & KM);
        i_l[s0 * i_ls] = *i_g; i_g += i_gs;
        if (i_z) i_rz[s0] = -1.0;
        if (k + 1 < T) { carry = *i_g; i_g += i_gs; }
      }
      __syncthreads();
      // Workers 2 and 3 (waves 4, 5) share their SIMDs with the serial waves, which are the older waves there and win the vector issue
      // whenever both have an instruction ready.  Measured (profiles/r25_cfg3_early_inputs.txt, sections 2 and 3): with the priority their
      // bin sums take 60 - 90 cycles less and their wait at B5 grows by as much -- they are NOT the last waves at B4 or B5 (workers 4 and
      // 5 are) -- and the plain instantiation's execute is 0.6 - 0.8 % shorter, 1.5 % with the prediction's window; no stamped slot shows
      // why.  Raised once for the launch; between B5 and B2 these two workers are idle and the serial waves have the SIMD.
      // Whoever changes the worker loop or what the serial waves do between B2 and B5: repeat the two A/Bs that hold this line, with
      // inst_iha8k8 alone rebuilt (tools/ab_libs.sh, bench.py --workload cfg3 --steps 3 --warmup 1) -- the parent's step with the line
      // against without it, and this step with it against without it (the prediction's window loses 1.1 - 1.5 % without it).
      if (wave == MSR_W0 + 2 || wave == MSR_W0 + 3) __builtin_amdgcn_s_setprio(1);
      for (; k < T; ++k) {
        wstep((int)(k & KM));
        // the window B5(k) .. B2(k+1): store the inputs of step k+1, load those of step k+2 (ahead of the stores below: the wait for a
        // load then leaves the younger stores alone), flush step k-1
        if (io) {
          if (i_on) {
            if (k + 1 < T) { const int s1 = (int)((k + 1) & KM); i_l[s1 * i_ls] = carry; if (i_z) i_rz[s1] = -1.0; }
            if (k + 2 < T) { carry = *i_g; i_g += i_gs; }
          }
          if (k > ip.k_start) flush((int)((k - 1) & KM));
        }
        WK_STAMP(6);                   // (the ring's work of the window)
      }
      __syncthreads();
      if (io && T > ip.k_start) flush((int)((T - 1) & KM));
    }
    if (wk_stamp)
      for (int i = 0; i < 8; ++i) mc.stamps[wk_slot + i] += wk[i];
#undef WK_STAMP
    return;
  }
  // ================= serial role (waves 0 and 1)
  MsrS<CD> x;
  msr_setup_S<CD>(x, mc, sp, ld.fmu, ld.HPH, ld.ws, msr_desc_p_base());      // (the reduction reads the level-2 slots of the workers' copy of the lists)
  MsrQ<CD> xq;                                       // Q / 2Q / v on wave 0
  MsrRT rt;                                          // table words of the reduction, read ahead of B5
  msr_setup_Q<CD>(xq, mc, ld.sW, ld.fmu, ld.HPH, ld.ws);

  // The two serial waves run separate copies of the loop below (WT = 0, 1: the wave index is a constant of the copy), so that each
  // holds the registers of its own chain only -- wave 0 the W row and the operands of Q / 2Q / v, wave 1 the link chain's constants.
  // Wave 1's copy exists once per link kind (LK = 0, 1: msr_link_serial; LK = -1: the kind is read where it is used, msp_link).
  auto serial = [&](auto WV, auto LKV) __attribute__((always_inline)) {
  constexpr int WT = decltype(WV)::value, LK = decltype(LKV)::value;
  const int wave = WT;
  const int lane = tid & 63;
  IhLane ln;
  double wrow[CD];      // (WT = 0: the W row is read again every step, p_w below)
  ih_lane_setup<CD>(ln, ld, sh, b, ip, NG, wave, lane, wrow);
  const msp_rp p_w = (msp_rp)(ld.sW + (ln.sub ? ln.n : 0) * CD);      // WT = 0: this sub-band's row of W, beside the reads of the reduction
  unsigned long long st_a = 0, st_b = 0, st[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  const bool stamp = STAMPS && mc.stamps && tid == ((ip.dbg_wave & 32) ? 64 : 0);      // time line of wave 0 (NAGP_STAMP_WORKER & 32: of wave 1)
#define IH_STAMP(slot) do { if constexpr (STAMPS) if (stamp) { st_b = __builtin_readcyclecounter(); st[slot] += st_b - st_a; st_a = st_b; } } while (0)

  // the look-up's constants live in vector registers from here on, so that the loop reads no kernel argument again
  double lk_lr0 = tb.lr0, lk_inv = tb.inv_dlr, lk_rmax = ld.rmax;
  int lk_ng2 = NG - 2;
  asm volatile("" : "+v"(lk_lr0), "+v"(lk_inv), "+v"(lk_rmax), "+v"(lk_ng2));
  // the look-up from ttau (nagp_lookup.hpp): t_beyond, t_inf and the seed's two integers from the table behind the grid; the steps
  // themselves are in LDS (p_thr), and the lane's H PP H' of index 0 -- what a site with ttau <= t_inf (R = Inf) selects -- is a register
  double lk_tbey = tb.r[2 * NG - 1], lk_tinf = tb.r[2 * NG];
  unsigned int lk_c1 = (unsigned int)tb.r[2 * NG + 1]; int lk_c0 = (int)tb.r[2 * NG + 2];
  asm volatile("" : "+v"(lk_tbey), "+v"(lk_tinf), "+v"(lk_c1), "+v"(lk_c0));
  const msp_rp p_thr = (msp_rp)ld.tail + opaque_zero();
  const bool hph_in_lds = ip.hph_lds != 0;
  double lk_h0 = hph_in_lds ? ln.p_hph[0] : ln.g_hph[0];
  asm volatile("" : "+v"(lk_h0));

  // head of step k: table look-up, A m, the cubature's inputs (wave 0, no barrier).  IN_LOOP: k > 0 is known (the tables of k = 0 are the
  // prologue's).  The straight-line look-up (nagp_lookup.hpp) -- one branch, for finite R beyond the grid; the three grid words and,
  // with the H PP H' table in LDS, its three entries round the seed in ONE batch of LDS reads, the index selects among them.
  // Inside the loop the look-up is the site update's, from ttau (ih_thr_reads / ih_thr_pick): the head only takes its index and H PP H'.
  // The prologue's head (k_start > 0: R of step k_start - 1 from memory) seeds from R and picks among three grid words as before -- the
  // same index (tests/test_ihgp_lookup_thresholds_host.py).
  double hph = 0.0, wc[4] = {0, 0, 0, 0}, Am[4] = {0, 0, 0, 0}, fmun = 0.0;
  int w_mid = 1;
  double w_r0 = 0.0, w_r1 = 0.0, w_r2 = 0.0, w_h0 = 0.0, w_h1 = 0.0, w_h2 = 0.0;
  int w_idx = 0;
  auto head = [&](int64_t k, auto IN_LOOP) __attribute__((always_inline)) {
    if (ln.act) {
      if (decltype(IN_LOOP)::value || k > 0) {
        int idx;
        {
          if constexpr (!decltype(IN_LOOP)::value) {
            w_mid = lookup_mid(lk_ng2, lk_lr0, lk_inv, ln.Rprev);
            ih_window_reads(ln.p_rg, ln.p_hph, hph_in_lds, w_mid, w_r0, w_r1, w_r2, w_h0, w_h1, w_h2);
            ih_window_pick(w_mid, w_r0, w_r1, w_r2, w_h0, w_h1, w_h2, ln.p_rg, ln.p_hph, ln.g_hph, hph_in_lds, lk_rmax, lk_ng2 + 2, ln.Rprev, w_idx, hph);
          }
          idx = w_idx;      // (IN_LOOP: picked in the site update of the step before)
          if (stamp) { asm volatile("" :: "v"(idx), "v"(hph)); IH_STAMP(6); }
        }
        const double2* w = reinterpret_cast<const double2*>(ln.g_wcol + (size_t)idx * 4);
        const double2 w0 = w[0], w1 = w[1];
        wc[0] = w0.x; wc[1] = w0.y; wc[2] = w1.x; wc[3] = w1.y;
      } else {
        hph = ld.tab[itab_hph0(sh, NG) + ln.n];
        const double* w = ld.tab + itab_wcol0(sh, NG) + (size_t)ln.n * 4;
#pragma unroll
        for (int i = 0; i < 4; ++i) wc[i] = w[i];
      }
      if constexpr (!decltype(IN_LOOP)::value) {
        // the prologue forms A m and fmu directly; inside the loop both come from the prediction's operands (lambda step, below):
        // the step before has stored fmu straight behind its gain and holds A m in Am
        ih_a4_times(ln.A4, ln.mreg, Am);
        fmun = ln.hn * Am[0];
        *ln.p_fmu = fmun;
      }
      *ln.p_HPH = hph;
      if (stamp) { IH_STAMP(7); }
    }
  };
  if (stamp) st_a = __builtin_readcyclecounter();      // (the prologue's head stamps slots 6 / 7 as the loop's do)
  if (wave <= 1) head(ip.k_start, std::false_type{});
  // what the two chains below need of the kernel's arguments is in vector registers from here on, like the look-up's constants
  double ls_shift = mc.link_shift;
  int qv_dlim = mc.D - (lane & 1);                   // msr_qv_serial, padded forms
  const bool ls_on = tid - 64 * x.lw >= 0 && tid - 64 * x.lw < CD * mc.nd;      // this lane's part in the link tables (msp_link)
  asm volatile("" : "+v"(ls_shift), "+v"(qv_dlim));
  // the address of the reduced sums as ONE register holding the whole address, so that the paired reads of msp_outputs_b reach every
  // sum through their 8-bit offsets (with the region's constant offset left outside the register, each pair took an address addition)
  msp_rp accp = x.accp;
  asm volatile("" : "+v"(accp));
  // wave 0: the static products of the second-moment contraction (msp_outputs_b), CD (CD + 1) / 2 registers of this copy of the loop
  // for the whole launch (zero on a lane without a sub-band)
  // D <= 32: the outputs on both halves of wave 0 (msp_outputs_h) -- lane d + 32 holds sub-band d's products as well, each half keeps the
  // static coefficients of its own terms in those registers and reads its own words of the sums (accp_h).  Decided once per launch: by the
  // form of Q / 2Q / v where that fixes D (K4: 16, K8: 32, K16-pad: more than 32), otherwise a scalar the loop branches on.
  constexpr int HALF_CT = (QF == QF_K4 || QF == QF_K8) ? 1 : ((QF == QF_K16P) ? 0 : -1);
  int half_s = (D <= 32) ? 1 : 0;
  if constexpr (HALF_CT < 0) {      // (opaque, so that the loop does not read D from the kernel's arguments again; uniform by the read of the first lane)
    asm volatile("" : "+v"(half_s));
    half_s = __builtin_amdgcn_readfirstlane(half_s);
  }
  const bool half = (WT == 0) && ((HALF_CT >= 0) ? (HALF_CT == 1) : (half_s != 0));
  const bool upper = lane >= 32;
  msp_rp accp_h = accp;
  double pw[(WT == 0) ? CD * (CD + 1) / 2 : 1] = {0.0};
  if constexpr (WT == 0) {
    if (half) {
      const int hd = lane & 31;
      double wh[CD];
#pragma unroll
      for (int j = 0; j < CD; ++j) wh[j] = (hd < D) ? ld.sW[hd * CD + j] : 0.0;
      msp_wproducts<CD>(wh, (ip.dbg_wave & 64) != 0, pw);
      msp_half_coeffs<CD>(wh, upper, pw);
      accp_h = accp + (upper ? msp_half_terms<CD>() : 0);
    } else {
      msp_wproducts<CD>(wrow, (ip.dbg_wave & 64) != 0, pw);
    }
#pragma unroll
    for (int q = 0; q < CD * (CD + 1) / 2; ++q) asm volatile("" : "+v"(pw[q]));
    asm volatile("" : "+v"(accp_h));
  }
  // the cubature's inputs of a step straight behind its head, each from this wave's own fmu / HPH stores (msp_wave_fence)
  auto qv_or_link = [&]() __attribute__((always_inline)) {
    msp_wave_fence();
    if (wave == 0) msr_qv_serial<CD, QF>(xq, mc, qv_dlim);
    else if constexpr (LK >= 0) msr_link_serial<CD, LK>(x, ls_on, ls_shift);
    else msp_link<CD>(x, mc);
  };
  qv_or_link();
  if (stamp) st_a = __builtin_readcyclecounter();

  // one step between its barriers; kk = the step's ring slot
  auto step = [&](const int64_t k, const int kk) __attribute__((always_inline)) {
      lds_barrier();                 // B2 (Q / 2Q / v and the link tables of step k, written by waves 0 and 1 on their way here)
      IH_STAMP(0);
      {
        if (wave == 1) msr_etable<CD>(x, mc);      // read behind B4 only (level 2 of msr_sums): beside the workers' weights
      }
      // (Gaussian weights: worker waves)
      lds_barrier();                 // B4
      IH_STAMP(1);
      // (bin sums: worker waves)
      // What the serial tail needs and what exists ahead of B5 is read here, while the workers form the bin sums -- the site's ttau and
      // tnu of the ring slot (in place since B2, next written by this lane), wave 0's row of W (static), and the link-table words of the
      // reduction (no reader of the tables is left behind B5).  Every lane reads: the addresses of idle lanes are those of site 0.
      const int ko = kk * M;
      double wr[CD], t_old = 0.0, n_old = 0.0;
      {
        t_old = ln.p_tt[ko]; n_old = ln.p_tn[ko];
#pragma unroll
        for (int j = 0; j < CD; ++j) wr[j] = (WT == 0 && !half) ? p_w[j] : 0.0;      // (2 CD registers of wave 0's copy, free again behind the outputs; the half-wave form holds the row among its coefficients)
        msr_reduce_tab<CD>(x, rt);
      }
      // The prediction's operands, formed here where the serial waves wait for the bin sums: with m_k = A m_{k-1} + wc g the next
      // prediction is A m_k = A (A m_{k-1}) + (A wc) g, and both products are known since the head of this step (wc: its load has long
      // returned).  P1 = A Am, P2 = A wc, pa = h P1[0], pb = h P2[0]: behind the gain, fmu of step k+1 is ONE fma (pb, g, pa), and
      // A m_k = fma(P2, g, P1) follows off the chain.  Pinned ahead of B5, so that none of it is scheduled into the tail.
      double P1[4], P2[4], pa, pb;
      ih_a4_times(ln.A4, Am, P1);
      ih_a4_times(ln.A4, wc, P2);
      pa = ln.hn * P1[0]; pb = ln.hn * P2[0];
#pragma unroll
      for (int i = 0; i < 4; ++i) asm volatile("" : "+v"(P1[i]), "+v"(P2[i]));
      asm volatile("" : "+v"(pa), "+v"(pb));
      lds_barrier();                 // B5
      IH_STAMP(2);
      {
        msr_reduce_bins<CD>(x, rt);
        msp_wave_fence();
        double Z = 0.0, d1 = 0.0, d2 = 0.0;
        if constexpr (WT == 0) {
          if (half) msp_outputs_h<CD>(accp, accp_h, pw, upper, ld.pEP1, mc.jitter, Z, d1, d2);      // every lane of the wave: the swap reads the upper half
        }
        if (ln.act) {
          if (!(WT == 0 && half)) msp_outputs_b<CD, WT == 0>(accp, ln.n - D, wr, pw, ld.pEP1, mc.jitter, Z, d1, d2);
          if (stamp) { asm volatile("" :: "v"(d2)); IH_STAMP(4); }
          // site update (:265-266): -d2/(1+d2 HPH), (d1 - fmu d2)/(1+d2 HPH) through one reciprocal
          const double r1 = rcp_nr(fma(d2, hph, 1.0));
          double tnew = fma(ip.w_new, -d2 * r1, ip.w_old * t_old);
          const double nnew = fma(ip.w_new, fma(-fmun, d2, d1) * r1, ip.w_old * n_old);
          if (!(tnew > 0.0)) ++ln.n_clamped;
          tnew = max0(tnew);                                               // :274 (NaN -> 0, C-3)
          {                                                                // beside the division; ahead of the ring stores
            w_mid = lookup_mid_bits(lk_ng2, lk_c1, lk_c0, tnew);
            ih_thr_reads(p_thr, ln.p_hph, hph_in_lds, w_mid, w_r0, w_r1, w_h0, w_h1, w_h2);
          }
          double Rn = 1.0 / tnew;                                          // R = 1/ttau, exact division: an output (ring, Rprev) and the key of the
          // side path beyond the grid; neither the gain nor the straight look-up waits for it
          // (for tnew > 0 the reference's R(:,k) = 1./ttau before the clamp is this value; otherwise :287 overwrites it with Inf)
          // R = inf: ttau = 0, or ttau of underflow size (1/ttau overflows while ys = tnu/ttau stays finite): the reference's
          // (ys - fmu)/(HPH + R) is 0 there.  ttau <= t_inf says the same as R = inf (lookup_thresholds finds t_inf with this division)
          double g = 0.0;                                                  // (ys - fmu)/(HPH + R), ys = tnu/ttau (:277, :289-292), both sides
          {                                                                // times ttau: (tnu - fmu ttau)/(1 + HPH ttau)
            double gx = fma(-fmun, tnew, nnew) * rcp_nr(fma(hph, tnew, 1.0));
            asm volatile("" : "+v"(gx));                                   // by a select: clamped sites are every-step business
            g = (tnew > lk_tinf) ? gx : 0.0;
          }
          typedef double d2v __attribute__((ext_vector_type(2)));
          d2v m01, m23;
          // fmu of step k+1: one fma behind the gain, and its store ahead of everything else that reads g (at k + 1 == T the store has
          // no reader: the word is the lane's own).  The mean of this step -- for the ring only -- and A m of the next follow.
          fmun = fma(pb, g, pa);
          *ln.p_fmu = fmun;
          asm volatile("" : "+v"(g));
#pragma unroll
          for (int i = 0; i < 4; ++i) { ln.mreg[i] = fma(wc[i], g, Am[i]); Am[i] = fma(P2[i], g, P1[i]); }
          m01.x = ln.mreg[0]; m01.y = ln.mreg[1]; m23.x = ln.mreg[2]; m23.y = ln.mreg[3];
          // the look-up of step k+1 from the window read above: ahead of the ring stores, so that the wait for the window takes no store
          // with it, and behind the gain in program order, so that the window's reads have the division and the gain's chain to return in
          ih_thr_pick(w_mid, w_r0, w_r1, w_h0, w_h1, w_h2, lk_h0, ln.p_rg, ln.p_hph, ln.g_hph, hph_in_lds, lk_tbey, lk_tinf, lk_ng2 + 2, tnew, Rn, w_idx, hph);
          ln.p_tt[ko] = tnew; ln.p_tn[ko] = nnew; ln.p_R[ko] = Rn;
          typedef d2v __attribute__((address_space(3))) * lds_d2p;
          lds_d2p mf = (lds_d2p)(ln.p_MF + 4 * ko);
          mf[0] = m01; mf[1] = m23;
          ln.p_fm[ko] = ln.hn * ln.mreg[0];
          ln.Rprev = Rn;
          if (ln.n == 0) ld.rZ[kk] = Z;
          if (stamp) { asm volatile("" :: "v"(ln.Rprev)); IH_STAMP(5); }
        }
        if (k + 1 < T) {
          head(k + 1, std::true_type{});
          qv_or_link(); IH_STAMP(3);      // (slot 3: Q / 2Q / v on wave 0, the link tables on wave 1)
        }
      }
  };
  {
    // the streamed ring: the I/O lanes of the worker role fill and flush it; the serial waves only index it by the step's slot
    __syncthreads();                 // the first step's inputs (prologue of the I/O lanes)
    for (int64_t k = ip.k_start; k < T; ++k) step(k, (int)(k & (KB - 1)));
    __syncthreads();                 // the last step's outputs, flushed by the I/O lanes
  }
#undef IH_STAMP
  ih_lane_end(ln, b);
  if (stamp)
    for (int i = 0; i < 8; ++i) mc.stamps[i] += st[i];
  };
  {
    using std::integral_constant;
    if (wave == 0) serial(integral_constant<int, 0>{}, integral_constant<int, -1>{});
    else if (mc.link_kind == 0) serial(integral_constant<int, 1>{}, integral_constant<int, 0>{});      // (link_eval: 0 softplus, else exp)
    else serial(integral_constant<int, 1>{}, integral_constant<int, 1>{});
  }
}

// The role-specialised sweep with barrier B1 and the block ring (fill, KB steps, flush by the whole workgroup round two __syncthreads):
// what ihgp_adf8_kernel does not serve.  TAB = false, CD = 7 (the 2 x 35 outputs of Q / 2Q / v do not fit the lanes of wave 0): FOUR
// barriers, B1 | Q / 2Q / v (workers 0..2), link tables (wave 1) | B2 | weights straight from Q, v and the link tables
// (msr_stage1b_direct); e table (wave 1) | B4 | bin sums | B5 | msr_reduce, serial tail, head of step k+1.  TAB = true, CD = 1 .. 7
// (developer switch NAGP_IH_TABLES=1, the form of the four-wave kernel, the in-build cross-check): B1 as above; behind B2 the tables
// e / t1 / ve on wave 1 and q0 / s0 on workers 3 and 4, one more barrier (B3), then the weights from those tables (msp_stage1b).
// One copy of the serial loop serves both serial waves; the stamps test the pointer.
template <int CD, bool TAB>
__global__ void __launch_bounds__(MSR_NT) ihgp_adf8b_kernel(Shape sh, Bufs b, MomCfg mc, MomSp sp, IhgpTabs tb, IhgpPar ip) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  constexpr int NT = MSR_NT;
  const int S = sh.S, M = sh.M, D = sh.D, KB = ip.kb;
  const int64_t T = sh.T;
  IhLds L;
  ih_lds_setup(L, lds, sh, b, mc, tb, ip, CD, 0, tid, NT);
  IhRows G;                                          // (both roles fill and flush the ring)
  ih_rows(G, sh, b);
  msr_init(CD, D, L.ws);
  __syncthreads();
  if (wave >= MSR_W0) {
    // ================= worker role: the parallel stages of the cubature; the same barriers as the serial role below
    const MspLay lay = msp_layout(CD, D, 1);
    MsrW<CD> xw;
    msr_setup_W<CD>(xw, mc, sp, L.sW, L.fmu, L.HPH, L.ws, true);
    // developer diagnostics (NAGP_STAMPS): time lines of worker (NAGP_STAMP_WORKER & 7) in stamps[8..15] and of the last worker in
    // stamps[16..23]
    const int wk_slot = (wave == MSR_W0 + (ip.dbg_wave & 7)) ? 8 : ((wave == MSR_W0 + MSR_NWK - 1) ? 16 : -1);
    IhSt wk;
    ih_st_start(wk, mc.stamps && wk_slot >= 0 && (tid & 63) == 0);
    for (int64_t k0 = ip.k_start; k0 < T; k0 += KB) {
      const int nb = (T - k0 < KB) ? (int)(T - k0) : KB;
      ih_ring_fill(L, G, k0, nb, M, tid, NT);
      ih_stamp(wk, 6);                 // (the ring section: from B5 of a block's last step through the flush and the next fill)
      for (int kk = 0; kk < nb; ++kk) {
        lds_barrier();                 // B1
        ih_stamp(wk, 0);               // (wait at B1: the serial waves' tail and head)
        msp_qv<CD>(xw, mc);            // workers 0..2
        ih_stamp(wk, 1);
        lds_barrier();                 // B2
        if constexpr (TAB) {
          if (wave == MSR_W0 + 3 || wave == MSR_W0 + 4) msr_q0_or_s0(xw, wave == MSR_W0 + 3, L.ws + lay.q0, L.ws + lay.s0);
          lds_barrier();                 // B3
          ih_stamp(wk, 2);               // (B2 .. B3: tables on wave 1, q0 / s0 on workers 3, 4)
          msp_stage1b<CD>(xw, mc, sp, L.sn2a, L.ry[kk], L.ws);
        } else {
          ih_stamp(wk, 2);               // (wait at B2: wave 1's link tables)
          msr_stage1b_direct<CD, false>(xw, L.sn2a, L.ry[kk]);
        }
        ih_stamp(wk, 3);
        lds_barrier();                 // B4
        ih_stamp(wk, 4);
        msr_sums(xw);                  // bin sums, then this wave's share of the 40 sums
        ih_stamp(wk, 5);
        lds_barrier();                 // B5
        ih_stamp(wk, 7);
      }
      ih_ring_flush(L, G, k0, nb, M, S, tid, NT);
    }
    if (wk.on) ih_st_store(wk, mc.stamps + wk_slot);
    return;
  }
  // ================= serial role (waves 0 and 1): one copy of the loop serves both
  MsrS<CD> x;
  msr_setup_S<CD>(x, mc, sp, L.fmu, L.HPH, L.ws);
  IhLane ln;
  double wrow[CD];
  ih_lane_setup<CD>(ln, L, sh, b, ip, tb.NG, wave, tid & 63, wrow);
  IhSt st;                                           // time line of wave 0 (NAGP_STAMP_WORKER & 32: of wave 1)
  ih_st_start(st, mc.stamps && tid == ((ip.dbg_wave & 32) ? 64 : 0));      // (the prologue's head stamps slots 6 / 7 as the loop's do)
  IhHead h = {0.0, {0, 0, 0, 0}, {0, 0, 0, 0}, 0.0};
  ih_head(ln, h, ip.k_start > 0, sh, tb, L, ip, st);
  if (st.on) st.a = __builtin_readcyclecounter();

  for (int64_t k0 = ip.k_start; k0 < T; k0 += KB) {
    const int nb = (T - k0 < KB) ? (int)(T - k0) : KB;
    ih_ring_fill(L, G, k0, nb, M, tid, NT);
    for (int kk = 0; kk < nb; ++kk) {
      lds_barrier();                 // B1: fmu, HPH of step k
      ih_stamp(st, 3);
      // (Q / 2Q / v: worker waves)
      // link tables of the step (the exp / log chain of the modulators' sigma-point coordinates, ~1 000 cycles on wave 1): behind B1, beside
      // the workers' Q / 2Q / v -- nothing reads them before the stages behind B2 (ahead of B1 they were the tail of the serial chain)
      if (wave == 1) msp_link<CD>(x, mc);
      lds_barrier();                 // B2
      ih_stamp(st, 0);
      if constexpr (TAB) {
        if (wave == 1) msp_tables<CD>(x, mc);
        lds_barrier();                 // B3
      } else {
        if (wave == 1) msr_etable<CD>(x, mc);      // read behind B4 only (level 2 of msr_sums): beside the workers' weights
      }
      // (Gaussian weights: worker waves)
      lds_barrier();                 // B4
      ih_stamp(st, 1);
      // (bin sums: worker waves)
      lds_barrier();                 // B5
      ih_stamp(st, 2);
      msr_reduce<CD>(x);
      msp_wave_fence();
      if (ln.act) {
        double Z, d1, d2;
        msp_outputs<CD>(x.accp, ln.sub, ln.n - D, wrow, L.pEP1, mc.jitter, Z, d1, d2);
        ih_site_update(ln, h, ip, L, kk, M, Z, d1, d2, st);
      }
      if (k0 + kk + 1 < T) ih_head(ln, h, true, sh, tb, L, ip, st);
    }
    ih_ring_flush(L, G, k0, nb, M, S, tid, NT);
  }
  ih_lane_end(ln, b);
  ih_st_store(st, mc.stamps);
}

// The role-specialised sweep for likModulatorPreCalcwn (experiments/likModulatorPreCalcwn.m:28-86; nagp_momsq.hpp): 512 threads, waves
// 0 / 1 carry the sites exactly as in ihgp_adf8_kernel, waves 2 .. MSQ_NWK + 1 the staged cubature of the square-root amplitudes.  sp.c0 = code of
// the centre coordinate.  D <= 32 sub-bands, <= 6 components, <= 336 sigma points (the host checks).
struct MsqS { int lw; double xdc; msp_rp a_mu, a_s2; msp_wp a_out; msp_rp accp, partp; };
__host__ __device__ inline size_t ihgp_adf8sq_lds_doubles(const Shape& s, int CD, int NG, int hph_lds, int kb) {
  return ihgp_adf_lds_doubles(s, CD, NG, hph_lds, kb) - msp_lds_doubles(CD, s.D) + msq_lds_doubles<MsqRole>(CD) + 512;
}
template <int CD>
__global__ void __launch_bounds__(MSQ_NT) ihgp_adf8sq_kernel(Shape sh, Bufs b, MomCfg mc, MomSp sp, IhgpTabs tb, IhgpPar ip) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  constexpr int NT = MSQ_NT;
  const int S = sh.S, M = sh.M, D = sh.D, KB = ip.kb;
  const int64_t T = sh.T;
  IhLds L;
  ih_lds_setup(L, lds, sh, b, mc, tb, ip, CD, 512, tid, NT);      // tail: [8][64] W transposed for t = W' s2 (stage A)
  IhRows G;                                          // (both roles fill and flush the ring)
  ih_rows(G, sh, b);
  msq_init<MsqRole>(CD, L.ws, NT);
  __syncthreads();
  const MsqLay lay = msq_layout<MsqRole>(CD);
  if (wave >= MSR_W0) {
    // ================= worker role: the parallel stages of the cubature; the same barriers as the serial role below
    MsqW<CD, MsqRole> xw;
    msq_setup_W<CD, MsqRole>(xw, mc, sp.c0, L.sW, L.fmu, L.HPH, L.ws, wave - MSR_W0, tid - 64 * MSR_W0, L.tail);
    double amp[2 * MsqRole::NST];
#pragma unroll
    for (int i = 0; i < 2 * MsqRole::NST; ++i) amp[i] = 0.0;
    // developer diagnostics (NAGP_STAMPS): time lines of worker 0 in stamps[8..15] and of the last worker (marginal sums) in stamps[16..23]
    const int wk_slot = (wave == MSR_W0 + (ip.dbg_wave & 7)) ? 8 : ((wave == MSR_W0 + MSQ_NWK - 1) ? 16 : -1);
    IhSt wk;
    ih_st_start(wk, mc.stamps && wk_slot >= 0 && (tid & 63) == 0);
    for (int64_t k0 = ip.k_start; k0 < T; k0 += KB) {
      const int nb = (T - k0 < KB) ? (int)(T - k0) : KB;
      ih_ring_fill(L, G, k0, nb, M, tid, NT);
      for (int kk = 0; kk < nb; ++kk) {
        lds_barrier();                 // B1
        ih_stamp(wk, 0);               // (wait at B1: the serial waves' tail and head)
        msq_stageA<CD, MsqRole>(xw);            // worker 0: t = W' s2_z
        ih_stamp(wk, 1);
        lds_barrier();                 // B2: link tables (wave 1)
        msq_stageS<CD, MsqRole>(xw, amp);       // gather, square roots, mu_p
        ih_stamp(wk, 2);
        lds_barrier();                 // B3
        msq_stage1b<CD, MsqRole>(xw, L.sn2a, L.ry[kk]);
        ih_stamp(wk, 3);
        lds_barrier();                 // B4
        ih_stamp(wk, 4);
        ih_stamp(wk, 5);
        msq_stageS2<CD, MsqRole>(xw, amp);
        ih_stamp(wk, 6);
        lds_barrier();                 // B5
        ih_stamp(wk, 7);
      }
      ih_ring_flush(L, G, k0, nb, M, S, tid, NT);
    }
    if (wk.on) ih_st_store(wk, mc.stamps + wk_slot);
    return;
  }
  // ================= serial role (waves 0 and 1)
  MsqS x;
  {
    const int nd = mc.nd, TN = CD * nd, tl = tid - 64;
    const int t = (tl >= 0 && tl < TN) ? tl : 0;
    const int j = t / nd, cc = t - j * nd;
    x.lw = 1; x.xdc = mc.xd[cc];
    x.a_mu = (msp_rp)(L.fmu + D + j); x.a_s2 = (msp_rp)(L.HPH + D + j);
    x.a_out = (msp_wp)(L.ws + t);
    x.accp = (msp_rp)(L.ws + lay.acc + ((wave == 1) ? 32 : 0)) + opaque_zero();
    const int dl = tid & 63;
    x.partp = (msp_rp)(L.ws + lay.part + (dl & 15) + 16 * ((dl >> 4) & 1));
  }
  MsqM xm;      // marginal sums of c0 -> g1, g2, Z: the serial waves, idle between B4 and B5, take half of the dimensions each
  msq_setup_M<CD, MsqRole>(xm, mc, sp.c0, L.ws, wave);

  IhLane ln;
  ih_lane_setup<0>(ln, L, sh, b, ip, tb.NG, wave, tid & 63, nullptr);
  IhSt st;                                           // time line of wave 0 (NAGP_STAMP_WORKER & 32: of wave 1)
  ih_st_start(st, mc.stamps && tid == ((ip.dbg_wave & 32) ? 64 : 0));
  IhHead h = {0.0, {0, 0, 0, 0}, {0, 0, 0, 0}, 0.0};
  ih_head(ln, h, ip.k_start > 0, sh, tb, L, ip, st);
  if (st.on) st.a = __builtin_readcyclecounter();

  for (int64_t k0 = ip.k_start; k0 < T; k0 += KB) {
    const int nb = (T - k0 < KB) ? (int)(T - k0) : KB;
    ih_ring_fill(L, G, k0, nb, M, tid, NT);
    for (int kk = 0; kk < nb; ++kk) {
      lds_barrier();                 // B1: fmu, HPH of step k
      ih_stamp(st, 3);
      // (t = W' s2_z: worker 0)
      // link tables of the step (the exp / log chain of the modulators' sigma-point coordinates, ~1 000 cycles on wave 1): behind B1, beside
      // the workers' stage A -- nothing reads them before the stages behind B2 (ahead of B1 they were the tail of the serial chain)
      if (wave == 1) msp_link<CD>(x, mc);
      lds_barrier();                 // B2
      ih_stamp(st, 0);
      // (gather, square roots, mu_p: worker waves)
      lds_barrier();                 // B3
      // (Gaussian weights: worker waves)
      lds_barrier();                 // B4
      ih_stamp(st, 1);
      msq_marginals<CD, MsqRole>(xm);         // (sum c1 a, sum c2 a^2: worker waves)
      lds_barrier();                 // B5
      ih_stamp(st, 2);
      if (ln.act) {
        double Z, d1, d2;
        msq_outputs<CD, MsqRole>(x.accp, x.partp, ln.sub, ln.n - D, L.pEP1, mc.jitter, Z, d1, d2);
        ih_site_update(ln, h, ip, L, kk, M, Z, d1, d2, st);
      }
      if (k0 + kk + 1 < T) ih_head(ln, h, true, sh, tb, L, ip, st);
    }
    ih_ring_flush(L, G, k0, nb, M, S, tid, NT);
  }
  ih_lane_end(ln, b);
  ih_st_store(st, mc.stamps);
}

// Backward mean recursion: m <- MF_k + G (m - A MF_k) with (P,G) looked up from R(:,k)
// (Inf -> last grid row, ihgp_ep_modulator_nmf.m:379-380).  One wave per problem, thread n = block n.
template <int BS>
static __global__ void __launch_bounds__(64) ihgp_scan_kernel(Shape sh, Bufs b, IhgpTabs tb, double* vprev /* [B][M] */) {
  const int n = threadIdx.x, pb = blockIdx.x;
  const int S = sh.S, M = sh.M, NG = tb.NG;
  const int64_t T = sh.T;
  const double* mdl = b.model + (size_t)pb * mdl_size(sh);
  const double* tab = tb.base + (size_t)pb * itab_size(sh, NG);
  double mxM = 0.0, mxP = 0.0;
  if (n < M) {
    double A4[BS * BS], mreg[BS];
#pragma unroll
    for (int i = 0; i < BS; ++i) mreg[i] = 0.0;
#pragma unroll
    for (int e = 0; e < BS * BS; ++e) A4[e] = mdl[mdl_A(sh) + (size_t)n * BS * BS + e];
    const double hn = mdl[mdl_h(sh) + n];
    const int o = sh.off[n], bs = sh.bsz[n];
    const double* g_MF = b.MF + (size_t)pb * T * S;
    double* g_MS = b.MS + (size_t)pb * T * S;
    const double* g_R = b.R + (size_t)pb * T * M;
    double* g_sm = b.sm + (size_t)pb * T * M;
    double* g_sv = b.sv + (size_t)pb * T * M;
    #pragma unroll
    for (int i = 0; i < BS; ++i) if (i < bs) { mreg[i] = g_MF[(size_t)(T - 1) * S + o + i]; g_MS[(size_t)(T - 1) * S + o + i] = mreg[i]; }
    double vlast = 0.0;   // P = zeros(size(A)) before the loop (:364)
    for (int64_t k = T - 2; k >= 0; --k) {
      const double Rk = g_R[(size_t)k * M + n];
      int idx = nearest_idx(tb, Rk);
      if (isinf(Rk)) idx = NG - 1;
      double G4[BS * BS], mf[BS], d[BS];
#pragma unroll
      for (int i = 0; i < BS; ++i) mf[i] = 0.0;
#pragma unroll
      for (int e = 0; e < BS * BS; ++e) G4[e] = tab[itab_g(sh, NG) + ((size_t)n * NG + idx) * BS * BS + e];
      vlast = tab[itab_v(sh, NG) + (size_t)n * NG + idx];
      #pragma unroll
      for (int i = 0; i < BS; ++i) if (i < bs) mf[i] = g_MF[(size_t)k * S + o + i];
#pragma unroll
      for (int i = 0; i < BS; ++i) {
        double a = mreg[i];
#pragma unroll
        for (int l = 0; l < BS; ++l) a = fma(-A4[BS * i + l], mf[l], a);
        d[i] = a;
      }
#pragma unroll
      for (int i = 0; i < BS; ++i) {
        double a = mf[i];
#pragma unroll
        for (int l = 0; l < BS; ++l) a = fma(G4[BS * i + l], d[l], a);
        mreg[i] = a;
      }
      #pragma unroll
      for (int i = 0; i < BS; ++i) if (i < bs) g_MS[(size_t)k * S + o + i] = mreg[i];
      const double mnew = hn * mreg[0];
      if (md_counts(b, pb, T, k)) mxM = fmax(mxM, fabs(g_sm[(size_t)k * M + n] - mnew));
      g_sm[(size_t)k * M + n] = mnew;
      g_sv[(size_t)k * M + n] = vlast;
    }
    // maxDiffP = max|H*PSP*H' - H*P*H'| with P = the last looked-up blocks (k = 0)
    mxP = fabs(vprev[(size_t)pb * M + n] - vlast);
    vprev[(size_t)pb * M + n] = vlast;
  }
  mxM = wave_max(mxM);
  mxP = wave_max(mxP);
  if (n == 0) { b.red[(size_t)pb * 8 + 1] = mxM; b.red[(size_t)pb * 8 + 2] = mxP; }
}


// ---------------------------------------------------------------------------------------------
// Parallel-in-time form of the two mean recursions that involve no `mom` call:
//   forward  (filter of sweeps >= 2, ihgp_ep_modulator_nmf.m:280-304 with fixed sites):
//            m_k = (A - K h A(1,:)) m_{k-1} + K ys          (or A m_{k-1} for clamped sites)
//   backward (smoother, :391):  m_k = MF_k + G_k (m_{k+1} - A MF_k)
// Both are affine maps x -> F x + g per diagonal block with F, g computable from stored arrays, so the
// sequence is cut into spans: compose (one thread per span and block), boundary (sequential over the
// spans, one thread per block), apply (replay inside the span, write outputs).
struct AffPar {
  int mode;        // 0 forward filter over k = 0 .. kend-1 ; 1 backward smoother over k = kend-1 .. 0
  int64_t kend;    // number of steps covered
  int L;           // span length
  int ns;          // spans
  double* spanbuf; // [B][ns][M][BS*BS + BS]  Phi + c   (BS = Shape::BS: 4, or 8 for blocks of 5 .. 8 states)
  double* bnd;     // [B][ns][M][BS]   value entering the span
  double* vprev;   // [B][M] (smoother: previous sweep's marginal variance at k = 0)
};

// coefficients of step k for block n: x_new = F x + g
template <int MODE, int BS = 4>
__device__ __forceinline__ void ihgp_coeffs(const Shape& sh, const Bufs& b, const IhgpTabs& tb, const double* tab,
                                            const double* A4, double hn, int n, int pb, int64_t k, int bs, int o,
                                            double* F, double* g, double& aux) {
  const int M = sh.M, NG = tb.NG;
  const int64_t T = sh.T;
  const size_t ix = ((size_t)pb * T + k) * M + n;
  if (MODE == 0) {
    const double tt = max0(b.ttau[ix]);
    if (tt == 0.0) {
#pragma unroll
      for (int e = 0; e < BS * BS; ++e) F[e] = A4[e];
#pragma unroll
      for (int i = 0; i < BS; ++i) g[i] = 0.0;
      aux = INFINITY;                       // R(n,k) = inf
    } else {
      const double Rk = b.R[ix];
      double hph, wc[BS];
      if (k > 0) {
        const double tprev = max0(b.ttau[ix - M]);
        const double Rprev = (tprev == 0.0) ? INFINITY : b.R[ix - M];
        const int idx = nearest_idx(tb, Rprev);
        hph = tab[itab_hph(sh, NG) + (size_t)n * NG + idx];
        const double* w = tab + itab_wcol(sh, NG) + ((size_t)n * NG + idx) * BS;
#pragma unroll
        for (int i = 0; i < BS; ++i) wc[i] = w[i];
      } else {
        hph = tab[itab_hph0(sh, NG) + n];
        const double* w = tab + itab_wcol0(sh, NG) + (size_t)n * BS;
#pragma unroll
        for (int i = 0; i < BS; ++i) wc[i] = w[i];
      }
      const double den = hph + Rk;
      const double ys = b.tnu[ix] / tt;
#pragma unroll
      for (int i = 0; i < BS; ++i) {
        const double Ki = wc[i] / den;
        g[i] = Ki * ys;
#pragma unroll
        for (int j = 0; j < BS; ++j) F[BS * i + j] = A4[BS * i + j] - Ki * hn * A4[j];
      }
      aux = Rk;
    }
  } else {
    const double Rk = b.R[ix];
    int idx = nearest_idx(tb, Rk);
    if (isinf(Rk)) idx = NG - 1;
#pragma unroll
    for (int e = 0; e < BS * BS; ++e) F[e] = tab[itab_g(sh, NG) + ((size_t)n * NG + idx) * BS * BS + e];
    aux = tab[itab_v(sh, NG) + (size_t)n * NG + idx];
    double mf[BS], amf[BS];
#pragma unroll
    for (int i = 0; i < BS; ++i) mf[i] = 0.0;
    const double* mfp = b.MF + ((size_t)pb * T + k) * sh.S + o;
#pragma unroll
    for (int i = 0; i < BS; ++i)
      if (i < bs) mf[i] = mfp[i];
#pragma unroll
    for (int i = 0; i < BS; ++i) {
      double a = 0.0;
#pragma unroll
      for (int l = 0; l < BS; ++l) a = fma(A4[BS * i + l], mf[l], a);
      amf[i] = a;
    }
#pragma unroll
    for (int i = 0; i < BS; ++i) {
      double a = mf[i];
#pragma unroll
      for (int l = 0; l < BS; ++l) a = fma(-F[BS * i + l], amf[l], a);
      g[i] = a;
    }
  }
}

// span j covers recursion steps [j*L, min((j+1)L, kend)) counted in recursion order; k = that index
// (forward) or kend-1-index (backward).
template <int MODE, int BS = 4>
__global__ void __launch_bounds__(256) ihgp_aff_compose_kernel(Shape sh, Bufs b, IhgpTabs tb, AffPar ap) {
  const int pb = blockIdx.y, M = sh.M;
  const int gid = blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= ap.ns * M) return;
  const int j = gid / M, n = gid - j * M;
  const double* mdl = b.model + (size_t)pb * mdl_size(sh);
  const double* tab = tb.base + (size_t)pb * itab_size(sh, tb.NG);
  double A4[BS * BS];
#pragma unroll
  for (int e = 0; e < BS * BS; ++e) A4[e] = mdl[mdl_A(sh) + (size_t)n * BS * BS + e];
  const double hn = mdl[mdl_h(sh) + n];
  const int bs = sh.bsz[n], o = sh.off[n];
  double Phi[BS * BS], c[BS];
#pragma unroll
  for (int e = 0; e < BS * BS; ++e) Phi[e] = ((e % BS) == (e / BS)) ? 1.0 : 0.0;
#pragma unroll
  for (int i = 0; i < BS; ++i) c[i] = 0.0;
  const int64_t s0 = (int64_t)j * ap.L, s1 = (s0 + ap.L < ap.kend) ? s0 + ap.L : ap.kend;
  for (int64_t s = s0; s < s1; ++s) {
    const int64_t k = (MODE == 0) ? s : (ap.kend - 1 - s);
    double F[BS * BS], g[BS], aux;
    ihgp_coeffs<MODE, BS>(sh, b, tb, tab, A4, hn, n, pb, k, bs, o, F, g, aux);
    double P2[BS * BS], c2[BS];
#pragma unroll
    for (int i = 0; i < BS; ++i) {
      double a = g[i];
#pragma unroll
      for (int l = 0; l < BS; ++l) a = fma(F[BS * i + l], c[l], a);
      c2[i] = a;
#pragma unroll
      for (int jj = 0; jj < BS; ++jj) {
        double q = 0.0;
#pragma unroll
        for (int l = 0; l < BS; ++l) q = fma(F[BS * i + l], Phi[BS * l + jj], q);
        P2[BS * i + jj] = q;
      }
    }
#pragma unroll
    for (int e = 0; e < BS * BS; ++e) Phi[e] = P2[e];
#pragma unroll
    for (int i = 0; i < BS; ++i) c[i] = c2[i];
  }
  double* out = ap.spanbuf + (((size_t)pb * ap.ns + j) * M + n) * (BS * BS + BS);
#pragma unroll
  for (int e = 0; e < BS * BS; ++e) out[e] = Phi[e];
#pragma unroll
  for (int i = 0; i < BS; ++i) out[BS * BS + i] = c[i];
}

template <int MODE, int BS = 4>
__global__ void __launch_bounds__(64) ihgp_aff_boundary_kernel(Shape sh, Bufs b, AffPar ap, int itt) {
  const int n = threadIdx.x, pb = blockIdx.x, M = sh.M, S = sh.S;
  const int64_t T = sh.T;
  if (n >= M) return;
  const int bs = sh.bsz[n], o = sh.off[n];
  double x[BS];
#pragma unroll
  for (int i = 0; i < BS; ++i) x[i] = 0.0;
  if (MODE == 0) {            // filter of sweep itt >= 2 starts from the smoothed mean at k = 0 (SURVEY C-22)
    if (itt > 1)
#pragma unroll
      for (int i = 0; i < BS; ++i) if (i < bs) x[i] = b.MS[(size_t)pb * T * S + o + i];
  } else {                    // smoother starts from the last filtered mean
#pragma unroll
    for (int i = 0; i < BS; ++i) if (i < bs) x[i] = b.MF[((size_t)pb * T + (T - 1)) * S + o + i];
  }
  for (int j = 0; j < ap.ns; ++j) {
    double* bj = ap.bnd + (((size_t)pb * ap.ns + j) * M + n) * BS;
    const double* sp = ap.spanbuf + (((size_t)pb * ap.ns + j) * M + n) * (BS * BS + BS);
    double y[BS];
#pragma unroll
    for (int i = 0; i < BS; ++i) {
      bj[i] = x[i];
      double a = sp[BS * BS + i];
#pragma unroll
      for (int l = 0; l < BS; ++l) a = fma(sp[BS * i + l], x[l], a);
      y[i] = a;
    }
#pragma unroll
    for (int i = 0; i < BS; ++i) x[i] = y[i];
  }
}

template <int MODE, int BS = 4>
__global__ void __launch_bounds__(256) ihgp_aff_apply_kernel(Shape sh, Bufs b, IhgpTabs tb, AffPar ap) {
  const int pb = blockIdx.y, M = sh.M, S = sh.S;
  const int64_t T = sh.T;
  const int gid = blockIdx.x * blockDim.x + threadIdx.x;
  double mxM = 0.0, mxP = 0.0;
  unsigned long long n_clamped = 0;      // (MODE == 0) sites the stored clamp acts on, counted as the sequential kernels count them
  if (gid < ap.ns * M) {
    const int j = gid / M, n = gid - j * M;
    const double* mdl = b.model + (size_t)pb * mdl_size(sh);
    const double* tab = tb.base + (size_t)pb * itab_size(sh, tb.NG);
    double A4[BS * BS];
#pragma unroll
    for (int e = 0; e < BS * BS; ++e) A4[e] = mdl[mdl_A(sh) + (size_t)n * BS * BS + e];
    const double hn = mdl[mdl_h(sh) + n];
    const int bs = sh.bsz[n], o = sh.off[n];
    double x[BS];
    const double* bj = ap.bnd + (((size_t)pb * ap.ns + j) * M + n) * BS;
#pragma unroll
    for (int i = 0; i < BS; ++i) x[i] = bj[i];
    const int64_t s0 = (int64_t)j * ap.L, s1 = (s0 + ap.L < ap.kend) ? s0 + ap.L : ap.kend;
    for (int64_t s = s0; s < s1; ++s) {
      const int64_t k = (MODE == 0) ? s : (ap.kend - 1 - s);
      double F[BS * BS], g[BS], aux;
      ihgp_coeffs<MODE, BS>(sh, b, tb, tab, A4, hn, n, pb, k, bs, o, F, g, aux);
      double y[BS];
#pragma unroll
      for (int i = 0; i < BS; ++i) {
        double a = g[i];
#pragma unroll
        for (int l = 0; l < BS; ++l) a = fma(F[BS * i + l], x[l], a);
        y[i] = a;
      }
#pragma unroll
      for (int i = 0; i < BS; ++i) x[i] = y[i];
      const size_t ix = ((size_t)pb * T + k) * M + n;
      if (MODE == 0) {
        double* mfp = b.MF + ((size_t)pb * T + k) * S + o;
#pragma unroll
        for (int i = 0; i < BS; ++i)
          if (i < bs) mfp[i] = x[i];
        b.fm[ix] = hn * x[0];
        if (!(b.ttau[ix] > 0.0)) ++n_clamped;
        b.ttau[ix] = max0(b.ttau[ix]);     // the clamp of :274 is stored
        b.R[ix] = aux;                      // unchanged, or Inf for clamped sites (:287)
      } else {
        double* msp = b.MS + ((size_t)pb * T + k) * S + o;
#pragma unroll
        for (int i = 0; i < BS; ++i)
          if (i < bs) msp[i] = x[i];
        const double mnew = hn * x[0];
        if (md_counts(b, pb, T, k)) mxM = fmax(mxM, fabs(b.sm[ix] - mnew));
        b.sm[ix] = mnew;
        b.sv[ix] = aux;
        if (k == 0) {
          mxP = fabs(ap.vprev[(size_t)pb * M + n] - aux);
          ap.vprev[(size_t)pb * M + n] = aux;
        }
      }
    }
  }
  if (MODE == 0 && n_clamped) atomicAdd(&b.counters[(size_t)pb * 4 + 1], n_clamped);
  if (MODE == 1) {
    mxM = wave_max(mxM);
    mxP = wave_max(mxP);
    if ((threadIdx.x & 63) == 0) {
      atomicMax(reinterpret_cast<unsigned long long*>(&b.red[(size_t)pb * 8 + 1]), (unsigned long long)__double_as_longlong(mxM));
      atomicMax(reinterpret_cast<unsigned long long*>(&b.red[(size_t)pb * 8 + 2]), (unsigned long long)__double_as_longlong(mxP));
    }
  }
}

}  // namespace nagp
