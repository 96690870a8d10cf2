// nagp_kernels.hpp -- HIP kernels of the full-covariance path (gf_ep_* / gf_giekf_*):
//   gf_filter_kernel   forward ADF/Kalman (or EKF) filter, one workgroup per problem, P resident in registers
//   rts_gain_kernel    per-step smoother gain (PSkp, Cholesky, G), one workgroup per (step, problem)
//   rts_scan_kernel    backward recursion E <- G (E+Delta) G', e <- G (e+delta), one workgroup per problem
//   ep_site_kernel     cavity + mom + damped power-EP site update, parallel over steps
//   reduce kernels     nlZ = -sum(lZ), maxDiff
// Reference lines: matlab/gf_ep_modulator_nmf.m:126-184 (filter), :207-234 (RTS), :236-268 (EP),
// matlab/iekf_update1.m:110-117 + gf_giekf_modulator_nmf_constraints.m:492-502 (EKF update).
#pragma once
#include "nagp_dev.hpp"
#include "nagp_momsq.hpp"

namespace nagp {

constexpr int LDS_INT_DOUBLES = 66;
constexpr int TS = 18;  // LDS tile stride in doubles (16 + 2 pad): consecutive tiles start 36 banks apart -> conflict-free b64/b128 reads  // (2*MAXM+2) ints rounded up to an even number of doubles

struct Shape {
  int S, M, D, N;
  int ntiles;  // M*M
  int64_t T;
  int off[MAXM + 1];
  int bsz[MAXM];
  // Blocks of more than four states (Matern-5/2 or -7/2 sub-bands, ss_modulators_nmf.m:13-33 with cf_matern52_to_ss.m:93-121):
  //   infinite-horizon plans keep a block per thread, BS = 8 doubles per block row in the packed model and the tables (4 otherwise);
  //   full-covariance plans split such a block over TWO tile rows -- its first four states stay in tile row n, the rest become tile
  //   row part[n] behind the Ms real sites ("tail rows": no measurement, h = 0, sites fixed at zero) -- and A, Q, Pinf gain the cross
  //   tiles of the pair (mdl_Ax ...).  Ms = number of real sites (= M when no block is split), part[n] = -1 for an unsplit block.
  int BS;
  int Ms;
  signed char part[MAXM];
};

// per-problem packed model (doubles): A blocks [M][BS^2] | Q blocks [M][BS^2] | Pinf blocks [M][BS^2] |
// h_val [M] | W [D][N] row-major | sn2 | split blocks only: cross tiles A(n, part[n]) [M][16] | Q(n, part[n]) [M][16] | Pinf(n, part[n]) [M][16]
__host__ __device__ inline size_t mdl_A(const Shape&) { return 0; }
__host__ __device__ inline size_t mdl_Q(const Shape& s) { return (size_t)s.M * s.BS * s.BS; }
__host__ __device__ inline size_t mdl_P(const Shape& s) { return (size_t)s.M * 2 * s.BS * s.BS; }
__host__ __device__ inline size_t mdl_h(const Shape& s) { return (size_t)s.M * 3 * s.BS * s.BS; }
__host__ __device__ inline size_t mdl_W(const Shape& s) { return (size_t)s.M * (3 * s.BS * s.BS + 1); }
__host__ __device__ inline size_t mdl_sn2(const Shape& s) { return mdl_W(s) + (size_t)s.D * s.N; }
__host__ __device__ inline size_t mdl_Ax(const Shape& s) { return ((mdl_sn2(s) + 1 + 1) / 2) * 2; }
__host__ __device__ inline size_t mdl_Qx(const Shape& s) { return mdl_Ax(s) + (size_t)s.M * 16; }
__host__ __device__ inline size_t mdl_Px(const Shape& s) { return mdl_Ax(s) + (size_t)s.M * 32; }
__host__ __device__ inline size_t mdl_size(const Shape& s) { return mdl_Ax(s) + ((s.Ms < s.M) ? (size_t)s.M * 48 : 0); }

struct Bufs {
  const double* model;  // [B][mdl_size]
  const double* y;      // [B][T]
  double* ttau;         // [B][T][M]
  double* tnu;          // [B][T][M]
  double* R;            // [B][T][M]
  double* lZ;           // [B][T]
  double* MF;           // [B][T][S]  filtered means
  double* MS;           // [B][T][S]  smoothed means
  double* PF;           // [B][T][ntiles][16] filtered covariances (tile-major), may be null (nlml, 1 sweep)
  double* PSs;          // [B][T][ntiles][16] smoothed covariances, optional (null unless requested)
  double* fm;           // [B][T][M] filtered marginal mean  H m
  double* fv;           // [B][T][M] filtered marginal var   diag(H P H')
  double* sm;           // [B][T][M] smoothed marginals
  double* sv;
  double* Gbuf;         // [B][chunk][2][ntiles][16]  (G, Delta) of the current smoother chunk
  double* dbuf;         // [B][chunk][S]              delta of the current chunk
  size_t gpstride;      // doubles between the problems of Gbuf; 0: chunk * (doubles of one step).  Non-zero for a buffer that lives inside
                        // PF (column-owner plans whose free memory does not hold a buffer per chunk: nagp_api.hip, "recycled")
  double* state;        // [B][ntiles*16 + S]         scan state (E, e) between chunks; smoothed (P,m) at k=0 for EKF
  double* red;          // [B][8] reduction outputs (sum lZ, maxDiffM, maxDiffP, ...)
  unsigned long long* counters;  // [B][4]
  int md_observed;      // maxDiffM / maxDiffP over the observed steps only: the mixture variant takes them where it refreshes (gf_ep_mods_nmf_mixture.m:261, 287-288)
};

__device__ __forceinline__ bool md_counts(const Bufs& b, size_t pb, int64_t T, int64_t k) { return !b.md_observed || !isnan(b.y[pb * T + k]); }

// One window of a time-parallel fixed-site launch: steps [k_warm, k_begin) are the warm-up -- computed, nothing stored --, steps
// [k_begin, k_end) store as usual.  seed = 0: start at k_warm from the prior (m = 0, P = Pinf; k_warm = 0 is the true start),
// seed = 1: continue from the stored (MF, PF) of step k_warm - 1.
struct FilterWin {
  int64_t k_warm, k_begin, k_end;
  int seed, pad;
};

struct FilterPar {
  int itt;            // 1-based sweep
  double ep_damp;
  int mom_all;        // call mom at every step (itt==1) -- otherwise only at k==T-1
  int legacy_update;  // nlml mode single-branch update (gf_ep_modulator_nmf.m:428-439)
  int clamp_always;   // nlml mode clamps ttau at every step (:425)
  int write_R;        // predict mode writes R
  int predict_k1;     // gf_ep_modulator.m:131-133
  int store_PF;
  int init_from_state;  // EKF sweeps >= 2: start from the smoothed (m,P) at k=0
  int reset_P;          // with init_from_state: P <- Pinf anyway (constraints variant)
  int l_iter;           // EKF inner iterations
  int kb;               // steps per I/O block (LDS ring)
  int64_t k_begin, k_end;  // steps processed by this launch; k_begin > 0 continues from (MF, PF) of step k_begin-1
  int spl_wave;            // EKF: the last wave of the workgroup owns no tiles and evaluates the softplus link
  // ADF site refresh  site <- w_old*site + w_new*(moment-matched site), mom evaluated at power mom_alpha:
  //   (1-d, d, 1) in gf_ep_modulator_nmf.m:147-148 ; (1-d, d/alpha, alpha) in experiments/gf_ep_mods_nmf_mixture.m:183-187
  double w_old, w_new, mom_alpha;
  int R_raw;               // mixture variant: R = 1/ttau before the clamp (gf_ep_mods_nmf_mixture.m:190,195)
  int ekf_energy;          // EKF nlml pass (gf_giekf_modulator_nmf_constraints.m:385-472): lZ_k = -(log(2pi)/2 + log sqrt(S) + v^2/(2S)),
                           // no isnan guard on y (a NaN observation poisons the energy, as in the reference)
  // chunk-pipelined smoother: progress[pb] = number of leading steps whose filter outputs (MF, PF, marginals) are in HBM and visible
  // to the rest of the device -- host-pinned memory the host polls to start the gain / compose launches of finished chunks on a
  // second stream while this workgroup filters on.  nullptr: nothing published.
  unsigned long long* progress;
  int progress_every;      // publish when the step count crosses a multiple of this (and at the end of the launch)
  int dbg;                 // developer switch (NAGP_FILTER_DBG): skip phases to time the others -- results are garbage.
                           // 1: rank-M covariance update, 2: PF stores, 4: prediction congruence, 8: W panel writes, 16: mean update
  int cpl_doubles;         // split blocks (Shape::part): doubles of the extra LDS region in FRONT of everything else (filter_cpl_doubles)
  int cpl_chunk;           // ... and the tiles per phase of the exchange (filter_cpl_chunk)
  // time-parallel fixed-site launches (template parameter WIN; nagp_plan_set_windows): workgroup (pb, blockIdx.y) runs window
  // win[blockIdx.y] and leaves its state at the end of the warm-up in win_state[pb][blockIdx.y] (filter_win_doubles each)
  const FilterWin* win;
  double* win_state;
};


// The filtered covariance is symmetric: PF holds only the lower-triangular tiles, tile (I,J), I >= J, at tile index I(I+1)/2 + J.
// Layout of ONE step (pf_step_doubles): groups of 64 consecutive tile indices, and inside a group the eight 16-byte pieces of the
// tiles piece-major -- [group][piece e = 0..7][tile in group = 0..63][2 doubles], element x = 4i+j of a tile in piece x/2.  The filter
// thread that owns tile t is lane t % 64 of its wave, so each of its eight stores writes 1 KB of contiguous memory per wave (with the
// tiles contiguous, a 16-byte store per lane touched 64 different 128-byte lines: 1.2 of the 6.0 us EKF step, 2.1 of the 20.6 us ADF
// step at S = 146 -- profiles/r03_filter_phase_costs.txt).  pf_load returns tile (I,J) of the full matrix (transposing for I < J).
__host__ __device__ inline int pf_ntiles(const Shape& s) { return s.M * (s.M + 1) / 2; }
__host__ __device__ inline size_t pf_step_doubles(const Shape& s) { return (size_t)((pf_ntiles(s) + 63) / 64) * 64 * 16; }
// record of one (problem, window): its state at the end of the warm-up -- the lower tiles of P in the layout of one PF step, then m -- and
// behind them (filter_win_nan) the NaN observations its stored steps counted (taken back from the counter when the window runs again)
__host__ __device__ inline size_t filter_win_nan(const Shape& s) { return pf_step_doubles(s) + (((size_t)s.S + 1) & ~(size_t)1); }
__host__ __device__ inline size_t filter_win_doubles(const Shape& s) { return filter_win_nan(s) + 2; }
__host__ __device__ inline size_t pf_off(int t, int x) { return ((((size_t)(t >> 6) * 8 + (x >> 1)) * 64) + (t & 63)) * 2 + (x & 1); }
// (32-bit index arithmetic on purpose: a step holds < 2^16 tiles, and the sequential filters have no scalar registers to spare)
__device__ __forceinline__ void pf_tile_load(double* t, const double* PFk, int tile) {
  const double2* q = reinterpret_cast<const double2*>(PFk);
  const int i0 = (tile >> 6) * 512 + (tile & 63);
#pragma unroll
  for (int e = 0; e < 8; ++e) { const double2 v = q[i0 + e * 64]; t[2 * e] = v.x; t[2 * e + 1] = v.y; }
}
__device__ __forceinline__ void pf_tile_store(double* PFk, int tile, const double* t) {
  double2* q = reinterpret_cast<double2*>(PFk);
  const int i0 = (tile >> 6) * 512 + (tile & 63);
#pragma unroll
  for (int e = 0; e < 8; ++e) q[i0 + e * 64] = make_double2(t[2 * e], t[2 * e + 1]);
}
__device__ __forceinline__ void pf_load(double* t, const double* PFk, int I, int J) {
  if (I >= J) {
    pf_tile_load(t, PFk, I * (I + 1) / 2 + J);
  } else {
    double u[16];
    pf_tile_load(u, PFk, J * (J + 1) / 2 + I);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) t[4 * i + j] = u[4 * j + i];
  }
}
__device__ __forceinline__ double pf_elem(const double* PFk, int I, int J, int i, int j) {
  return (I >= J) ? PFk[pf_off(I * (I + 1) / 2 + J, 4 * i + j)] : PFk[pf_off(J * (J + 1) / 2 + I, 4 * j + i)];
}

// thread tid owns tiles t = tid + q*NT (q < TPT)
template <int TPT>
struct TileOwner {
  int I[TPT], J[TPT];
  bool ok[TPT];
  __device__ void init(int M, int ntiles) {
#pragma unroll
    for (int q = 0; q < TPT; ++q) {
      const int t = threadIdx.x + q * blockDim.x;
      ok[q] = t < ntiles;
      const int tt = ok[q] ? t : 0;
      I[q] = tt / M;
      J[q] = tt - I[q] * M;
    }
  }
};

// ---------------------------------------------------------------------------------------------
// Forward filter.  MEAS = 0: Power-EP / ADF sites (gf_ep_modulator*.m), MEAS = 1: EKF (gf_giekf_*).
// One workgroup per problem, sequential in k.  The covariance lives in registers (4x4 tile per
// thread); W = P H', H P travel through LDS panels laid out [site][row-in-block][block] so that the
// rank-M update reads them bank-conflict free.  All small per-step global traffic (y, sites, lZ,
// filtered mean/marginals) goes through an LDS ring of `kb` steps that is filled / flushed with
// coalesced transfers once per block; the only global operations inside the sequential loop are the
// fire-and-forget stores of the filtered covariance tiles.
__host__ __device__ inline size_t filter_ring_doubles(const Shape& s, int kb) { return (size_t)kb * (5 * s.M + s.S + 3); }
// split blocks: partner table [MAXM ints] | cross tiles of A [M][TS] | of Q [M][TS] | exchange buffer of the lower tiles [M(M+1)/2][TS]
// (the exchange runs in filter_cpl_phases() phases of filter_cpl_chunk() tiles each, so that the buffer takes at most 48 KB of the LDS: one phase up to 25 tile rows)
// (16 KB beyond 45 tile rows, where the panel W = P H' alone takes 65 KB and more)
__host__ __device__ inline int filter_cpl_phases(const Shape& s) { const size_t bud = (s.M > 45) ? 16 * 1024 : 48 * 1024; return (int)(((size_t)(s.M * (s.M + 1) / 2) * TS * sizeof(double) + bud - 1) / bud); }
__host__ __device__ inline int filter_cpl_chunk(const Shape& s) { const int ph = filter_cpl_phases(s); return (s.M * (s.M + 1) / 2 + ph - 1) / ph; }
__host__ __device__ inline size_t filter_cpl_doubles(const Shape& s) {
  return (s.Ms < s.M) ? (size_t)(MAXM / 2) + 2 * (size_t)s.M * TS + (size_t)filter_cpl_chunk(s) * TS : 0;
}
__host__ __device__ inline size_t filter_lds_doubles(const Shape& s, const MomCfg& mc, int meas, int kb) {
  size_t n = LDS_INT_DOUBLES + 2 * (size_t)s.M * TS + s.M + (size_t)s.D * s.N + s.S + 4 * (size_t)s.M * s.M +
             6 * (size_t)s.M + 2 * 68 + 8 + 2 /* the W panel starts on a 16-byte boundary */ + filter_ring_doubles(s, kb);
  // mom workspace: the staged sparse-point form when the plan enabled it, else the generic one
  const size_t wmom = mc.sq_form ? msq_lds_doubles<MsqFlat>(mc.cdim) + 512 : ((mc.sp.enabled && mc.cdim <= MSP_MAXCD) ? msp_lds_doubles(mc.cdim, s.D) : mom_lds_doubles(mc));
  n += (meas == 0) ? wmom : (size_t)(2 * s.M + 2 * s.S + 2 * s.N);
  return (n + 1) & ~(size_t)1;
}

// MV: mom variant (see mom_eval) for MEAS == 0; MV = -1: no mom code at all (the steps k < T-1 of the sweeps
// with fixed sites -- a much smaller kernel without the cubature's register pressure); the EKF filter is
// instantiated with MV = 0 only
// LB: launch bound.  The ADF launches (MV >= 0) run with <= 256 threads whenever the tiles fit: one wave per SIMD
// may then use all 512 registers (the cubature's pressure lands in AGPRs instead of scratch memory).
// SP = 1: the ADF steps use the staged sparse-point form of likModulatorNMFPower (nagp_momsp.hpp) and the generic mom_eval is not
// compiled into the instantiation at all (both side by side cost hundreds of registers); SP = 2: likModulatorPreCalcwn in the staged
// form of nagp_momsq.hpp (flat layout), likewise without the generic code
// CPL: plans with split blocks (Shape::part): the prediction couples the two tile rows of a block -- every thread leaves its tiles in an LDS
// exchange buffer and forms  P(I,J) <- sum_{a in {I, part I}} sum_{b in {J, part J}} A(I,a) P(a,b) A(J,b)'  from up to four of them --
// and the tail rows behind the Ms real sites take no part in the site arithmetic (h = 0, sites fixed at zero)
// WIN: time-parallel form of the fixed-site launches (MV = -1): the grid carries a window index in y, the steps come from fp.win[blockIdx.y]
// (FilterWin).  The warm-up predicate is uniform per workgroup and per ring block and gates stores only (PF tiles, the ring flush, the
// NaN counter): the arithmetic of a stored step is that of the sequential launch.  A warm-up READS sites (and, with clamp_always, ttau)
// of steps the window in front of it rewrites at the same time -- with the values they already hold (tnu, R) or with max(ttau, 0), which
// this kernel applies to what it reads anyway: either value gives the same step.
template <int TPT, int MEAS, int MV, int LB = 512, int SP = 0, bool CPL = false, bool WIN = false>
__global__ void __launch_bounds__(LB) gf_filter_kernel(Shape sh, Bufs b, MomCfg mc, FilterPar fp) {
  static_assert(!WIN || (MEAS == 0 && MV < 0), "windows exist for the fixed-site launches only");
  extern __shared__ __attribute__((aligned(16))) double lds_raw[];
  double* lds = lds_raw + (CPL ? fp.cpl_doubles : 0);
  const int tid = threadIdx.x, NT = blockDim.x;
  const int S = sh.S, M = sh.M, D = sh.D, KB = fp.kb;
  const int Ms = CPL ? sh.Ms : M;      // real sites
  int* ipart = reinterpret_cast<int*>(lds_raw);                  // CPL: [MAXM] partner tile row or -1
  double* sAx = lds_raw + MAXM / 2;                              //      A(n, part n) [M][TS]
  double* sQx = sAx + (size_t)M * TS;                            //      Q(n, part n) [M][TS]
  double* sX = sQx + (size_t)M * TS;                             //      exchange buffer: the lower tiles [lo, lo + fp.cpl_chunk) of one phase, tile t at (t - lo) * TS
  const int64_t T = sh.T;
  const int pb = blockIdx.x;
  const double* mdl = b.model + (size_t)pb * mdl_size(sh);
  // steps of this workgroup: [kw_first, kw_store) warm-up (WIN only), [kw_store, kw_end) stored
  int64_t kw_first = fp.k_begin, kw_store = fp.k_begin, kw_end = fp.k_end;
  bool from_store = fp.k_begin > 0;
  if constexpr (WIN) {
    const FilterWin w = fp.win[blockIdx.y];
    kw_first = w.k_warm; kw_store = w.k_begin; kw_end = w.k_end; from_store = w.seed != 0;
  }

  int* ioff = reinterpret_cast<int*>(lds);          // [MAXM+1]
  int* ibsz = ioff + (MAXM + 1);                     // [MAXM]
  double* sA = lds + LDS_INT_DOUBLES;                // A blocks, stride TS
  double* sQ = sA + (size_t)M * TS;                  // Q blocks, stride TS
  double* shv = sQ + (size_t)M * TS;
  double* sW = shv + M;
  double* m = sW + (size_t)sh.D * sh.N;
  // Wl[n][h][I][2] = h_n P(off_I + 2h + {0,1}, c_n): rows 0-1 and rows 2-3 of block I in two planes, 16-byte aligned: the rank-M
  // update reads a site's column vector with two 16-byte loads per operand, and consecutive blocks sit 16 bytes apart (conflict-free
  // ds_read_b128; with the four rows contiguous the 32-byte stride halves the LDS rate of the three-waves-per-SIMD launches)
  double* Wl = lds + ((((size_t)((m + S) - lds)) + 1) & ~(size_t)1);
  double* fmu = Wl + (size_t)M * 4 * M;    // fmu, HPH: 68 entries, zero beyond the M sites
  double* HPH = fmu + 68;                  // (stage A of the sparse-point cubature reads up to 64 of them against zero weights)
  double* tt = HPH + 68;
  double* tn = tt + M;
  double* cA = tn + M;
  double* cm = cA + M;
  double* dl = cm + M;
  double* d2l = dl + M;
  double* misc = d2l + M;  // [0]=lZ
  double* ry = misc + 8;                   // ring: y[KB]
  double* rlZ = ry + KB;                   //       lZ[KB]
  double* rZ = rlZ + KB;                   //       Z of the steps that called mom (< 0: none); log taken at the flush
  double* rtt = rZ + KB;                   //       ttau[KB][M]
  double* rtn = rtt + (size_t)KB * M;
  double* rR = rtn + (size_t)KB * M;
  double* rfm = rR + (size_t)KB * M;       //       H m  (filtered)
  double* rfv = rfm + (size_t)KB * M;      //       diag(H P H') (filtered)
  double* rMF = rfv + (size_t)KB * M;      //       m (filtered) [KB][S]
  double* ws = rMF + (size_t)KB * S;       // mom workspace | EKF: part[M], PJ[S]

  for (int i = tid; i <= M; i += NT) ioff[i] = sh.off[i];
  for (int i = tid; i < M; i += NT) ibsz[i] = sh.bsz[i];
  for (int i = tid; i < M * 16; i += NT) {
    sA[(i >> 4) * TS + (i & 15)] = mdl[mdl_A(sh) + i];
    sQ[(i >> 4) * TS + (i & 15)] = mdl[mdl_Q(sh) + i];
  }
  for (int i = tid; i < M; i += NT) shv[i] = mdl[mdl_h(sh) + i];
  for (int i = tid; i < sh.D * sh.N; i += NT) sW[i] = mdl[mdl_W(sh) + i];
  for (int i = tid; i < 68; i += NT) { fmu[i] = 0.0; HPH[i] = 0.0; }
  if constexpr (CPL && MEAS == 1)      // EKF: Jacobian entries and mean terms of the tail rows stay zero
    for (int i = Ms + tid; i < M; i += NT) { ws[i] = 0.0; ws[(size_t)M + 2 * S + 2 * sh.N + i] = 0.0; }
  if constexpr (CPL) {
    for (int i = tid; i < M; i += NT) ipart[i] = sh.part[i];
    for (int i = tid; i < M * 16; i += NT) {
      sAx[(i >> 4) * TS + (i & 15)] = mdl[mdl_Ax(sh) + i];
      sQx[(i >> 4) * TS + (i & 15)] = mdl[mdl_Qx(sh) + i];
    }
  }
  const double sn2 = mdl[mdl_sn2(sh)];
  // likModulatorNMFPower on a fully symmetric sigma-point set: the staged form of nagp_momsp.hpp (256-thread ADF launches)
  constexpr bool SPK = SP == 1 && (MEAS == 0 && MV >= 1 && MV <= MSP_MAXCD);
  constexpr bool SQK = SP == 2 && (MEAS == 0 && MV >= 1 && MV <= MSQ_MAXCD);
  static_assert(SP == 0 || SPK || SQK, "the staged forms exist for the NMF likelihoods with 1..7 (sqrt amplitudes: 1..6) components");
  constexpr int CDX = (SPK || SQK) ? MV : 1;
  if constexpr (MEAS == 0 && MV >= 0 && !SPK && !SQK) mom_cache_tables(mc, ws);
  const double pEP1 = (MEAS == 0 && MV >= 0) ? mom_pEP(mc, sn2, fp.mom_alpha) : 1.0;
  MspCtx<CDX> xsp;
  double wrow[CDX];
#pragma unroll
  for (int j = 0; j < CDX; ++j) wrow[j] = 0.0;
  // staged sqrt amplitudes (SP = 2): ws = [W transposed: 512][workspace of nagp_momsq.hpp]
  MsqW<CDX, MsqFlat> xq; MsqLink xl; MsqM xm;
  double amp[SQK ? 2 * MsqFlat::NST : 1];
  msp_rp q_accp = nullptr, q_partp = nullptr;
  if constexpr (SQK) {
    __syncthreads();      // sW, fmu / HPH padding
    double* wsq = ws + 512;
    msq_init<MsqFlat>(CDX, wsq, NT);
    __syncthreads();
    const MsqLay lay = msq_layout<MsqFlat>(CDX);
    const int wv = tid >> 6;
    msq_setup_W<CDX, MsqFlat>(xq, mc, mc.sp.c0, sW, fmu, HPH, wsq, wv, tid, ws, 1);
    msqf_setup_link<CDX>(xl, mc, fmu, HPH, wsq);
    msq_setup_M<CDX, MsqFlat>(xm, mc, mc.sp.c0, wsq, (wv >= 2) ? wv - 2 : 2);
    q_accp = (msp_rp)(wsq + lay.acc) + opaque_zero();
    q_partp = (msp_rp)(wsq + lay.part + (tid & 15) + 16 * ((tid >> 4) & 1));
#pragma unroll
    for (int i = 0; i < 2 * MsqFlat::NST; ++i) amp[i] = 0.0;
  }
  if constexpr (SPK) {
    __syncthreads();      // sW, fmu / HPH padding
    msp_setup<CDX>(xsp, mc, mc.sp, sW, fmu, HPH, ws);
    if (tid < D) {
#pragma unroll
      for (int j = 0; j < CDX; ++j) wrow[j] = sW[tid * CDX + j];
    }
  }

  // The covariance is kept exactly symmetric: only the lower-triangular tiles (I >= J) are held (one thread
  // per tile); K*H*P and K*W' coincide, W = P H' is the only panel needed, and the filtered covariance is
  // stored as the tile and its transpose.
  struct { int I[TPT], J[TPT]; bool ok[TPT]; } own;
  const int nlow = M * (M + 1) / 2;
#pragma unroll
  for (int q = 0; q < TPT; ++q) {
    const int t = tid + q * NT;
    own.ok[q] = t < nlow;
    const int tt_ = own.ok[q] ? t : 0;
    int I = (int)((sqrt(8.0 * tt_ + 1.0) - 1.0) * 0.5);
    while ((I + 1) * (I + 2) / 2 <= tt_) ++I;
    while (I * (I + 1) / 2 > tt_) --I;
    own.I[q] = I; own.J[q] = tt_ - I * (I + 1) / 2;
  }
  double P[TPT][16];
  const double* st = b.state + (size_t)pb * ((size_t)sh.ntiles * 16 + S);
#pragma unroll
  for (int q = 0; q < TPT; ++q) {
    tile_zero(P[q]);
    if (own.ok[q]) {
      if (from_store)
        pf_tile_load(P[q], b.PF + ((size_t)pb * T + (kw_first - 1)) * (size_t)(((nlow + 63) & ~63) * 16), tid + q * NT);
      else if (fp.init_from_state && !fp.reset_P)
        tile_load(P[q], st + (size_t)(own.I[q] * M + own.J[q]) * 16);
      else if (own.I[q] == own.J[q])
        tile_load(P[q], mdl + mdl_P(sh) + (size_t)own.I[q] * 16);
      else if (CPL && sh.part[own.I[q]] == own.J[q])
        tile_load(P[q], mdl + mdl_Px(sh) + (size_t)own.I[q] * 16);      // Pinf(rows of the tail row I, columns of its head row)
    }
  }
  for (int i = tid; i < S; i += NT)
    m[i] = from_store ? b.MF[((size_t)pb * T + (kw_first - 1)) * S + i]
                            : (fp.init_from_state ? st[(size_t)sh.ntiles * 16 + i] : 0.0);
  __syncthreads();
  // State lanes.  The vector work of a step (mean prediction, mean update, the filtered mean's way to the ring) belongs to thread
  // soff + i for state i.  One-tile-per-thread launches of the EP filters whose workgroup has whole waves beyond the tile threads
  // (the fixed-site kernel of small models: 190 tiles on a 384-thread launch at 19 sites) put it on those waves, beside the tile
  // waves instead of in front of them; otherwise soff = 0.
  const int tile_threads = (nlow + 63) & ~63;
  const int soff = (MEAS == 0 && TPT == 1 && NT >= tile_threads + ((S + 63) & ~63)) ? tile_threads : 0;
  const int sid = tid - soff;
  const bool slane = sid >= 0 && sid < S;
  // which block / row-in-block does state sid belong to
  int myblk = 0, myrow = 0;
  int my_o = 0, my_bs = 0;      // offset and size of that block (registers: the step loop does not go back to the LDS tables for them)
  if (slane) {
    while (ioff[myblk + 1] <= sid) ++myblk;
    myrow = sid - ioff[myblk];
    my_o = ioff[myblk]; my_bs = ibsz[myblk];
  }

  // CPL: the partner's share of row `row` of (A m) for block blk:  sum_l A(blk, part blk)[row][l] m[off(part blk) + l]
  auto cross_mean = [&](int blk, int row) -> double {
    double r = 0.0;
    if constexpr (CPL) {
      const int pp = ipart[blk];
      if (pp >= 0) {
        const double* ax = sAx + (size_t)blk * TS + 4 * row;
        const double* mp_ = m + ioff[pp];
        const int bp = ibsz[pp];
#pragma unroll
        for (int l = 0; l < 4; ++l)
          if (l < bp) r = fma(ax[l], mp_[l], r);
      }
    }
    return r;
  };
  // CPL: tile (a, c) of the symmetric matrix if it lies in the phase [lo, hi) of the exchange buffer (false: not in this phase)
  auto x_tile = [&](double* t, int a, int c, int lo, int hi) -> bool {
    const int ix = (a >= c) ? a * (a + 1) / 2 + c : c * (c + 1) / 2 + a;
    if (ix < lo || ix >= hi) return false;
    if (a >= c) tile_load(t, sX + (size_t)(ix - lo) * TS);
    else {
      double u[16];
      tile_load(u, sX + (size_t)(ix - lo) * TS);
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) t[4 * i + j] = u[4 * j + i];
    }
    return true;
  };
  const double* yv = b.y + (size_t)pb * T;
  double* g_tt = b.ttau + (size_t)pb * T * M;
  double* g_tn = b.tnu + (size_t)pb * T * M;
  double* g_R = b.R + (size_t)pb * T * M;
  double* g_lZ = b.lZ + (size_t)pb * T;
  double* g_MF = b.MF + (size_t)pb * T * S;
  double* g_fm = b.fm + (size_t)pb * T * M;
  double* g_fv = b.fv + (size_t)pb * T * M;
  const int pf_tiles = (nlow + 63) & ~63;       // tiles per step of PF, padded to whole groups of 64 (pf_step_doubles = 16 * pf_tiles)
  double* g_PF = (b.PF && fp.store_PF) ? b.PF + (size_t)pb * T * pf_tiles * 16 : nullptr;
  unsigned long long n_clamped = 0, n_nan = 0;
  unsigned long long stp[8] = {0, 0, 0, 0, 0, 0, 0, 0}, st_a = 0, st_b = 0;   // developer diagnostics (mc.stamps)
#define EKF_STAMP(slot) do { if ((MEAS == 1 || MV == -1) && mc.stamps && tid == 0) { st_b = __builtin_readcyclecounter(); stp[slot] += st_b - st_a; st_a = st_b; } } while (0)
  if (mc.stamps && tid == 0) st_a = __builtin_readcyclecounter();

  // the state this window starts its stored steps from (its estimate of (m, P) after step kw_store - 1), for the boundary check
  auto win_state_store = [&]() {
    if constexpr (WIN) {
      double* wst = fp.win_state + ((size_t)pb * gridDim.y + blockIdx.y) * filter_win_doubles(sh);
#pragma unroll
      for (int q = 0; q < TPT; ++q)
        if (own.ok[q]) pf_tile_store(wst, tid + q * NT, P[q]);
      for (int i = tid; i < S; i += NT) wst[(size_t)pf_tiles * 16 + i] = m[i];
    }
  };
  if constexpr (WIN) { if (kw_first == kw_store) win_state_store(); }      // (no warm-up: the seed itself)

  for (int64_t k0 = kw_first; k0 < kw_end;) {
    const bool warm = WIN && k0 < kw_store;      // uniform over the workgroup and over the ring block
    const int64_t k_lim = warm ? kw_store : kw_end;
    const int nb = (k_lim - k0 < KB) ? (int)(k_lim - k0) : KB;
    // ---- fill the ring
    for (int i = tid; i < nb; i += NT) { ry[i] = yv[k0 + i]; rlZ[i] = g_lZ[k0 + i]; rZ[i] = -1.0; }
    if (MEAS == 0)
      for (int i = tid; i < nb * M; i += NT) {
        rtt[i] = g_tt[(size_t)k0 * M + i]; rtn[i] = g_tn[(size_t)k0 * M + i]; rR[i] = g_R[(size_t)k0 * M + i];
      }
    __syncthreads();

    for (int kk = 0; kk < nb; ++kk) {
      const int64_t k = k0 + kk;
      const double yk = ry[kk];
      const bool pred = (k > 0) || fp.predict_k1;
      const bool do_mom = (MEAS == 0) && (MV >= 0) && (fp.mom_all || (k == T - 1));
      // steps without a mom call: the owner of diagonal tile (n,n) also forms the gain coefficients of site n,
      // which removes one barrier-separated phase from the step
      const bool early = (MEAS == 0) && !do_mom && !(yk != yk);
      // ---- S0: prediction (registers), publish W = P H', H P, diag(H P H'), fmu = H m
      double rm = 0.0;
      if (slane) {
        if (pred) {
          const double* a = sA + (size_t)myblk * TS + 4 * myrow;
          const double* mb = m + my_o;
          const int bs = my_bs;
#pragma unroll
          for (int l = 0; l < 4; ++l)
            if (l < bs) rm = fma(a[l], mb[l], rm);
          if constexpr (CPL) rm += cross_mean(myblk, myrow);
        } else {
          rm = m[sid];
        }
        if (myrow == 0) fmu[myblk] = shv[myblk] * rm;
      }
      EKF_STAMP(4);   // (loop top, ring, mean prediction of the state lanes)
      const bool upd = !(yk != yk) || (MEAS == 1 && fp.ekf_energy);   // ~isnan(y_k), or the guard-less nlml loop
      if (MEAS == 1 && fp.spl_wave && tid >= NT - 64 && upd) {
        // EKF: the launch carries one extra wave without tiles; it evaluates softplus(g_j) and its derivative of the first
        // inner iteration here, next to the prediction phase of the tile waves (one exp + log chain off the critical path)
        const int j = tid - (NT - 64);
        if (j < sh.N) {
          const int blk = D + j, o_ = ioff[blk];
          double g = 0.0;
          if (pred) {
            const double* a = sA + (size_t)blk * TS;
#pragma unroll
            for (int l = 0; l < 4; ++l)
              if (l < ibsz[blk]) g = fma(a[l], m[o_ + l], g);
            if constexpr (CPL) g += cross_mean(blk, 0);
          } else {
            g = m[o_];
          }
          const double eg = exp(shv[blk] * g);
          double* spl0 = ws + M + S;
          spl0[j] = log(1.0 + eg);
          spl0[sh.N + j] = eg / (eg + 1.0);
        }
      }
      if constexpr (CPL) {
        if (pred) {
          // P(I,J) <- sum_{a in {I, part I}} sum_{b in {J, part J}} A(I,a) P(a,b) A(J,b)': the tiles travel through the exchange buffer in phases of
          // fp.cpl_chunk lower tiles; every thread adds the terms whose source tile lies in the phase (the readers of the previous step's last phase
          // are five barriers back)
          double acc[TPT][16];
#pragma unroll
          for (int q = 0; q < TPT; ++q) tile_zero(acc[q]);
          for (int lo = 0; lo < nlow; lo += fp.cpl_chunk) {
            const int hi = (lo + fp.cpl_chunk < nlow) ? lo + fp.cpl_chunk : nlow;
#pragma unroll
            for (int q = 0; q < TPT; ++q) {
              const int t = tid + q * NT;
              if (own.ok[q] && t >= lo && t < hi) tile_store(sX + (size_t)(t - lo) * TS, P[q]);
            }
            lds_barrier();
#pragma unroll
            for (int q = 0; q < TPT; ++q) {
              if (own.ok[q]) {
                const int I = own.I[q], J = own.J[q], Ip = ipart[I], Jp = ipart[J];
                auto term = [&](int a_, const double* Aia, int b_, const double* Ajb) {
                  double pt[16], t1[16];
                  if (!x_tile(pt, a_, b_, lo, hi)) return;
                  tile_zero(t1);
                  tile_mma_nt(t1, pt, Ajb);
                  tile_mma(acc[q], Aia, t1);
                };
                term(I, sA + (size_t)I * TS, J, sA + (size_t)J * TS);
                if (Jp >= 0) term(I, sA + (size_t)I * TS, Jp, sAx + (size_t)J * TS);
                if (Ip >= 0) {
                  term(Ip, sAx + (size_t)I * TS, J, sA + (size_t)J * TS);
                  if (Jp >= 0) term(Ip, sAx + (size_t)I * TS, Jp, sAx + (size_t)J * TS);
                }
              }
            }
            if (hi < nlow) lds_barrier();      // the buffer is overwritten by the next phase
          }
#pragma unroll
          for (int q = 0; q < TPT; ++q)
            if (own.ok[q] && !(fp.dbg & 4)) {
#pragma unroll
              for (int e = 0; e < 16; ++e) P[q][e] = acc[q][e];
            }
        }
      }
#pragma unroll
      for (int q = 0; q < TPT; ++q) {
        if (own.ok[q]) {
          const int I = own.I[q], J = own.J[q];
          if (pred && !(fp.dbg & 4)) {
            if constexpr (CPL) {
              if (J == ipart[I]) {      // the pair's cross tile of Q (I = tail row, J = its head row)
                const double* Qb = sQx + (size_t)I * TS;
#pragma unroll
                for (int e = 0; e < 16; ++e) P[q][e] += Qb[e];
              }
            } else {
              tile_congruence(P[q], sA + (size_t)I * TS, sA + (size_t)J * TS);
            }
            if (I == J) {
              const double* Qb = sQ + (size_t)I * TS;
#pragma unroll
              for (int e = 0; e < 16; ++e) P[q][e] += Qb[e];
            }
          }
          const double hJ = shv[J], hI = shv[I];
          // P(rows of I, c_J)
          if (!(fp.dbg & 8))
#pragma unroll
          for (int i = 0; i < 4; ++i) Wl[(((size_t)J * 2 + (i >> 1)) * M + I) * 2 + (i & 1)] = hJ * P[q][4 * i];
          if (I == J) {
            const double hp = hI * hI * P[q][0];
            HPH[I] = hp;
            if (early) {
              double f;
              if (pred) {
                const double* a = sA + (size_t)I * TS;
                const double* mb = m + ioff[I];
                f = 0.0;
#pragma unroll
                for (int l = 0; l < 4; ++l)
                  if (l < ibsz[I]) f = fma(a[l], mb[l], f);
                if constexpr (CPL) f += cross_mean(I, 0);
                f *= hI;
              } else {
                f = hI * m[ioff[I]];
              }
              double t = rtt[kk * M + I];
              if (fp.clamp_always) { t = max0(t); rtt[kk * M + I] = t; }
              const double n_ = rtn[kk * M + I];
              bool formA = (t == 0.0);
              if (fp.legacy_update) {
                double mn = max0(rtt[kk * M]);
                for (int u = 1; u < Ms; ++u) mn = fmin(mn, max0(rtt[kk * M + u]));
                formA = (mn == 0.0);
              }
              if (CPL && I >= Ms) formA = true;      // tail rows (t = 0, h = 0): the form without 1 / t
              if (formA) { const double z = t * hp + 1.0; cA[I] = t / z; cm[I] = -(t * f - n_) / z; }
              else { const double s = 1.0 / (hp + 1.0 / t); cA[I] = s; cm[I] = s * (n_ / t - f); }
            }
          } else if (!(fp.dbg & 8)) {             // P(rows of J, c_I) = P(c_I, cols of J) by symmetry
#pragma unroll
            for (int j = 0; j < 4; ++j) Wl[(((size_t)I * 2 + (j >> 1)) * M + J) * 2 + (j & 1)] = hI * P[q][j];
          }
        }
      }
      EKF_STAMP(5);   // (congruence, panel: this wave's tiles)
      lds_barrier();  // B1
      EKF_STAMP(0);   // (prediction, panel, mean prediction, softplus wave)
      if (slane) m[sid] = rm;

      if (upd) {
        if (MEAS == 0) {
          if constexpr (MV >= 0) if (do_mom) {
            if (mc.stamps && tid == 0) { st_b = __builtin_readcyclecounter(); stp[4] += st_b - st_a; }
            double d1v = 0.0, d2v = 0.0;
            if constexpr (SPK) {
              msp_stageA<CDX>(xsp, mc);
              lds_barrier();
              msp_stageB<CDX>(xsp, mc, ws);
              lds_barrier();
              msp_stage1b<CDX>(xsp, mc, mc.sp, sn2 / fp.mom_alpha, yk, ws);
              lds_barrier();
              msp_stage2<CDX>(xsp, mc, ws);
              lds_barrier();
              if (tid < 64) {       // the sites live in wave 0: partial sums and outputs without another workgroup barrier
                msp_reduce<CDX>(xsp);
                msp_wave_fence();
                if (tid < M) {
                  double Zv;
                  msp_outputs<CDX>(xsp.accp, tid < D, tid - D, wrow, pEP1, mc.jitter, Zv, d1v, d2v);
                  if (tid == 0) rZ[kk] = Zv;
                }
              }
            }
            if constexpr (SQK) {
              double Zv = 0.0;
              msqf_eval<CDX>(xq, xl, xm, mc, amp, sn2 / fp.mom_alpha, yk, q_accp, q_partp, tid < D, tid - D, pEP1, tid < M, Zv, d1v, d2v);
              if (tid == 0) rZ[kk] = Zv;
            }
            if constexpr (!SPK && !SQK) {
              mom_eval<MV, false, false>(mc, sW, pEP1, sn2, fp.mom_alpha, yk, fmu, HPH, ws, &misc[0], dl, d2l, stp);
              if (tid < Ms) { d1v = dl[tid]; d2v = d2l[tid]; }
              if (tid == 0) rZ[kk] = misc[0];
            }
            if (mc.stamps && tid == 0) st_a = __builtin_readcyclecounter();
            if (CPL && tid >= Ms && tid < M) { tt[tid] = 0.0; tn[tid] = 0.0; }      // tail rows: no site
            if (tid < Ms) {
              const double d2 = d2v, d1 = d1v, hp = HPH[tid], f = fmu[tid];
              const double t_old = rtt[kk * M + tid], n_old = rtn[kk * M + tid];
              double tnew = fp.w_old * t_old + fp.w_new * (-d2 / (1.0 + d2 * hp));
              const double nnew = fp.w_old * n_old + fp.w_new * ((d1 - f * d2) / (1.0 + d2 * hp));
              if (!(tnew > 0.0)) ++n_clamped;
              const double traw = tnew;
              tnew = max0(tnew);
              tt[tid] = tnew; tn[tid] = nnew;
              rtt[kk * M + tid] = tnew; rtn[kk * M + tid] = nnew;
              if (fp.write_R) rR[kk * M + tid] = 1.0 / (fp.R_raw ? traw : tnew);
            }
          }
          if (do_mom && fp.legacy_update) lds_barrier();
          if (do_mom && tid < M) {
            const double t = tt[tid], n = tn[tid], hp = HPH[tid], f = fmu[tid];
            bool formA = (t == 0.0);
            if (fp.legacy_update) {
              double mn = tt[0];
              for (int q = 1; q < Ms; ++q) mn = fmin(mn, tt[q]);   // MATLAB min ignores NaN like fmin
              formA = (mn == 0.0);
            }
            if (CPL && tid >= Ms) formA = true;      // tail rows
            if (formA) {   // z = t*hp+1; K = W*(t/z); v = t*f - n; m -= W*(v/z); P -= K*W'
              const double z = t * hp + 1.0;
              cA[tid] = t / z;
              cm[tid] = -(t * f - n) / z;
            } else {       // K = W/(hp+1/t); v = n/t - f; m += K*v; P -= K*H*P
              const double s = 1.0 / (hp + 1.0 / t);
              cA[tid] = s;
              cm[tid] = s * (n / t - f);
            }
            if (tid == 0) misc[1] = formA ? 1.0 : 0.0;
          }
          if (do_mom) lds_barrier();  // B4
          if (slane && !(fp.dbg & 16)) {
            double a0 = rm, a1 = 0.0, a2 = 0.0, a3 = 0.0;
            const double* wp = Wl + ((size_t)(myrow >> 1) * M + myblk) * 2 + (myrow & 1);
            int n = 0;
            for (; n + 8 <= M; n += 8) {   // sixteen LDS reads in flight per trip (the four-term trips waited for their reads one by one)
              double w8[8], c8[8];
#pragma unroll
              for (int u = 0; u < 8; ++u) { w8[u] = wp[(size_t)(n + u) * 4 * M]; c8[u] = cm[n + u]; }
              a0 = fma(w8[0], c8[0], a0); a1 = fma(w8[1], c8[1], a1); a2 = fma(w8[2], c8[2], a2); a3 = fma(w8[3], c8[3], a3);
              a0 = fma(w8[4], c8[4], a0); a1 = fma(w8[5], c8[5], a1); a2 = fma(w8[6], c8[6], a2); a3 = fma(w8[7], c8[7], a3);
            }
            for (; n + 4 <= M; n += 4) {
              a0 = fma(wp[(size_t)(n + 0) * 4 * M], cm[n + 0], a0);
              a1 = fma(wp[(size_t)(n + 1) * 4 * M], cm[n + 1], a1);
              a2 = fma(wp[(size_t)(n + 2) * 4 * M], cm[n + 2], a2);
              a3 = fma(wp[(size_t)(n + 3) * 4 * M], cm[n + 3], a3);
            }
            if (n < M) {      // tail (< 4 terms, all on chain a0 as before): its reads together, then the same fused multiply-adds
              double wt[3], ct[3];
#pragma unroll
              for (int u = 0; u < 3; ++u) { const int nn = (n + u < M) ? n + u : M - 1; wt[u] = wp[(size_t)nn * 4 * M]; ct[u] = cm[nn]; }
#pragma unroll
              for (int u = 0; u < 3; ++u) if (n + u < M) a0 = fma(wt[u], ct[u], a0);
            }
            rm = (a0 + a1) + (a2 + a3);
            m[sid] = rm;
          }
          EKF_STAMP(1);   // (fixed-site kernel: mean update)
          // P -= sum_n cA[n] W[:,n] W[:,n]'   (K*H*P and K*W' coincide for the symmetric P)
#pragma unroll
          for (int q = 0; q < TPT; ++q) {
            if (own.ok[q] && !(fp.dbg & 1)) {
              const double* wbase = Wl + (size_t)own.I[q] * 2;
              const double* rbase = Wl + (size_t)own.J[q] * 2;
              int n0 = 0;
              for (; n0 + 2 <= M; n0 += 2) {   // two sites per trip: eight 16-byte LDS reads in flight before the FMAs
                double w4[2][4], r4[2][4];
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                  const double c = -cA[n0 + u];
                  const double2* wq = reinterpret_cast<const double2*>(wbase + (size_t)(n0 + u) * 4 * M);
                  const double2* rq = reinterpret_cast<const double2*>(rbase + (size_t)(n0 + u) * 4 * M);
                  const double2 w01 = wq[0], w23 = wq[M], r01 = rq[0], r23 = rq[M];      // second plane: 2*M doubles on
                  w4[u][0] = w01.x * c; w4[u][1] = w01.y * c; w4[u][2] = w23.x * c; w4[u][3] = w23.y * c;
                  r4[u][0] = r01.x; r4[u][1] = r01.y; r4[u][2] = r23.x; r4[u][3] = r23.y;
                }
#pragma unroll
                for (int u = 0; u < 2; ++u)
#pragma unroll
                  for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j) P[q][4 * i + j] = fma(w4[u][i], r4[u][j], P[q][4 * i + j]);
              }
              if (n0 < M) {
                const double c = -cA[n0];
                double w1[4], r1[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) w1[i] = wbase[(size_t)n0 * 4 * M + (size_t)(i >> 1) * 2 * M + (i & 1)] * c;
#pragma unroll
                for (int j = 0; j < 4; ++j) r1[j] = rbase[(size_t)n0 * 4 * M + (size_t)(j >> 1) * 2 * M + (j & 1)];
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                  for (int j = 0; j < 4; ++j) P[q][4 * i + j] = fma(w1[i], r1[j], P[q][4 * i + j]);
              }
            }
          }
        } else {
          // ---------------- EKF measurement update (iekf_update1.m:110-117)
          double* part = ws;
          double* PJ = ws + M;
          double* Kv = PJ + S + 2 * sh.N;   // [S] gain of the last inner iteration
          const int N = sh.N;
          double Sx = 1.0, MU = 0.0;
          // Three barriers per inner iteration: partials | P J' | everything else.  S = R + J P J' and MU = h(m) are summed by EVERY
          // wave for itself (same terms, same order: no broadcast, no barrier in front of the gain); the state lanes write fmu -- and
          // the modulators' softplus / sigmoid -- of the NEXT iteration straight from their updated mean.
          double* mp = Kv + S;             // [M] z_d * dh/dz_d: the terms of MU
          for (int it = 0; it < fp.l_iter; ++it) {
            double* spl = PJ + S;        // [N] softplus(g), [N] sigmoid(g)
            if (it == 0 && !fp.spl_wave) {
              if (tid < N) {
                const double eg = exp(fmu[D + tid]);
                spl[tid] = log(1.0 + eg);
                spl[N + tid] = eg / (eg + 1.0);
              }
              lds_barrier();
            }
            // The modulators' partials are D-term sums: eight lanes of wave 1 per modulator (fixed tree over the lanes) beside the
            // sub-band lanes of wave 0, instead of one lane each behind them in the same wave (<= 8 modulators; otherwise as before)
            const bool mod_w1 = (N <= 8) && (NT >= 128);
            if (mod_w1 && tid >= 64 && tid < 128) {
              const int g = (tid - 64) >> 3, sub = tid & 7;
              double f8[8], w8[8];
#pragma unroll
              for (int u = 0; u < 8; ++u) {
                const int d = sub + 8 * u;
                const bool ok = (g < N) && (d < D);
                f8[u] = ok ? fmu[d] : 0.0; w8[u] = ok ? sW[d * N + g] : 0.0;
              }
              double z = 0.0;
#pragma unroll
              for (int u = 0; u < 8; ++u) z = fma(f8[u], w8[u], z);
              z = group_sum(z, 8);
              if (sub == 0 && g < N) { part[D + g] = z * spl[N + g]; mp[D + g] = 0.0; }
            }
            if (tid < (mod_w1 ? D : Ms)) {
              double pv = 0.0;
              if (tid < D) {
                for (int j0 = 0; j0 < N; j0 += 4) {      // (reads of four terms together; same order of the fused multiply-adds)
                  double w4[4], s4[4];
#pragma unroll
                  for (int u = 0; u < 4; ++u) { const int jj = (j0 + u < N) ? j0 + u : N - 1; w4[u] = sW[tid * N + jj]; s4[u] = spl[jj]; }
#pragma unroll
                  for (int u = 0; u < 4; ++u) if (j0 + u < N) pv = fma(w4[u], s4[u], pv);
                }
              } else {
                const int j = tid - D;
                double z0 = 0.0, z1 = 0.0, z2 = 0.0, z3 = 0.0;   // four independent chains (same terms, fixed order)
                int d = 0;
                for (; d + 8 <= D; d += 8) {   // sixteen LDS reads in flight per trip
                  double f8[8], w8[8];
#pragma unroll
                  for (int u = 0; u < 8; ++u) { f8[u] = fmu[d + u]; w8[u] = sW[(d + u) * N + j]; }
                  z0 = fma(f8[0], w8[0], z0); z1 = fma(f8[1], w8[1], z1); z2 = fma(f8[2], w8[2], z2); z3 = fma(f8[3], w8[3], z3);
                  z0 = fma(f8[4], w8[4], z0); z1 = fma(f8[5], w8[5], z1); z2 = fma(f8[6], w8[6], z2); z3 = fma(f8[7], w8[7], z3);
                }
                for (; d + 4 <= D; d += 4) {
                  z0 = fma(fmu[d], sW[d * N + j], z0); z1 = fma(fmu[d + 1], sW[(d + 1) * N + j], z1);
                  z2 = fma(fmu[d + 2], sW[(d + 2) * N + j], z2); z3 = fma(fmu[d + 3], sW[(d + 3) * N + j], z3);
                }
                if (d < D) {      // tail: reads together, then the same fused multiply-adds on chain z0
                  double ft[3], wt[3];
#pragma unroll
                  for (int u = 0; u < 3; ++u) { const int dd = (d + u < D) ? d + u : D - 1; ft[u] = fmu[dd]; wt[u] = sW[dd * N + j]; }
#pragma unroll
                  for (int u = 0; u < 3; ++u) if (d + u < D) z0 = fma(ft[u], wt[u], z0);
                }
                pv = ((z0 + z1) + (z2 + z3)) * spl[N + j];
              }
              part[tid] = pv;
              mp[tid] = (tid < D) ? fmu[tid] * pv : 0.0;
            }
            lds_barrier();
            EKF_STAMP(1);   // (partials of the Jacobian row)
            if (slane) {
              double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
              const double* wp = Wl + ((size_t)(myrow >> 1) * M + myblk) * 2 + (myrow & 1);
              int n = 0;
              for (; n + 8 <= M; n += 8) {   // sixteen LDS reads in flight per trip
                double w8[8], c8[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) { w8[u] = wp[(size_t)(n + u) * 4 * M]; c8[u] = part[n + u]; }
                a0 = fma(w8[0], c8[0], a0); a1 = fma(w8[1], c8[1], a1); a2 = fma(w8[2], c8[2], a2); a3 = fma(w8[3], c8[3], a3);
                a0 = fma(w8[4], c8[4], a0); a1 = fma(w8[5], c8[5], a1); a2 = fma(w8[6], c8[6], a2); a3 = fma(w8[7], c8[7], a3);
              }
              for (; n + 4 <= M; n += 4) {
                a0 = fma(wp[(size_t)(n + 0) * 4 * M], part[n + 0], a0); a1 = fma(wp[(size_t)(n + 1) * 4 * M], part[n + 1], a1);
                a2 = fma(wp[(size_t)(n + 2) * 4 * M], part[n + 2], a2); a3 = fma(wp[(size_t)(n + 3) * 4 * M], part[n + 3], a3);
              }
              if (n < M) {      // tail: reads together, then the same fused multiply-adds on chain a0
                double wt[3], ct[3];
#pragma unroll
                for (int u = 0; u < 3; ++u) { const int nn = (n + u < M) ? n + u : M - 1; wt[u] = wp[(size_t)nn * 4 * M]; ct[u] = part[nn]; }
#pragma unroll
                for (int u = 0; u < 3; ++u) if (n + u < M) a0 = fma(wt[u], ct[u], a0);
              }
              PJ[sid] = (a0 + a1) + (a2 + a3);
            }
            lds_barrier();
            EKF_STAMP(2);   // (P J')
            {
              double tj = 0.0, tm = 0.0;
              for (int n = tid & 63; n < M; n += 64) { tj = fma(part[n] * shv[n], PJ[ioff[n]], tj); tm += mp[n]; }
              tj = wave_sum(tj); tm = wave_sum(tm);
              MU = tm;
              Sx = sn2 + tj;
            }
            if (fp.ekf_energy) {
              if (!(Sx > 0.0)) Sx += 0.5e-4;            // chol(S) failed: jitter 1e-4*rand, rand -> 0.5 (:417-420, SURVEY C-7)
              if (tid == 0) {
                const double LS = sqrt(Sx), v = yk - MU;  // !(S > 0) after the jitter: NaN energy, like `nan*edata` (:423-426)
                rlZ[kk] = -(0.9189385332046727 + log(LS) + 0.5 * ((v / LS) / LS) * v);
              }
            }
            if (slane) {
              const double Kt = PJ[sid] / Sx; Kv[sid] = Kt; rm = rm + Kt * (yk - MU);     // K = P J' / S, once per state
              if (it + 1 < fp.l_iter && myrow == 0) {
                const double f = shv[myblk] * rm;
                fmu[myblk] = f;
                if (myblk >= D && myblk < Ms) {      // a modulator row (the tail rows of split blocks lie behind the Ms real sites)
                  const double eg = exp(f);
                  spl[myblk - D] = log(1.0 + eg);
                  spl[N + myblk - D] = eg / (eg + 1.0);
                }
              }
              if (it + 1 == fp.l_iter) m[sid] = rm;
            }
            lds_barrier();   // Kv (and fmu, spl of the next iteration) visible
            EKF_STAMP(3);   // (wave sums, gain, mean)
          }
          // P -= K S K'
#pragma unroll
          for (int q = 0; q < TPT; ++q) {
            if (own.ok[q] && !(fp.dbg & 1)) {
              const int oI = ioff[own.I[q]], oJ = ioff[own.J[q]];
              const int bI = ibsz[own.I[q]], bJ = ibsz[own.J[q]];
              // the gain entries of the two blocks, zero on the padding rows: eight selects in place of sixteen guarded updates
              double ki[4], kj[4];
#pragma unroll
              for (int i = 0; i < 4; ++i) {
                const double a = Kv[oI + ((i < bI) ? i : 0)], c = Kv[oJ + ((i < bJ) ? i : 0)];
                ki[i] = (i < bI) ? a * Sx : 0.0;
                kj[i] = (i < bJ) ? c : 0.0;
              }
#pragma unroll
              for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) P[q][4 * i + j] -= ki[i] * kj[j];
            }
          }
        }
      } else {
        if (!warm) ++n_nan;
      }
      EKF_STAMP(6);   // (P -= K S K')
      // ---- per-step outputs -> ring ; covariance tiles -> HBM
      if (slane) {
        rMF[(size_t)kk * S + sid] = rm;
        if (myrow == 0) rfm[kk * M + myblk] = shv[myblk] * rm;
      }
#pragma unroll
      for (int q = 0; q < TPT; ++q)
        if (own.ok[q] && own.I[q] == own.J[q])
          rfv[kk * M + own.I[q]] = shv[own.I[q]] * shv[own.I[q]] * P[q][0];
      if (g_PF && !(fp.dbg & 2) && !warm) {
#pragma unroll
        for (int q = 0; q < TPT; ++q)
          if (own.ok[q]) pf_tile_store(g_PF + (size_t)k * pf_tiles * 16, tid + q * NT, P[q]);   // lower tile index == ownership index
      }
      lds_barrier();  // B5
      EKF_STAMP(7);   // (outputs, PF stores, B5)
      if (mc.stamps && tid == 0 && do_mom) { st_b = __builtin_readcyclecounter(); stp[5] += st_b - st_a; st_a = st_b; }
    }
    if (warm) {      // a warm-up block stores nothing; the last one leaves (m, P) for the boundary check
      if (k0 + nb == kw_store) win_state_store();
      __syncthreads();
      k0 += nb;
      continue;
    }
    // ---- flush the ring
    if constexpr (MEAS == 0 && MV >= 0) {
      for (int i = tid; i < nb; i += NT) g_lZ[k0 + i] = (rZ[i] < 0.0) ? rlZ[i] : log(rZ[i]);
    } else if constexpr (MEAS == 1) {
      for (int i = tid; i < nb; i += NT) g_lZ[k0 + i] = rlZ[i];   // (the EKF energy of the nlml pass travels through rlZ)
    }
    // (MEAS == 0, MV < 0: the fixed-site launches never call mom and leave lZ alone -- in the cross-sweep schedule they run on the main
    // stream while the reduction of the previous sweep's lZ is still reading it on the side stream; nagp_api.hip, ev_red)
    for (int i = tid; i < nb * M; i += NT) {
      if (MEAS == 0) {
        g_tt[(size_t)k0 * M + i] = rtt[i]; g_tn[(size_t)k0 * M + i] = rtn[i];
        if (fp.write_R) g_R[(size_t)k0 * M + i] = rR[i];
      }
      g_fm[(size_t)k0 * M + i] = rfm[i]; g_fv[(size_t)k0 * M + i] = rfv[i];
    }
    for (int i = tid; i < nb * S; i += NT) g_MF[(size_t)k0 * S + i] = rMF[i];
    const bool publish = fp.progress && ((k0 + nb) / fp.progress_every != k0 / fp.progress_every || k0 + nb == kw_end);
    if (publish) __threadfence_system();      // this thread's stores (its PF tiles, its share of the flush) before the flag
    __syncthreads();
    if (publish && tid == 0)
      __hip_atomic_store(&fp.progress[pb], (unsigned long long)(k0 + nb), __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    k0 += WIN ? nb : KB;
  }
  if (tid < M && n_clamped) atomicAdd(&b.counters[(size_t)pb * 4 + 1], n_clamped);
  if (tid == 0 && n_nan) atomicAdd(&b.counters[(size_t)pb * 4 + 2], n_nan);
  if constexpr (WIN) {
    if (tid == 0) fp.win_state[((size_t)pb * gridDim.y + blockIdx.y) * filter_win_doubles(sh) + filter_win_nan(sh)] = (double)n_nan;
  }
  if (mc.stamps && tid == 0)
    for (int i = 0; i < 8; ++i) mc.stamps[i] += stp[i];
}

// ---------------------------------------------------------------------------------------------
// RTS gain.  One workgroup per (step, problem) of the current chunk:
//   B = PS_k A' ; PSkp = A B + Q ; L = chol(PSkp,'lower') (jitter retry) ; G = B / L' / L
//   Delta_k = PS_{k+1} - PSkp ; delta_k = MF_{k+1} - A MF_k          (gf_ep_modulator_nmf.m:210-230)
// Right-looking blocked algorithms on the 4x4 tiles; every thread keeps its B/X/G tile and its
// L tile in registers; panels travel through LDS (double buffered).
struct GainPar {
  int64_t k0;   // first step of the chunk
  int nk;       // steps in the chunk
  int chunk;    // chunk capacity (buffer stride)
  int dense_sp; // 0: (G, Delta) tile-major ; > 0: dense row-major Sp x Sp (input layout of the MFMA smoother passes)
  int dbg;      // developer switch of rts_gain_mfma_kernel (NAGP_GAINM_DBG): skip phases to time the others (results are garbage)
  int dpacked;  // dense_sp > 0: Delta is stored as its lower-triangular 16x16 tiles, tile (TI,TJ), TI >= TJ, at [TI(TI+1)/2+TJ][16][16]
                // (all the column-owner smoother passes read of it): a step of the slot is Sp^2 + NTL(NTL+1)/2*256 doubles instead of 2 Sp^2
  int cpl_doubles;              // split blocks (Shape::part): doubles of the extra LDS region in front of everything else (gain_cpl_doubles)
  const double* ainv;           // rts_gain_mfma_kernel<.., true>: [B][M][32] per block A^-1 (16) and A^-1 Q (16), zero padded (host: gain_inverse_blocks)
  unsigned long long* stamps;   // developer diagnostics (NAGP_STAMPS): cycles of thread 0 of every 64th workgroup per phase of rts_gain_kernel:
                // [0] prologue (loads, B = PS A', PSkp, Delta) [1] diagonal tiles [2] column solves [3] trailing updates [4] backward
                // solve [5] G store [6] workgroups sampled
};
__host__ __device__ inline size_t gd_step_doubles(int Sp, int dpacked) {      // doubles of (G, Delta) of one step in a dense slot
  const size_t ntl = (size_t)Sp / 16;
  return dpacked ? (size_t)Sp * Sp + ntl * (ntl + 1) / 2 * 256 : 2 * (size_t)Sp * Sp;
}

__host__ __device__ inline size_t gain_lds_doubles(const Shape& s) {
  return LDS_INT_DOUBLES + (size_t)s.M * 16 * 2 + 4 * (size_t)s.M * TS + 8;
}
// split blocks: partner table [MAXM ints] | cross tiles A(n, part n) [M][16]
__host__ __device__ inline size_t gain_cpl_doubles(const Shape& s) { return (s.Ms < s.M) ? (size_t)(MAXM / 2) + (size_t)s.M * 16 : 0; }
// the 768-thread instantiation (one workgroup per CU anyway) and the one-tile-per-thread one stage PS_k in LDS: its tiles are read three
// times (PSkp by the lower owners, B = PS A' by the owners of (I,J) and of (J,I)), at 768 threads by lanes that have no registers to hoist the
// loads with.  Measured (tools/ab_libs.sh, same box): gain launches of 32 x 12 500 steps at S = 146 899 -> ~780 ms (cfg5_fill 1 873 -> 1 755 ms,
// cfg5 x 8 4 762 -> 4 681), cfg2_batch 557 -> 551 ms; two tiles per thread: no change (not staged: the LDS would cost the second workgroup of a CU
// at 30+ sites)
__host__ __device__ inline size_t gain_lds_doubles_staged(const Shape& s) { return ((gain_lds_doubles(s) + 1) & ~(size_t)1) + pf_step_doubles(s); }

// in-place Cholesky of the leading bs x bs lower triangle of a 4x4 tile; padding -> identity.
// rd[j] = 1 / L(j,j): the triangular solves below multiply by it (sixteen f64 divisions per tile solve otherwise --
// the divisions, not the multiply-adds, were most of the instructions of the column phases)
__device__ __forceinline__ bool tile_chol(double* t, int bs, double* rd) {
  bool ok = true;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (j < bs) {
      double s = t[4 * j + j];
#pragma unroll
      for (int l = 0; l < 4; ++l)
        if (l < j) s = fma(-t[4 * j + l], t[4 * j + l], s);
      if (!(s > 0.0)) ok = false;
      // 1/sqrt(s) from the hardware estimate and two Newton steps, sqrt(s) = s * (1/sqrt(s)): a third of the dependent
      // instructions of sqrt() followed by a division, on the one thread every other thread of the column is waiting for
      const double r = rsqrt_nr(s);
      const double d = s * r;
      t[4 * j + j] = d; rd[j] = r;
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (i > j && i < bs) {
          double v = t[4 * i + j];
#pragma unroll
          for (int l = 0; l < 4; ++l)
            if (l < j) v = fma(-t[4 * i + l], t[4 * j + l], v);
          t[4 * i + j] = v * r;
        }
    } else {
      t[4 * j + j] = 1.0; rd[j] = 1.0;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (i < j) t[4 * i + j] = 0.0;   // upper part
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (i > j && (i >= bs || j >= bs)) t[4 * i + j] = 0.0;
  }
  return ok;
}
// rows of t:  x * L' = t   (forward substitution, L lower 4x4 with unit padding, RECIPROCAL diagonal)
__device__ __forceinline__ void tile_solve_Lt(double* t, const double* L) {
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      double v = t[4 * i + c];
#pragma unroll
      for (int l = 0; l < 4; ++l)
        if (l < c) v = fma(-t[4 * i + l], L[4 * c + l], v);
      t[4 * i + c] = v * L[4 * c + c];
    }
}
// rows of t:  x * L = t   (backward substitution, RECIPROCAL diagonal)
__device__ __forceinline__ void tile_solve_L(double* t, const double* L) {
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int c = 3; c >= 0; --c) {
      double v = t[4 * i + c];
#pragma unroll
      for (int l = 0; l < 4; ++l)
        if (l > c) v = fma(-t[4 * i + l], L[4 * l + c], v);
      t[4 * i + c] = v * L[4 * c + c];
    }
}

// one tile per thread: capped at 128 VGPRs (four waves per SIMD; measured best of 2..6) so that two workgroups share a CU -- the kernel is a chain of ~3M short
// barrier-separated phases and lives on latency hiding across workgroups
// LB = 768 (two tiles of B and ONE of the lower triangle per thread, 168 registers): the shapes with 1025 .. 1536 tiles whose lower
// triangle fits 768 threads (32-channel / 6-component: 1444 and 741) -- three tiles per thread under the 512 bound spill ~280 registers
// CPL: plans with split blocks (Shape::part): B = PS A' and PSkp = A B + Q with the cross tiles of the pairs,
//   B(I,J) = PS(I,J) A(J,J)' + PS(I,Jp) A(J,Jp)' ,  PSkp(I,J) = A(I,I) B(I,J) + A(I,Ip) B(Ip,J)  (every thread forms the B tiles it needs itself)
template <int TPT, int LB = 512, bool CPL = false>
__global__ void __launch_bounds__(LB) __attribute__((amdgpu_waves_per_eu(LB > 512 ? 3 : (TPT == 1 ? 4 : 2)))) rts_gain_kernel(Shape sh, Bufs b, GainPar gp) {
  extern __shared__ __attribute__((aligned(16))) double lds_raw[];
  double* lds = lds_raw + (CPL ? gp.cpl_doubles : 0);
  int* ipart = reinterpret_cast<int*>(lds_raw);      // CPL: [MAXM]
  double* sAx = lds_raw + MAXM / 2;                  //      [M][16]
  const int tid = threadIdx.x, NT = blockDim.x;
  const int S = sh.S, M = sh.M;
  const int64_t T = sh.T;
  const int kk = blockIdx.x, pb = blockIdx.y;
  const int64_t k = gp.k0 + kk;
  const double* mdl = b.model + (size_t)pb * mdl_size(sh);

  int* ioff = reinterpret_cast<int*>(lds);
  int* ibsz = ioff + (MAXM + 1);
  const bool stamp = gp.stamps && tid == ((gp.dbg > 0 && gp.dbg < NT) ? gp.dbg : 0) && (blockIdx.x & 63) == 0;      // (NAGP_GAINM_DBG = the stamped thread)
  unsigned long long st_a = 0, st_b = 0, st[6] = {0, 0, 0, 0, 0, 0};
  if (stamp) st_a = __builtin_readcyclecounter();
#define GK_STAMP(slot) do { if (stamp) { st_b = __builtin_readcyclecounter(); st[slot] += st_b - st_a; st_a = st_b; } } while (0)
  double* sA = lds + LDS_INT_DOUBLES;          // [M][16]
  double* sLd = sA + (size_t)M * 16;           // [M][16] diagonal Cholesky factors
  double* bufX = sLd + (size_t)M * 16;         // [2][M][TS]
  double* bufP = bufX + 2 * (size_t)M * TS;    // [2][M][TS]
  int* flag = reinterpret_cast<int*>(bufP + 2 * (size_t)M * TS);

  // B = PS A' (all M x M tiles; becomes X, then G) and PSkp = A B + Q (symmetric: only the lower tiles are factored; becomes L).
  // Three or four tiles per thread (SPLIT): the lower triangle has its own owners, TPL tiles per thread instead of one PSkp tile
  // beside every B tile.  One or two tiles per thread: the owner of B(I,J) also holds PSkp(I,J).
  constexpr bool SPLIT = TPT >= 3 || LB > 512;
  constexpr int TPL = SPLIT ? (LB > 512 ? 1 : (TPT + 2) / 2) : TPT;
  // COLUMN-major ownership (tile t = J*M + I): the phases of block column jb touch the tiles of one column (the solves) or of the
  // columns behind it (the trailing updates) -- consecutive threads, so whole waves skip a phase they have no tile in.  With the
  // row-major order of the span kernels every wave executed every phase for one or two active lanes.
  TileOwner<TPT> own;
#pragma unroll
  for (int q = 0; q < TPT; ++q) {
    const int t = tid + q * NT;
    own.ok[q] = t < sh.ntiles;
    const int tt_ = own.ok[q] ? t : 0;
    own.J[q] = tt_ / M; own.I[q] = tt_ - own.J[q] * M;
  }
  struct { int I[TPL], J[TPL]; bool ok[TPL]; } low;
#pragma unroll
  for (int q = 0; q < TPL; ++q) {
    if constexpr (SPLIT) {
      // lower triangle, column by column: column J holds rows J .. M-1 and starts at J*M - J(J-1)/2
      const int nlow = M * (M + 1) / 2;
      const int t = tid + q * NT;
      low.ok[q] = t < nlow;
      const int tt_ = low.ok[q] ? t : 0;
      int J = 0;
      while (J + 1 < M && (J + 1) * M - (J + 1) * J / 2 <= tt_) ++J;
      low.J[q] = J; low.I[q] = J + (tt_ - (J * M - J * (J - 1) / 2));
    } else {
      low.I[q] = own.I[q]; low.J[q] = own.J[q]; low.ok[q] = own.ok[q] && own.I[q] >= own.J[q];
    }
  }
  const double* PFk = b.PF + ((size_t)pb * T + k) * pf_step_doubles(sh);
  const double* PFk1 = PFk + pf_step_doubles(sh);
  constexpr bool STAGE = LB > 512 || TPT == 1;      // (one tile per thread: <= 22 sites, 50 KB of LDS with the staged tiles -- three workgroups per CU still fit)
  double* sPF = lds + ((gain_lds_doubles(sh) + 1) & ~(size_t)1);       // STAGE: PS_k in the layout of PF (pf_off)
  const double* PSk = STAGE ? sPF : PFk;
  if constexpr (STAGE) {
    const double2* src = reinterpret_cast<const double2*>(PFk);
    double2* dst = reinterpret_cast<double2*>(sPF);
    const int n2 = (int)(pf_step_doubles(sh) / 2);
    // eight loads in flight per trip (as a plain loop the compiler waits for every 16-byte load before it issues the next: eight
    // dependent HBM round trips at the head of a 145 us kernel -- profiles/r04_gain_phases.txt)
    constexpr int NLD = 8;
    for (int base = tid; base < n2; base += NLD * NT) {
      double2 v[NLD];
#pragma unroll
      for (int u = 0; u < NLD; ++u) { const int i = base + u * NT; v[u] = (i < n2) ? src[i] : make_double2(0.0, 0.0); }
#pragma unroll
      for (int u = 0; u < NLD; ++u) { const int i = base + u * NT; if (i < n2) dst[i] = v[u]; }
    }
  }
  const size_t mstride = gp.dense_sp ? (size_t)gp.dense_sp * gp.dense_sp : (size_t)sh.ntiles * 16;
  const size_t gstep = gp.dense_sp ? gd_step_doubles(gp.dense_sp, gp.dpacked) : 2 * mstride;
  double* Gout = b.Gbuf + (b.gpstride ? (size_t)pb * b.gpstride + (size_t)kk * gstep : ((size_t)pb * gp.chunk + kk) * gstep);
  double* Dout = Gout + mstride;
  if (b.gpstride && gp.dense_sp) {
    // a buffer in recycled memory is not zero-filled: write the padding rows / columns (4M .. Sp-1) the tiles below do not cover
    const int Sp = gp.dense_sp, R4 = 4 * M, np = Sp - R4, NTLd = Sp / 16;
    for (int i = tid; i < np * Sp; i += NT) Gout[(size_t)(R4 + i / Sp) * Sp + i % Sp] = 0.0;
    for (int i = tid; i < R4 * np; i += NT) Gout[(size_t)(i / np) * Sp + R4 + i % np] = 0.0;
    if (gp.dpacked) {      // the last row of 16x16 tiles
      double* Dl = Dout + (size_t)((NTLd - 1) * NTLd / 2) * 256;
      for (int i = tid; i < NTLd * 256; i += NT) {
        const int TJ = i >> 8, r = (i >> 4) & 15, cc = i & 15;
        if (16 * (NTLd - 1) + r >= R4 || 16 * TJ + cc >= R4) Dl[i] = 0.0;
      }
    } else {
      for (int i = tid; i < np * Sp; i += NT) Dout[(size_t)(R4 + i / Sp) * Sp + i % Sp] = 0.0;
      for (int i = tid; i < R4 * np; i += NT) Dout[(size_t)(i / np) * Sp + R4 + i % np] = 0.0;
    }
  }
  // tile (I,J) -> output location (tile-major: 16 contiguous doubles; dense: 4 rows of 4 at row stride Sp)
  auto put_tile = [&](double* base, int I, int J, const double* t16) {
    if (gp.dense_sp && gp.dpacked && base == Dout) {
      // packed Delta: 4x4 tile (I,J) sits in 16x16 tile (I/4, J/4); only the lower 16x16 tiles exist (both halves of a diagonal one)
      const int TI = I >> 2, TJ = J >> 2;
      if (TI < TJ) return;
      double2* d0 = reinterpret_cast<double2*>(base + (size_t)(TI * (TI + 1) / 2 + TJ) * 256 + (size_t)(4 * (I & 3)) * 16 + 4 * (J & 3));
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        d0[i * 8] = make_double2(t16[4 * i], t16[4 * i + 1]);
        d0[i * 8 + 1] = make_double2(t16[4 * i + 2], t16[4 * i + 3]);
      }
      return;
    }
    if (gp.dense_sp) {
      double2* d0 = reinterpret_cast<double2*>(base + ((size_t)(4 * I) * gp.dense_sp + 4 * J));
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        double2* dr = reinterpret_cast<double2*>(reinterpret_cast<double*>(d0) + (size_t)i * gp.dense_sp);
        dr[0] = make_double2(t16[4 * i], t16[4 * i + 1]);
        dr[1] = make_double2(t16[4 * i + 2], t16[4 * i + 3]);
      }
    } else {
      tile_store(base + ((size_t)I * sh.M + J) * 16, t16);
    }
  };
  // PSkp(I,J) = A_I PS(I,J) A_J' (+ Q, + the jitter of the second attempt), I >= J
  // B(I,J) = PS(I,:) A(J,:)'
  auto b_tile = [&](double* bt, int I, int J) {
    double ps[16];
    pf_load(ps, PSk, I, J);
    tile_zero(bt);
    tile_mma_nt(bt, ps, sA + (size_t)J * 16);
    if constexpr (CPL) {
      const int Jp = ipart[J];
      if (Jp >= 0) { pf_load(ps, PSk, I, Jp); tile_mma_nt(bt, ps, sAx + (size_t)J * 16); }
    }
  };
  auto pskp_tile = [&](double* Lq, int I, int J, bool jitter) {
    double bt[16];
    b_tile(bt, I, J);
    tile_zero(Lq);
    tile_mma(Lq, sA + (size_t)I * 16, bt);
    if constexpr (CPL) {
      const int Ip = ipart[I];
      if (Ip >= 0) { b_tile(bt, Ip, J); tile_mma(Lq, sAx + (size_t)I * 16, bt); }
      if (J == Ip) {      // the pair's cross tile of Q
        const double* Qx = mdl + mdl_Qx(sh) + (size_t)I * 16;
#pragma unroll
        for (int e = 0; e < 16; ++e) Lq[e] += Qx[e];
      }
    }
    if (I == J) {
      const double* Qb = mdl + mdl_Q(sh) + (size_t)I * 16;
#pragma unroll
      for (int e = 0; e < 16; ++e) Lq[e] += Qb[e];
      if (jitter) {      // sqrt(1e-4)*diag(rand): deterministic 0.5 in place of rand
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (i < ibsz[I]) Lq[5 * i] += 0.01 * 0.5;
      }
    }
  };

  // The raw tiles first: PS_k for B, PS_{k+1} where PSkp will live (Delta = PS_{k+1} - PSkp).
  // Their global latency runs beside the LDS fill and its barrier instead of in front of every product.
  double Bt[TPT][16], Lt[TPL][16];
  // (one or two tiles per thread only: with separate lower-triangle owners the early loads cost more in spilled registers than the
  // latency they hide -- measured at the 32-channel shape)
  constexpr bool HOIST = !SPLIT;
#pragma unroll
  for (int q = 0; q < TPT; ++q) {
    tile_zero(Bt[q]);
    if (HOIST && !STAGE && own.ok[q]) pf_load(Bt[q], PFk, own.I[q], own.J[q]);
  }
#pragma unroll
  for (int q = 0; q < TPL; ++q) {
    tile_zero(Lt[q]);
    if (HOIST && own.ok[q]) pf_load(Lt[q], PFk1, own.I[q], own.J[q]);
  }
  for (int i = tid; i <= M; i += NT) ioff[i] = sh.off[i];
  for (int i = tid; i < M; i += NT) ibsz[i] = sh.bsz[i];
  for (int i = tid; i < M * 16; i += NT) sA[i] = mdl[mdl_A(sh) + i];
  if constexpr (CPL) {
    for (int i = tid; i < M; i += NT) ipart[i] = sh.part[i];
    for (int i = tid; i < M * 16; i += NT) sAx[i] = mdl[mdl_Ax(sh) + i];
  }
  if (tid == 0) { flag[0] = 0; flag[1] = 0; }
  lds_barrier();

  if constexpr (SPLIT) {
#pragma unroll
    for (int q = 0; q < TPL; ++q)
      if (low.ok[q]) {
        const int I = low.I[q], J = low.J[q];
        pskp_tile(Lt[q], I, J, false);                            // PSkp = A (PS A') (+Q)
        double d[16];
        pf_load(d, PFk1, I, J);
#pragma unroll
        for (int e = 0; e < 16; ++e) d[e] -= Lt[q][e];
        put_tile(Dout, I, J, d);                                  // Delta_k, and its mirror tile
        if (I != J) {
          double dt[16];
#pragma unroll
          for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) dt[4 * i + j] = d[4 * j + i];
          put_tile(Dout, J, I, dt);
        }
      }
  }
#pragma unroll
  for (int q = 0; q < TPT; ++q) {
    if (own.ok[q]) {
      const int I = own.I[q], J = own.J[q];
      double ps[16];
      if constexpr (CPL) {
        b_tile(Bt[q], I, J);
      } else {
      if constexpr (HOIST && !STAGE) {
#pragma unroll
        for (int e = 0; e < 16; ++e) ps[e] = Bt[q][e];
        tile_zero(Bt[q]);
      } else {
        pf_load(ps, PSk, I, J);
      }
      tile_mma_nt(Bt[q], ps, sA + (size_t)J * 16);          // B = PS A'
      }
      if constexpr (!SPLIT) {
        double pk[16];
        if constexpr (CPL) {
          pskp_tile(pk, I, J, false);
        } else {
        tile_zero(pk);
        tile_mma(pk, sA + (size_t)I * 16, Bt[q]);           // PSkp = A B (+Q)
        if (I == J) {
          const double* Qb = mdl + mdl_Q(sh) + (size_t)I * 16;
#pragma unroll
          for (int e = 0; e < 16; ++e) pk[e] += Qb[e];
        }
        }
        double d[16];
#pragma unroll
        for (int e = 0; e < 16; ++e) { d[e] = Lt[q][e] - pk[e]; Lt[q][e] = pk[e]; }
        put_tile(Dout, I, J, d);                            // Delta_k
      }
    }
  }
  // delta_k = MF_{k+1} - A MF_k
  if (tid < S) {
    int blk = 0;
    while (ioff[blk + 1] <= tid) ++blk;
    const int row = tid - ioff[blk];
    const double* mf = b.MF + ((size_t)pb * T + k) * S;
    double acc = mf[S + tid];
    for (int l = 0; l < ibsz[blk]; ++l) acc = fma(-sA[(size_t)blk * 16 + 4 * row + l], mf[ioff[blk] + l], acc);
    if constexpr (CPL) {
      const int pp = ipart[blk];
      if (pp >= 0)
        for (int l = 0; l < ibsz[pp]; ++l) acc = fma(-sAx[(size_t)blk * 16 + 4 * row + l], mf[ioff[pp] + l], acc);
    }
    b.dbuf[((size_t)pb * gp.chunk + kk) * S + tid] = acc;
  }

  GK_STAMP(0);
  // ---- Cholesky of the lower triangle (two attempts: plain, then + jitter, SURVEY C-7)
  bool failed = false;
  for (int attempt = 0; attempt < 2; ++attempt) {
    if (attempt == 1) {
      // the first attempt solved X L' = B in place: rebuild B = PS A' and PSkp = A B + Q + jitter
#pragma unroll
      for (int q = 0; q < TPT; ++q)
        if (own.ok[q]) {
          if constexpr (CPL) b_tile(Bt[q], own.I[q], own.J[q]);
          else {
          double ps[16];
          pf_load(ps, PSk, own.I[q], own.J[q]);
          tile_zero(Bt[q]);
          tile_mma_nt(Bt[q], ps, sA + (size_t)own.J[q] * 16);
          }
        }
#pragma unroll
      for (int q = 0; q < TPL; ++q)
        if (low.ok[q]) {
          if constexpr (SPLIT || CPL) pskp_tile(Lt[q], low.I[q], low.J[q], true);
          else {
            const int I = low.I[q];
            tile_zero(Lt[q]);
            tile_mma(Lt[q], sA + (size_t)I * 16, Bt[q]);
            if (I == low.J[q]) {
              const double* Qb = mdl + mdl_Q(sh) + (size_t)I * 16;
#pragma unroll
              for (int e = 0; e < 16; ++e) Lt[q][e] += Qb[e];
#pragma unroll
              for (int i = 0; i < 4; ++i)
                if (i < ibsz[I]) Lt[q][5 * i] += 0.01 * 0.5;      // sqrt(1e-4)*diag(rand): deterministic 0.5 in place of rand
            }
          }
        }
    }
    for (int jb = 0; jb < M; ++jb) {
      const int par = jb & 1;
#pragma unroll
      for (int q = 0; q < TPL; ++q)
        if (low.ok[q] && low.I[q] == jb && low.J[q] == jb) {
          double rd[4];
          if (!tile_chol(Lt[q], ibsz[jb], rd)) flag[attempt] = 1;
          tile_store(sLd + (size_t)jb * 16, Lt[q]);
#pragma unroll
          for (int j = 0; j < 4; ++j) sLd[(size_t)jb * 16 + 5 * j] = rd[j];      // the solves want 1 / L(j,j)
        }
      lds_barrier();
      GK_STAMP(1);
      // column jb of L (rows below the diagonal) and -- fused, it needs nothing else -- column jb of X in X L' = B
#pragma unroll
      for (int q = 0; q < TPL; ++q)
        if (low.ok[q] && low.J[q] == jb && low.I[q] > jb) {
          tile_solve_Lt(Lt[q], sLd + (size_t)jb * 16);
          tile_store(bufP + ((size_t)par * M + low.I[q]) * TS, Lt[q]);
        }
#pragma unroll
      for (int q = 0; q < TPT; ++q)
        if (own.ok[q] && own.J[q] == jb) {
          tile_solve_Lt(Bt[q], sLd + (size_t)jb * 16);
          tile_store(bufX + ((size_t)par * M + own.I[q]) * TS, Bt[q]);
        }
      lds_barrier();
      GK_STAMP(2);
      // trailing updates: L (lower tiles) and the remaining columns of B
#pragma unroll
      for (int q = 0; q < TPL; ++q)
        if (low.ok[q] && low.J[q] > jb) {
          tile_mms_nt(Lt[q], bufP + ((size_t)par * M + low.I[q]) * TS, bufP + ((size_t)par * M + low.J[q]) * TS);
          __builtin_amdgcn_sched_barrier(0);      // one tile's operands at a time: the reads of all slots hoisted together spill
        }
#pragma unroll
      for (int q = 0; q < TPT; ++q)
        if (own.ok[q] && own.J[q] > jb) {
          tile_mms_nt(Bt[q], bufX + ((size_t)par * M + own.I[q]) * TS, bufP + ((size_t)par * M + own.J[q]) * TS);
          __builtin_amdgcn_sched_barrier(0);
        }
      GK_STAMP(3);
    }
    lds_barrier();
    failed = (flag[attempt] != 0);
    if (!failed) break;
  }
  if (tid == 0) {
    if (flag[0]) atomicAdd(&b.counters[(size_t)pb * 4 + 0], 1ull);
    if (flag[0] && flag[1]) atomicAdd(&b.counters[(size_t)pb * 4 + 3], 1ull);
  }

  // (X L' = B was solved column by column inside the factorisation loop)
  // ---- G L = X  (backward over block columns)
  for (int jb = M - 1; jb >= 0; --jb) {
    const int par = jb & 1;
#pragma unroll
    for (int q = 0; q < TPT; ++q)
      if (own.ok[q] && own.J[q] == jb) {
        tile_solve_L(Bt[q], sLd + (size_t)jb * 16);
        tile_store(bufX + ((size_t)par * M + own.I[q]) * TS, Bt[q]);
      }
#pragma unroll
    for (int q = 0; q < TPL; ++q)
      if (low.ok[q] && low.I[q] == jb && low.J[q] < jb) tile_store(bufP + ((size_t)par * M + low.J[q]) * TS, Lt[q]);
    lds_barrier();
#pragma unroll
    for (int q = 0; q < TPT; ++q)
      if (own.ok[q] && own.J[q] < jb) {
        tile_mms(Bt[q], bufX + ((size_t)par * M + own.I[q]) * TS, bufP + ((size_t)par * M + own.J[q]) * TS);
        __builtin_amdgcn_sched_barrier(0);
      }
  }
  GK_STAMP(4);
#pragma unroll
  for (int q = 0; q < TPT; ++q)
    if (own.ok[q]) {
      // clean padding, then store G
      const int bI = ibsz[own.I[q]], bJ = ibsz[own.J[q]];
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (i >= bI || j >= bJ) Bt[q][4 * i + j] = 0.0;
      put_tile(Gout, own.I[q], own.J[q], Bt[q]);
    }
  GK_STAMP(5);
  if (stamp) {
    for (int i = 0; i < 6; ++i) atomicAdd(&gp.stamps[i], st[i]);
    atomicAdd(&gp.stamps[6], 1ull);
  }
#undef GK_STAMP
}

// ---------------------------------------------------------------------------------------------
// RTS backward recursion, parallel in time.  In difference form (E_k = P^s_k - PS_k, e_k = m^s_k - MF_k)
// the reference's smoother step (gf_ep_modulator_nmf.m:229-230) is the affine map
//     E_k = G_k (E_{k+1} + Delta_k) G_k' ,   e_k = G_k (e_{k+1} + delta_k)
// with G_k, Delta_k, delta_k known from the filter pass (rts_gain_kernel).  A chunk of steps is cut into
// spans; three passes:
//   pass 1 (one workgroup per span, all CUs):  compose the span's map  E_bot = Phi E_top Phi' + C,
//           e_bot = Phi e_top + c   by  Phi <- G Phi,  C <- G (C + Delta) G',  c <- G (c + delta)
//   pass 2 (one workgroup per problem, sequential over spans): boundary values E_top, e_top of every span
//   pass 3 (one workgroup per span): the reference recursion inside the span from its boundary value;
//           writes the smoothed means, marginals (and covariances when asked).
// All three are panel GEMMs on 4x4 register tiles: operands stream global(L2) -> registers -> LDS panels
// (double buffered, padded tiles, one LDS barrier per panel); every thread loads at most one tile per
// operand panel, one panel ahead of the arithmetic.
// One smoother chunk of a MERGED apply launch (the apply passes of all chunks whose boundary values exist run as one grid: every
// workgroup finds its chunk from its span index and takes the chunk's geometry and buffers from this table, which lives in
// host-pinned memory).
struct ChunkTab {
  long long k0;
  int nk, L, ns, first, span0, cap;    // span0: index of the chunk's first span in the merged grid; cap: stride of the chunk's buffer
  double *G, *d, *spanbuf, *spanvec, *bnd, *xbuf;
  size_t gps;                          // Bufs::gpstride of the chunk's buffer
};

struct SpanPar {
  int64_t k0;       // first step of the chunk
  int nk;           // steps in the chunk
  int chunk;        // chunk capacity (Gbuf stride)
  int L;            // span length
  int ns;           // spans in this chunk
  int ns_max;       // span-buffer stride
  int LP1, LP2;     // panel widths (tiles) of the dual / single operand GEMMs
  int first;        // first chunk of the sweep: E = 0, e = 0 at the top
  int write_PSs;
  double* spanbuf;  // [B][ns_max][2][ntiles*16]  Phi, C
  double* spanvec;  // [B][ns_max][S]             c
  double* bnd;      // [B][ns_max][ntiles*16 + S] E_top, e_top
  double* xbuf;     // [B][ns_max][ntiles*16]     per-workgroup scratch for X
  const ChunkTab* tab;  // merged apply launch: chunk table (nullptr: the fields above describe the one chunk of the launch)
  int ntab;
};

// merged launch: span index of the grid -> (chunk, span inside the chunk); the chunk's geometry and buffers replace those of the
// by-value parameter copies (all uniform over the workgroup)
template <class Par>
__device__ __forceinline__ int chunk_select(Par& sp, Bufs& b, int j) {
  int c = 0;
  while (c + 1 < sp.ntab && j >= sp.tab[c + 1].span0) ++c;
  const ChunkTab t = sp.tab[c];
  sp.k0 = t.k0; sp.nk = t.nk; sp.L = t.L; sp.ns = t.ns; sp.first = t.first; sp.chunk = t.cap;
  sp.spanbuf = t.spanbuf; sp.spanvec = t.spanvec; sp.bnd = t.bnd; sp.xbuf = t.xbuf;
  b.Gbuf = t.G; b.dbuf = t.d; b.gpstride = t.gps;
  return j - t.span0;
}

template <int TPT>
struct GemmCtx {
  int tid, NT, M, S;
  TileOwner<TPT> own;
  double* pan;       // LDS panels
  const int* ioff; const int* ibsz;
  int myblk, myrow;  // state row handled by this thread (tid < S)
};

// acc1 += A * (B1a + B1b) ; if DUAL: acc2 += A * (B2a + B2b)   (B?b may be null)
// optional: yv (register of thread tid < S) += sum_j A[tid, j] * v[j]   (v in LDS)
template <int TPT, bool DUAL>
__device__ __forceinline__ void gemm_nn(const GemmCtx<TPT>& c, int LP, double (*acc1)[16], double (*acc2)[16],
                                        const double* __restrict__ A, const double* __restrict__ B1a,
                                        const double* __restrict__ B1b, const double* __restrict__ B2a,
                                        const double* __restrict__ B2b, const double* v, double& yv) {
  const int M = c.M, nop = DUAL ? 3 : 2;
  const size_t panOp = (size_t)M * LP * TS;
  const int npan = (M + LP - 1) / LP;
  double t16[16];
  // task of this thread inside a panel of width lw: it -> (operand, tile)
  auto fetch = [&](int p) {
    const int l0 = p * LP, lw = (M - l0 < LP) ? (M - l0) : LP;
    const int it = c.tid;
    if (it < nop * M * lw) {
      const int op = it / (M * lw), r = it - op * M * lw;
      if (op == 0) {
        const int I = r / lw, l = r - I * lw;
        tile_load(t16, A + ((size_t)I * M + l0 + l) * 16);
      } else {
        const int l = r / M, J = r - l * M;
        const size_t tix = ((size_t)(l0 + l) * M + J) * 16;
        const double* Ba = (op == 1) ? B1a : B2a;
        const double* Bb = (op == 1) ? B1b : B2b;
        tile_load(t16, Ba + tix);
        if (Bb) {
          double u16[16];
          tile_load(u16, Bb + tix);
#pragma unroll
          for (int e = 0; e < 16; ++e) t16[e] += u16[e];
        }
      }
    }
  };
  auto publish = [&](int p) {
    const int l0 = p * LP, lw = (M - l0 < LP) ? (M - l0) : LP;
    double* base = c.pan + (size_t)(p & 1) * nop * panOp;
    const int it = c.tid;
    if (it < nop * M * lw) {
      const int op = it / (M * lw), r = it - op * M * lw;
      if (op == 0) {
        const int I = r / lw, l = r - I * lw;
        tile_store(base + ((size_t)l * M + I) * TS, t16);
      } else {
        const int l = r / M, J = r - l * M;
        tile_store(base + (size_t)op * panOp + ((size_t)l * M + J) * TS, t16);
      }
    }
  };
  fetch(0);
  for (int p = 0; p < npan; ++p) {
    const int l0 = p * LP, lw = (M - l0 < LP) ? (M - l0) : LP;
    publish(p);
    lds_barrier();
    if (p + 1 < npan) fetch(p + 1);
    const double* pg = c.pan + (size_t)(p & 1) * nop * panOp;
    const double* pb1 = pg + panOp;
    const double* pb2 = pb1 + panOp;
#pragma unroll
    for (int q = 0; q < TPT; ++q)
      if (c.own.ok[q]) {
#pragma unroll 2
        for (int l = 0; l < lw; ++l) {
          const double* a = pg + ((size_t)l * M + c.own.I[q]) * TS;
          tile_mma(acc1[q], a, pb1 + ((size_t)l * M + c.own.J[q]) * TS);
          if (DUAL) tile_mma(acc2[q], a, pb2 + ((size_t)l * M + c.own.J[q]) * TS);
        }
      }
    if (v && c.tid < c.S) {
      for (int l = 0; l < lw; ++l) {
        const double* g = pg + ((size_t)l * M + c.myblk) * TS + 4 * c.myrow;
        const double* vv = v + c.ioff[l0 + l];
        const int bs = c.ibsz[l0 + l];
        for (int j = 0; j < bs; ++j) yv = fma(g[j], vv[j], yv);
      }
    }
  }
}

// acc += A * Bt'   (A[I,L] and Bt[J,L] both global tile-major)
template <int TPT>
__device__ __forceinline__ void gemm_nt(const GemmCtx<TPT>& c, int LP, double (*acc)[16],
                                        const double* __restrict__ A, const double* __restrict__ Bt) {
  const int M = c.M;
  const size_t panOp = (size_t)M * LP * TS;
  const int npan = (M + LP - 1) / LP;
  double t16[16];
  auto fetch = [&](int p) {
    const int l0 = p * LP, lw = (M - l0 < LP) ? (M - l0) : LP;
    const int it = c.tid;
    if (it < 2 * M * lw) {
      const int op = it / (M * lw), r = it - op * M * lw;
      const int I = r / lw, l = r - I * lw;
      tile_load(t16, (op == 0 ? A : Bt) + ((size_t)I * M + l0 + l) * 16);
    }
  };
  auto publish = [&](int p) {
    const int l0 = p * LP, lw = (M - l0 < LP) ? (M - l0) : LP;
    double* base = c.pan + (size_t)(p & 1) * 2 * panOp;
    const int it = c.tid;
    if (it < 2 * M * lw) {
      const int op = it / (M * lw), r = it - op * M * lw;
      const int I = r / lw, l = r - I * lw;
      tile_store(base + (size_t)op * panOp + ((size_t)l * M + I) * TS, t16);
    }
  };
  fetch(0);
  for (int p = 0; p < npan; ++p) {
    const int l0 = p * LP, lw = (M - l0 < LP) ? (M - l0) : LP;
    publish(p);
    lds_barrier();
    if (p + 1 < npan) fetch(p + 1);
    const double* px = c.pan + (size_t)(p & 1) * 2 * panOp;
    const double* pg = px + panOp;
#pragma unroll
    for (int q = 0; q < TPT; ++q)
      if (c.own.ok[q]) {
#pragma unroll 2
        for (int l = 0; l < lw; ++l)
          tile_mma_nt(acc[q], px + ((size_t)l * M + c.own.I[q]) * TS, pg + ((size_t)l * M + c.own.J[q]) * TS);
      }
  }
}

template <int TPT>
__device__ __forceinline__ void span_setup(GemmCtx<TPT>& c, const Shape& sh, double* lds, double*& shv, double*& v0,
                                           double*& v1, double*& v2, const double* mdl) {
  c.tid = threadIdx.x; c.NT = blockDim.x; c.M = sh.M; c.S = sh.S;
  int* ioff = reinterpret_cast<int*>(lds);
  int* ibsz = ioff + (MAXM + 1);
  shv = lds + LDS_INT_DOUBLES;
  v0 = shv + ((sh.M + 2) & ~1);
  v1 = v0 + ((sh.S + 2) & ~1);
  v2 = v1 + ((sh.S + 2) & ~1);
  c.pan = v2 + ((sh.S + 2) & ~1);
  for (int i = c.tid; i <= sh.M; i += c.NT) ioff[i] = sh.off[i];
  for (int i = c.tid; i < sh.M; i += c.NT) ibsz[i] = sh.bsz[i];
  for (int i = c.tid; i < sh.M; i += c.NT) shv[i] = mdl[mdl_h(sh) + i];
  __syncthreads();
  c.ioff = ioff; c.ibsz = ibsz;
  c.myblk = 0; c.myrow = 0;
  if (c.tid < sh.S) {
    while (ioff[c.myblk + 1] <= c.tid) ++c.myblk;
    c.myrow = c.tid - ioff[c.myblk];
  }
  c.own.init(sh.M, sh.ntiles);
}
__host__ __device__ inline size_t span_lds_doubles(const Shape& s, int LP1, int LP2) {
  const size_t p1 = 2 * 3 * (size_t)s.M * LP1 * TS, p2 = 2 * 2 * (size_t)s.M * LP2 * TS;
  return LDS_INT_DOUBLES + (size_t)(s.M + 2) + 3 * (size_t)(s.S + 2) + (p1 > p2 ? p1 : p2) + 8;
}

// ---- pass 1: compose the affine map of one span
template <int TPT>
__global__ void __launch_bounds__(512) rts_compose_kernel(Shape sh, Bufs b, SpanPar sp) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int j = blockIdx.x, pb = blockIdx.y;
  const int ntl = sh.ntiles, S = sh.S, M = sh.M;
  const double* mdl = b.model + (size_t)pb * mdl_size(sh);
  GemmCtx<TPT> c; double *shv, *cv, *vv, *v2;
  span_setup(c, sh, lds, shv, cv, vv, v2, mdl);
  const int tid = c.tid, NT = c.NT;
  double* Phi = sp.spanbuf + (((size_t)pb * sp.ns_max + j) * 2) * ntl * 16;
  double* Cm = Phi + (size_t)ntl * 16;
  double* Xb = sp.xbuf + ((size_t)pb * sp.ns_max + j) * ntl * 16;
  // Phi = I, C = 0, c = 0
  for (int t = tid; t < ntl; t += NT) {
    double z[16]; tile_zero(z);
    tile_store(Cm + (size_t)t * 16, z);
    const int I = t / M, J = t - I * M;
    if (I == J) for (int i = 0; i < c.ibsz[I]; ++i) z[5 * i] = 1.0;
    tile_store(Phi + (size_t)t * 16, z);
  }
  if (tid < S) cv[tid] = 0.0;
  __syncthreads();
  const int a = j * sp.L, e = (a + sp.L < sp.nk) ? a + sp.L : sp.nk;
  for (int kk = e - 1; kk >= a; --kk) {
    const double* Gk = b.Gbuf + (((size_t)pb * sp.chunk + kk) * 2) * ntl * 16;
    const double* Dk = Gk + (size_t)ntl * 16;
    const double* dk = b.dbuf + ((size_t)pb * sp.chunk + kk) * S;
    if (tid < S) vv[tid] = cv[tid] + dk[tid];
    lds_barrier();
    double accX[TPT][16];
    double cn = 0.0;
    if constexpr (TPT <= 2) {
      // G [Phi | C + Delta] in one pass over the G panels (two accumulator sets)
      double accP[TPT][16];
#pragma unroll
      for (int q = 0; q < TPT; ++q) { tile_zero(accP[q]); tile_zero(accX[q]); }
      gemm_nn<TPT, true>(c, sp.LP1, accP, accX, Gk, Phi, nullptr, Cm, Dk, vv, cn);
      __syncthreads();   // every read of Phi / C (global) and vv is done
#pragma unroll
      for (int q = 0; q < TPT; ++q)
        if (c.own.ok[q]) {
          tile_store(Phi + (size_t)(tid + q * NT) * 16, accP[q]);
          tile_store(Xb + (size_t)(tid + q * NT) * 16, accX[q]);
        }
    } else {
      // three and more tiles per thread: two accumulator sets would not fit the registers (407 spilled VGPRs at
      // TPT = 3) -- two passes over the G panels with one set instead
#pragma unroll
      for (int q = 0; q < TPT; ++q) tile_zero(accX[q]);
      double dummy = 0.0;
      gemm_nn<TPT, false>(c, sp.LP1, accX, accX, Gk, Phi, nullptr, nullptr, nullptr, nullptr, dummy);
      __syncthreads();
#pragma unroll
      for (int q = 0; q < TPT; ++q) {
        if (c.own.ok[q]) tile_store(Phi + (size_t)(tid + q * NT) * 16, accX[q]);
        tile_zero(accX[q]);
      }
      gemm_nn<TPT, false>(c, sp.LP1, accX, accX, Gk, Cm, Dk, nullptr, nullptr, vv, cn);
      __syncthreads();
#pragma unroll
      for (int q = 0; q < TPT; ++q)
        if (c.own.ok[q]) tile_store(Xb + (size_t)(tid + q * NT) * 16, accX[q]);
    }
    if (tid < S) cv[tid] = cn;
    __syncthreads();   // X visible
#pragma unroll
    for (int q = 0; q < TPT; ++q) tile_zero(accX[q]);
    gemm_nt<TPT>(c, sp.LP2, accX, Xb, Gk);
#pragma unroll
    for (int q = 0; q < TPT; ++q)
      if (c.own.ok[q]) tile_store(Cm + (size_t)(tid + q * NT) * 16, accX[q]);
    __syncthreads();   // C visible, panels free
  }
  if (tid < S) sp.spanvec[((size_t)pb * sp.ns_max + j) * S + tid] = cv[tid];
}

// ---- pass 2: boundary values, sequential over the spans of the chunk (top span first)
template <int TPT>
__global__ void __launch_bounds__(512) rts_boundary_kernel(Shape sh, Bufs b, SpanPar sp) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int pb = blockIdx.x;
  const int ntl = sh.ntiles, S = sh.S;
  const double* mdl = b.model + (size_t)pb * mdl_size(sh);
  GemmCtx<TPT> c; double *shv, *ev, *v1, *v2;
  span_setup(c, sh, lds, shv, ev, v1, v2, mdl);
  const int tid = c.tid, NT = c.NT;
  double* Est = b.state + (size_t)pb * ((size_t)ntl * 16 + S);
  double* est = Est + (size_t)ntl * 16;
  double* Xb = sp.xbuf + ((size_t)pb * sp.ns_max) * ntl * 16;
  if (sp.first) {
    for (int i = tid; i < ntl * 16; i += NT) Est[i] = 0.0;
    for (int i = tid; i < S; i += NT) est[i] = 0.0;
  }
  __syncthreads();
  for (int j = sp.ns - 1; j >= 0; --j) {
    const double* Phi = sp.spanbuf + (((size_t)pb * sp.ns_max + j) * 2) * ntl * 16;
    const double* Cm = Phi + (size_t)ntl * 16;
    double* Bj = sp.bnd + ((size_t)pb * sp.ns_max + j) * ((size_t)ntl * 16 + S);
    // E_top of span j
    for (int i = tid; i < ntl * 8; i += NT) reinterpret_cast<double2*>(Bj)[i] = reinterpret_cast<const double2*>(Est)[i];
    if (tid < S) { const double e0 = est[tid]; Bj[(size_t)ntl * 16 + tid] = e0; ev[tid] = e0; }
    lds_barrier();
    double acc[TPT][16], dummy[1][16];
#pragma unroll
    for (int q = 0; q < TPT; ++q) tile_zero(acc[q]);
    double en = 0.0;
    gemm_nn<TPT, false>(c, sp.LP2, acc, reinterpret_cast<double(*)[16]>(dummy), Phi, Est, nullptr, nullptr, nullptr, ev, en);
    __syncthreads();
#pragma unroll
    for (int q = 0; q < TPT; ++q)
      if (c.own.ok[q]) tile_store(Xb + (size_t)(tid + q * NT) * 16, acc[q]);
    __syncthreads();
#pragma unroll
    for (int q = 0; q < TPT; ++q)
      if (c.own.ok[q]) tile_load(acc[q], Cm + (size_t)(tid + q * NT) * 16); else tile_zero(acc[q]);
    gemm_nt<TPT>(c, sp.LP2, acc, Xb, Phi);
#pragma unroll
    for (int q = 0; q < TPT; ++q)
      if (c.own.ok[q]) tile_store(Est + (size_t)(tid + q * NT) * 16, acc[q]);
    if (tid < S) est[tid] = en + sp.spanvec[((size_t)pb * sp.ns_max + j) * S + tid];
    __syncthreads();
  }
}

// ---- pass 3: the recursion inside one span, outputs
template <int TPT>
__global__ void __launch_bounds__(512) rts_apply_kernel(Shape sh, Bufs b, SpanPar sp) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  int j = blockIdx.x; const int pb = blockIdx.y;
  if (sp.tab) j = chunk_select(sp, b, j);
  const int ntl = sh.ntiles, S = sh.S, M = sh.M;
  const int64_t T = sh.T;
  const double* mdl = b.model + (size_t)pb * mdl_size(sh);
  GemmCtx<TPT> c; double *shv, *ec, *vv, *v2;
  span_setup(c, sh, lds, shv, ec, vv, v2, mdl);
  const int tid = c.tid, NT = c.NT;
  double* Bj = sp.bnd + ((size_t)pb * sp.ns_max + j) * ((size_t)ntl * 16 + S);   // E (updated in place), e_top
  double* Xb = sp.xbuf + ((size_t)pb * sp.ns_max + j) * ntl * 16;
  if (tid < S) ec[tid] = Bj[(size_t)ntl * 16 + tid];
  lds_barrier();
  double mxM = 0.0, mxP = 0.0;
  const int a = j * sp.L, e = (a + sp.L < sp.nk) ? a + sp.L : sp.nk;
  for (int kk = e - 1; kk >= a; --kk) {
    const int64_t k = sp.k0 + kk;
    const double* Gk = b.Gbuf + (((size_t)pb * sp.chunk + kk) * 2) * ntl * 16;
    const double* Dk = Gk + (size_t)ntl * 16;
    const double* dk = b.dbuf + ((size_t)pb * sp.chunk + kk) * S;
    if (tid < S) vv[tid] = ec[tid] + dk[tid];
    lds_barrier();
    double acc[TPT][16], dummy[1][16];
#pragma unroll
    for (int q = 0; q < TPT; ++q) tile_zero(acc[q]);
    double en = 0.0;
    gemm_nn<TPT, false>(c, sp.LP2, acc, reinterpret_cast<double(*)[16]>(dummy), Gk, Bj, Dk, nullptr, nullptr, vv, en);
    __syncthreads();
#pragma unroll
    for (int q = 0; q < TPT; ++q)
      if (c.own.ok[q]) tile_store(Xb + (size_t)(tid + q * NT) * 16, acc[q]);
    if (tid < S) ec[tid] = en;
    __syncthreads();
#pragma unroll
    for (int q = 0; q < TPT; ++q) tile_zero(acc[q]);
    gemm_nt<TPT>(c, sp.LP2, acc, Xb, Gk);
    // ---- store E_k, outputs
    const double* PFk = b.PF + ((size_t)pb * T + k) * pf_step_doubles(sh);
#pragma unroll
    for (int q = 0; q < TPT; ++q)
      if (c.own.ok[q]) {
        const int t = tid + q * NT;
        tile_store(Bj + (size_t)t * 16, acc[q]);
        if (c.own.I[q] == c.own.J[q]) {
          const int n = c.own.I[q];
          const size_t ix = ((size_t)pb * T + k) * M + n;
          const double vnew = b.fv[ix] + shv[n] * shv[n] * acc[q][0];
          if (md_counts(b, pb, T, k)) mxP = fmax(mxP, fabs(b.sv[ix] - vnew));
          b.sv[ix] = vnew;
        }
        if (sp.write_PSs || k == 0) {
          double ps[16];
          pf_load(ps, PFk, c.own.I[q], c.own.J[q]);
#pragma unroll
          for (int x = 0; x < 16; ++x) ps[x] += acc[q][x];
          if (sp.write_PSs) tile_store(b.PSs + (((size_t)pb * T + k) * ntl + t) * 16, ps);
          if (k == 0) tile_store(b.state + (size_t)pb * ((size_t)ntl * 16 + S) + (size_t)t * 16, ps);   // smoothed P_0 (EKF restart)
        }
      }
    if (tid < S) {
      const double ms = b.MF[((size_t)pb * T + k) * S + tid] + en;
      b.MS[((size_t)pb * T + k) * S + tid] = ms;
      if (k == 0) b.state[(size_t)pb * ((size_t)ntl * 16 + S) + (size_t)ntl * 16 + tid] = ms;
      if (c.myrow == 0) {
        const size_t ix = ((size_t)pb * T + k) * M + c.myblk;
        const double mnew = shv[c.myblk] * ms;
        if (md_counts(b, pb, T, k)) mxM = fmax(mxM, fabs(b.sm[ix] - mnew));
        b.sm[ix] = mnew;
      }
    }
    __syncthreads();
  }
  mxM = wave_max(mxM);
  mxP = wave_max(mxP);
  if ((tid & 63) == 0) {
    atomicMax(reinterpret_cast<unsigned long long*>(&b.red[(size_t)pb * 8 + 1]), (unsigned long long)__double_as_longlong(mxM));
    atomicMax(reinterpret_cast<unsigned long long*>(&b.red[(size_t)pb * 8 + 2]), (unsigned long long)__double_as_longlong(mxP));
  }
}

// ---------------------------------------------------------------------------------------------
// Power-EP site refresh, parallel over steps (gf_ep_modulator_nmf.m:236-268,
// ihgp_ep_modulator_nmf.m:397-436): cavity from the smoothed marginals, mom(alpha), damped update.
struct EpPar {
  int64_t k_end;       // steps 0 .. k_end-1 are refreshed (T-1)
  int steps_per_wg;
  double alpha;
  double w_old, w_new; // site <- w_old*site + w_new*(...): (1-d*alpha, d) gf_ep_modulator_nmf.m:259-262 ; (1-d, d/alpha) gf_ep_mods_nmf_mixture.m:280-281
  int clamp;           // gf predict mode: ttau = max(ttau,0) after the update, R = 1/ttau for all sites
  int write_R;         // 0: none (nlml), 1: all sites (gf predict), 2: updated sites only (ihgp)
  double* lZ_out;      // [B][T] where the per-step log Z goes (gf: b.lZ ; ihgp: separate array ; null: dropped, gf_ep_mods_nmf_mixture.m:277)
  int const_var;       // ihgp: marginal variance is read from sv[k] as usual (kept for clarity)
  int64_t k_begin;     // first step of this launch (0: the whole sequence; > 0: one smoother chunk of the cross-sweep schedule)
};

__host__ __device__ inline size_t ep_lds_doubles(const Shape& s, const MomCfg& mc) {
  return (size_t)s.D * s.N + 4 * (size_t)s.M + 8 + mom_lds_doubles(mc);
}

// throughput kernel (one workgroup per few steps): capped at 256 registers so that two workgroups share a CU
template <int MV>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) ep_site_kernel(Shape sh, Bufs b, MomCfg mc, EpPar ep) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int tid = threadIdx.x, NT = blockDim.x;
  const int M = sh.M, Ms = sh.Ms;      // Ms < M: tail rows of split blocks behind the real sites (no site arithmetic there)
  const int64_t T = sh.T;
  const int pb = blockIdx.y;
  const double* mdl = b.model + (size_t)pb * mdl_size(sh);
  double* sW = lds;
  double* mc_ = sW + (size_t)sh.D * sh.N;   // m_cav [M]
  double* vc_ = mc_ + M;                    // v_cav [M]
  double* dl = vc_ + M;
  double* d2l = dl + M;
  double* misc = d2l + M;
  double* ws = misc + 8;
  for (int i = tid; i < sh.D * sh.N; i += NT) sW[i] = mdl[mdl_W(sh) + i];
  const double sn2 = mdl[mdl_sn2(sh)];
  mom_cache_tables(mc, ws);
  const double pEPa = mom_pEP(mc, sn2, ep.alpha);
  lds_barrier();
  const int64_t kb = ep.k_begin + (int64_t)blockIdx.x * ep.steps_per_wg;
  unsigned long long n_clamped = 0;
  for (int64_t k = kb; k < kb + ep.steps_per_wg && k < ep.k_end; ++k) {
    const double yk = b.y[(size_t)pb * T + k];
    if (yk != yk) continue;   // isnan(y_k): no EP update (uniform)
    const size_t ix = ((size_t)pb * T + k) * M + tid;
    double t_old = 0.0, n_old = 0.0, vcav = 0.0, mcav = 0.0;
    if (tid < Ms) {
      t_old = b.ttau[ix]; n_old = b.tnu[ix];
      const double vm = b.sv[ix], mm = b.sm[ix];
      vcav = 1.0 / (1.0 / vm - ep.alpha * t_old);
      mcav = vcav * (mm / vm - ep.alpha * n_old);
      mc_[tid] = mcav; vc_[tid] = vcav;
    }
    lds_barrier();
    mom_eval<MV>(mc, sW, pEPa, sn2, ep.alpha, yk, mc_, vc_, ws, &misc[0], dl, d2l);
    if (tid < Ms) {
      const bool upd = vcav > 0.0;
      double tnew = t_old, nnew = n_old;
      if (upd) {
        const double d1 = dl[tid], d2 = d2l[tid];
        tnew = ep.w_old * t_old + ep.w_new * (-d2 / (1.0 + d2 * vcav));
        nnew = ep.w_old * n_old + ep.w_new * ((d1 - mcav * d2) / (1.0 + d2 * vcav));
      }
      if (ep.clamp) { if (!(tnew > 0.0)) ++n_clamped; tnew = max0(tnew); }
      b.ttau[ix] = tnew; b.tnu[ix] = nnew;
      if (ep.write_R == 1 || (ep.write_R == 2 && upd)) b.R[ix] = 1.0 / tnew;
    }
    if (tid == 0 && ep.lZ_out) ep.lZ_out[(size_t)pb * T + k] = misc[0];
    lds_barrier();
  }
  if (tid < Ms && n_clamped) atomicAdd(&b.counters[(size_t)pb * 4 + 1], n_clamped);
}

// The same refresh with likModulatorNMFPower in the staged sparse-point form of nagp_momsp.hpp (fully symmetric sigma-point sets,
// <= 7 components, <= 320 points: what the ADF launches of the filters use): the cavity marginals go where the stages read the
// predicted ones, the sites live in wave 0.  Four times fewer instructions per evaluation than the generic mom_eval.
__host__ __device__ inline size_t ep_sp_lds_doubles(const Shape& s, int CD) { return (size_t)s.D * CD + 2 * 68 + msp_lds_doubles(CD, s.D); }
template <int CD>
__global__ void __launch_bounds__(MSP_NT) __attribute__((amdgpu_waves_per_eu(2))) ep_site_sp_kernel(Shape sh, Bufs b, MomCfg mc, EpPar ep) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int tid = threadIdx.x, NT = blockDim.x;
  const int M = sh.M, D = sh.D;
  const int64_t T = sh.T;
  const int pb = blockIdx.y;
  const double* mdl = b.model + (size_t)pb * mdl_size(sh);
  double* sW = lds;                          // [D][CD]
  double* fmu = sW + (size_t)D * CD;         // cavity means, 68 entries (zero beyond the M sites: stage A reads 4*K of them)
  double* HPH = fmu + 68;                    // cavity variances
  double* ws = HPH + 68;
  for (int i = tid; i < D * CD; i += NT) sW[i] = mdl[mdl_W(sh) + i];
  for (int i = tid; i < 68; i += NT) { fmu[i] = 0.0; HPH[i] = 0.0; }
  const double sn2 = mdl[mdl_sn2(sh)];
  const double pEPa = mom_pEP(mc, sn2, ep.alpha), sn2a = sn2 / ep.alpha;
  __syncthreads();
  MspCtx<CD> xsp;
  msp_setup<CD>(xsp, mc, mc.sp, sW, fmu, HPH, ws);
  double wrow[CD];
#pragma unroll
  for (int j = 0; j < CD; ++j) wrow[j] = (tid < D) ? sW[tid * CD + j] : 0.0;
  __syncthreads();
  const int64_t kb = ep.k_begin + (int64_t)blockIdx.x * ep.steps_per_wg;
  unsigned long long n_clamped = 0;
  for (int64_t k = kb; k < kb + ep.steps_per_wg && k < ep.k_end; ++k) {
    const double yk = b.y[(size_t)pb * T + k];
    if (yk != yk) continue;   // isnan(y_k): no EP update (uniform)
    const size_t ix = ((size_t)pb * T + k) * M + tid;
    double t_old = 0.0, n_old = 0.0, vcav = 0.0, mcav = 0.0;
    if (tid < M) {
      t_old = b.ttau[ix]; n_old = b.tnu[ix];
      const double vm = b.sv[ix], mm = b.sm[ix];
      vcav = 1.0 / (1.0 / vm - ep.alpha * t_old);
      mcav = vcav * (mm / vm - ep.alpha * n_old);
      fmu[tid] = mcav; HPH[tid] = vcav;
    }
    lds_barrier();
    msp_stageA<CD>(xsp, mc);
    lds_barrier();
    msp_stageB<CD>(xsp, mc, ws);
    lds_barrier();
    msp_stage1b<CD>(xsp, mc, mc.sp, sn2a, yk, ws);
    lds_barrier();
    msp_stage2<CD>(xsp, mc, ws);
    lds_barrier();
    if (tid < 64) {       // the sites live in wave 0: partial sums and outputs without another workgroup barrier
      msp_reduce<CD>(xsp);
      msp_wave_fence();
      if (tid < M) {
        double Zv, d1, d2;
        msp_outputs<CD>(xsp.accp, tid < D, tid - D, wrow, pEPa, mc.jitter, Zv, d1, d2);
        const bool upd = vcav > 0.0;
        double tnew = t_old, nnew = n_old;
        if (upd) {
          tnew = ep.w_old * t_old + ep.w_new * (-d2 / (1.0 + d2 * vcav));
          nnew = ep.w_old * n_old + ep.w_new * ((d1 - mcav * d2) / (1.0 + d2 * vcav));
        }
        if (ep.clamp) { if (!(tnew > 0.0)) ++n_clamped; tnew = max0(tnew); }
        b.ttau[ix] = tnew; b.tnu[ix] = nnew;
        if (ep.write_R == 1 || (ep.write_R == 2 && upd)) b.R[ix] = 1.0 / tnew;
        if (tid == 0 && ep.lZ_out) ep.lZ_out[(size_t)pb * T + k] = log(Zv);
      }
    }
    lds_barrier();        // fmu / HPH and the tables are rewritten by the next step
  }
  if (tid < M && n_clamped) atomicAdd(&b.counters[(size_t)pb * 4 + 1], n_clamped);
}

// The refresh with likModulatorPreCalcwn in the staged form of nagp_momsq.hpp (flat layout: four waves in every stage): symmetric rules,
// <= 6 components, <= 32 sub-bands, <= 320 points; mc.sp.c0 = code of the centre coordinate.
__host__ __device__ inline size_t ep_sq_lds_doubles(const Shape& s, int CD) { return (size_t)s.D * CD + 2 * 68 + 512 + msq_lds_doubles<MsqFlat>(CD); }
template <int CD>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) ep_site_sq_kernel(Shape sh, Bufs b, MomCfg mc, EpPar ep) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int tid = threadIdx.x, NT = blockDim.x;
  const int M = sh.M, D = sh.D;
  const int64_t T = sh.T;
  const int pb = blockIdx.y;
  const double* mdl = b.model + (size_t)pb * mdl_size(sh);
  double* sW = lds;                          // [D][CD]
  double* fmu = sW + (size_t)D * CD;         // cavity means, 68 entries (zero beyond the M sites)
  double* HPH = fmu + 68;                    // cavity variances
  double* wt = HPH + 68;                     // [8][64] W transposed (stage A)
  double* ws = wt + 512;
  for (int i = tid; i < D * CD; i += NT) sW[i] = mdl[mdl_W(sh) + i];
  for (int i = tid; i < 68; i += NT) { fmu[i] = 0.0; HPH[i] = 0.0; }
  msq_init<MsqFlat>(CD, ws, NT);
  const double sn2 = mdl[mdl_sn2(sh)];
  const double pEPa = mom_pEP(mc, sn2, ep.alpha), sn2a = sn2 / ep.alpha;
  __syncthreads();
  const MsqLay lay = msq_layout<MsqFlat>(CD);
  const int wave = tid >> 6;
  MsqW<CD, MsqFlat> xq;
  msq_setup_W<CD, MsqFlat>(xq, mc, mc.sp.c0, sW, fmu, HPH, ws, wave, tid, wt, 1);
  MsqLink xl;
  msqf_setup_link<CD>(xl, mc, fmu, HPH, ws);
  MsqM xm;
  msq_setup_M<CD, MsqFlat>(xm, mc, mc.sp.c0, ws, (wave >= 2) ? wave - 2 : 2);      // marginal sums on waves 2, 3
  const msp_rp accp = (msp_rp)(ws + lay.acc) + opaque_zero();
  const msp_rp partp = (msp_rp)(ws + lay.part + (tid & 15) + 16 * ((tid >> 4) & 1));
  double amp[2 * MsqFlat::NST];
#pragma unroll
  for (int i = 0; i < 2 * MsqFlat::NST; ++i) amp[i] = 0.0;
  __syncthreads();
  const int64_t kb = ep.k_begin + (int64_t)blockIdx.x * ep.steps_per_wg;
  unsigned long long n_clamped = 0;
  for (int64_t k = kb; k < kb + ep.steps_per_wg && k < ep.k_end; ++k) {
    const double yk = b.y[(size_t)pb * T + k];
    if (yk != yk) continue;   // isnan(y_k): no EP update (uniform)
    const size_t ix = ((size_t)pb * T + k) * M + tid;
    double t_old = 0.0, n_old = 0.0, vcav = 0.0, mcav = 0.0;
    if (tid < M) {
      t_old = b.ttau[ix]; n_old = b.tnu[ix];
      const double vm = b.sv[ix], mm = b.sm[ix];
      vcav = 1.0 / (1.0 / vm - ep.alpha * t_old);
      mcav = vcav * (mm / vm - ep.alpha * n_old);
      fmu[tid] = mcav; HPH[tid] = vcav;
    }
    lds_barrier();
    double Zv = 0.0, d1 = 0.0, d2 = 0.0;
    msqf_eval<CD>(xq, xl, xm, mc, amp, sn2a, yk, accp, partp, tid < D, tid - D, pEPa, tid < M, Zv, d1, d2);
    if (tid < M) {
      const bool upd = vcav > 0.0;
      double tnew = t_old, nnew = n_old;
      if (upd) {
        tnew = ep.w_old * t_old + ep.w_new * (-d2 / (1.0 + d2 * vcav));
        nnew = ep.w_old * n_old + ep.w_new * ((d1 - mcav * d2) / (1.0 + d2 * vcav));
      }
      if (ep.clamp) { if (!(tnew > 0.0)) ++n_clamped; tnew = max0(tnew); }
      b.ttau[ix] = tnew; b.tnu[ix] = nnew;
      if (ep.write_R == 1 || (ep.write_R == 2 && upd)) b.R[ix] = 1.0 / tnew;
      if (tid == 0 && ep.lZ_out) ep.lZ_out[(size_t)pb * T + k] = log(Zv);
    }
    lds_barrier();        // fmu / HPH and the tables are rewritten by the next step
  }
  if (tid < M && n_clamped) atomicAdd(&b.counters[(size_t)pb * 4 + 1], n_clamped);
}

// ---------------------------------------------------------------------------------------------
// Deterministic reductions: out[pb*8 + slot] = sum_{k in [k_lo,k_hi)} v[pb][k]   (skipping nothing:
// entries that were never written are zero, like the reference's zeros(1,T) initialisation).
static __global__ void __launch_bounds__(1024) sum_kernel(const double* v, int64_t T, int64_t k_lo, int64_t k_hi, double* out, int slot) {
  __shared__ double part[16];
  const int tid = threadIdx.x, NT = blockDim.x, pb = blockIdx.x;
  const double* p = v + (size_t)pb * T;
  // fixed blocking: thread t sums a contiguous slice in order, then a fixed tree
  const int64_t n = k_hi - k_lo;
  const int64_t per = (n + NT - 1) / NT;
  const int64_t a = k_lo + (int64_t)tid * per;
  const int64_t e = (a + per < k_hi) ? a + per : k_hi;
  double s = 0.0;
  for (int64_t k = a; k < e; ++k) s += p[k];
  s = wave_sum(s);
  if ((tid & 63) == 0) part[tid >> 6] = s;
  __syncthreads();
  if (tid == 0) {
    double tot = 0.0;
    for (int w = 0; w < (NT >> 6); ++w) tot += part[w];
    out[(size_t)pb * 8 + slot] = tot;
  }
}


// ---------------------------------------------------------------------------------------------
// The reference's `mom` callback on its own (likModulatorPower.m:25-100, likModulatorNMFPower.m:28-87,
// experiments/likModulatorPreCalcwn.m:28-86): one workgroup per evaluation, inputs (y, mu[M], s2[M]).
struct MomPar {
  int D, N, M;
  double sn2, alpha;
  const double* W;    // [D][N] row-major (device) or null
  const double* y;    // [n]
  const double* mu;   // [n][M]
  const double* s2;   // [n][M]
  double* lZ;         // [n]
  double* dl;         // [n][M]
  double* d2l;        // [n][M]
  int64_t n;
};
__host__ __device__ inline size_t momk_lds_doubles(int D, int N, int M, const MomCfg& mc) {
  return (size_t)D * N + 4 * (size_t)M + 8 + mom_lds_doubles(mc);
}
template <int MV>
__global__ void __launch_bounds__(256) mom_kernel(MomCfg mc, MomPar mp) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int tid = threadIdx.x, NT = blockDim.x, M = mp.M;
  double* sW = lds;
  double* mu = sW + (size_t)mp.D * mp.N;
  double* s2 = mu + M;
  double* dl = s2 + M;
  double* d2l = dl + M;
  double* misc = d2l + M;
  double* ws = misc + 8;
  for (int i = tid; i < mp.D * mp.N; i += NT) sW[i] = mp.W ? mp.W[i] : 0.0;
  mom_cache_tables(mc, ws);
  const double pEPa = mom_pEP(mc, mp.sn2, mp.alpha);
  for (int64_t e = blockIdx.x; e < mp.n; e += gridDim.x) {
    if (tid < M) { mu[tid] = mp.mu[(size_t)e * M + tid]; s2[tid] = mp.s2[(size_t)e * M + tid]; }
    lds_barrier();
    mom_eval<MV>(mc, sW, pEPa, mp.sn2, mp.alpha, mp.y[e], mu, s2, ws, &misc[0], dl, d2l);
    if (tid < M) { mp.dl[(size_t)e * M + tid] = dl[tid]; mp.d2l[(size_t)e * M + tid] = d2l[tid]; }
    if (tid == 0) mp.lZ[e] = misc[0];
    lds_barrier();
  }
}


// ---------------------------------------------------------------------------------------------
// iekf_update1.m:110-117 / ekf_update1.m:106-109 on their own, with the measurement model of
// gf_giekf_modulator_nmf_constraints.m:492-502:  h(x) = (H_z x)' W softplus(H_g x),  J = dh/dx.
//   for it = 1:iters:  J = dh(M); MU = h(M); S = R + J P J'; K = P J'/S; M = M + K (y - MU);   P = P - K S K'
// One workgroup; P dense column-major in HBM (S <= 512 states), H given as (column, value) per site.
struct EkfPar {
  int S, D, N, iters;
  double R, y;
  const int* hcol;      // [D+N]
  const double* hval;   // [D+N]
  const double* W;      // [D][N] row-major
  double* m;            // [S]    in/out
  double* P;            // [S][S] column-major, in/out
  double* K;            // [S]    out
  double* MU_S;         // [2]    out: MU, S of the last iteration
};
static __global__ void __launch_bounds__(256) iekf_update1_kernel(EkfPar ep) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int tid = threadIdx.x, NT = blockDim.x, S = ep.S, D = ep.D, N = ep.N, M = D + N;
  double* m = lds;          // [S]
  double* f = m + S;        // [M]  H m
  double* J = f + M;        // [M]  non-zeros of the Jacobian row
  double* PJ = J + M;       // [S]
  double* red = PJ + S;     // [2]
  for (int i = tid; i < S; i += NT) m[i] = ep.m[i];
  __syncthreads();
  double Sx = 1.0, MU = 0.0;
  for (int it = 0; it < ep.iters; ++it) {
    for (int n = tid; n < M; n += NT) f[n] = ep.hval[n] * m[ep.hcol[n]];
    __syncthreads();
    for (int n = tid; n < M; n += NT) {
      double pv = 0.0;
      if (n < D) {
        for (int j = 0; j < N; ++j) pv = fma(ep.W[n * N + j], log(1.0 + exp(f[D + j])), pv);
      } else {
        const int j = n - D;
        double zw = 0.0;
        for (int dd = 0; dd < D; ++dd) zw = fma(f[dd], ep.W[dd * N + j], zw);
        const double eg = exp(f[D + j]);
        pv = zw * (eg / (eg + 1.0));
      }
      J[n] = pv * ep.hval[n];
    }
    __syncthreads();
    for (int i = tid; i < S; i += NT) {
      double acc = 0.0;
      for (int n = 0; n < M; ++n) acc = fma(ep.P[(size_t)ep.hcol[n] * S + i], J[n], acc);   // (P J')_i = sum_n P(i, c_n) J_n
      PJ[i] = acc;
    }
    if (tid == 0) {
      double mu = 0.0;
      for (int dd = 0; dd < D; ++dd) mu = fma(f[dd], J[dd] / ep.hval[dd], mu);   // h = sum_d z_d (W softplus(g))_d
      red[1] = mu;
    }
    __syncthreads();
    if (tid == 0) {
      double jpj = 0.0;
      for (int n = 0; n < M; ++n) jpj = fma(J[n], PJ[ep.hcol[n]], jpj);
      red[0] = ep.R + jpj;
    }
    __syncthreads();
    Sx = red[0]; MU = red[1];
    for (int i = tid; i < S; i += NT) m[i] = m[i] + (PJ[i] / Sx) * (ep.y - MU);
    __syncthreads();
  }
  for (size_t e = tid; e < (size_t)S * S; e += NT) {
    const int i = (int)(e % S), j = (int)(e / S);
    const double Ki = PJ[i] / Sx, Kj = PJ[j] / Sx;
    ep.P[e] -= (Ki * Sx) * Kj;
  }
  for (int i = tid; i < S; i += NT) { ep.m[i] = m[i]; ep.K[i] = PJ[i] / Sx; }
  if (tid == 0) { ep.MU_S[0] = MU; ep.MU_S[1] = Sx; }
}


// ---------------------------------------------------------------------------------------------
// Stationary filterbank: infinite-horizon Kalman filter and steady-state RTS smoother of
// unifying_prob_tf/kernel_ss_kalmanFastFB.m.  Both recursions are affine with time-constant matrices
//   filter   (:83-110)   m_k = M_k m_{k-1} + u_k,   M_k = AKHA, u_k = K y_k   (y_k observed)  |  M_k = A, u_k = 0  (NaN)
//   smoother (:134-151)  m_k = G m_{k+1} + (MS_k - G A MS_k)
// so they run PARALLEL IN TIME over spans of L steps: pass 1 composes every span to (Phi_j, c_j) with the span's own
// matrices, pass 2 walks the span boundaries, pass 3 replays the reference recursion inside every span from its exact
// boundary value.  All matrices live in LDS, transposed (thread i walks along row i with conflict-free reads).
constexpr int FB_CHK = 16;
struct FbPar {
  int S;
  int64_t T;
  const double* A;      // [S][S] column-major  (predict-only steps / smoother)
  const double* B;      // filter: AKHA = A - K H A ; smoother: G      [S][S] column-major
  const double* HA;     // [S]  H*A        (filter)
  const double* K;      // [S]  gain       (filter)
  const double* y;      // [T]             (filter)
  double* MS;           // [T][S] filtered (filter: out) / smoothed (smoother: in-out)
  double* sum_v2;       // [ns] per span: sum over observed steps of (y - HA m)^2   (filter)
  int64_t L;            // span length; span j = steps [j L, min((j+1) L, n)) of n = T (filter) or T-1 (smoother) steps
  int ns;               // spans
  double* Phi;          // [ns][S][SP]  pass 1 out (row-major, SP = S + 4; column S = c_j)
  double* starts;       // [ns][S]      pass 2 out: value entering span j
  int mat_global;       // filter / smoother pass: the two S x S matrices stay in global memory (L2-resident, coalesced column reads) -- S > 96, where they do not fit the LDS
};
__host__ __device__ inline size_t fb_lds_doubles(int S, int mat_global = 0) { return (mat_global ? 0 : 2 * (size_t)S * S) + 5 * (size_t)S + (size_t)FB_CHK * (S + 1) + 8; }
__host__ __device__ inline size_t fb_compose_lds_doubles(int S) { return 2 * (size_t)S * S + 2 * (size_t)(S + 4) * (S + 4) + 3 * (size_t)S + 8; }

// pass 3 (and the whole job when ns == 1):  if ~isnan(y): v = y - HA*m; m = AKHA*m + K*y; else m = A*m
static __global__ void __launch_bounds__(256) fastfb_filter_kernel(FbPar fp) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int tid = threadIdx.x, NT = blockDim.x, S = fp.S;
  const bool mg = fp.mat_global != 0;
  const double* At = mg ? fp.A : lds;                       // At[j*S + i] = A(i,j): the column-major input is already this layout
  const double* Bt = mg ? fp.B : lds + (size_t)S * S;
  double* ha = lds + (mg ? 0 : 2 * (size_t)S * S);
  double* kg = ha + S;
  double* m0 = kg + S;
  double* m1 = m0 + S;
  double* yc = m1 + S + S;                // [FB_CHK]
  double* msc = yc + FB_CHK;              // [FB_CHK][S] staged output
  const int64_t ka = (int64_t)blockIdx.x * fp.L, kb = (ka + fp.L < fp.T) ? ka + fp.L : fp.T;
  if (!mg) for (int e = tid; e < S * S; e += NT) { lds[e] = fp.A[e]; lds[(size_t)S * S + e] = fp.B[e]; }
  for (int i = tid; i < S; i += NT) { ha[i] = fp.HA[i]; kg[i] = fp.K[i]; m0[i] = fp.starts ? fp.starts[(size_t)blockIdx.x * S + i] : 0.0; }
  double sv2 = 0.0;
  __syncthreads();
  double* mc = m0;
  double* mn = m1;
  for (int64_t k0 = ka; k0 < kb; k0 += FB_CHK) {
    const int nb = (kb - k0 < FB_CHK) ? (int)(kb - k0) : FB_CHK;
    for (int i = tid; i < nb; i += NT) yc[i] = fp.y[k0 + i];
    __syncthreads();
    for (int kk = 0; kk < nb; ++kk) {
      const double yk = yc[kk];
      const bool obs = !(yk != yk);
      if (tid < S) {
        const double* Mt = obs ? Bt : At;
        double a0 = 0.0, a1 = 0.0, h0 = 0.0, h1 = 0.0;
        int j = 0;
        for (; j + 2 <= S; j += 2) {
          const double x0 = mc[j], x1 = mc[j + 1];
          a0 = fma(Mt[(size_t)j * S + tid], x0, a0); a1 = fma(Mt[(size_t)(j + 1) * S + tid], x1, a1);
          h0 = fma(ha[j], x0, h0); h1 = fma(ha[j + 1], x1, h1);
        }
        if (j < S) { a0 = fma(Mt[(size_t)j * S + tid], mc[j], a0); h0 = fma(ha[j], mc[j], h0); }
        double mi = a0 + a1;
        if (obs) {
          const double v = yk - (h0 + h1);
          mi = mi + kg[tid] * yk;
          if (tid == 0) sv2 = fma(v, v, sv2);
        }
        mn[tid] = mi;
        msc[(size_t)kk * S + tid] = mi;
      }
      lds_barrier();
      double* t_ = mc; mc = mn; mn = t_;
    }
    for (int e = tid; e < nb * S; e += NT) fp.MS[(size_t)k0 * S + e] = msc[e];
    __syncthreads();
  }
  if (tid == 0) fp.sum_v2[blockIdx.x] = sv2;
}

// pass 3:  m = MS_k + G*(m - A*MS_k), k descending inside span j of the n = T-1 smoothing steps
static __global__ void __launch_bounds__(256) fastfb_smoother_kernel(FbPar fp) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int tid = threadIdx.x, NT = blockDim.x, S = fp.S;
  const bool mg = fp.mat_global != 0;
  const double* At = mg ? fp.A : lds;
  const double* Gt = mg ? fp.B : lds + (size_t)S * S;
  double* m = lds + (mg ? 0 : 2 * (size_t)S * S) + 2 * (size_t)S;   // [S] current smoothed mean
  double* dv = m + S;                                // [S] m - A*MS_k
  double* msc = dv + 2 * (size_t)S + FB_CHK;         // [FB_CHK][S]
  const int64_t n = fp.T - 1;
  const int64_t ka = (int64_t)blockIdx.x * fp.L, kb = (ka + fp.L < n) ? ka + fp.L : n;   // steps ka .. kb-1
  if (!mg) for (int e = tid; e < S * S; e += NT) { lds[e] = fp.A[e]; lds[(size_t)S * S + e] = fp.B[e]; }
  for (int i = tid; i < S; i += NT) m[i] = fp.starts ? fp.starts[(size_t)blockIdx.x * S + i] : fp.MS[(size_t)(fp.T - 1) * S + i];
  __syncthreads();
  for (int64_t k1 = kb; k1 > ka; k1 -= FB_CHK) {            // steps k1-1 ... k1-nb, descending
    const int nb = (k1 - ka < FB_CHK) ? (int)(k1 - ka) : FB_CHK;
    const int64_t kl = k1 - nb;
    for (int e = tid; e < nb * S; e += NT) msc[e] = fp.MS[(size_t)kl * S + e];
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
    for (int e = tid; e < nb * S; e += NT) fp.MS[(size_t)kl * S + e] = msc[e];
    __syncthreads();
  }
}

// pass 1: span j -> Phi_j (product of the span's step matrices) and c_j (the span run from a zero entry value), as the
// S x (S+1) matrix recursion  X <- M_k X (+ input in column S)  on 4 x 4 register tiles.
template <bool SMOOTH>
__global__ void __launch_bounds__(256) fastfb_compose_kernel(FbPar fp) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int tid = threadIdx.x, NT = blockDim.x, S = fp.S, SP = S + 4;
  double* At = lds;
  double* Bt = At + (size_t)S * S;
  double* Xa = Bt + (size_t)S * S;          // [SP rows][SP]: X[j][c], rows >= S are zero padding
  double* Xb = Xa + (size_t)SP * SP;
  double* kg = Xb + (size_t)SP * SP;        // filter: K ; smoother: MS_k
  double* dv = kg + S;                      // smoother: X[:,S] - A MS_k
  const int64_t n = SMOOTH ? fp.T - 1 : fp.T;
  const int j = blockIdx.x;
  const int64_t ka = (int64_t)j * fp.L, kb = (ka + fp.L < n) ? ka + fp.L : n;
  for (int e = tid; e < S * S; e += NT) { At[e] = fp.A[e]; Bt[e] = fp.B[e]; }
  for (int e = tid; e < SP * SP; e += NT) { const int r = e / SP, c = e - r * SP; Xa[e] = (r == c && r < S) ? 1.0 : 0.0; Xb[e] = 0.0; }
  if (!SMOOTH) for (int i = tid; i < S; i += NT) kg[i] = fp.K[i];
  __syncthreads();
  double* Xc = Xa;
  double* Xn = Xb;
  const int RT = (S + 3) >> 2, CT = (S + 1 + 3) >> 2;       // row / column tiles (column S is the affine part)
  const int64_t nsteps = kb - ka;
  for (int64_t q = 0; q < nsteps; ++q) {
    const int64_t k = SMOOTH ? (kb - 1 - q) : (ka + q);
    const double* Mt = Bt;
    double yk = 0.0;
    bool obs = true;
    if (SMOOTH) {
      // d = X[:,S] - A MS_k replaces column S of the input; MS_k is added to column S of the output
      for (int i = tid; i < S; i += NT) kg[i] = fp.MS[(size_t)k * S + i];
      __syncthreads();
      if (tid < S) {
        double a0 = 0.0;
        for (int l = 0; l < S; ++l) a0 = fma(At[(size_t)l * S + tid], kg[l], a0);
        dv[tid] = Xc[(size_t)tid * SP + S] - a0;
      }
      __syncthreads();
      if (tid < S) Xc[(size_t)tid * SP + S] = dv[tid];
      __syncthreads();
    } else {
      yk = fp.y[k];
      obs = !(yk != yk);
      Mt = obs ? Bt : At;
    }
    for (int t = tid; t < RT * CT; t += NT) {
      const int ti = t / CT, tc = t - ti * CT, i0 = 4 * ti, c0 = 4 * tc;
      double acc[16];
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[e] = 0.0;
      for (int l = 0; l < S; ++l) {
        double mr[4], xr[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) { mr[u] = (i0 + u < S) ? Mt[(size_t)l * S + i0 + u] : 0.0; xr[u] = Xc[(size_t)l * SP + c0 + u]; }
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
          for (int w = 0; w < 4; ++w) acc[4 * u + w] = fma(mr[u], xr[w], acc[4 * u + w]);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int w = 0; w < 4; ++w) {
          const int i = i0 + u, c = c0 + w;
          if (i < S && c <= S) {
            double v = acc[4 * u + w];
            if (c == S) v += SMOOTH ? kg[i] : (obs ? kg[i] * yk : 0.0);
            Xn[(size_t)i * SP + c] = v;
          }
        }
    }
    __syncthreads();
    double* t_ = Xc; Xc = Xn; Xn = t_;
  }
  double* out = fp.Phi + (size_t)j * S * SP;
  for (int e = tid; e < S * SP; e += NT) out[e] = Xc[e];
}

// pass 2: boundary values.  Filter: s_0 = 0, s_{j+1} = Phi_j s_j + c_j.  Smoother: s_{ns-1} = MS_{T-1}, s_{j-1} = Phi_j s_j + c_j.
template <bool SMOOTH>
__global__ void __launch_bounds__(256) fastfb_boundary_kernel(FbPar fp) {
  __shared__ double sv[256];
  const int tid = threadIdx.x, S = fp.S, SP = S + 4;
  if (tid < S) sv[tid] = SMOOTH ? fp.MS[(size_t)(fp.T - 1) * S + tid] : 0.0;
  __syncthreads();
  for (int q = 0; q < fp.ns; ++q) {
    const int j = SMOOTH ? (fp.ns - 1 - q) : q;
    if (tid < S) fp.starts[(size_t)j * S + tid] = sv[tid];
    double nv = 0.0;
    if (tid < S) {
      const double* ph = fp.Phi + ((size_t)j * S + tid) * SP;
      double a0 = 0.0, a1 = 0.0;
      int l = 0;
      for (; l + 2 <= S; l += 2) { a0 = fma(ph[l], sv[l], a0); a1 = fma(ph[l + 1], sv[l + 1], a1); }
      if (l < S) a0 = fma(ph[l], sv[l], a0);
      nv = (a0 + a1) + ph[S];
    }
    __syncthreads();
    if (tid < S) sv[tid] = nv;
    __syncthreads();
  }
}

}  // namespace nagp
