/*
 * nagp.h -- C ABI of libnagp.so: MI355X-native (gfx950, HIP) Kalman-filter / RTS-smoother /
 * Power-EP / iterated-EKF inference loops of the GT-NMF audio model.
 *
 * The reference (AaltoML/nonstationary-audio-gp) is 100 % MATLAB and has no FFI; the entry points
 * below are what a MEX gateway (or ctypes / any FFI) binds to replace the per-time-step loops of
 *
 *   nagp_*_KIND_GF_EP   -> matlab/gf_ep_modulator.m:113-283 (predict) / :383-522 (nlml)
 *                          matlab/gf_ep_modulator_nmf.m:113-283 / :384-522
 *                          matlab/gf_ep_modulator_nmf_constraints.m:148-334 / :436-573
 *   nagp_*_KIND_IHGP    -> matlab/ihgp_ep_modulator_nmf.m:223-454,
 *                          matlab/ihgp_ep_modulator_nmf_constraints.m:257-480
 *   nagp_*_KIND_GIEKF   -> matlab/gf_giekf_modulator_nmf.m:126-221 (+ iekf_update1.m:110-117,
 *                          ekf_update1.m:106-109), matlab/gf_giekf_modulator_nmf_constraints.m:162-257
 *   mom callbacks       -> matlab/likModulatorPower.m:25-100, likModulatorNMFPower.m:28-87,
 *                          experiments/likModulatorPreCalcwn.m:28-86 (selected by lik_kind)
 *
 * Everything outside those loops (parameter unpacking, ss_modulators*, balance, lti_disc, DARE
 * tables, sigma-point tables) stays on the host side of the boundary and arrives here as plain
 * arrays.  All matrices are column-major IEEE doubles (MATLAB layout); all pointers are HOST
 * pointers owned by the caller; inputs are read-only; outputs are caller-allocated and may be
 * NULL (= not wanted).  No exceptions cross the ABI: every function returns 0 or a negative
 * nagp_status.  Single caller thread per plan; safe to call repeatedly from a long-lived process.
 */
#ifndef NAGP_H
#define NAGP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NAGP_VERSION 300 /* 0.3.0 */

typedef enum nagp_status {
  NAGP_OK = 0,
  NAGP_EINVAL = -1,       /* bad argument / inconsistent sizes */
  NAGP_EUNSUPPORTED = -2, /* shape outside what the kernels handle (e.g. block size > 4) */
  NAGP_EHIP = -3,         /* HIP runtime error (see nagp_last_error) */
  NAGP_ENOMEM = -4,       /* device memory exhausted */
  NAGP_ENODEVICE = -5,    /* no gfx950 device visible */
  NAGP_ENOTPD = -6,       /* Cholesky failed even after the jitter retry (where MATLAB's chol throws, gf_ep_modulator_nmf.m:219-222);
                             returned by the execute / run calls after the sweeps have finished: outputs can still be downloaded */
  NAGP_ERCCL = -7         /* RCCL failure in nagp_batch_run (see nagp_last_error) */
} nagp_status;

typedef enum nagp_kind { NAGP_KIND_GF_EP = 0, NAGP_KIND_IHGP = 1, NAGP_KIND_GIEKF = 2 } nagp_kind;
typedef enum nagp_mode { NAGP_MODE_PREDICT = 0, NAGP_MODE_NLML = 1 } nagp_mode;
/* mom callbacks of the reference, by file */
typedef enum nagp_lik {
  NAGP_LIK_POWER = 0,          /* likModulatorPower.m        (W = I, jitter 1e-8)  */
  NAGP_LIK_POWER_NMF = 1,      /* likModulatorNMFPower.m     (jitter 1e-10, pEP_const = 1) */
  NAGP_LIK_POWER_NMF_SQRT = 2  /* experiments/likModulatorPreCalcwn.m (sqrt amplitude, true pEP_const) */
} nagp_lik;
/* link functions seen in the drivers: log(1+exp(g-shift)) and exp(g) */
typedef enum nagp_link { NAGP_LINK_SOFTPLUS = 0, NAGP_LINK_EXP = 1 } nagp_link;

/* flags (nagp_opts.flags) */
#define NAGP_FLAG_IHGP_CONSTRAINTS 0x1u /* ihgp_ep_modulator_nmf_constraints.m: R starts at 0, no abs(Varft) */
#define NAGP_FLAG_EKF_RESET_P      0x2u /* gf_giekf_modulator_nmf_constraints.m:168: P=Pinf every global iteration */
#define NAGP_FLAG_MIXTURE_RULE     0x8u /* experiments/{gf,ihgp}_ep_mods_nmf_mixture.m: mom at power ep_fraction in the filter too,
                                           site <- (1-d) site + d/ep_fraction (...), clamp in the filter pass only, R starts at 0 */
#define NAGP_FLAG_WANT_PS          0x4u /* keep the smoothed covariances so that nagp_out.PS can be filled */

/* Discrete-time model of ONE problem (segment / hyper-parameter replica).
 * State ordering and block structure as built by ss_modulators_nmf.m:128-132: M diagonal blocks,
 * block n spanning states block_offsets[n] .. block_offsets[n+1]-1 (0-based); A, Q, Pinf are
 * block-diagonal with these blocks (only the diagonal blocks are read); row n of H has its single
 * non-zero h_val[n] at column block_offsets[n] (1 before `balance`, a power of two after).
 * Blocks hold 1 .. 8 states: 1 .. 4 for the kernels every driver uses (exp / Matern-3/2 sub-bands, Matern-5/2 modulators), 6 or 8 for
 * Matern-5/2 / -7/2 sub-bands (ss_modulators_nmf.m:13-33, cf_matern52_to_ss.m:93-121, cf_matern72_to_ss.m:93-124).  The state order of
 * every input and output is the caller's; how blocks of more than four states are laid out on the device is DESIGN.md section 3.
 * Larger blocks (the SE kernel's 12-state form) are refused with NAGP_EUNSUPPORTED. */
typedef struct nagp_model {
  int32_t S;                    /* state dimension */
  int32_t M;                    /* sites per step: D+N (NMF) or 2*D (gf_ep_modulator) */
  int32_t D;                    /* sub-bands */
  int32_t N;                    /* modulators / NMF components */
  const int32_t* block_offsets; /* M+1 */
  const double* A;              /* S x S */
  const double* Q;              /* S x S */
  const double* Pinf;           /* S x S */
  const double* h_val;          /* M */
  const double* Wnmf;           /* D x N, or NULL for NAGP_LIK_POWER */
  double lik_param;             /* w(1): log observation-noise variance */
} nagp_model;

/* IHGP look-up tables of one problem (ihgp_ep_modulator_nmf.m:107-134, 150-191), n_grid rows each,
 * channel-major: PPlist[n] is n_grid x b_n^2 (column-major b x b per row, as MATLAB's PP(:)'),
 * PGlist[n] is n_grid x 2 b_n^2 = [PS2(:)' G(:)'].  Stored flat: channel n starts at
 * pp_offsets[n] / pg_offsets[n] (in doubles), row stride b_n^2 / 2 b_n^2. */
typedef struct nagp_ihgp_tables {
  int32_t n_grid;          /* 200 in the reference */
  const double* r_grid;    /* n_grid ascending (logspace(-2,4,200)) */
  const double* PPlist;
  const int64_t* pp_offsets; /* M */
  const double* PGlist;
  const int64_t* pg_offsets; /* M */
} nagp_ihgp_tables;

typedef struct nagp_opts {
  int32_t kind;            /* nagp_kind */
  int32_t mode;            /* nagp_mode (NLML: GF_EP; GIEKF = the GradObj=off energy of gf_giekf_modulator_nmf_constraints.m:332-480, model Q = Pinf-A*Pinf*A') */
  int32_t lik_kind;        /* nagp_lik */
  int32_t link_kind;       /* nagp_link */
  double link_shift;       /* softplus shift (mod_sparsity) */
  int32_t n_pts;           /* sigma points */
  int32_t cub_dim;         /* N (NMF) or D (POWER) */
  const double* wn;        /* n_pts weights  (utp_ws / mvhermgauss) */
  const double* xn_unscaled; /* cub_dim x n_pts unit sigma points, column-major */
  double ep_fraction;      /* power-EP alpha */
  int32_t ep_itts;         /* EP sweeps (GIEKF: g_iter) */
  const double* ep_damping; /* ep_itts values */
  int32_t l_iter;          /* GIEKF inner iterations (iekf_update1 `iters`) */
  int32_t predict_at_k1;   /* gf_ep_modulator.m:131-133 predicts at k=1 in predict mode */
  uint32_t flags;
  int32_t device;          /* HIP device ordinal */
  int32_t chunk;           /* smoother chunk length (0 = default) */
  /* Warm start (one-shot entry points; plans: nagp_plan_upload_sites): initial site parameters, M x T column-major, in
   * place of the reference's zeros (gf_ep_modulator_nmf.m:96-97) -- e.g. the ttau / tnu a previous call returned
   * (the `out` struct of the reference carries them for this purpose).  NULL = zeros. */
  const double* ttau0;
  const double* tnu0;
} nagp_opts;

/* Caller-allocated outputs of ONE problem; any pointer may be NULL. */
typedef struct nagp_out {
  double* Eft;      /* M x T   H*MS                                  */
  double* Varft;    /* M x T   diag(H*PS_k*H')  (IHGP: time-constant) */
  double* MS;       /* S x T   smoothed means                        */
  double* PS;       /* S x S x T smoothed covariances (GF_EP / GIEKF) */
  double* ttau;     /* M x T */
  double* tnu;      /* M x T */
  double* R;        /* M x T */
  double* lZ;       /* T      (GF_EP: per-step log Z as left by the last pass) */
  double* nlZ;      /* ep_itts (predict) ; nlZ[0] = edata in NLML mode */
  double* maxDiffM; /* ep_itts */
  double* maxDiffP; /* ep_itts */
  int64_t* counters; /* NAGP_N_COUNTERS: chol retries, clamped sites, NaN observations, not-PD */
  double* MF;       /* S x T   filtered means of the last forward pass (the reference's out.MF, gf_ep_modulator_nmf.m:191-198) */
} nagp_out;

#define NAGP_N_COUNTERS 4
#define NAGP_CNT_CHOL_RETRY 0
#define NAGP_CNT_CLAMPED 1
#define NAGP_CNT_NAN_OBS 2
#define NAGP_CNT_NOTPD 3

/* Per-kernel device time of the last nagp_plan_execute, measured with HIP events on the plan's
 * own stream (ms, summed over launches) and launch counts. */
#define NAGP_N_KERNELS 8
#define NAGP_K_FILTER 0      /* gf/ekf forward filter  | ihgp ADF filter          */
#define NAGP_K_GAIN 1        /* RTS gain (PSkp, Cholesky, G)                       */
#define NAGP_K_SCAN 2        /* RTS backward recursion | ihgp backward mean scan  */
#define NAGP_K_EPSITE 3      /* cavity + mom + site update (parallel over k)      */
#define NAGP_K_REDUCE 4      /* nlZ / maxDiff reductions                          */
#define NAGP_K_FILTER_LIN 5  /* ihgp fixed-site (linear) filter of sweeps >= 2    */
#define NAGP_K_OUTPUT 6      /* output formatting (tile-major -> column-major)    */
#define NAGP_K_OTHER 7
typedef struct nagp_timings {
  double ms[NAGP_N_KERNELS];
  int64_t launches[NAGP_N_KERNELS];
  double total_ms; /* whole execute, events on the same stream */
} nagp_timings;

typedef struct nagp_plan nagp_plan; /* opaque */

int nagp_version(void);
int nagp_device_count(void);
const char* nagp_strerror(int status);
const char* nagp_last_error(void); /* text of the last HIP failure on this thread */

/* One-shot host-buffer entry points (create + upload + execute + download + destroy).  The three
 * names mirror the reference's function families; `tables` only for IHGP. */
int nagp_ep_run(const nagp_model* model, const double* y, int64_t T, const nagp_opts* opts, nagp_out* out);
int nagp_ihgp_run(const nagp_model* model, const nagp_ihgp_tables* tables, const double* y, int64_t T,
                  const nagp_opts* opts, nagp_out* out);
int nagp_giekf_run(const nagp_model* model, const double* y, int64_t T, const nagp_opts* opts, nagp_out* out);

/* The `mom` callback itself for n_eval independent inputs -- replaces likModulatorPower.m:25-100,
 * likModulatorNMFPower.m:28-87 and experiments/likModulatorPreCalcwn.m:28-86 as called through the handles of
 * demo_toy_modulators.m:81 / demo_toy_modulators_nmf.m:81 / train_GTFNMF.m:149:
 *   [lZ, dlZ, d2lZ] = mom(hyp, mu, s2, [Wnmf,] ep_frac, yall, k)
 * opts supplies lik_kind, link, cubature (n_pts, cub_dim, wn, xn_unscaled), ep_fraction and device; D, N as in
 * nagp_model (M = D+N for the NMF likelihoods, 2*D for NAGP_LIK_POWER); Wnmf is D x N column-major (NULL for POWER);
 * lik_param = hyp = log observation-noise variance.  y[n_eval]; mu, s2, dlZ, d2lZ are M x n_eval column-major. */
int nagp_mom_eval(const nagp_opts* opts, int32_t D, int32_t N, const double* Wnmf, double lik_param, int64_t n_eval,
                  const double* y, const double* mu, const double* s2, double* lZ, double* dlZ, double* d2lZ);

/* [M,P,K,MU,S] = iekf_update1(M,P,y,H,R,h,V,param,iters) -- iekf_update1.m:110-117 (ekf_update1.m:106-109 is
 * iters = 1) for the measurement model the reference passes through its handles (funh / funhd,
 * gf_giekf_modulator_nmf_constraints.m:492-502): h(x) = (H_z x)' W softplus(H_g x).  Row n of H has its single
 * non-zero h_val[n] at (0-based) column h_col[n]; n < D: sub-bands, then N modulators.  m (S) and P (S x S
 * column-major) are updated in place; K (S), *MU, *Sinn receive the last iteration's gain, prediction and innovation
 * variance (any of the three may be NULL). */
int nagp_iekf_update1(int32_t S, int32_t D, int32_t N, const int32_t* h_col, const double* h_val, const double* Wnmf,
                      double R, double y, int32_t iters, double* m, double* P, double* K, double* MU, double* Sinn,
                      int32_t device);

/* The EKF training objective WITH its gradient recursion -- matlab/gf_giekf_modulator_nmf_constraints.m:332-480 with GradObj = 'on'
 * (gf_giekf_modulator_nmf.m:296-439): one plain EKF pass (as NAGP_MODE_NLML of the GIEKF kind: prediction at the first step too,
 * one update per step, no isnan guard) and, per parameter slice j, the sensitivity recursion of (m, P) (:387-401, :437-466).
 * models[q].A = expm(F), models[q].Q = Pinf - A*Pinf*A' (:377-378).  Per problem and slice, S x S column-major, block diagonal with
 * the blocks of the model (only those blocks are read): dA[q][j] = lower-left block of expm([F 0; dF_j F]) (:355-366),
 * dQ[q][j] = dPinf_j - dA_j*Pinf*A' - A*dPinf_j*A' - (dA_j*Pinf*A')' (:392-394), dPinf[q][j]; dR[j] (:124).
 * What the Jacobian derivative `dmdJH` of slice j is made of is data: hess[j] != 0 adds dm_j' * d2h (:439), w_index[j] >= 0 adds
 * dh(.; W_) with W_ the unit matrix at column-major position w_index[j] of Wnmf (:441-443), w_direct[j] != 0 adds h(.; W_) to the
 * derivative of the predicted measurement (a term the reference's statements leave out).  The reference as written:
 * hess = 1, w_index = -1 for j < n_param - D*N and hess = 0, w_index = j - (n_param - D*N) for the last D*N slices, w_direct = 0.
 * edata[q], gdata[q * n_param + j]; NaN for a problem whose innovation variance is not positive even with the jitter (:423-426).
 * Shapes: M = D + N <= 32 sites, blocks of <= 4 states. */
int nagp_giekf_nlml_grad(int32_t n_problems, const nagp_model* models, const double* const* ys, int64_t T, int32_t n_param,
                         const double* const* dA, const double* const* dQ, const double* const* dPinf, const double* dR,
                         const int32_t* hess, const int32_t* w_index, const int32_t* w_direct, double* edata, double* gdata,
                         int32_t device);

/* Stationary filterbank (the step before the hot path in every real-audio script, e.g. train_GTFNMF.m:56-65):
 * the two loops of unifying_prob_tf/kernel_ss_kalmanFastFB.m -- infinite-horizon Kalman filter (:83-110)
 *     if ~isnan(y_k): v = y_k - HA*m; m = AKHA*m + K*y_k; else m = A*m;   MS(:,k) = m
 * and steady-state RTS smoother (:134-151)   m = MS(:,k) + G*(m - A*MS(:,k)),  k = T-1 .. 1.
 * The caller keeps the set-up lines of the .m (dare, K, AKHA = A-K*H*A, HA = H*A, G = PF2*A'/PP) and passes the constant
 * matrices: A, AKHA, G are S x S column-major (G = NULL: filter only, the KF = 1 option); HA, K have S entries.
 * MS (S x T, column-major) receives the filtered / smoothed means, *sum_v2 the sum of squared innovations of the observed
 * steps (lik = -( T/2 log(2 pi S_inn) + sum_v2 / (2 S_inn) ), :80,:101,:158).  S <= 256 (a thread per state; up to S = 96 both matrices of a pass live in the LDS,
 * beyond that they are read from global memory: 32 Matern-3/2 channels = S 128).  Series of T >= 2048 steps run parallel in time
 * over min(512, T/128) spans when S <= 69 (the span composition keeps two more (S+4) x (S+4) matrices in the LDS); every other
 * call runs as one span, sequentially. */
int nagp_fastfb_run(int32_t S, const double* A, const double* AKHA, const double* HA, const double* K, const double* G,
                    const double* y, int64_t T, double* MS, double* sum_v2, int32_t device);

/* Joint posterior draws of the stationary filterbank by the simulation smoother (Durbin & Koopman 2002): whole trajectories,
 * correlated in time -- what fills a gap with texture and gives error bars on functionals that couple time steps (the
 * missing-data experiment of demo_stationary_filterbank.m:168-200 fills its gap with the smoother MEAN, which decays to zero
 * inside a long gap).  Inputs are those of nagp_fastfb_run plus the observation row H (S entries), the observation variance R
 * and lower factors Lp, Lq (S x S column-major) with Lp Lp' = Pinf, Lq Lq' = Q.  Write S_y(.) for the smoothed means
 * nagp_fastfb_run returns for an observation sequence (filter from m = 0, smoother with G, NaN = missing).  Draw i of n_draws:
 *     z[t][j] = normals(T, j, n_draws, seed)[t, i]  (j = 0..S-1),   e[t] = normals(T, S, n_draws, seed)[t, i]
 *     x*_0 = Lp z[0];  x*_t = A x*_{t-1} + Lq z[t]  (t >= 1)
 *     y*_t = H x*_t + sqrt(R) e[t] where y_t is observed, NaN where y_t is NaN
 *     X_i = x* + S_y(y - y*)   (S x T),      Ydraw_i[t] = H X_i[:, t]
 * `normals` is the counter-based generator of nagp_reconstruct (Philox4x32-10 keyed by seed, counter = (t low, t high,
 * sample block i / 4, site), Box-Muller), restated on the host in oracle/recon.py:normals: draw i does not depend on
 * n_draws or on how the draws are batched on the device.  The mean over draws is S_y(y) in expectation; the covariance is the
 * error covariance of the steady-state smoother under the model: Psm away from the ends and from gaps, larger inside gaps.
 * Outputs (each may be NULL, not all three): Ydraw n_draws x T draw-major; Xdraw n_draws blocks of S x T column-major;
 * MS = S_y(y), S x T, the bits of nagp_fastfb_run.  NAGP_EINVAL: a NULL input (G included: there is no filter-only form),
 * S, T or n_draws < 1, R not positive and finite, no output; NAGP_EUNSUPPORTED: S > 256; NAGP_ENOMEM: one draw (2 T S
 * doubles and change) does not fit the device-memory budget of a call -- all decided on the host before any device call. */
int nagp_fastfb_sample(int32_t S, const double* A, const double* AKHA, const double* HA, const double* K, const double* G,
                       const double* H, double R, const double* Lp, const double* Lq,
                       const double* y, int64_t T, int32_t n_draws, uint64_t seed,
                       double* Ydraw /* n_draws x T, draw-major; may be NULL */,
                       double* Xdraw /* n_draws x (S x T column-major); may be NULL */,
                       double* MS    /* S x T: S_y(y); may be NULL */, int32_t device);

/* The exact form of the stationary filterbank: the Kalman filter and RTS smoother of unifying_prob_tf/kernel_ss_kalmanSlowFB_rewrite.m
 * (the `slow = 1` branch of kernel_ss_probFB.m) with a time-varying covariance and an observation variance of its own at every step --
 * what the missing-data experiment of demo_stationary_filterbank.m:178-199 runs with vary = 1e-4 on observed steps and 1e5 inside the gaps,
 * what gives true posterior covariances at the ends of a series and inside gaps, and the exact log-likelihood.
 * Per series, from m = 0, P = P0 (:55-84):  k >= 1: m = A m, P = A P A' + Q;  s = H P H' + vary_k, K = P H'/s, v = y_k - H m, m += K v,
 * P -= K H P;  lik -= 1/2 log 2 pi + 1/2 log s + 1/2 v^2/s.  Backward (:100-134), k = T-2 .. 0:  PSkp = A PS_k A' + Q, G = PS_k A' / PSkp,
 * m = MS_k + G (m - A MS_k), P = PS_k + G (P - PSkp) G'.  filter_only != 0 (the .m's KF = 1): the outputs are the filtered moments.
 * Two deliberate differences from the .m:
 *   - a NaN y_k skips that step's update and its lik term (the library's "NaN = missing", the vary_k -> infinity limit); the .m has no
 *     guard and returns NaN everywhere;
 *   - the smoothed moments are computed by the adjoint recursion r_k = H'v_k/s_k + C_k'A'r_{k+1}, N_k = H'H/s_k + C_k'A'N_{k+1}A C_k
 *     (C_k = I - K_k H), MS_k = m-_k + P-_k r_k, PS_k = P-_k - P-_k N_k P-_k on the predicted pair (m-_k, P-_k), which is the RTS result
 *     in exact arithmetic and factorises nothing: the jitter retry of :114-121 has no counterpart.
 * One model serves n_series independent series (each its own y and vary); they run concurrently and a series' result does not depend
 * on its batch mates.  A, Q: S x S column-major, block diagonal with blocks of `block` states; only the lower triangles of P0 and of
 * the blocks of Q are read.  sub_idx selects the rows and columns of the covariances returned in Psub (n_sub = S, 0..S-1: all of PS_k);
 * Psub is symmetric to the bit.  Outputs per series: lik; MS, Pdiag (S x T column-major); Psub (n_sub x n_sub x T).
 * All of the following is decided on the host before any device call.
 * NAGP_EINVAL: a NULL input; S, T or n_series < 1; block < 1 or S % block != 0; a vary entry negative or not finite; sub_idx not strictly
 *   ascending inside [0, S); Psub without n_sub > 0 or n_sub > 0 without Psub; lik, MS, Pdiag, Psub all NULL.
 * NAGP_EUNSUPPORTED: S > 128 (the covariance of a series lives in the 160 KiB LDS of one workgroup); block > 8; a non-zero of A or Q
 *   outside the declared blocks (dense transitions are not served).
 * NAGP_ENOMEM: the per-step storage of one series does not fit the device-memory budget of a call, 48 GiB.  A series takes
 *     8 T (W + 2 + S + [Pdiag: S] + n_sub^2) bytes,   W = 2 S^2 + 3 S + 2  (smoother: m-, P-, v, 1/s, K, r, N)  or  S^2 + S  (filter_only),
 *   plus 8 (2 S^2 + 2 S block + S) + 4 n_sub + 4096 bytes per call; a batch whose series do not all fit runs in device batches of as many
 *   series as do.  There is no checkpointing or recompute scheme: a single series beyond the budget is refused.
 * NAGP_ENOTPD (after the run; every output is written): an innovation variance s <= 0, possible only with vary_k = 0; that series has
 *   lik = NaN, the other series of the batch are unaffected. */
int nagp_slowfb_run(int32_t S, int32_t block,
                    const double* A, const double* Q,   /* S x S column-major, block diagonal, blocks of `block` states */
                    const double* H,                    /* S entries: the observation row */
                    const double* P0,                   /* S x S symmetric: covariance of the first state (mean 0) */
                    int32_t n_series, const double* y,  /* n_series x T, series-major; NaN = missing */
                    const double* vary,                 /* n_series x T: observation variance of every step, >= 0 */
                    int64_t T, int32_t filter_only,
                    int32_t n_sub, const int32_t* sub_idx, /* 0-based, strictly ascending; n_sub = 0 with Psub = NULL */
                    double* lik,                        /* n_series */
                    double* MS,                         /* n_series blocks of S x T column-major; may be NULL */
                    double* Pdiag,                      /* n_series blocks of S x T: marginal variances; may be NULL */
                    double* Psub,                       /* n_series blocks of n_sub x n_sub x T: P(sub_idx, sub_idx, k); may be NULL */
                    int32_t device);
/* Device time of the three kernels of the last nagp_slowfb_run on this thread, in ms (HIP events, summed over its device batches):
 * ms[0] forward filter, ms[1] backward recursion (0 with filter_only), ms[2] the time-parallel combination. */
int nagp_slowfb_timings(double* ms /* 3 */);

/* The factorisation that gives the reference's real-audio drivers their W (demo_nonstationary_filterbank.m:93-97,
 * experiments/train_GTFNMF.m:64-89): the fixed-point NMF of experiments/nmf/nmf_fp.m and nmf_inf_fp.m on the sub-band amplitudes
 * A = abs(Z') (T x D, >= 0), A ~ H W with W K x D and H T x K (H is T x K in the code, whatever the header comment of the .m says).
 * One iteration, kept literally (nmf_fp.m:65-87; the objective is getObj_nmf_temp.m:48-54, :134):
 *     AHat = H W + vary;  H = ((A .* AHat.^-2) W') ./ (AHat.^-1 W') .* H;             Obj(end+1) = sum(A ./ (H W + vary) + log(H W + vary)) / T
 *     AHat = H W;         W = (H' (A .* AHat.^-2)) ./ (H' AHat.^-1) .* W;  W = diag(1 ./ sum(W,2)) W;   Obj(end+1) = the same with the new W
 * -- vary IS added in the H update and in the objective and is NOT added in the W update (:81), as in the .m.  update_w = 0 runs the
 * first line only, one Obj per iteration: nmf_inf_fp.m:50-55.  getObj_nmf_temp renormalises W and goes through exp(log(.)); on a W whose
 * rows already sum to 1 that is a few ulp, and the kernels skip both.
 * n_problems independent problems (the restarts of nmf_fp.m:44-56) share A and vary and run concurrently; a problem's result does not depend
 * on its batch mates, and every sum over t is formed in a fixed order (per-workgroup partial sums, reduced by a second kernel; no
 * floating-point atomics): the same call gives the same bits.  All matrices column-major; W0 / W: n_problems blocks of K x D; H0 / H:
 * n_problems blocks of T x K; Obj: (update_w ? 2 : 1) * n_its entries per problem, problem-major.
 * The entry point does not normalise W0: that is the caller's line (nmf_fp.m:63, nmf_inf_fp.m:37-40).  n_its = 0 copies W0, H0 through.
 * A row of A that is entirely zero with vary = 0 gives what IEEE arithmetic gives in the .m too (H(t,:) = 0/..., then NaN); it is not refused.
 * All of the following is decided on the host before any device call.
 * NAGP_EINVAL: A, W0 or H0 NULL; n_problems, T, D or K < 1; n_its < 0; an input that is not finite; a negative entry of A or vary; an
 *   entry of H0 that is not > 0; a negative entry of W0; a W0 with an all-zero row or column.
 * NAGP_EUNSUPPORTED: D > 64 or K > 16 (W lives in the LDS, H(t,:) in registers, K is padded to one MFMA tile).
 * NAGP_ENOMEM: one problem does not fit the device-memory budget of a call, 8 GiB.  A call takes 8 T D (twice with vary) + 4096 bytes and
 *   every problem 8 (T K + K D + ceil(T / 256) (2 K D + 2) + its Obj entries) bytes; a batch whose problems do not all fit runs in
 *   device batches of as many problems as do, with results bit-equal to an unbatched call. */
int nagp_nmf_fp(int32_t n_problems, int64_t T, int32_t D, int32_t K,
                const double* A,    /* T x D, shared */
                const double* vary, /* T x D shared, or NULL = zeros */
                const double* W0,   /* K x D x n_problems */
                const double* H0,   /* T x K x n_problems */
                int32_t n_its, int32_t update_w,
                double* W, double* H,   /* as W0 / H0; either may be NULL */
                double* Obj,            /* (update_w ? 2 : 1) * n_its per problem, problem-major; may be NULL */
                int32_t device);
/* Device time of the enqueued kernel sequence of the last nagp_nmf_fp on this thread, in ms (HIP events, summed over its device batches). */
int nagp_nmf_timings(double* ms /* 1 */);

/* The objective that unifying_prob_tf/fit_probSTFT_SD.m minimises, the first call of every real-audio driver of the reference
 * (demo_nonstationary_filterbank.m:56, experiments/train_GTFNMF.m:56): get_Obj_pSTFT_{exp,matern32,matern52}.m (form = 0) and
 * get_Obj_pSTFT_all.m (form = 1) with its gradient, for a batch of problems.  With the transforms of :61-67,
 *     mVar = minVar + exp(theta(1:D)),  om = limOm(:,1) + (limOm(:,2) - limOm(:,1)) ./ (1 + exp(-theta(D+1:2D))),  lam likewise from limLam,
 * and the grid omegas = [linspace(0, pi, ceil(N/2)), -omegas(floor(N/2):-1:1)] (:72-74; 0 and pi twice for even N, pi once for odd N),
 *     spec_i = vary + sum_d (1 - lam_d^2) S_d(omegas_i),   Obj = (sum_i log spec_i + sum_i specTar_i / spec_i + bet sum_d mVar_d) / N,
 * and dObj as each file writes it (the cosh(theta/2)^-2 / 4 factors, bet dVar on the variance part only, the / N).
 * Quirks kept: the generic file sets len = sqrt(5) / lam for every kernel except exp (1 / lam) and matern32 (sqrt(3) / lam), so matern72
 * runs with sqrt(5) against cf_matern72_to_ss's lambda = sqrt(7) / len (_all.m:81-94); ss_func(mVar, len, 4).
 * The generic file's complex solves are evaluated through their closed form (the rotation diagonalises the product model into two
 * Matern companion systems in omega -+ om, each a power of 1 / (lm^2 + (omega -+ om)^2)), which for exp, matern32 and matern52 IS the
 * kernel-specific file: form = 0 and form = 1 give the same bits for those three (csrc/nagp_pstft.hpp).
 * theta: 3 D per problem, problem-major.  specTar: N entries shared by the problems (spec_stride = 0) or N per problem (spec_stride = N).
 * minVar (D), limOm, limLam (D x 2 column-major) are shared.  dObj = NULL: the objective only (the same Obj bits).
 * Every sum over the frequencies is formed in a fixed order (a butterfly inside a wave, waves and workgroups in ascending order; no
 * floating-point atomics): a problem's result is the same to the bit alone, in a batch, and however the call is cut into device batches.
 * All of the following is decided on the host before any device call.
 * NAGP_EUNSUPPORTED: a kernel other than the four NAGP_PSTFT_* (se is not served); form = 0 with NAGP_PSTFT_MATERN72 (no such file);
 *   D > 64 (the per-component constants live in the LDS); one problem beyond the device-memory budget of a call, 1 GiB: a call takes
 *   8 (5 D + N when specTar is shared) + 4096 bytes and every problem 8 (ceil(N / 256) (3 D + 2, objective only: 2) + 6 D + 3 + N when
 *   specTar is per problem) bytes -- no O(N D) scratch: the gradient pass recomputes S_d.  A batch whose problems do not all fit runs in
 *   device batches of as many as do.
 * NAGP_EINVAL: a NULL input or Obj; n_problems or D < 1; form not 0 or 1; N < 4; spec_stride not 0 or N; an input that is not finite;
 *   specTar < 0; vary < 0; minVar < 0; limOm or limLam with upper <= lower; limLam outside [0, 1] (beyond it a component's spectrum is
 *   negative); vary = 0 for a problem none of whose components has 0 < lam < 1 in float64 -- spec would be 0.  A limLam range with
 *   0 < lower and upper < 1 rules that out for every theta; fit_probSTFT_SD's own ranges [0, lam_max] do so for every theta that has
 *   not saturated onto the lower end. */
enum { NAGP_PSTFT_EXP = 0, NAGP_PSTFT_MATERN32 = 1, NAGP_PSTFT_MATERN52 = 2, NAGP_PSTFT_MATERN72 = 3 };
int nagp_pstft_obj(int32_t n_problems, int32_t kernel, int32_t form /* 0 closed, 1 generic */, int32_t D, int64_t N,
                   const double* theta /* n_problems x 3D */, const double* specTar, int64_t spec_stride /* 0 = shared, N = per problem */,
                   const double* vary, const double* bet /* n_problems each */,
                   const double* minVar /* D */, const double* limOm, const double* limLam /* D x 2, column-major */,
                   double* Obj /* n_problems */, double* dObj /* n_problems x 3D, or NULL = objective only */, int32_t device);
/* Device time of the two kernels of the last nagp_pstft_obj on this thread, in ms (HIP events, summed over its device batches). */
int nagp_pstft_timings(double* ms /* 1 */);

/* The objective that experiments/toolsGP/trainSEGP_RS.m minimises -- the modulator prior fit of the training drivers
 * (experiments/train_model.m:132-149, train_GTFNMF.m:91-108): toolsGP/getObjSEGP.m on toolsGP/getGPSESpec.m with its gradient, the
 * negative log-likelihood of a regularly sampled squared-exponential GP plus white noise in the spectral domain, for a batch of
 * problems.  With len = exp(param[0]) and the frequency list of getGPSESpec.m:18, [0:ceil(T/2), -floor(T/2)+1:-1],
 *     f_j = j for j <= ceil(T/2), else j - T   (j = 0 .. T-1),     w_j = 2 pi f_j / T,
 *     c_j = sqrt(2 pi len^2) exp(-w_j^2 len^2 / 2),   dc_j = c_j (1/len - w_j^2 len),   S_j = varx c_j + vary,
 *     g_j = 1/(2 S_j) - specy_j / (2 T S_j^2),
 *     Obj = (1/2 sum_j log S_j + 1/(2T) sum_j specy_j / S_j) / T,
 *     dObj = [len varx sum_j g_j dc_j,  varx sum_j g_j c_j,  vary sum_j g_j] / T      (the first n_param entries).
 * The list is kept as the .m writes it: for odd T entry j = (T+1)/2 has f = +(T+1)/2, not -(T-1)/2 (it enters through w^2).
 * n_param = 3: varx = exp(param[1]), vary = exp(param[2]); 2: varx = exp(param[1]), vary given; 1: varx and vary given -- the three
 * nargin branches of the .m (specy = abs(fft(y)).^2 there).
 * param: n_param per problem, problem-major.  specy: T entries shared by the problems (spec_stride = 0) or T per problem
 * (spec_stride = T).  dObj = NULL: the objective only (the same Obj bits).
 * Every sum over the frequencies is formed in a fixed order (a butterfly inside a wave, waves and workgroups in ascending order, the
 * order over the workgroups a function of T alone; no floating-point atomics): a problem's result is the same to the bit alone, in a
 * batch, with shared or per-problem specy, and however the call is cut into device batches.
 * All of the following is decided on the host before any device call.
 * NAGP_EUNSUPPORTED: one problem beyond the device-memory budget of a call, 1 GiB: a call takes 8 T (when specy is shared) + 4096
 *   bytes and every problem 8 (ceil(T / 256) (2 + n_param, objective only: 2) + 2 n_param + 3 + T when specy is per problem) bytes.
 *   A batch whose problems do not all fit runs in device batches of as many as do.
 * NAGP_EINVAL: a NULL param, specy or Obj; a NULL vary (n_param <= 2) or varx (n_param = 1); n_problems < 1; n_param not 1, 2 or 3;
 *   T < 2; spec_stride not 0 or T; an input that is not finite; specy < 0; a given vary <= 0; a given varx < 0.
 * A result that is not finite (exp(param) overflowing, or varx and vary both underflowing to 0) is returned as it is: minimize halves
 * its step on a non-finite objective. */
int nagp_segp_obj(int32_t n_problems, int32_t n_param /* 1, 2, 3 */, int64_t T,
                  const double* param /* n_problems x n_param */,
                  const double* specy, int64_t spec_stride /* 0 = shared, T = per problem */,
                  const double* vary /* n_problems, read when n_param <= 2 */,
                  const double* varx /* n_problems, read when n_param == 1 */,
                  double* Obj, double* dObj /* n_problems x n_param, or NULL */, int32_t device);
/* Device time of the two kernels of the last nagp_segp_obj on this thread, in ms (HIP events, summed over its device batches). */
int nagp_segp_timings(double* ms /* 1 */);

/* The objective that experiments/gppad/GPModelFast/MAPGPFast.m minimises -- the envelope inference of GPPAD(real(Z)', fs/10) in the
 * training drivers (experiments/train_model.m:113): GPModelFast/GetGPObjFast.m with its gradient, for a batch of problems (one
 * channel at one resolution each).  With a = GetAmp(x_t) (x > 500: x; x < -30: exp(x); else log(1 + exp(x))), s = 1/(1 + exp(-x_t)),
 * v_t = a^2 varc + vary_t + 1e-5 for t < T, xe = x - mux (length Tx) and c = fftCov (length Tx, real):
 *     ObjA = sum_t 1/2 log v_t + 1/2 y_t^2 / v_t,      dA_t = s a / v_t (1 - y_t^2 / v_t) varc,
 *     u = real(ifft(fft(xe) ./ c)),   ObjB = (u' xe) / (2 varx),   Obj = ObjA + ObjB,   dObj = u / varx, dA added to its first T entries.
 * x: Tx per problem, problem-major; y: T per problem.  vary: one per problem (vary_stride = 0) or T per problem (vary_stride = T, the
 * drivers' zeros(T, D) and the missing-data use).  The prior spectrum is either given -- fftCov, Tx entries shared by the problems
 * (cov_stride = 0) or per problem (cov_stride = Tx), len = NULL -- or formed on the device from len, one per problem, by
 * GetFFTCovFast.m:10-16, sqrt(2 pi len^2) exp(-w^2 len^2 / 2) + 1e-6 on w = 2 pi [0:Tx/2, -Tx/2+1:-1] / Tx (fftCov = NULL).
 * dObj = NULL: the objective only (the same Obj bits).
 * The transform is a complex FP64 FFT of the whole sequence with twiddles from a table built in extended precision: in LDS for
 * Tx <= 4096, as a four-step Tx = (Tx / 4096) x 4096 split of three kernels above.  u' xe and the sum of ObjA are formed in a fixed order
 * (a thread's samples ascending, a butterfly inside a wave, waves and workgroups in ascending order, all a function of Tx alone; no
 * floating-point atomics): a problem's result is the same to the bit alone, in a batch, with shared or own fftCov, with or without
 * dObj, through the one-shot or the resident form, and however the call is cut into device batches.
 * The resident form keeps y, vary, 1 / (c Tx), the parameters and the twiddles on the device: nagp_gppad_eval moves x in and Obj, dObj
 * out.  nagp_gppad_obj is create + eval + destroy.
 * All of the following is decided on the host before any device call.
 * NAGP_EUNSUPPORTED: Tx not a power of two, or outside 2 .. 2^20; one problem beyond the budget of the per-evaluation buffers, 1 GiB:
 *   every problem takes 8 (2 Tx (4 Tx when Tx > 4096) + 2 max(1, Tx / 4096) + 1) bytes of them.  A batch whose problems do not all fit is
 *   evaluated in device batches of as many as do.  (The resident arrays, 8 (T + 1 or T + Tx or 1) + 24 bytes per problem, are outside it.)
 * NAGP_EINVAL: a NULL handle, x, y, vary, varx, mux, varc or Obj; n_problems < 1; T < 1; T > Tx; vary_stride not 0 or T; cov_stride not
 *   0 or Tx; both or neither of len and fftCov; y, vary, len, fftCov, varx, mux or varc not finite; vary < 0; varx <= 0; varc <= 0;
 *   len <= 0; fftCov <= 0.
 * x is not examined: a result that is not finite is returned as it is (minimize halves its step on one). */
typedef struct nagp_gppad nagp_gppad; /* opaque */
int nagp_gppad_obj(int32_t n_problems, int64_t T, int64_t Tx,
                   const double* x /* n_problems x Tx */, const double* y /* n_problems x T */,
                   const double* vary, int64_t vary_stride /* 0 = one per problem, T = per sample */,
                   const double* len /* n_problems, read when fftCov == NULL */,
                   const double* fftCov, int64_t cov_stride /* NULL, or 0 = shared, Tx = per problem */,
                   const double* varx, const double* mux, const double* varc /* n_problems each */,
                   double* Obj /* n_problems */, double* dObj /* n_problems x Tx, or NULL */, int32_t device);
int nagp_gppad_create(nagp_gppad** handle, int32_t n_problems, int64_t T, int64_t Tx, const double* y,
                      const double* vary, int64_t vary_stride, const double* len, const double* fftCov, int64_t cov_stride,
                      const double* varx, const double* mux, const double* varc, int32_t device);
int nagp_gppad_eval(nagp_gppad* handle, const double* x, double* Obj, double* dObj /* or NULL */);
void nagp_gppad_destroy(nagp_gppad* handle);
/* Device time of the kernels of the last nagp_gppad_eval (or nagp_gppad_obj) on this thread, in ms (HIP events, summed over its device
 * batches). */
int nagp_gppad_timings(double* ms /* 1 */);

/* The objective that experiments/gppad/Cascade/MAPGPCasFast.m minimises -- the joint fine tuning of a cascade of M modulators,
 * GPPAD(Y,[len1;...;lenM]): Cascade/GetObjCasGPFAST.m:19-50 with its gradient, for a batch of cascades.  One cascade is X (Tx x M, the
 * .m's x = X(:)), y (T), one varc, and per column m a spectrum c_m (Tx, real), varx_m and mux_m.  With amp = GetAmp as above and
 * s = 1/(1 + exp(-x)):
 *     A_tm = amp(X_tm) (t < T),   P_t = prod_m A_tm (m ascending),   ObjA = sum_m sum_t log A_tm + (sum_t 1/2 (y_t / P_t)^2) / varc,
 *     D_t = 1 - y_t^2 / (varc P_t^2),   u_m = real(ifft(fft(X_:m - mux_m) ./ c_m)),   ObjB = sum_m (u_m' (X_:m - mux_m)) / (2 varx_m),
 *     dObj_tm = u_tm / varx_m + (t < T ? s_tm / A_tm D_t : 0),   Obj = ObjA + ObjB.
 * (No vary, no 1/2 log v and no 1e-5 in this objective.)  Wherever the .m's plain log(1 + exp(x)) is finite amp equals it to rounding,
 * and it stays finite beyond; entries of x outside +-700 give Inf or NaN as the .m does.
 * Layout, C order: x and dObj (n_problems, M, Tx) -- per cascade the .m's X(:) --, y (n_problems, T), len, varx, mux (n_problems, M), varc
 * (n_problems).  The spectra are either given -- fftCovs (M, Tx) shared by the cascades (cov_stride = 0) or (n_problems, M, Tx)
 * (cov_stride = M Tx), len = NULL -- or formed on the device from len (fftCovs = NULL) as for nagp_gppad_obj.  dObj = NULL: the
 * objective only (the same Obj bits).
 * The transforms are those of nagp_gppad_obj, one per column.  A pre-pass (one thread per sample) forms P_t, D_t and the sums of ObjA
 * over workgroups of 256 samples; the per-sample pass behind the inverse transform adds D_t; a finish kernel adds the workgroups, then the
 * columns, in ascending order (no floating-point atomics): the bits of a cascade are a function of (M, T, Tx) and its own data alone --
 * the same alone, in a batch, with shared or own spectra, with or without dObj, one-shot or resident, however the call is cut into
 * device batches.
 * All of the following is decided on the host before any device call.
 * NAGP_EUNSUPPORTED: M outside 1 .. 8; Tx not a power of two, or outside 2 .. 2^20; one cascade beyond the budget of the per-evaluation
 *   buffers (the 1 GiB of nagp_gppad_obj and its developer switch): a cascade takes
 *   8 (M (2 Tx (4 Tx when Tx > 4096) + 2 max(1, Tx / 4096)) + T + 2 ceil(T / 256) + 1) bytes of them.
 * NAGP_EINVAL: a NULL handle, x, y, varx, mux, varc or Obj; n_problems < 1; T < 1; T > Tx; cov_stride not 0 or M Tx; both or neither of
 *   len and fftCovs; y, len, fftCovs, varx, mux or varc not finite; varx <= 0; varc <= 0; len <= 0; fftCovs <= 0.
 * x is not examined. */
typedef struct nagp_gppad_cas nagp_gppad_cas; /* opaque */
int nagp_gppad_cas_obj(int32_t n_problems, int32_t M, int64_t T, int64_t Tx,
                       const double* x /* n_problems x M x Tx */, const double* y /* n_problems x T */,
                       const double* len /* n_problems x M, read when fftCovs == NULL */,
                       const double* fftCovs, int64_t cov_stride /* NULL, or 0 = M x Tx shared, M Tx = per cascade */,
                       const double* varx, const double* mux /* n_problems x M each */, const double* varc /* n_problems */,
                       double* Obj /* n_problems */, double* dObj /* n_problems x M x Tx, or NULL */, int32_t device);
int nagp_gppad_cas_create(nagp_gppad_cas** handle, int32_t n_problems, int32_t M, int64_t T, int64_t Tx, const double* y,
                          const double* len, const double* fftCovs, int64_t cov_stride,
                          const double* varx, const double* mux, const double* varc, int32_t device);
int nagp_gppad_cas_eval(nagp_gppad_cas* handle, const double* x, double* Obj, double* dObj /* or NULL */);
void nagp_gppad_cas_destroy(nagp_gppad_cas* handle);
/* Device time of the kernels of the last nagp_gppad_cas_eval (or nagp_gppad_cas_obj) on this thread, in ms. */
int nagp_gppad_cas_timings(double* ms /* 1 */);

/* The Laplace step of GPPAD -- experiments/gppad/GPModelFast/Laplace: the error bars of the envelope (GetErrorBarGPPAD.m) and the three
 * terms of the approximate marginal likelihood that the time-scale is learnt with (GetLaplaceObjGPPADOneChunk.m) -- for a batch of
 * problems (one chunk of one channel at one time-scale each) that share T and Tx.  With y, vary, len, varx, mux, varc as for
 * nagp_gppad_create, amp and s as there, c2 = 1/4 / cosh(x/2)^2, v = amp^2 varc + (vary + 1e-5), dv = 2 varc amp s (GetHessian.m):
 *     d_t = (c2 amp + s^2)/v (1 - y^2/v) varc - s amp/v^2 (1 - y^2/v) varc dv + s amp/v y^2/v^2 varc dv          (t < T),
 *     h = c varx (c = GetFFTCovFast(len, Tx)),   A v = ifft(h^1/2 .* fft([d .* a(1:T); 0])) with a = ifft(h^1/2 .* fft(v))   (SigDSigTimesV.m).
 * nagp_gppad_lap_hess sets the MAP point x (n_problems x Tx) and leaves d resident; nagp_gppad_lap_apply is A on given vectors.
 * nagp_gppad_lap_eig runs LanczosGPPAD.m on every problem from its own vstart (n_problems x Tx) with at most jmax steps (GetEigSigDSig.m:
 * jmax = 2 nev, tresh = 1e-12, tolconv = 1e-8): the three-term recurrence, the omega-recurrence with sign(0) = 0, the selective
 * reorthogonalisation (classical Gram-Schmidt of [v_j r] against v_1 .. v_{j-1}, a second pass when the spectral norm of h1 exceeds
 * 10 sqrt(eps), then r against v_j; beta(j+1) is not recomputed, as in the .m), the convergence test after a reorthogonalisation, at
 * jmax and when beta(j+1) < epert, the stop at beta(j+1) < epert or nconv >= nev.  The problems of a device batch run in lock-step; a
 * problem that has stopped is masked out of the later launches.  Per step alpha and beta (and h1 on a reorthogonalisation) come to the
 * host, which holds the recurrences and solves the tridiagonal eigenproblems (implicit QL; no LAPACK); the basis stays on the device.
 * Outputs: lmb (n_problems x jmax) the converged Ritz values in descending order, NaN beyond nconv; info per problem (steps,
 * reorthogonalisations, status: 0 fine, 1 a tridiagonal entry that is not finite, 2 the QL iteration did not converge -- with either,
 * nconv = 0 and the caller may draw another vstart); anorm the .m's estimate of |A|; xv (n_problems x jmax x Tx, rows beyond nconv not
 * written) = V s.  It also leaves Varx = varx - sum_k |ifft(h^1/2 .* fft(xv_k))|^2 l_k/(l_k + 1), l = max(lmb, 0), k ascending, on
 * the device; nagp_gppad_lap_varx(handle, 0, NULL, NULL, ...) fetches it, and with (K, xv, lmb) (n_problems x K x Tx, n_problems x K; a
 * NaN lmb skips its pair) forms it from given pairs instead.  n_negative counts the entries of Varx below 0 per problem (the .m stops
 * in the debugger there).  nconv = 0 is legal: Varx = varx, Obj0 = 0.
 * nagp_gppad_lap_obj: Obj (n_problems x 3) = Obj0 = -1/2 sum_k log|1 + l_k| (NaN before an eigen-solve), Obj1 = -1/2 sum_t (log v +
 * y^2/v), Obj2 = -(u' xe)/(2 varx): Obj1 + Obj2 is minus nagp_gppad_obj at x, from the same kernels.
 * Deviation: the Lanczos vectors are kept real (the .m carries the imaginary rounding noise of ifft along and drops it with real(lmb)).
 * Sums are formed in a fixed order without atomics: a problem's bits depend neither on its batch mates nor on the device batches.
 * NAGP_EUNSUPPORTED: Tx not a power of two, or outside 2 .. 2^20; one problem beyond the budget of the per-solve buffers (the 1 GiB of
 *   nagp_gppad_obj and its developer switch): a problem takes 8 ((2 jmax + 2 (+ 2 when Tx > 4096)) Tx + jmax^2 + 3 jmax +
 *   2 max(Tx / 256, 1) + 8) bytes of them (the basis and the Ritz vectors, jmax slots each).  The resident arrays (8 (4 Tx + 2 T) bytes
 *   per problem and the parameters) are outside it.
 * NAGP_EINVAL: a NULL argument that is not marked optional; n_problems < 1; T < 1; T > Tx; vary_stride not 0 or T; jmax outside
 *   1 .. min(Tx, 4096); the data not finite or out of range as for nagp_gppad_create; nev < 1; tresh or tolconv not > 0; K outside
 *   0 .. jmax; xv without lmb; apply, eig or obj before hess; varx without pairs before eig. */
typedef struct nagp_gppad_lap nagp_gppad_lap; /* opaque */
int nagp_gppad_lap_create(nagp_gppad_lap** handle, int32_t n_problems, int64_t T, int64_t Tx, const double* y,
                          const double* vary, int64_t vary_stride, const double* len, const double* varx, const double* mux,
                          const double* varc, int32_t jmax, int32_t device);
int nagp_gppad_lap_hess(nagp_gppad_lap* handle, const double* x /* n_problems x Tx */, double* d /* n_problems x T, or NULL */);
int nagp_gppad_lap_apply(nagp_gppad_lap* handle, const double* v, double* Av /* n_problems x Tx each */);
int nagp_gppad_lap_eig(nagp_gppad_lap* handle, int32_t nev, double tresh, double tolconv, const double* vstart /* n_problems x Tx */,
                       double* lmb /* n_problems x jmax */, int32_t* nconv /* n_problems */, int32_t* info /* n_problems x 3, or NULL */,
                       double* anorm /* n_problems, or NULL */, double* xv /* n_problems x jmax x Tx, or NULL */);
int nagp_gppad_lap_varx(nagp_gppad_lap* handle, int32_t K, const double* xv /* or NULL */, const double* lmb /* or NULL */,
                        double* Varx /* n_problems x Tx */, int64_t* n_negative /* n_problems, or NULL */);
int nagp_gppad_lap_obj(nagp_gppad_lap* handle, double* Obj /* n_problems x 3 */);
void nagp_gppad_lap_destroy(nagp_gppad_lap* handle);
/* Device span of the last nagp_gppad_lap_eig on this thread, in ms (HIP events around each device batch: the kernels and the host's
 * control between them). */
int nagp_gppad_lap_timings(double* ms /* 1 */);

/* The objectives that experiments/nmf/nmf.m and nmf_inf.m minimise by conjugate gradients -- the NMF with temporal priors on the
 * activations that the training drivers keep next to their nmf_fp call (train_model.m:123), and its inference-only form for missing
 * data and denoising: getObj_nmf_temp.m (learning form, W = NULL: x = [log H(:); log W(:)], T K + K D entries per problem) and
 * getObj_nmf_temp_inf.m (inference form, W given, K x D per problem: x = log H(:), T K entries), with their gradients, for a batch of
 * problems (restarts) that share A and vary.  All matrices column-major: A, vary T x D, H T x K, W K x D.  Kept literally (:45-66):
 *     H = exp(logH);   learning form: W = exp(logW), W = diag(1 ./ sum(W,2)) W;   inference form: W as given, NOT renormalised
 *     Ahat = H W + vary,   obj1 = sum(A ./ Ahat + log(Ahat)),   dA = (Ahat - A) ./ Ahat.^2,   dlogh = (dA W') .* H,
 *     learning form: dW = H' dA, dWW = dW .* W, dlogw = dWW - diag(sum(dWW,2)) W.
 * The prior stands for the .m's nargin branches:
 *   NAGP_NMFT_NONE: obj = obj1 / T.
 *   NAGP_NMFT_TG (:109-131), truncated-Gaussian AR(1) chain with varinf, lam (K each):
 *     obj2 = sum_k (1+lam^2)/(2 varinf) sum_{t=2..T-1} H^2 + 1/(2 varinf) H(T)^2 + lam^2/(2 varinf) H(1)^2 - lam/varinf sum_{t=2..T} H(t) H(t-1),
 *     dobj2dH: t = 1: lam^2/varinf H(1) - lam/varinf H(2);   1 < t < T: (1+lam^2)/varinf H(t) - lam/varinf (H(t+1) + H(t-1));
 *              t = T: 1/varinf H(T) - lam/varinf H(T-1)      -- three different row forms, as the .m has them.
 *   NAGP_NMFT_IG (:69-107), inverse-gamma Markov chain with muinf, varinf, lam: alp1 = muinf^2/varinf + 2, bet1 = (alp1 - 1) muinf,
 *     alp = 2 + lam^2 + muinf^2/varinf, a = (alp - 1) lam, b = (alp - 1)(1 - lam) muinf, ahtpb(t) = a H(t) + b (t < T),
 *     obj2 = sum_k bet1/H(1) + (alp1+1) logH(1) - alp sum_{t<T} log ahtpb(t) + (alp+1) sum_{t>1} logH(t) + sum_{t>1} ahtpb(t-1)/H(t),
 *     dobj2dH: t = 1: a/H(2) - bet1/H(1)^2 + (alp1+1)/H(1) - alp a/ahtpb(1);
 *              1 < t < T: a/H(t+1) - ahtpb(t-1)/H(t)^2 + (alp+1)/H(t) - alp a/ahtpb(t);   t = T: -ahtpb(T-1)/H(T)^2 + (1+alp)/H(T).
 *   With a prior obj = (obj1 + obj2) / T and dlogh += dobj2dH .* H; the whole gradient is divided by T.
 * muinf, varinf, lam: K each, shared by the problems; NULL where the prior does not read them.  vary = NULL: zeros.  dObj = NULL: the
 * objective only (the same Obj bits).  Every sum over t is formed in an order that depends on the shape alone (a butterfly inside a
 * wave, the waves of a workgroup and the workgroups in a fixed order; the K x D products H' dA on the matrix cores per workgroup; no
 * floating-point atomics): a problem's result is the same to the bit alone, in a batch, with or without dObj, through the one-shot or
 * the resident form, and however the call is cut into device batches.
 * The resident form keeps A, vary, a given W, the prior parameters and the partial-sum buffers on the device: nagp_nmf_temp_eval moves x
 * in and Obj, dObj out.  nagp_nmf_temp_obj is create + eval + destroy.
 * All of the following is decided on the host before any device call.
 * NAGP_EINVAL: a NULL handle, x, A or Obj; n_problems, D or K < 1; T < 1, or T < 2 with a prior (the .m indexes H(2,:)); an unknown
 *   prior; a prior parameter array NULL where it is read; A, vary, W or a prior parameter not finite; a negative A or vary; a negative
 *   entry or an all-zero row of a given W; varinf <= 0; for NAGP_NMFT_IG muinf <= 0 or lam outside [0, 1] (beyond that ahtpb can be
 *   negative and its log fails).
 * NAGP_EUNSUPPORTED: D > 64 or K > 16 (W lives in the LDS, H(t,:) in registers, K is padded to one MFMA tile); one problem beyond the
 *   budget of the per-evaluation buffers, 1 GiB: with nx = T K (+ K D in the learning form) and nq = 0, 4, 5 for NONE, TG, IG every
 *   problem takes 8 (2 nx + ceil(T / 256) ((K D in the learning form) + 1 + nq K) + 1) bytes of them.  A batch whose problems do not all
 *   fit is evaluated in device batches of as many as do.  (The resident arrays, 8 T D (twice with vary) + 8 K D per problem of a given
 *   W + 24 K bytes, are outside it.)
 * x is not examined: a result that is not finite is returned as it is (minimize halves its step on one). */
enum { NAGP_NMFT_NONE = 0, NAGP_NMFT_TG = 1, NAGP_NMFT_IG = 2 };
typedef struct nagp_nmf_temp nagp_nmf_temp; /* opaque */
int nagp_nmf_temp_obj(int32_t n_problems, int64_t T, int32_t D, int32_t K, int32_t prior,
                      const double* x /* n_problems x (T K + K D), or x (T K) with W */,
                      const double* A /* T x D, shared */, const double* vary /* T x D shared, or NULL = zeros */,
                      const double* W /* NULL: learning form; else K x D per problem: inference form */,
                      const double* muinf, const double* varinf, const double* lam /* K each, shared; NULL where not read */,
                      double* Obj /* n_problems */, double* dObj /* as x, or NULL = objective only */, int32_t device);
int nagp_nmf_temp_create(nagp_nmf_temp** handle, int32_t n_problems, int64_t T, int32_t D, int32_t K, int32_t prior,
                         const double* A, const double* vary, const double* W,
                         const double* muinf, const double* varinf, const double* lam, int32_t device);
int nagp_nmf_temp_eval(nagp_nmf_temp* handle, const double* x, double* Obj, double* dObj /* or NULL */);
void nagp_nmf_temp_destroy(nagp_nmf_temp* handle);
/* Device time of the two kernels of the last nagp_nmf_temp_eval (or nagp_nmf_temp_obj) on this thread, in ms (HIP events, summed over
 * its device batches). */
int nagp_nmf_temp_timings(double* ms /* 1 */);

/* The NMF whose activations are exp(mux + a squared-exponential GP) in its basis-function form -- experiments/nmf/tnmf.m, tnmf_inf.m and
 * experiments/toolsGP/fitSEGP_BF.m minimise the three objectives below by conjugate gradients -- and the primitive they share,
 * basis2SEGP.m:21-28, per column with its own lenx, varx:
 *     tau = ceil(lenx / sqrt(2) * tol),   bh = sqrt(varx sqrt(2) / (lenx sqrt(pi))),   bas(s) = bh exp(-1 / lenx^2 * s^2),  s = -tau .. tau,
 *     conv(Z)(t) = sum_{s = -tau .. tau} bas(s) Z(t - s),   Z = 0 outside 1 .. T      (conv(Z, bas, 'same'), 2 tau + 1 odd).
 * Any tau >= 0, also 2 tau + 1 > T; no tap is dropped however small it is.  The taps are built on the host, once per handle (per call of
 * the one-shot forms).  Every output adds its taps in ascending s, by a direct sum (there is no FFT form): no floating-point atomics and
 * no order that depends on the grid, so a column's result is the same to the bit alone, in a batch, with or without dObj, through the
 * one-shot or the resident form, and however the call is cut into device batches.  All matrices column-major.
 *   nagp_sebf_conv (basis2SEGP.m): Y(:, q) = conv(Z(:, q)) for n_cols columns of T samples, lenx, varx n_cols each.
 *   nagp_sebf_fit_* (getObj_fitSE_basis_func.m:25-43), n_problems columns, each with its own target x (T), lenx, varx:
 *     xHat = conv(z), dx = xHat - x, obj = (1/2 sum dx^2 + 1/2 sum z^2) / T, dobj = (conv(dx) + z) / T.
 *   nagp_tnmf_* (getObj_nmf_log_norm.m:31-83 with W = NULL, the learning form: x = [X(:); log W(:)], T K + K D entries per problem;
 *   getObj_nmf_log_norm_inf.m:32-74 with W given, K x D per problem, used as it is and NOT renormalised: x = X(:), T K entries), for a
 *   batch of problems that share A (T x D), vary, lenx, mux, varx (K each) and tol:
 *     H(:, k) = exp(conv(X(:, k)) + mux(k)),   learning form: W = exp(logW), W = diag(1 ./ sum(W,2)) W,   Ahat = H W + vary,
 *     obj1 = sum(A ./ Ahat + log(Ahat)),   dA = (Ahat - A) ./ Ahat.^2,   dX(:, k) = conv((dA W')(:, k) .* H(:, k)),
 *     learning form: dW = H' dA, dWW = dW .* W, dlogw = dWW - diag(sum(dWW,2)) W,
 *     obj = (obj1 + 1/2 sum X^2) / T,   dobj = [dX(:) + X(:); dlogw(:)] / T.
 *   Between the two convolutions the row arithmetic is that of nagp_nmf_temp_obj with NAGP_NMFT_NONE on logH = conv(X) + mux (the same
 *   kernels, on the device-resident array); the division by T is applied to (dA W') .* H before the second convolution and to X, and to
 *   obj1 and 1/2 sum X^2 each.  1/2 sum X^2, sum dx^2 and sum z^2 are formed in an order that depends on the shape alone.
 * vary = NULL: zeros.  dObj = NULL: the objective only (the same Obj bits).  The resident forms keep the taps, the targets (fit), A,
 * vary, a given W and every intermediate on the device: *_eval moves x (z) in and Obj, dObj out.  *_obj is create + eval + destroy.
 * All of the following is decided on the host before any device call.
 * NAGP_EINVAL: a NULL handle, Z, Y, z, x, A, Obj, lenx, varx or mux; n_cols, n_problems, T, D or K < 1; lenx not finite or <= 0; varx not
 *   finite or < 0; tol not finite or < 0; mux not finite; A, vary or W not finite or negative; an all-zero row of a given W.
 * NAGP_EUNSUPPORTED: tau > 2^30 - 1 (2 tau + 1 taps are counted in an int32); D > 64 or K > 16 (the limits of nagp_nmf_temp_obj, whose
 *   row kernels run here); one column or problem beyond the budget of the per-evaluation buffers, 1 GiB: a column of nagp_sebf_conv takes
 *   16 T bytes of them, a problem of nagp_sebf_fit 8 (3 T + 1), a problem of nagp_tnmf, with nx = T K (+ K D in the learning form),
 *   8 (4 nx + ceil(T / 256) ((K D in the learning form) + 1) + 1).  A batch that does not fit is evaluated in device batches of as many
 *   as do.  (The taps, 8 (2 tau + 1) bytes per column, the targets and A, vary, W are outside it.)
 * x, z, Z and the targets of the fit are not examined: a result that is not finite is returned as it is. */
int nagp_sebf_conv(int32_t n_cols, int64_t T, const double* Z /* T x n_cols */, const double* lenx, const double* varx /* n_cols each */,
                   double tol, double* Y /* T x n_cols */, int32_t device);
typedef struct nagp_sebf_fit nagp_sebf_fit; /* opaque */
int nagp_sebf_fit_obj(int32_t n_problems, int64_t T, const double* z /* T x n_problems */, const double* x /* T x n_problems: the targets */,
                      const double* lenx, const double* varx /* n_problems each */, double tol,
                      double* Obj /* n_problems */, double* dObj /* as z, or NULL = objective only */, int32_t device);
int nagp_sebf_fit_create(nagp_sebf_fit** handle, int32_t n_problems, int64_t T, const double* x, const double* lenx, const double* varx,
                         double tol, int32_t device);
int nagp_sebf_fit_eval(nagp_sebf_fit* handle, const double* z, double* Obj, double* dObj /* or NULL */);
void nagp_sebf_fit_destroy(nagp_sebf_fit* handle);
typedef struct nagp_tnmf nagp_tnmf; /* opaque */
int nagp_tnmf_obj(int32_t n_problems, int64_t T, int32_t D, int32_t K,
                  const double* x /* n_problems x (T K + K D), or x (T K) with W */,
                  const double* A /* T x D, shared */, const double* vary /* T x D shared, or NULL = zeros */,
                  const double* W /* NULL: learning form; else K x D per problem: inference form */,
                  const double* lenx, const double* mux, const double* varx /* K each, shared */, double tol,
                  double* Obj /* n_problems */, double* dObj /* as x, or NULL = objective only */, int32_t device);
int nagp_tnmf_create(nagp_tnmf** handle, int32_t n_problems, int64_t T, int32_t D, int32_t K, const double* A, const double* vary,
                     const double* W, const double* lenx, const double* mux, const double* varx, double tol, int32_t device);
int nagp_tnmf_eval(nagp_tnmf* handle, const double* x, double* Obj, double* dObj /* or NULL */);
void nagp_tnmf_destroy(nagp_tnmf* handle);
/* Device time of the last nagp_tnmf_eval, nagp_sebf_fit_eval (or their one-shot forms) or nagp_sebf_conv on this thread, in ms (HIP
 * events, summed over its device batches): the forward convolution, the rows (the reduction of the fit), the adjoint convolution. */
int nagp_tnmf_timings(double* ms /* 3: forward conv, rows, adjoint conv */);

/* What the drivers do next with Eft / Varft (demo_toy_modulators_nmf.m:119-158, the same block in the other
 * demos): the reconstructed signal sig = sum_d (W link(g))_d z_d and the modulator amplitudes link(g_n) under the independent
 * posterior marginals z_d ~ N(Eft_d, Varft_d), g_n ~ N(Eft_{D+n}, Varft_{D+n}) of every time step:
 *   Eft_mod (N x T) = mean link(g_n), Varft_mod = var link(g_n), Esig (T) = mean sig, Vsig = var sig.
 * n_samples = 0: the population values (Gauss-Hermite rule gh_x, gh_w of n_gh points for the standard normal weight per
 *   modulator -- exp link: closed form -- then closed-form combination);
 * n_samples >= 2: the reference's estimator (s = 250 there): sample mean and variance (s-1) over draws of a counter-based
 *   generator (Philox4x32-10 keyed by `seed`, Box-Muller), reproducible on the host.
 * Eft, Varft: M x T column-major as returned by the *_run calls; Wnmf D x N column-major. */
int nagp_reconstruct(int32_t D, int32_t N, int64_t T, const double* Eft, const double* Varft, const double* Wnmf,
                     int32_t link_kind, double link_shift, int32_t n_gh, const double* gh_x, const double* gh_w,
                     int32_t n_samples, uint64_t seed, double* Esig, double* Vsig, double* Eft_mod, double* Varft_mod, int32_t device);

/* The same post-processing as the experiment scripts write it (experiments/noise_reduction_speech.m:142, missing_data_music.m:173,
 * test_missing_data.m:159, synthetic_data_experiment.m:221, source_sep_piano.m:165-244): an amplitude kind -- a_d = W_d.lk (the demos,
 * nagp_reconstruct) or a_d = sqrt(W_d.lk) (the model of NAGP_LIK_POWER_NMF_SQRT), lk = link(g) --, a partition of the sub-bands into
 * J sources and the envelopes.  Under the independent marginals of every step (as above)
 *     sig = sum_d a_d z_d,   sig_j = sum_{d in source j} a_d z_d,   env_d = a_d
 * and the outputs are Esig / Vsig (T), Esrc / Vsrc (J x T: Esig1..3 / Vsig1..3 of source_sep_piano.m:229-234), Eenv (D x T: `envs`, :218,
 * :225) and Eft_mod / Varft_mod (N x T) as in nagp_reconstruct.  sig is summed on its own, not as sum_j sig_j.
 * n_samples >= 2: the scripts' estimator (mean, var with s-1, Eenv = mean over the draws) on the draws of nagp_reconstruct (same generator,
 *   same counters: with NAGP_AMP_LINEAR and one source Esig, Vsig, Eft_mod, Varft_mod are those of nagp_reconstruct).
 * n_samples = 0: the population values.  Eft_mod / Varft_mod from the 1-D rule gh_x, gh_w (exp link: closed form).  NAGP_AMP_LINEAR: the
 *   closed forms of nagp_reconstruct restricted to each source, Eenv = W E lk.  NAGP_AMP_SQRT: E a_d^2 = W_d.E lk is exact from the 1-D
 *   rule; E a_d and the moments of u_j(g) = sum_{d in j} a_d(g) Eft_d come from the caller's N-dimensional rule (wn, xn_unscaled: unit
 *   points for the standard normal weight, as in nagp_opts; g_n = Eft_n + sqrt(Varft_n) x_n):
 *     Esig_j = E u_j,   Vsig_j = sum_{d in j} (W_d.E lk) Varft_d + E u_j^2 - (E u_j)^2,
 *   the last difference accumulated about u_j at the centre g = Eft (exact for weights of any sum).
 * A negative W_d.lk under NAGP_AMP_SQRT gives NaN in that sub-band's envelope, its source and the total (MATLAB goes complex there).
 * N <= 9, D + N <= 64, J <= 8.  NAGP_EINVAL (host checks, before any device call): NULL inputs, bad sizes, unknown amp / link kind,
 * n_samples < 0 or == 1, source_offsets not 0 = off[0] < ... < off[J] = D (NULL only with J = 1), population form without the rule
 * it needs (softplus: the 1-D rule; NAGP_AMP_SQRT: the N-dimensional rule), every pointer of `out` NULL. */
typedef enum nagp_amp { NAGP_AMP_LINEAR = 0, NAGP_AMP_SQRT = 1 } nagp_amp;
typedef struct nagp_recon_opts {
  int32_t amp_kind;                 /* nagp_amp */
  int32_t link_kind; double link_shift;
  int32_t n_sources;                /* J >= 1 */
  const int32_t* source_offsets;    /* J+1 ascending, [0] = 0, [J] = D: source j owns sub-bands [off[j], off[j+1]); NULL only with J = 1 */
  int32_t n_samples; uint64_t seed; /* >= 2: sampling form; 0: population form */
  int32_t n_gh; const double* gh_x; const double* gh_w;                 /* 1-D rule, population form */
  int32_t n_pts; const double* wn; const double* xn_unscaled;           /* N x n_pts rule (as nagp_opts), population form with NAGP_AMP_SQRT */
  int32_t device;
} nagp_recon_opts;
typedef struct nagp_recon_out {     /* caller-allocated, any pointer may be NULL */
  double *Esig, *Vsig;              /* T */
  double *Esrc, *Vsrc;              /* J x T column-major */
  double *Eenv;                     /* D x T: mean amplitude a_d (source_sep_piano.m:218,225) */
  double *Eft_mod, *Varft_mod;      /* N x T */
} nagp_recon_out;
int nagp_reconstruct_sources(int32_t D, int32_t N, int64_t T, const double* Eft, const double* Varft, const double* Wnmf,
                             const nagp_recon_opts* opts, nagp_recon_out* out);

/* Joint posterior draws of a full-covariance EP run -- gf_ep_modulator.m, gf_ep_modulator_nmf.m, gf_ep_modulator_nmf_constraints.m in
 * predict mode -- whole state paths, correlated in time.  The drivers draw sub_samp / mod_samp independently per time step from Eft / Varft
 * (demo_nonstationary_filterbank.m:226-258, noise_reduction_speech.m:107-145; nagp_reconstruct* restates that): error bars on anything that
 * couples time steps (the energy of a separated source over a note, a filled gap of missing_data_music.m) need joint draws, and a gap can be
 * filled with texture only by one -- the argument made for the filterbank above.
 * The law.  The last forward pass of a run (gf_ep_modulator_nmf.m:126-184) is a linear recursion in the sites (ttau, tnu) the run returned,
 * and the RTS smoother on top of it (:207-234) defines one Gaussian over the state path.  Forward, from m = 0, P = Pinf:
 *     k > 0 (and k = 0 with predict_at_k1):  m = A m,  P = A P A' + Q;
 *     where y_k is not NaN, with fmu = H m, W = P H', HPH = diag(H P H') and the sites of step k (:159-176; no mom call anywhere: the
 *     returned sites hold the refresh of step T-1):
 *       sites with ttau == 0:  z = ttau HPH + 1,  K = W ttau / z,  m = m - W (ttau fmu - tnu) / z,  P = P - K W'  (K = 0: P stays);
 *       the other sites:       K = W / (HPH + 1 / ttau)  (diagonal innovation),  m = m + K (tnu / ttau - fmu),  P = P - (K H) P;
 *     MF_k = m, PF_k = P.
 * Per step k < T-1, independent of the other steps:
 *     PSkp = A PF_k A' + Q  (its lower triangle, as chol(., 'lower') reads it),  L = chol(PSkp), after a failure once more with
 *     sqrt(1e-4) 0.5 I added (:216-223 with rand -> 0.5), counted in counters[0];   G_k = PF_k A' / L' / L  (the two triangular solves);
 *     C_k = (I - G_k A) PF_k (I - G_k A)' + G_k Q G_k'  (lower triangle),   Lc_k = chol(C_k): a pivot <= 0 zeroes its column and is counted
 *     in counters[1] -- never a NaN, never silent;   Lc_{T-1} = chol(PF_{T-1}) likewise.
 * Draw i:
 *     x_{T-1} = MF_{T-1} + Lc_{T-1} z_{T-1},      x_k = MF_k + G_k (x_{k+1} - A MF_k) + Lc_k z_k    (k = T-2 .. 0),
 *     z_k[j] = z[(i T + k) S + j] when the caller passes its normals, else normals(T, j, n_draws, seed)[k, i]: the counter-based generator of
 *     nagp_reconstruct with the counter word "site" set to the state index j, as nagp_fastfb_sample uses it.  Draw i does not depend on
 *     n_draws or on how the draws are batched on the device.
 * The marginals of this chain are exactly the MS_k, PS_k (hence Eft, Varft) of the run, its lag-one covariances G_k PS_{k+1}.
 * Outputs (each may be NULL, not all four):  Xdraw, n_draws blocks of S x T column-major;  Fdraw, n_draws blocks of M x T,
 *     Fdraw_i[n, k] = h_val[n] x_k[block_offsets[n]];  MS (S x T), the chain with every z = 0: the RTS means;
 *     Sdraw (n_draws x T, needs sig):  Sdraw_i[k] = sum_d a_d z_d with z_d = Fdraw_i[d, k], g_n = Fdraw_i[D + n, k] and
 *     a_d = W_d.link(g) (NAGP_AMP_LINEAR) or sqrt(W_d.link(g)) (NAGP_AMP_SQRT), link as nagp_link: the amplitudes of nagp_reconstruct_sources
 *     on the draw's own values (gf_ep_modulator: D = N, Wnmf = I).  sig uses the model's D and N (D + N = M).
 * counters (2, may be NULL): jitter retries of PSkp, clamped pivots of C_k and PF_{T-1}.  Both are zero on every model the suite runs.
 * nagp_ep_sample_timings: device time of the last call on this thread in ms (HIP events): the filter, the factorisation, the draws (the mean
 * chain and every device batch).
 * Limits, all decided on the host before any device call:
 * NAGP_EUNSUPPORTED: a block of more than 8 states; S > 80 -- the factorisation of a step keeps three S x S operands (3 * 8 S^2 bytes) in
 *   the 160 KiB LDS of one workgroup, and the filter P, M staged rows and M gain columns (8 (S^2 + 2 S M) bytes and change).
 * NAGP_ENOMEM: the per-step storage does not fit the device-memory budget of a call, 48 GiB: a call takes
 *     8 (T (2 S^2 + 2 S + 2 M + 1) + 3 S^2 + 2 sum_n b_n^2 + M + D N + 8) + 4 (2 M + 2 + S) + 4096 bytes   (PF_k / G_k, Lc_k, MF, MS, the sites, y)
 *   and every draw 8 T ([z: S] + [Xdraw: S] + [Fdraw or Sdraw: M] + [Sdraw: 1]) bytes; the draws run in device batches of as many as fit
 *   (whole blocks of 16 when more than 16 do).  There is no checkpoint scheme: a T beyond the budget is refused.
 * NAGP_EINVAL: a NULL model, ttau, tnu or y, or a NULL array of the model; T or n_draws < 1; S or M < 1, M > S, block_offsets not strictly
 *   ascending from 0 to S; a negative or non-finite ttau; a non-finite tnu; Sdraw without sig; sig with a NULL or non-finite Wnmf, an unknown
 *   amplitude or link kind, or D + N != M; no output at all.
 * NAGP_ENOTPD (after the run): PSkp not positive definite even with the jitter, where MATLAB's chol throws.
 * Out of scope: the EKF family (nagp_giekf_run: its filter is not a function of sites; it could take (MF, PF) later); the
 * infinite-horizon family (no per-step covariances: the law of a draw is not defined there); the mixture drivers, whose rule
 * (NAGP_FLAG_MIXTURE_RULE) has not been checked against the fixed-site step above and which the Python and MATLAB wrappers therefore do
 * not offer; per-source signal draws (Fdraw is enough to form them). */
typedef struct nagp_epsample_sig {
  const double* Wnmf;   /* D x N column-major */
  int32_t amp_kind;     /* nagp_amp */
  int32_t link_kind;    /* nagp_link */
  double link_shift;    /* softplus shift */
} nagp_epsample_sig;
int nagp_ep_sample(const nagp_model* model, const double* ttau, const double* tnu /* M x T column-major */,
                   const double* y /* T: only which entries are NaN is read */, int64_t T,
                   int32_t predict_at_k1, int32_t n_draws, uint64_t seed,
                   const double* z /* optional: caller's normals, n_draws x T x S, draw-major then column-major S x T; NULL = generator */,
                   const nagp_epsample_sig* sig /* optional: Wnmf, amp kind, link kind, shift for Sdraw; NULL = no Sdraw */,
                   double* Xdraw /* n_draws x (S x T) */, double* Fdraw /* n_draws x (M x T) */,
                   double* Sdraw /* n_draws x T */, double* MS /* S x T */,
                   int64_t* counters /* 2: PSkp jitter retries, clamped pivots of C_k */, int32_t device);
int nagp_ep_sample_timings(double* ms /* 3: filter, factor, draw */);

/* Batched / device-resident form: n_problems independent problems of identical shape
 * (S, M, block structure, T) -- audio segments or hyper-parameter replicas -- run concurrently. */
int nagp_plan_create(nagp_plan** plan, int32_t n_problems, const nagp_model* models,
                     const nagp_ihgp_tables* tables /* n_problems or NULL */, int64_t T, const nagp_opts* opts);
int nagp_plan_upload_y(nagp_plan* plan, const double* const* ys); /* n_problems pointers to T doubles (NaN = missing) */
int nagp_plan_execute(nagp_plan* plan);                          /* enqueue all sweeps; returns after stream sync */
int nagp_plan_timings(const nagp_plan* plan, nagp_timings* t);
int nagp_plan_download(nagp_plan* plan, nagp_out* outs);          /* n_problems outs */
int nagp_plan_upload_sites(nagp_plan* plan, const double* const* ttau0, const double* const* tnu0); /* warm start: n_problems pointers to
                                                                     M x T doubles each, or NULL/NULL to return to cold starts */
int64_t nagp_plan_device_bytes(const nagp_plan* plan);

/* Opt-in time-parallel schedule of the fixed-site Kalman filter (NAGP_KIND_GF_EP, sweeps >= 2, predict and nlml mode).  In those sweeps the
 * sites are fixed for the steps k < T-1 and the filter is one workgroup per problem, sequential in k.  With the option set, [0, T-1) is cut
 * into n_windows windows that run at the same time, one workgroup per (problem, window): window j >= 1 starts `overlap` steps early from the
 * prior (m = 0, P = Pinf), runs those warm-up steps without storing anything and stores from its first own step on -- a Kalman filter with
 * fixed sites forgets its start (profiles/r07_window_contraction.txt: how fast, per model).  Nothing is taken on trust: the state a window
 * started its own steps from is compared with what the window in front of it stored for that step,
 *     mismatch_m = max|dm| / max(max|m|, sqrt(max|P|)),   mismatch_P = max|dP| / max|P|,
 * boundary by boundary in increasing order, and a window whose boundary is above `tol` in either figure runs again from the stored state
 * (the sequential continuation), after which the next boundary is checked against the re-run.  Worst case: the sequential time plus the
 * warm-ups; tol = 0 re-runs every window and gives the sequential result bit for bit.  What a window within tol leaves in the outputs is
 * its boundary mismatch propagated (and contracted further) through its own steps.
 * n_windows <= 1 turns the option off: every launch, buffer and output is then what a plan that never called this is.  The option holds for
 * every later nagp_plan_execute.  On a windowed sweep the smoother starts behind the filter (no chunk pipeline beside it) and the cross-sweep
 * schedule is not used: windows pay where compute units are idle -- one long sequence, or fewer segments than compute units.
 * NAGP_EUNSUPPORTED for n_windows > 1 on NAGP_KIND_IHGP / NAGP_KIND_GIEKF plans, NAGP_EINVAL for overlap < 0 or tol < 0 (host checks, before any device call). */
int nagp_plan_set_windows(nagp_plan* plan, int32_t n_windows, int32_t overlap, double tol);
/* What the windows of the last nagp_plan_execute did, summed over its sweeps.  A window counts once however many problems the plan holds
 * (its workgroups run, pass or re-run together: a boundary passes when every problem is within tol). */
typedef struct nagp_window_stats {
  int64_t windows_run;        /* windows launched in the time-parallel launches */
  int64_t boundaries_checked; /* boundary comparisons read by the host */
  int64_t reruns;             /* windows run again from the stored state */
  int64_t warmup_steps;       /* warm-up steps of those windows (per problem) */
  double worst_m;             /* largest mismatch_m seen at a checked boundary (Inf: a NaN state) */
  double worst_P;             /* largest mismatch_P */
} nagp_window_stats;
int nagp_plan_window_stats(const nagp_plan* plan, nagp_window_stats* stats);
/* The geometry nagp_plan_set_windows uses (pure host code): the fixed-site pass covers the steps [0, T-1); they are cut into
 * P = min(n_windows, T-1) windows (at least one) of equal length to within a step.  Returns P (or a negative status);
 * t_start[0 .. P] (P+1 entries, t_start[P] = T-1; room for n_windows + 1): window j stores the steps [t_start[j], t_start[j+1]);
 * t_warm[0 .. P-1] (room for n_windows): its warm-up starts at t_warm[j] = max(0, t_start[j] - overlap), t_warm[0] = 0. */
int nagp_window_partition(int64_t T, int32_t n_windows, int32_t overlap, int64_t* t_start, int64_t* t_warm);
void nagp_plan_destroy(nagp_plan* plan);

/* Multi-GPU form of the batched call (one process, the GPUs of one node) -- what a MEX caller uses to spread audio segments
 * or the numel(w)+1 objective evaluations of a fminunc iteration (train_GTFNMF.m:186-201) over the node:
 * problem i runs on device i mod n_gpus (nagp_batch_partition), one host thread, plan and stream per device, host buffers in
 * and out as in nagp_plan_*; the only exchange is the sum over ALL problems of the per-sweep negative log marginal likelihood
 * nlZ[itt] = -sum_k lZ_k (gf_ep_modulator_nmf.m:187, 277, 525), all-reduced over the devices with RCCL
 * (ncclAllReduce, ncclDouble, ncclSum, count = ep_itts) and returned in nlZ_total (ep_itts doubles, may be NULL).
 * opts->device is ignored; opts->ttau0 / tnu0 must be NULL (they describe ONE problem: NAGP_EINVAL otherwise -- warm-started
 * batches go through nagp_plan_create + nagp_plan_upload_sites).  n_gpus = 1 involves no collective unless the environment sets NAGP_FORCE_RCCL.  The RCCL
 * communicators are created on first use and kept until nagp_shutdown(). */
int nagp_batch_partition(int32_t n_problems, int32_t n_gpus, int32_t* device_of_problem /* n_problems */);
int nagp_batch_run(int32_t n_problems, const nagp_model* models, const nagp_ihgp_tables* tables /* n_problems or NULL */,
                   const double* const* ys, int64_t T, const nagp_opts* opts, nagp_out* outs, int32_t n_gpus,
                   double* nlZ_total);
void nagp_shutdown(void); /* releases cached RCCL communicators; never resets a device */

#ifdef __cplusplus
}
#endif
#endif /* NAGP_H */
