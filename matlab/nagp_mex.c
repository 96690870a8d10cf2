/*
 * nagp_mex.c -- MEX gateway between the reference-named MATLAB wrappers in this directory and the C ABI of
 * include/nagp.h (libnagp.so: HIP kernels for gfx950).  Logic-free by design: it maps mxArray fields to the structs of
 * nagp.h, allocates the outputs and turns status codes into MATLAB errors.
 *
 *   mex -R2017b -I<repo>/include nagp_mex.c -L<repo>/nonstationary-audio-gp_amd -lnagp
 *
 *   [Eft,Varft,ttau,tnu,R,lZ,nlZ,maxDiffM,maxDiffP,counters,MS,PS] = nagp_mex(model, y, opts)
 *   [Eft,...] = nagp_mex(model, y, opts, tables)            % infinite-horizon kind
 *
 * model  struct: A, Q, Pinf (S x S double), block_offsets (int32, M+1, 0-based), h_val (M x 1), Wnmf (D x N or []),
 *                D, N, lik_param                                         -> nagp_model
 * y      double vector (NaN = missing)
 * opts   struct: kind, mode, lik_kind, link_kind, link_shift, wn, xn_unscaled, ep_fraction, ep_damping, l_iter,
 *                predict_at_k1, flags, device [, chunk, ttau0, tnu0, ep_itts, windows, window_overlap, window_tol]  -> nagp_opts (windows: nagp_plan_set_windows)
 *                (ep_itts defaults to numel(ep_damping); the EKF kind passes it explicitly as g_iter)
 * tables struct: r (n_grid x 1), PP, PG (double vectors), pp_off, pg_off (int64, M)          -> nagp_ihgp_tables
 *
 * Further entry points of include/nagp.h, selected by a command string in the first argument:
 *   [M,P,K,MU,S] = nagp_mex('iekf_update1', M, P, y, h_col(int32, 0-based), h_val, Wnmf, R, iters [,device])   nagp_iekf_update1
 *   [MS, sum_v2] = nagp_mex('fastfb', A, AKHA, HA, K, G ([] = filter only), y [,device])                       nagp_fastfb_run
 *   [Ydraw, Xdraw, MS] = nagp_mex('fastfb_sample', A, AKHA, HA, K, G, H, R, Lp, Lq, y, n_draws, seed [,device])   nagp_fastfb_sample
 *                                    Ydraw T x n_draws, Xdraw S x T x n_draws (computed only when asked for), MS S x T
 *   [Fdraw, Xdraw, Sdraw, MS, counters] = nagp_mex('ep_sample', model, ttau, tnu, y, predict_at_k1, n_draws, seed, z, sig [,device])   nagp_ep_sample
 *                                    joint posterior draws of a full-covariance EP run from its sites: ttau, tnu M x T; z [] (the generator) or
 *                                    S x T x n_draws normals of the caller; sig [] or a struct Wnmf (D x N), amp_kind, link_kind, link_shift;
 *                                    Fdraw M x T x n_draws, Xdraw S x T x n_draws, Sdraw T x n_draws ([] without sig), MS S x T, counters 2 x 1
 *                                    (Xdraw, Sdraw, MS computed only when asked for)
 *   [lik, MS, Pcov] = nagp_mex('slowfb', A, Q, H, P0, block, y, vary, filter_only, cov, sub_idx [,device])       nagp_slowfb_run
 *                                    y, vary T x n_series; cov 0: none, 1: Pcov = marginal variances S x T x n_series, 2: Pcov =
 *                                    P(sub_idx, sub_idx, k), n_sub x n_sub x T x n_series (sub_idx int32, 0-based, ascending; [] unless cov = 2);
 *                                    lik n_series x 1, MS S x T x n_series
 *   [W, H, Obj] = nagp_mex('nmf_fp', A, vary, W0, H0, n_its, update_w [,device])                               nagp_nmf_fp
 *                                    A T x D; vary T x D or [] (= zeros); W0 K x D x P, H0 T x K x P (P problems on the same A); W, H as
 *                                    W0, H0; Obj ((update_w ? 2 : 1) * n_its) x P
 *   [Obj, dObj] = nagp_mex('pstft_obj', kernel, form, theta, vary, specTar, minVar, limOm, limLam, bet [,device])  nagp_pstft_obj
 *                                    kernel 'exp' | 'matern32' | 'matern52' | 'matern72'; form 0 (get_Obj_pSTFT_<kernel>.m) or 1
 *                                    (get_Obj_pSTFT_all.m); theta 3D x P; specTar N x 1 (shared) or N x P; vary, bet scalars or P entries;
 *                                    minVar D x 1, limOm, limLam D x 2; Obj P x 1, dObj 3D x P (formed only with two outputs)
 *   [Obj, dObj] = nagp_mex('segp_obj', param, specy, vary, varx [,device])                                     nagp_segp_obj
 *                                    param n_param x P (n_param = 1, 2, 3: log len [, log varx [, log vary]]); specy T x 1 (shared) or T x P;
 *                                    vary (read when n_param <= 2), varx (read when n_param = 1): scalars or P entries, [] where not read;
 *                                    Obj P x 1, dObj n_param x P (formed only with two outputs)
 *   [Obj, dObj] = nagp_mex('gppad_obj', x, y, fftCov, varx, mux, varc, vary [,device])                         nagp_gppad_obj
 *                                    x Tx x P; y T x P; fftCov Tx x 1 (shared) or Tx x P; varx, mux, varc: scalars or P entries;
 *                                    vary a scalar, T x 1 (the same for every problem) or T x P; Obj P x 1, dObj Tx x P (formed only with two outputs)
 *   [Obj, dObj] = nagp_mex('gppad_cas_obj', x, y, fftCovs, varx, mux, varc [,device])                          nagp_gppad_cas_obj
 *                                    x (M Tx) x P, a column the X(:) of one cascade; y T x P; fftCovs Tx x M (shared) or Tx x M x P; varx, mux:
 *                                    M entries or M x P; varc a scalar or P entries; Obj P x 1, dObj (M Tx) x P (formed only with two outputs)
 *   [Obj, dObj] = nagp_mex('nmf_temp_obj', x, A, vary, W, muinf, varinf, lam [,device])                        nagp_nmf_temp_obj
 *                                    A T x D; vary T x D or [] (zeros); W [] -- the learning form, x (T K + K D) x P -- or K x D (shared) or
 *                                    K x D x P -- the inference form, x (T K) x P; muinf, varinf, lam: K entries or []: varinf empty = no prior,
 *                                    muinf empty = the truncated-Gaussian chain, none empty = the inverse-gamma chain (nmf.m:119-131);
 *                                    Obj P x 1, dObj as x (formed only with two outputs)
 *   [Obj, dObj] = nagp_mex('tnmf_obj', x, A, vary, W, lenx, mux, varx, tol [,device])                          nagp_tnmf_obj
 *                                    A T x D; vary T x D or [] (zeros); W [] -- the learning form, x (T K + K D) x P -- or K x D (shared) or
 *                                    K x D x P -- the inference form, x (T K) x P; lenx, mux, varx: K entries; tol a scalar;
 *                                    Obj P x 1, dObj as x (formed only with two outputs)
 *   [Obj, dObj] = nagp_mex('sebf_fit_obj', z, x, lenx, varx, tol [,device])                                    nagp_sebf_fit_obj
 *                                    z and the targets x T x P; lenx, varx: scalars or P entries; Obj P x 1, dObj T x P (with two outputs)
 *   Y = nagp_mex('sebf_conv', Z, lenx, varx, tol [,device])                                                    nagp_sebf_conv
 *                                    Z T x K; lenx, varx: scalars or K entries; Y T x K
 *   [Esig,Vsig,Eft_mod,Varft_mod] = nagp_mex('reconstruct', Eft, Varft, Wnmf, link_kind, link_shift, gh_x, gh_w, n_samples, seed [,device])
 *                                                                                                              nagp_reconstruct
 *   [Esig,Vsig,Esrc,Vsrc,Eenv,Eft_mod,Varft_mod] = nagp_mex('reconstruct_sources', Eft, Varft, Wnmf, ropts)    nagp_reconstruct_sources
 *                                    ropts struct: amp_kind, link_kind, link_shift, source_offsets (int32, 0-based, J+1 entries; [] = one source),
 *                                    n_samples, seed, gh_x, gh_w, wn, xn_unscaled, device                      -> nagp_recon_opts
 *   [nlZ_total, Eft, Varft, nlZ] = nagp_mex('batch', models {cell of model structs}, ys {cell}, opts, n_gpus [, tables {cell}])
 *                                    Eft, Varft, nlZ: cells, one entry per problem                             nagp_batch_run
 *   [e, g] = nagp_mex('giekf_grad', model, y, dA, dQ, dPinf, dR, hess, w_index, w_direct [,device])            nagp_giekf_nlml_grad
 *
 * The kernels replace the loops of matlab/gf_ep_modulator_nmf.m:113-283 / :384-522 (and the other functions listed in
 * include/nagp.h); everything before those loops stays in the .m wrappers.
 */
#include <stdlib.h>
#include <string.h>

#include "mex.h"
#include "nagp.h"

static const mxArray* field(const mxArray* s, const char* name, int required) {
  const mxArray* f = mxIsStruct(s) ? mxGetField(s, 0, name) : NULL;
  if (!f && required) mexErrMsgIdAndTxt("nagp:arg", "missing field '%s'", name);
  return f;
}
static double scalar_or(const mxArray* s, const char* name, double dflt) {
  const mxArray* f = field(s, name, 0);
  return (f && !mxIsEmpty(f)) ? mxGetScalar(f) : dflt;
}
static const double* doubles(const mxArray* s, const char* name, int required, size_t* n) {
  const mxArray* f = field(s, name, required);
  if (n) *n = 0;
  if (!f || mxIsEmpty(f)) return NULL;
  if (!mxIsDouble(f) || mxIsComplex(f)) mexErrMsgIdAndTxt("nagp:arg", "field '%s' must be real double", name);
  if (n) *n = mxGetNumberOfElements(f);
  return mxGetPr(f);
}

static const double* dvec(const mxArray* a, const char* what, size_t* n) {
  if (n) *n = 0;
  if (!a || mxIsEmpty(a)) return NULL;
  if (!mxIsDouble(a) || mxIsComplex(a)) mexErrMsgIdAndTxt("nagp:arg", "%s must be real double", what);
  if (n) *n = mxGetNumberOfElements(a);
  return mxGetPr(a);
}
static void fail_if(int st) {
  if (st != NAGP_OK) mexErrMsgIdAndTxt("nagp:fail", "%s (%d): %s", nagp_strerror(st), st, nagp_last_error());
}

static void read_model(const mxArray* sm, nagp_model* m) {
  const mxArray* f; size_t n;
  memset(m, 0, sizeof *m);
  f = field(sm, "A", 1);
  m->S = (int32_t)mxGetM(f);
  m->A = doubles(sm, "A", 1, &n);
  if (n != (size_t)m->S * m->S) mexErrMsgIdAndTxt("nagp:arg", "A must be S x S");
  m->Q = doubles(sm, "Q", 1, &n);
  if (n != (size_t)m->S * m->S) mexErrMsgIdAndTxt("nagp:arg", "Q must be S x S");
  m->Pinf = doubles(sm, "Pinf", 1, &n);
  if (n != (size_t)m->S * m->S) mexErrMsgIdAndTxt("nagp:arg", "Pinf must be S x S");
  m->h_val = doubles(sm, "h_val", 1, &n);
  m->M = (int32_t)n;
  f = field(sm, "block_offsets", 1);
  if (!mxIsInt32(f) || mxGetNumberOfElements(f) != (size_t)m->M + 1) mexErrMsgIdAndTxt("nagp:arg", "block_offsets must be int32 with M+1 entries");
  m->block_offsets = (const int32_t*)mxGetData(f);
  m->Wnmf = doubles(sm, "Wnmf", 0, &n);
  m->D = (int32_t)scalar_or(sm, "D", 0);
  m->N = (int32_t)scalar_or(sm, "N", 0);
  if (m->Wnmf && n != (size_t)m->D * m->N) mexErrMsgIdAndTxt("nagp:arg", "Wnmf must be D x N");
  m->lik_param = scalar_or(sm, "lik_param", 0);
}

static void read_opts(const mxArray* so, nagp_opts* o, int M, size_t T) {
  size_t n, nd;
  memset(o, 0, sizeof *o);
  o->kind = (int32_t)scalar_or(so, "kind", NAGP_KIND_GF_EP);
  o->mode = (int32_t)scalar_or(so, "mode", NAGP_MODE_PREDICT);
  o->lik_kind = (int32_t)scalar_or(so, "lik_kind", NAGP_LIK_POWER_NMF);
  o->link_kind = (int32_t)scalar_or(so, "link_kind", NAGP_LINK_SOFTPLUS);
  o->link_shift = scalar_or(so, "link_shift", 0.0);
  o->wn = doubles(so, "wn", 0, &n);
  o->n_pts = (int32_t)n;
  o->xn_unscaled = doubles(so, "xn_unscaled", 0, &nd);
  if (o->wn) {
    if (!o->xn_unscaled || nd % n) mexErrMsgIdAndTxt("nagp:arg", "xn_unscaled must be cub_dim x n_pts");
    o->cub_dim = (int32_t)(nd / n);
  }
  o->ep_fraction = scalar_or(so, "ep_fraction", 0.5);
  o->ep_damping = doubles(so, "ep_damping", 0, &n);
  o->ep_itts = (int32_t)scalar_or(so, "ep_itts", (double)n);
  if (o->ep_damping && (size_t)o->ep_itts > n) mexErrMsgIdAndTxt("nagp:arg", "ep_damping has fewer than ep_itts entries");
  o->l_iter = (int32_t)scalar_or(so, "l_iter", 0);
  o->predict_at_k1 = (int32_t)scalar_or(so, "predict_at_k1", 0);
  o->flags = (uint32_t)scalar_or(so, "flags", 0);
  o->device = (int32_t)scalar_or(so, "device", 0);
  o->chunk = (int32_t)scalar_or(so, "chunk", 0);
  o->ttau0 = doubles(so, "ttau0", 0, &n);
  if (o->ttau0 && n != (size_t)M * T) mexErrMsgIdAndTxt("nagp:arg", "ttau0 must be M x T");
  o->tnu0 = doubles(so, "tnu0", 0, &n);
  if (o->tnu0 && n != (size_t)M * T) mexErrMsgIdAndTxt("nagp:arg", "tnu0 must be M x T");
  if (o->ep_itts < 1) mexErrMsgIdAndTxt("nagp:arg", "ep_itts < 1");
}

static void read_tables(const mxArray* stb, nagp_ihgp_tables* tb, int M) {
  const mxArray* f; size_t n;
  memset(tb, 0, sizeof *tb);
  tb->r_grid = doubles(stb, "r", 1, &n);
  tb->n_grid = (int32_t)n;
  tb->PPlist = doubles(stb, "PP", 1, NULL);
  tb->PGlist = doubles(stb, "PG", 1, NULL);
  f = field(stb, "pp_off", 1);
  if (!mxIsInt64(f) || mxGetNumberOfElements(f) != (size_t)M) mexErrMsgIdAndTxt("nagp:arg", "pp_off must be int64 with M entries");
  tb->pp_offsets = (const int64_t*)mxGetData(f);
  f = field(stb, "pg_off", 1);
  if (!mxIsInt64(f) || mxGetNumberOfElements(f) != (size_t)M) mexErrMsgIdAndTxt("nagp:arg", "pg_off must be int64 with M entries");
  tb->pg_offsets = (const int64_t*)mxGetData(f);
}

/* ---- the command forms (first argument a string) */
static void cmd_giekf_grad(int nlhs, mxArray* plhs[], int nrhs, const mxArray* prhs[]) {
  /* ('giekf_grad', model, y, dA, dQ, dPinf (S x S x n_param each), dR, hess, w_index, w_direct (int32, n_param each) [,device]) -> [e, g]
     the EKF energy with its gradient recursion, gf_giekf_modulator_nmf_constraints.m:332-480 with GradObj = 'on' */
  nagp_model m; size_t T, n, np_; const double *y, *dA, *dQ, *dP, *dR; const double* ys[1]; const double* a1[1]; const double* a2[1]; const double* a3[1];
  double e = 0; int32_t dev;
  if (nrhs < 10 || nrhs > 11) mexErrMsgIdAndTxt("nagp:arg", "usage: [e,g] = nagp_mex('giekf_grad',model,y,dA,dQ,dPinf,dR,hess,w_index,w_direct[,device])");
  read_model(prhs[1], &m);
  y = dvec(prhs[2], "y", &T);
  dR = dvec(prhs[6], "dR", &np_);
  dA = dvec(prhs[3], "dA", &n); if (n != (size_t)m.S * m.S * np_) mexErrMsgIdAndTxt("nagp:arg", "dA must be S x S x numel(dR)");
  dQ = dvec(prhs[4], "dQ", &n); if (n != (size_t)m.S * m.S * np_) mexErrMsgIdAndTxt("nagp:arg", "dQ must be S x S x numel(dR)");
  dP = dvec(prhs[5], "dPinf", &n); if (n != (size_t)m.S * m.S * np_) mexErrMsgIdAndTxt("nagp:arg", "dPinf must be S x S x numel(dR)");
  if (!mxIsInt32(prhs[7]) || !mxIsInt32(prhs[8]) || !mxIsInt32(prhs[9]) || mxGetNumberOfElements(prhs[7]) != np_ ||
      mxGetNumberOfElements(prhs[8]) != np_ || mxGetNumberOfElements(prhs[9]) != np_) mexErrMsgIdAndTxt("nagp:arg", "hess, w_index, w_direct must be int32 with numel(dR) entries");
  dev = nrhs > 10 ? (int32_t)mxGetScalar(prhs[10]) : 0;
  plhs[0] = mxCreateDoubleMatrix(1, 1, mxREAL);
  { mxArray* g = mxCreateDoubleMatrix(1, np_, mxREAL);
    ys[0] = y; a1[0] = dA; a2[0] = dQ; a3[0] = dP;
    fail_if(nagp_giekf_nlml_grad(1, &m, ys, (int64_t)T, (int32_t)np_, a1, a2, a3, dR, (const int32_t*)mxGetData(prhs[7]), (const int32_t*)mxGetData(prhs[8]),
                                 (const int32_t*)mxGetData(prhs[9]), &e, mxGetPr(g), dev));
    mxGetPr(plhs[0])[0] = e;
    if (nlhs > 1) plhs[1] = g; }
}

static void cmd_iekf_update1(int nlhs, mxArray* plhs[], int nrhs, const mxArray* prhs[]) {
  /* ('iekf_update1', M, P, y, h_col, h_val, Wnmf, R, iters [,device]) -> [M,P,K,MU,S]  (iekf_update1.m:48, :110-117) */
  size_t S, n, nm; int32_t D, N, iters, dev; const double *m0, *P0, *hv, *W; double *m, *P, *K, MU = 0, Sx = 0;
  if (nrhs < 9 || nrhs > 10) mexErrMsgIdAndTxt("nagp:arg", "usage: [M,P,K,MU,S] = nagp_mex('iekf_update1',M,P,y,h_col,h_val,Wnmf,R,iters[,device])");
  m0 = dvec(prhs[1], "M", &S); P0 = dvec(prhs[2], "P", &n);
  if (!m0 || n != S * S) mexErrMsgIdAndTxt("nagp:arg", "P must be S x S for M of S entries");
  hv = dvec(prhs[5], "h_val", &nm);
  if (!mxIsInt32(prhs[4]) || mxGetNumberOfElements(prhs[4]) != nm) mexErrMsgIdAndTxt("nagp:arg", "h_col must be int32 with as many entries as h_val");
  W = dvec(prhs[6], "Wnmf", &n);
  D = (int32_t)mxGetM(prhs[6]); N = D ? (int32_t)(n / (size_t)D) : 0;
  if ((size_t)(D + N) != nm) mexErrMsgIdAndTxt("nagp:arg", "Wnmf must be D x N with D + N = numel(h_val)");
  iters = (int32_t)mxGetScalar(prhs[8]); dev = nrhs > 9 ? (int32_t)mxGetScalar(prhs[9]) : 0;
  plhs[0] = mxCreateDoubleMatrix(S, 1, mxREAL); m = mxGetPr(plhs[0]); memcpy(m, m0, S * sizeof(double));
  { mxArray* Pa = mxCreateDoubleMatrix(S, S, mxREAL); mxArray* Ka = mxCreateDoubleMatrix(S, 1, mxREAL);
    P = mxGetPr(Pa); memcpy(P, P0, S * S * sizeof(double)); K = mxGetPr(Ka);
    fail_if(nagp_iekf_update1((int32_t)S, D, N, (const int32_t*)mxGetData(prhs[4]), hv, W, mxGetScalar(prhs[7]), mxGetScalar(prhs[3]), iters, m, P, K, &MU, &Sx, dev));
    if (nlhs > 1) plhs[1] = Pa;
    if (nlhs > 2) plhs[2] = Ka; }
  if (nlhs > 3) { plhs[3] = mxCreateDoubleMatrix(1, 1, mxREAL); mxGetPr(plhs[3])[0] = MU; }
  if (nlhs > 4) { plhs[4] = mxCreateDoubleMatrix(1, 1, mxREAL); mxGetPr(plhs[4])[0] = Sx; }
}

static void cmd_fastfb(int nlhs, mxArray* plhs[], int nrhs, const mxArray* prhs[]) {
  /* ('fastfb', A, AKHA, HA, K, G, y [,device]) -> [MS, sum_v2]  (kernel_ss_kalmanFastFB.m:83-110, :134-151) */
  size_t n, S, T; const double *A, *AK, *HA, *K, *G, *y; double sv2 = 0; int32_t dev;
  if (nrhs < 7 || nrhs > 8) mexErrMsgIdAndTxt("nagp:arg", "usage: [MS,sum_v2] = nagp_mex('fastfb',A,AKHA,HA,K,G,y[,device])");
  A = dvec(prhs[1], "A", &n); S = mxGetM(prhs[1]);
  if (!A || n != S * S) mexErrMsgIdAndTxt("nagp:arg", "A must be S x S");
  AK = dvec(prhs[2], "AKHA", &n); if (n != S * S) mexErrMsgIdAndTxt("nagp:arg", "AKHA must be S x S");
  HA = dvec(prhs[3], "HA", &n); if (n != S) mexErrMsgIdAndTxt("nagp:arg", "HA must have S entries");
  K = dvec(prhs[4], "K", &n); if (n != S) mexErrMsgIdAndTxt("nagp:arg", "K must have S entries");
  G = dvec(prhs[5], "G", &n); if (G && n != S * S) mexErrMsgIdAndTxt("nagp:arg", "G must be S x S or []");
  y = dvec(prhs[6], "y", &T); dev = nrhs > 7 ? (int32_t)mxGetScalar(prhs[7]) : 0;
  plhs[0] = mxCreateDoubleMatrix(S, T, mxREAL);
  fail_if(nagp_fastfb_run((int32_t)S, A, AK, HA, K, G, y, (int64_t)T, mxGetPr(plhs[0]), &sv2, dev));
  if (nlhs > 1) { plhs[1] = mxCreateDoubleMatrix(1, 1, mxREAL); mxGetPr(plhs[1])[0] = sv2; }
}

static void cmd_fastfb_sample(int nlhs, mxArray* plhs[], int nrhs, const mxArray* prhs[]) {
  /* ('fastfb_sample', A, AKHA, HA, K, G, H, R, Lp, Lq, y, n_draws, seed [,device]) -> [Ydraw, Xdraw, MS]: joint posterior draws of the
     stationary filterbank by the simulation smoother; states and the smoother mean only when asked for */
  size_t n, S, T; const double *A, *AK, *HA, *K, *G, *H, *Lp, *Lq, *y; int32_t dev, nd; mwSize dims3[3];
  if (nrhs < 13 || nrhs > 14 || nlhs > 3) mexErrMsgIdAndTxt("nagp:arg", "usage: [Ydraw,Xdraw,MS] = nagp_mex('fastfb_sample',A,AKHA,HA,K,G,H,R,Lp,Lq,y,n_draws,seed[,device])");
  A = dvec(prhs[1], "A", &n); S = mxGetM(prhs[1]);
  if (!A || n != S * S) mexErrMsgIdAndTxt("nagp:arg", "A must be S x S");
  AK = dvec(prhs[2], "AKHA", &n); if (n != S * S) mexErrMsgIdAndTxt("nagp:arg", "AKHA must be S x S");
  HA = dvec(prhs[3], "HA", &n); if (n != S) mexErrMsgIdAndTxt("nagp:arg", "HA must have S entries");
  K = dvec(prhs[4], "K", &n); if (n != S) mexErrMsgIdAndTxt("nagp:arg", "K must have S entries");
  G = dvec(prhs[5], "G", &n); if (n != S * S) mexErrMsgIdAndTxt("nagp:arg", "G must be S x S");
  H = dvec(prhs[6], "H", &n); if (n != S) mexErrMsgIdAndTxt("nagp:arg", "H must have S entries");
  Lp = dvec(prhs[8], "Lp", &n); if (n != S * S) mexErrMsgIdAndTxt("nagp:arg", "Lp must be S x S");
  Lq = dvec(prhs[9], "Lq", &n); if (n != S * S) mexErrMsgIdAndTxt("nagp:arg", "Lq must be S x S");
  y = dvec(prhs[10], "y", &T);
  nd = (int32_t)mxGetScalar(prhs[11]);
  if (!y || nd < 1) mexErrMsgIdAndTxt("nagp:arg", "y must not be empty and n_draws must be at least 1");
  dev = nrhs > 13 ? (int32_t)mxGetScalar(prhs[13]) : 0;
  plhs[0] = mxCreateDoubleMatrix(T, (mwSize)nd, mxREAL);
  if (nlhs > 1) { dims3[0] = S; dims3[1] = T; dims3[2] = (mwSize)nd; plhs[1] = mxCreateNumericArray(3, dims3, mxDOUBLE_CLASS, mxREAL); }
  if (nlhs > 2) plhs[2] = mxCreateDoubleMatrix(S, T, mxREAL);
  fail_if(nagp_fastfb_sample((int32_t)S, A, AK, HA, K, G, H, mxGetScalar(prhs[7]), Lp, Lq, y, (int64_t)T, nd, (uint64_t)mxGetScalar(prhs[12]),
                             mxGetPr(plhs[0]), nlhs > 1 ? mxGetPr(plhs[1]) : NULL, nlhs > 2 ? mxGetPr(plhs[2]) : NULL, dev));
}

static void cmd_ep_sample(int nlhs, mxArray* plhs[], int nrhs, const mxArray* prhs[]) {
  /* ('ep_sample', model, ttau, tnu, y, predict_at_k1, n_draws, seed, z, sig [,device]) -> [Fdraw, Xdraw, Sdraw, MS, counters]: joint posterior
     draws of a full-covariance EP run by forward filtering with its sites and backward sampling; states, signal and means only when asked for */
  nagp_model m; nagp_epsample_sig sg; const nagp_epsample_sig* psg = NULL;
  size_t n, T; const double *tt, *tn, *y, *z; int32_t dev, nd; int64_t cnt[2] = {0, 0}; mwSize d3[3]; int want_s;
  if (nrhs < 10 || nrhs > 11 || nlhs > 5) mexErrMsgIdAndTxt("nagp:arg", "usage: [Fdraw,Xdraw,Sdraw,MS,counters] = nagp_mex('ep_sample',model,ttau,tnu,y,predict_at_k1,n_draws,seed,z,sig[,device])");
  read_model(prhs[1], &m);
  y = dvec(prhs[4], "y", &T);
  nd = (int32_t)mxGetScalar(prhs[6]);
  if (!y || nd < 1) mexErrMsgIdAndTxt("nagp:arg", "y must not be empty and n_draws must be at least 1");
  tt = dvec(prhs[2], "ttau", &n); if (n != (size_t)m.M * T) mexErrMsgIdAndTxt("nagp:arg", "ttau must be M x T");
  tn = dvec(prhs[3], "tnu", &n); if (n != (size_t)m.M * T) mexErrMsgIdAndTxt("nagp:arg", "tnu must be M x T");
  z = dvec(prhs[8], "z", &n); if (z && n != (size_t)m.S * T * (size_t)nd) mexErrMsgIdAndTxt("nagp:arg", "z must be S x T x n_draws or []");
  if (!mxIsEmpty(prhs[9])) {
    sg.Wnmf = doubles(prhs[9], "Wnmf", 1, &n);
    if (n != (size_t)m.D * m.N) mexErrMsgIdAndTxt("nagp:arg", "sig.Wnmf must be D x N");
    sg.amp_kind = (int32_t)scalar_or(prhs[9], "amp_kind", 0); sg.link_kind = (int32_t)scalar_or(prhs[9], "link_kind", 0);
    sg.link_shift = scalar_or(prhs[9], "link_shift", 0);
    psg = &sg;
  }
  dev = nrhs > 10 ? (int32_t)mxGetScalar(prhs[10]) : 0;
  want_s = nlhs > 2 && psg;
  d3[0] = (mwSize)m.M; d3[1] = T; d3[2] = (mwSize)nd; plhs[0] = mxCreateNumericArray(3, d3, mxDOUBLE_CLASS, mxREAL);
  if (nlhs > 1) { d3[0] = (mwSize)m.S; plhs[1] = mxCreateNumericArray(3, d3, mxDOUBLE_CLASS, mxREAL); }
  if (nlhs > 2) plhs[2] = want_s ? mxCreateDoubleMatrix(T, (mwSize)nd, mxREAL) : mxCreateDoubleMatrix(0, 0, mxREAL);
  if (nlhs > 3) plhs[3] = mxCreateDoubleMatrix((mwSize)m.S, T, mxREAL);
  if (nlhs > 4) plhs[4] = mxCreateDoubleMatrix(2, 1, mxREAL);
  fail_if(nagp_ep_sample(&m, tt, tn, y, (int64_t)T, (int32_t)mxGetScalar(prhs[5]), nd, (uint64_t)mxGetScalar(prhs[7]), z, psg, nlhs > 1 ? mxGetPr(plhs[1]) : NULL,
                         mxGetPr(plhs[0]), want_s ? mxGetPr(plhs[2]) : NULL, nlhs > 3 ? mxGetPr(plhs[3]) : NULL, cnt, dev));
  if (nlhs > 4) { mxGetPr(plhs[4])[0] = (double)cnt[0]; mxGetPr(plhs[4])[1] = (double)cnt[1]; }
}

static void cmd_slowfb(int nlhs, mxArray* plhs[], int nrhs, const mxArray* prhs[]) {
  /* ('slowfb', A, Q, H, P0, block, y, vary, filter_only, cov, sub_idx [,device]) -> [lik, MS, Pcov]: the exact filterbank filter / smoother with
     an observation variance per step (kernel_ss_kalmanSlowFB_rewrite.m:55-84, :100-134); means and covariances only when asked for */
  size_t n, S, T, ns, nv, nsub = 0; const double *A, *Q, *H, *P0, *y, *vary; const int32_t* sub = NULL; int32_t dev, cov; mwSize d[4];
  double *MS = NULL, *Pd = NULL, *Ps = NULL;
  if (nrhs < 11 || nrhs > 12 || nlhs > 3) mexErrMsgIdAndTxt("nagp:arg", "usage: [lik,MS,Pcov] = nagp_mex('slowfb',A,Q,H,P0,block,y,vary,filter_only,cov,sub_idx[,device])");
  A = dvec(prhs[1], "A", &n); S = mxGetM(prhs[1]);
  if (!A || n != S * S) mexErrMsgIdAndTxt("nagp:arg", "A must be S x S");
  Q = dvec(prhs[2], "Q", &n); if (n != S * S) mexErrMsgIdAndTxt("nagp:arg", "Q must be S x S");
  H = dvec(prhs[3], "H", &n); if (n != S) mexErrMsgIdAndTxt("nagp:arg", "H must have S entries");
  P0 = dvec(prhs[4], "P0", &n); if (n != S * S) mexErrMsgIdAndTxt("nagp:arg", "P0 must be S x S");
  y = dvec(prhs[6], "y", &n); T = mxGetM(prhs[6]);
  if (!y || !T) mexErrMsgIdAndTxt("nagp:arg", "y must not be empty (T x n_series)");
  ns = n / T;
  vary = dvec(prhs[7], "vary", &nv);
  if (nv != n || mxGetM(prhs[7]) != T) mexErrMsgIdAndTxt("nagp:arg", "vary must have the size of y (T x n_series)");
  cov = (int32_t)mxGetScalar(prhs[9]);
  if (cov < 0 || cov > 2) mexErrMsgIdAndTxt("nagp:arg", "cov must be 0 (none), 1 (marginal variances) or 2 (sub_idx)");
  if (cov == 2) {
    if (!mxIsInt32(prhs[10]) || mxIsEmpty(prhs[10])) mexErrMsgIdAndTxt("nagp:arg", "sub_idx must be int32 (0-based) and not empty with cov = 2");
    sub = (const int32_t*)mxGetData(prhs[10]); nsub = mxGetNumberOfElements(prhs[10]);
  }
  dev = nrhs > 11 ? (int32_t)mxGetScalar(prhs[11]) : 0;
  plhs[0] = mxCreateDoubleMatrix((mwSize)ns, 1, mxREAL);
  if (nlhs > 1) { d[0] = S; d[1] = T; d[2] = (mwSize)ns; plhs[1] = mxCreateNumericArray(3, d, mxDOUBLE_CLASS, mxREAL); MS = mxGetPr(plhs[1]); }
  if (nlhs > 2 && cov == 1) { d[0] = S; d[1] = T; d[2] = (mwSize)ns; plhs[2] = mxCreateNumericArray(3, d, mxDOUBLE_CLASS, mxREAL); Pd = mxGetPr(plhs[2]); }
  if (nlhs > 2 && cov == 2) { d[0] = nsub; d[1] = nsub; d[2] = T; d[3] = (mwSize)ns; plhs[2] = mxCreateNumericArray(4, d, mxDOUBLE_CLASS, mxREAL); Ps = mxGetPr(plhs[2]); }
  if (nlhs > 2 && cov == 0) plhs[2] = mxCreateDoubleMatrix(0, 0, mxREAL);
  fail_if(nagp_slowfb_run((int32_t)S, (int32_t)mxGetScalar(prhs[5]), A, Q, H, P0, (int32_t)ns, y, vary, (int64_t)T, mxGetScalar(prhs[8]) != 0.0,
                          Ps ? (int32_t)nsub : 0, Ps ? sub : NULL, mxGetPr(plhs[0]), MS, Pd, Ps, dev));
}

static void cmd_nmf_fp(int nlhs, mxArray* plhs[], int nrhs, const mxArray* prhs[]) {
  /* ('nmf_fp', A, vary, W0, H0, n_its, update_w [,device]) -> [W, H, Obj]: the fixed-point NMF of experiments/nmf/nmf_fp.m:65-87 (update_w ~= 0)
     or nmf_inf_fp.m:42-55 (update_w = 0) on P problems that share A and vary; W0 is used as given (the wrappers normalise it) */
  size_t n, nv, nw, nh, T, D, K, P; const double *A, *vary, *W0, *H0; int32_t dev, n_its, uw; mwSize d[3]; mxArray* o[3]; int i;
  if (nrhs < 7 || nrhs > 8 || nlhs > 3) mexErrMsgIdAndTxt("nagp:arg", "usage: [W,H,Obj] = nagp_mex('nmf_fp',A,vary,W0,H0,n_its,update_w[,device])");
  A = dvec(prhs[1], "A", &n); T = mxGetM(prhs[1]);
  if (!A || !T) mexErrMsgIdAndTxt("nagp:arg", "A must not be empty (T x D)");
  D = n / T;
  vary = dvec(prhs[2], "vary", &nv);
  if (vary && (nv != n || mxGetM(prhs[2]) != T)) mexErrMsgIdAndTxt("nagp:arg", "vary must have the size of A (T x D) or be []");
  W0 = dvec(prhs[3], "W0", &nw); K = mxGetM(prhs[3]);
  if (!W0 || !K || nw % (K * D) != 0) mexErrMsgIdAndTxt("nagp:arg", "W0 must be K x D x P with the D of A");
  P = nw / (K * D);
  H0 = dvec(prhs[4], "H0", &nh);
  if (!H0 || mxGetM(prhs[4]) != T || nh != T * K * P) mexErrMsgIdAndTxt("nagp:arg", "H0 must be T x K x P with the T of A and the K, P of W0");
  n_its = (int32_t)mxGetScalar(prhs[5]); uw = mxGetScalar(prhs[6]) != 0.0;
  if (n_its < 0) mexErrMsgIdAndTxt("nagp:arg", "n_its must be >= 0");
  dev = nrhs > 7 ? (int32_t)mxGetScalar(prhs[7]) : 0;
  d[0] = K; d[1] = D; d[2] = P; o[0] = mxCreateNumericArray(3, d, mxDOUBLE_CLASS, mxREAL);
  d[0] = T; d[1] = K; d[2] = P; o[1] = mxCreateNumericArray(3, d, mxDOUBLE_CLASS, mxREAL);
  o[2] = mxCreateDoubleMatrix((mwSize)((uw ? 2 : 1) * (size_t)n_its), (mwSize)P, mxREAL);
  fail_if(nagp_nmf_fp((int32_t)P, (int64_t)T, (int32_t)D, (int32_t)K, A, vary, W0, H0, n_its, uw, mxGetPr(o[0]), mxGetPr(o[1]),
                      n_its ? mxGetPr(o[2]) : NULL, dev));
  for (i = 0; i < (nlhs > 1 ? nlhs : 1); ++i) plhs[i] = o[i];
}

static void cmd_pstft_obj(int nlhs, mxArray* plhs[], int nrhs, const mxArray* prhs[]) {
  /* ('pstft_obj', kernel, form, theta, vary, specTar, minVar, limOm, limLam, bet [,device]) -> [Obj, dObj]: the objective of
     unifying_prob_tf/get_Obj_pSTFT_<kernel>.m (form 0) / get_Obj_pSTFT_all.m (form 1) for P problems; dObj only when asked for */
  static const char* names[4] = {"exp", "matern32", "matern52", "matern72"};
  char kn[16]; size_t nt, nv, ns, nm, no, nl, nb, D, P, N, q; const double *theta, *vary, *spec, *minVar, *limOm, *limLam, *bet;
  double *vy, *bt; int32_t dev, form, kernel = -1; int i; mxArray* o[2] = {NULL, NULL};
  if (nrhs < 10 || nrhs > 11 || nlhs > 2) mexErrMsgIdAndTxt("nagp:arg", "usage: [Obj,dObj] = nagp_mex('pstft_obj',kernel,form,theta,vary,specTar,minVar,limOm,limLam,bet[,device])");
  if (!mxIsChar(prhs[1]) || mxGetString(prhs[1], kn, sizeof kn)) mexErrMsgIdAndTxt("nagp:arg", "kernel must be a string");
  for (i = 0; i < 4; ++i) if (!strcmp(kn, names[i])) kernel = i;
  if (kernel < 0) mexErrMsgIdAndTxt("nagp:arg", "kernel '%s': exp, matern32, matern52 and matern72 are served", kn);
  form = (int32_t)mxGetScalar(prhs[2]);
  theta = dvec(prhs[3], "theta", &nt);
  minVar = dvec(prhs[6], "minVar", &nm); D = nm;
  if (!theta || !minVar || !D || nt % (3 * D) != 0 || mxGetM(prhs[3]) != 3 * D) mexErrMsgIdAndTxt("nagp:arg", "theta must be 3D x P with the D of minVar");
  P = nt / (3 * D);
  spec = dvec(prhs[5], "specTar", &ns);
  N = (spec && mxGetN(prhs[5]) == 1 && mxGetM(prhs[5]) == ns) ? ns : (spec ? mxGetM(prhs[5]) : 0);
  if (!N || (ns != N && ns != N * P)) mexErrMsgIdAndTxt("nagp:arg", "specTar must be N x 1 or N x P");
  limOm = dvec(prhs[7], "limOm", &no); limLam = dvec(prhs[8], "limLam", &nl);
  if (!limOm || !limLam || no != 2 * D || nl != 2 * D || mxGetM(prhs[7]) != D || mxGetM(prhs[8]) != D) mexErrMsgIdAndTxt("nagp:arg", "limOm and limLam must be D x 2");
  vary = dvec(prhs[4], "vary", &nv); bet = dvec(prhs[9], "bet", &nb);
  if (!vary || !bet || (nv != 1 && nv != P) || (nb != 1 && nb != P)) mexErrMsgIdAndTxt("nagp:arg", "vary and bet must be scalars or hold P entries");
  dev = nrhs > 10 ? (int32_t)mxGetScalar(prhs[10]) : 0;
  vy = (double*)mxCalloc(P, sizeof *vy); bt = (double*)mxCalloc(P, sizeof *bt);
  for (q = 0; q < P; ++q) { vy[q] = vary[nv == 1 ? 0 : q]; bt[q] = bet[nb == 1 ? 0 : q]; }
  o[0] = mxCreateDoubleMatrix((mwSize)P, 1, mxREAL);
  if (nlhs > 1) o[1] = mxCreateDoubleMatrix((mwSize)(3 * D), (mwSize)P, mxREAL);
  fail_if(nagp_pstft_obj((int32_t)P, kernel, form, (int32_t)D, (int64_t)N, theta, spec, ns == N ? 0 : (int64_t)N, vy, bt, minVar, limOm, limLam,
                         mxGetPr(o[0]), o[1] ? mxGetPr(o[1]) : NULL, dev));
  mxFree(vy); mxFree(bt);
  for (i = 0; i < (nlhs > 1 ? nlhs : 1); ++i) plhs[i] = o[i];
}

static void cmd_segp_obj(int nlhs, mxArray* plhs[], int nrhs, const mxArray* prhs[]) {
  /* ('segp_obj', param, specy, vary, varx [,device]) -> [Obj, dObj]: the objective of experiments/toolsGP/getObjSEGP.m for P problems;
     vary / varx may be [] where n_param says they are not read; dObj only when asked for */
  size_t npar, ns, nv, nx, np, P, T, q; const double *param, *spec, *vary, *varx; double *vy = NULL, *vx = NULL; int32_t dev; int i;
  mxArray* o[2] = {NULL, NULL};
  if (nrhs < 5 || nrhs > 6 || nlhs > 2) mexErrMsgIdAndTxt("nagp:arg", "usage: [Obj,dObj] = nagp_mex('segp_obj',param,specy,vary,varx[,device])");
  param = dvec(prhs[1], "param", &npar); np = param ? mxGetM(prhs[1]) : 0;
  if (!param || np < 1 || np > 3 || npar % np != 0) mexErrMsgIdAndTxt("nagp:arg", "param must be n_param x P with n_param = 1, 2 or 3");
  P = npar / np;
  spec = dvec(prhs[2], "specy", &ns);
  T = (spec && mxGetN(prhs[2]) == 1 && mxGetM(prhs[2]) == ns) ? ns : (spec ? mxGetM(prhs[2]) : 0);
  if (!T || (ns != T && ns != T * P)) mexErrMsgIdAndTxt("nagp:arg", "specy must be T x 1 or T x P");
  vary = dvec(prhs[3], "vary", &nv); varx = dvec(prhs[4], "varx", &nx);
  if (np <= 2 && (!vary || (nv != 1 && nv != P))) mexErrMsgIdAndTxt("nagp:arg", "vary must be a scalar or hold P entries when param has %d rows", (int)np);
  if (np == 1 && (!varx || (nx != 1 && nx != P))) mexErrMsgIdAndTxt("nagp:arg", "varx must be a scalar or hold P entries when param has one row");
  dev = nrhs > 5 ? (int32_t)mxGetScalar(prhs[5]) : 0;
  if (np <= 2) { vy = (double*)mxCalloc(P, sizeof *vy); for (q = 0; q < P; ++q) vy[q] = vary[nv == 1 ? 0 : q]; }
  if (np == 1) { vx = (double*)mxCalloc(P, sizeof *vx); for (q = 0; q < P; ++q) vx[q] = varx[nx == 1 ? 0 : q]; }
  o[0] = mxCreateDoubleMatrix((mwSize)P, 1, mxREAL);
  if (nlhs > 1) o[1] = mxCreateDoubleMatrix((mwSize)np, (mwSize)P, mxREAL);
  fail_if(nagp_segp_obj((int32_t)P, (int32_t)np, (int64_t)T, param, spec, ns == T ? 0 : (int64_t)T, vy, vx,
                        mxGetPr(o[0]), o[1] ? mxGetPr(o[1]) : NULL, dev));
  if (vy) mxFree(vy);
  if (vx) mxFree(vx);
  for (i = 0; i < (nlhs > 1 ? nlhs : 1); ++i) plhs[i] = o[i];
}

static void cmd_gppad_obj(int nlhs, mxArray* plhs[], int nrhs, const mxArray* prhs[]) {
  /* ('gppad_obj', x, y, fftCov, varx, mux, varc, vary [,device]) -> [Obj, dObj]: the objective of gppad/GPModelFast/GetGPObjFast.m for P
     problems; dObj only when asked for */
  size_t nx, ny, nc, nv, n3[3], P, Tx, T, q, t; const double *x, *y, *cov, *vary, *par[3]; double *sc[3], *vy; int32_t dev; int i, k;
  mxArray* o[2] = {NULL, NULL};
  static const char* names[3] = {"varx", "mux", "varc"};
  if (nrhs < 8 || nrhs > 9 || nlhs > 2) mexErrMsgIdAndTxt("nagp:arg", "usage: [Obj,dObj] = nagp_mex('gppad_obj',x,y,fftCov,varx,mux,varc,vary[,device])");
  x = dvec(prhs[1], "x", &nx); Tx = x ? mxGetM(prhs[1]) : 0;
  if (!x || !Tx || nx % Tx != 0) mexErrMsgIdAndTxt("nagp:arg", "x must be Tx x P");
  P = nx / Tx;
  y = dvec(prhs[2], "y", &ny); T = y ? mxGetM(prhs[2]) : 0;
  if (!y || !T || ny != T * P) mexErrMsgIdAndTxt("nagp:arg", "y must be T x P");
  cov = dvec(prhs[3], "fftCov", &nc);
  if (!cov || (nc != Tx && nc != Tx * P)) mexErrMsgIdAndTxt("nagp:arg", "fftCov must be Tx x 1 or Tx x P");
  for (k = 0; k < 3; ++k) {
    par[k] = dvec(prhs[4 + k], names[k], &n3[k]);
    if (!par[k] || (n3[k] != 1 && n3[k] != P)) mexErrMsgIdAndTxt("nagp:arg", "%s must be a scalar or hold P entries", names[k]);
  }
  vary = dvec(prhs[7], "vary", &nv);
  if (!vary || (nv != 1 && nv != T && nv != T * P)) mexErrMsgIdAndTxt("nagp:arg", "vary must be a scalar, T x 1 or T x P");
  dev = nrhs > 8 ? (int32_t)mxGetScalar(prhs[8]) : 0;
  for (k = 0; k < 3; ++k) { sc[k] = (double*)mxCalloc(P, sizeof(double)); for (q = 0; q < P; ++q) sc[k][q] = par[k][n3[k] == 1 ? 0 : q]; }
  vy = (double*)mxCalloc(nv == 1 ? P : T * P, sizeof *vy);
  if (nv == 1) for (q = 0; q < P; ++q) vy[q] = vary[0];
  else for (q = 0; q < P; ++q) for (t = 0; t < T; ++t) vy[q * T + t] = vary[nv == T ? t : q * T + t];
  o[0] = mxCreateDoubleMatrix((mwSize)P, 1, mxREAL);
  if (nlhs > 1) o[1] = mxCreateDoubleMatrix((mwSize)Tx, (mwSize)P, mxREAL);
  fail_if(nagp_gppad_obj((int32_t)P, (int64_t)T, (int64_t)Tx, x, y, vy, nv == 1 ? 0 : (int64_t)T, NULL, cov, nc == Tx * P && P > 1 ? (int64_t)Tx : 0,
                         sc[0], sc[1], sc[2], mxGetPr(o[0]), o[1] ? mxGetPr(o[1]) : NULL, dev));
  for (k = 0; k < 3; ++k) mxFree(sc[k]);
  mxFree(vy);
  for (i = 0; i < (nlhs > 1 ? nlhs : 1); ++i) plhs[i] = o[i];
}

static void cmd_gppad_cas_obj(int nlhs, mxArray* plhs[], int nrhs, const mxArray* prhs[]) {
  /* ('gppad_cas_obj', x, y, fftCovs, varx, mux, varc [,device]) -> [Obj, dObj]: the objective of gppad/Cascade/GetObjCasGPFAST.m for P
     cascades of M modulators; dObj only when asked for */
  size_t nx, ny, nc, n3[3], P, M, MTx, Tx, T, q, m; const double *x, *y, *cov, *par[3]; double* sc[3]; int32_t dev; int i, k;
  mxArray* o[2] = {NULL, NULL};
  static const char* names[3] = {"varx", "mux", "varc"};
  if (nrhs < 7 || nrhs > 8 || nlhs > 2) mexErrMsgIdAndTxt("nagp:arg", "usage: [Obj,dObj] = nagp_mex('gppad_cas_obj',x,y,fftCovs,varx,mux,varc[,device])");
  x = dvec(prhs[1], "x", &nx); MTx = x ? mxGetM(prhs[1]) : 0;
  cov = dvec(prhs[3], "fftCovs", &nc); Tx = cov ? mxGetM(prhs[3]) : 0;
  if (!x || !MTx || nx % MTx != 0) mexErrMsgIdAndTxt("nagp:arg", "x must be (M Tx) x P");
  if (!cov || !Tx || MTx % Tx != 0) mexErrMsgIdAndTxt("nagp:arg", "fftCovs must be Tx x M or Tx x M x P, with the M Tx rows of x");
  P = nx / MTx; M = MTx / Tx;
  if (nc != MTx && nc != MTx * P) mexErrMsgIdAndTxt("nagp:arg", "fftCovs must be Tx x M or Tx x M x P, with the M Tx rows of x");
  y = dvec(prhs[2], "y", &ny); T = y ? mxGetM(prhs[2]) : 0;
  if (!y || !T || ny != T * P) mexErrMsgIdAndTxt("nagp:arg", "y must be T x P");
  for (k = 0; k < 3; ++k) {
    const size_t per = k < 2 ? M : 1;
    par[k] = dvec(prhs[4 + k], names[k], &n3[k]);
    if (!par[k] || (n3[k] != per && n3[k] != per * P)) mexErrMsgIdAndTxt("nagp:arg", k < 2 ? "%s must hold M entries or be M x P" : "%s must be a scalar or hold P entries", names[k]);
  }
  dev = nrhs > 7 ? (int32_t)mxGetScalar(prhs[7]) : 0;
  for (k = 0; k < 3; ++k) {
    const size_t per = k < 2 ? M : 1;
    sc[k] = (double*)mxCalloc(per * P, sizeof(double));
    for (q = 0; q < P; ++q) for (m = 0; m < per; ++m) sc[k][q * per + m] = par[k][n3[k] == per ? m : q * per + m];
  }
  o[0] = mxCreateDoubleMatrix((mwSize)P, 1, mxREAL);
  if (nlhs > 1) o[1] = mxCreateDoubleMatrix((mwSize)MTx, (mwSize)P, mxREAL);
  fail_if(nagp_gppad_cas_obj((int32_t)P, (int32_t)M, (int64_t)T, (int64_t)Tx, x, y, NULL, cov, nc == MTx * P && P > 1 ? (int64_t)MTx : 0,
                             sc[0], sc[1], sc[2], mxGetPr(o[0]), o[1] ? mxGetPr(o[1]) : NULL, dev));
  for (k = 0; k < 3; ++k) mxFree(sc[k]);
  for (i = 0; i < (nlhs > 1 ? nlhs : 1); ++i) plhs[i] = o[i];
}

static void cmd_nmf_temp_obj(int nlhs, mxArray* plhs[], int nrhs, const mxArray* prhs[]) {
  /* ('nmf_temp_obj', x, A, vary, W, muinf, varinf, lam [,device]) -> [Obj, dObj]: the objectives of experiments/nmf/getObj_nmf_temp.m (W = [])
     and getObj_nmf_temp_inf.m for P problems; dObj only when asked for */
  size_t nx, na, nv, nw, n3[3], P, T, D, K, X, q; const double *x, *A, *vary, *W, *par[3]; double* wp = NULL; int32_t dev, prior; int i, k;
  mxArray* o[2] = {NULL, NULL};
  static const char* names[3] = {"muinf", "varinf", "lam"};
  if (nrhs < 8 || nrhs > 9 || nlhs > 2) mexErrMsgIdAndTxt("nagp:arg", "usage: [Obj,dObj] = nagp_mex('nmf_temp_obj',x,A,vary,W,muinf,varinf,lam[,device])");
  A = dvec(prhs[2], "A", &na); T = A ? mxGetM(prhs[2]) : 0;
  if (!A || !T || na % T != 0) mexErrMsgIdAndTxt("nagp:arg", "A must be T x D");
  D = na / T;
  vary = dvec(prhs[3], "vary", &nv);
  if (vary && nv != na) mexErrMsgIdAndTxt("nagp:arg", "vary must be T x D or []");
  x = dvec(prhs[1], "x", &nx); X = x ? mxGetM(prhs[1]) : 0;
  if (!x || !X || nx % X != 0) mexErrMsgIdAndTxt("nagp:arg", "x must hold one column per problem");
  P = nx / X;
  W = dvec(prhs[4], "W", &nw);
  if (W) {
    K = mxGetM(prhs[4]);
    if (!K || (nw != K * D && nw != K * D * P)) mexErrMsgIdAndTxt("nagp:arg", "W must be K x D or K x D x P");
    if (X != T * K) mexErrMsgIdAndTxt("nagp:arg", "x must be (T K) x P with a given W");
  } else {
    K = X / (T + D);
    if (!K || K * (T + D) != X) mexErrMsgIdAndTxt("nagp:arg", "x must be (T K + K D) x P without W");
  }
  for (k = 0; k < 3; ++k) {
    par[k] = dvec(prhs[5 + k], names[k], &n3[k]);
    if (par[k] && n3[k] != K) mexErrMsgIdAndTxt("nagp:arg", "%s must hold K entries or be []", names[k]);
  }
  prior = !par[1] ? NAGP_NMFT_NONE : (!par[0] ? NAGP_NMFT_TG : NAGP_NMFT_IG);
  if (prior != NAGP_NMFT_NONE && !par[2]) mexErrMsgIdAndTxt("nagp:arg", "lam is empty but varinf is not");
  dev = nrhs > 8 ? (int32_t)mxGetScalar(prhs[8]) : 0;
  if (W && nw == K * D && P > 1) {                         /* a shared W: one copy per problem */
    wp = (double*)mxCalloc(K * D * P, sizeof *wp);
    for (q = 0; q < P; ++q) memcpy(wp + q * K * D, W, K * D * sizeof *wp);
  }
  o[0] = mxCreateDoubleMatrix((mwSize)P, 1, mxREAL);
  if (nlhs > 1) o[1] = mxCreateDoubleMatrix((mwSize)X, (mwSize)P, mxREAL);
  fail_if(nagp_nmf_temp_obj((int32_t)P, (int64_t)T, (int32_t)D, (int32_t)K, prior, x, A, vary, wp ? wp : W, prior == NAGP_NMFT_IG ? par[0] : NULL,
                            prior != NAGP_NMFT_NONE ? par[1] : NULL, prior != NAGP_NMFT_NONE ? par[2] : NULL, mxGetPr(o[0]), o[1] ? mxGetPr(o[1]) : NULL, dev));
  if (wp) mxFree(wp);
  for (i = 0; i < (nlhs > 1 ? nlhs : 1); ++i) plhs[i] = o[i];
}

static void cmd_tnmf_obj(int nlhs, mxArray* plhs[], int nrhs, const mxArray* prhs[]) {
  /* ('tnmf_obj', x, A, vary, W, lenx, mux, varx, tol [,device]) -> [Obj, dObj]: the objectives of experiments/nmf/getObj_nmf_log_norm.m (W = [])
     and getObj_nmf_log_norm_inf.m for P problems; dObj only when asked for */
  size_t nx, na, nv, nw, n3[3], nt, P, T, D, K, X, q; const double *x, *A, *vary, *W, *par[3], *tol; double* wp = NULL; int32_t dev; int i, k;
  mxArray* o[2] = {NULL, NULL};
  static const char* names[3] = {"lenx", "mux", "varx"};
  if (nrhs < 9 || nrhs > 10 || nlhs > 2) mexErrMsgIdAndTxt("nagp:arg", "usage: [Obj,dObj] = nagp_mex('tnmf_obj',x,A,vary,W,lenx,mux,varx,tol[,device])");
  A = dvec(prhs[2], "A", &na); T = A ? mxGetM(prhs[2]) : 0;
  if (!A || !T || na % T != 0) mexErrMsgIdAndTxt("nagp:arg", "A must be T x D");
  D = na / T;
  vary = dvec(prhs[3], "vary", &nv);
  if (vary && nv != na) mexErrMsgIdAndTxt("nagp:arg", "vary must be T x D or []");
  x = dvec(prhs[1], "x", &nx); X = x ? mxGetM(prhs[1]) : 0;
  if (!x || !X || nx % X != 0) mexErrMsgIdAndTxt("nagp:arg", "x must hold one column per problem");
  P = nx / X;
  W = dvec(prhs[4], "W", &nw);
  if (W) {
    K = mxGetM(prhs[4]);
    if (!K || (nw != K * D && nw != K * D * P)) mexErrMsgIdAndTxt("nagp:arg", "W must be K x D or K x D x P");
    if (X != T * K) mexErrMsgIdAndTxt("nagp:arg", "x must be (T K) x P with a given W");
  } else {
    K = X / (T + D);
    if (!K || K * (T + D) != X) mexErrMsgIdAndTxt("nagp:arg", "x must be (T K + K D) x P without W");
  }
  for (k = 0; k < 3; ++k) {
    par[k] = dvec(prhs[5 + k], names[k], &n3[k]);
    if (!par[k] || n3[k] != K) mexErrMsgIdAndTxt("nagp:arg", "%s must hold K entries", names[k]);
  }
  tol = dvec(prhs[8], "tol", &nt);
  if (!tol || nt != 1) mexErrMsgIdAndTxt("nagp:arg", "tol must be a scalar");
  dev = nrhs > 9 ? (int32_t)mxGetScalar(prhs[9]) : 0;
  if (W && nw == K * D && P > 1) {                         /* a shared W: one copy per problem */
    wp = (double*)mxCalloc(K * D * P, sizeof *wp);
    for (q = 0; q < P; ++q) memcpy(wp + q * K * D, W, K * D * sizeof *wp);
  }
  o[0] = mxCreateDoubleMatrix((mwSize)P, 1, mxREAL);
  if (nlhs > 1) o[1] = mxCreateDoubleMatrix((mwSize)X, (mwSize)P, mxREAL);
  fail_if(nagp_tnmf_obj((int32_t)P, (int64_t)T, (int32_t)D, (int32_t)K, x, A, vary, wp ? wp : W, par[0], par[1], par[2], tol[0], mxGetPr(o[0]),
                        o[1] ? mxGetPr(o[1]) : NULL, dev));
  if (wp) mxFree(wp);
  for (i = 0; i < (nlhs > 1 ? nlhs : 1); ++i) plhs[i] = o[i];
}

/* lenx, varx of the basis: a scalar or one entry per column -> n entries (mxCalloc) */
static double* per_column(const mxArray* a, const char* what, size_t n) {
  size_t m, q; const double* v = dvec(a, what, &m); double* out;
  if (!v || (m != 1 && m != n)) mexErrMsgIdAndTxt("nagp:arg", "%s must be a scalar or hold one entry per column", what);
  out = (double*)mxCalloc(n, sizeof *out);
  for (q = 0; q < n; ++q) out[q] = v[m == 1 ? 0 : q];
  return out;
}

static void cmd_sebf_fit_obj(int nlhs, mxArray* plhs[], int nrhs, const mxArray* prhs[]) {
  /* ('sebf_fit_obj', z, x, lenx, varx, tol [,device]) -> [Obj, dObj]: experiments/toolsGP/getObj_fitSE_basis_func.m for P columns */
  size_t nz, nx, nt, T, P; const double *z, *x, *tol; double *len, *vx; int32_t dev; int i;
  mxArray* o[2] = {NULL, NULL};
  if (nrhs < 6 || nrhs > 7 || nlhs > 2) mexErrMsgIdAndTxt("nagp:arg", "usage: [Obj,dObj] = nagp_mex('sebf_fit_obj',z,x,lenx,varx,tol[,device])");
  z = dvec(prhs[1], "z", &nz); T = z ? mxGetM(prhs[1]) : 0;
  if (!z || !T || nz % T != 0) mexErrMsgIdAndTxt("nagp:arg", "z must be T x P");
  P = nz / T;
  x = dvec(prhs[2], "x", &nx);
  if (!x || nx != nz || mxGetM(prhs[2]) != T) mexErrMsgIdAndTxt("nagp:arg", "x must be T x P as z");
  len = per_column(prhs[3], "lenx", P); vx = per_column(prhs[4], "varx", P);
  tol = dvec(prhs[5], "tol", &nt);
  if (!tol || nt != 1) mexErrMsgIdAndTxt("nagp:arg", "tol must be a scalar");
  dev = nrhs > 6 ? (int32_t)mxGetScalar(prhs[6]) : 0;
  o[0] = mxCreateDoubleMatrix((mwSize)P, 1, mxREAL);
  if (nlhs > 1) o[1] = mxCreateDoubleMatrix((mwSize)T, (mwSize)P, mxREAL);
  fail_if(nagp_sebf_fit_obj((int32_t)P, (int64_t)T, z, x, len, vx, tol[0], mxGetPr(o[0]), o[1] ? mxGetPr(o[1]) : NULL, dev));
  mxFree(len); mxFree(vx);
  for (i = 0; i < (nlhs > 1 ? nlhs : 1); ++i) plhs[i] = o[i];
}

static void cmd_sebf_conv(int nlhs, mxArray* plhs[], int nrhs, const mxArray* prhs[]) {
  /* ('sebf_conv', Z, lenx, varx, tol [,device]) -> Y: experiments/toolsGP/basis2SEGP.m */
  size_t nz, nt, T, K; const double *Z, *tol; double *len, *vx; int32_t dev; mxArray* y;
  if (nrhs < 5 || nrhs > 6 || nlhs > 1) mexErrMsgIdAndTxt("nagp:arg", "usage: Y = nagp_mex('sebf_conv',Z,lenx,varx,tol[,device])");
  Z = dvec(prhs[1], "Z", &nz); T = Z ? mxGetM(prhs[1]) : 0;
  if (!Z || !T || nz % T != 0) mexErrMsgIdAndTxt("nagp:arg", "Z must be T x K");
  K = nz / T;
  len = per_column(prhs[2], "lenx", K); vx = per_column(prhs[3], "varx", K);
  tol = dvec(prhs[4], "tol", &nt);
  if (!tol || nt != 1) mexErrMsgIdAndTxt("nagp:arg", "tol must be a scalar");
  dev = nrhs > 5 ? (int32_t)mxGetScalar(prhs[5]) : 0;
  y = mxCreateDoubleMatrix((mwSize)T, (mwSize)K, mxREAL);
  fail_if(nagp_sebf_conv((int32_t)K, (int64_t)T, Z, len, vx, tol[0], mxGetPr(y), dev));
  mxFree(len); mxFree(vx);
  plhs[0] = y;
}

static void cmd_reconstruct(int nlhs, mxArray* plhs[], int nrhs, const mxArray* prhs[]) {
  /* ('reconstruct', Eft, Varft, Wnmf, link_kind, link_shift, gh_x, gh_w, n_samples, seed [,device])  (demo_toy_modulators_nmf.m:119-158) */
  size_t n, nv, ngx, ngw, D, N, M, T; const double *E, *V, *W, *gx, *gw; int32_t dev; mxArray* o[4]; int i;
  if (nrhs < 10 || nrhs > 11) mexErrMsgIdAndTxt("nagp:arg", "usage: [Esig,Vsig,Eft_mod,Varft_mod] = nagp_mex('reconstruct',Eft,Varft,Wnmf,link_kind,link_shift,gh_x,gh_w,n_samples,seed[,device])");
  E = dvec(prhs[1], "Eft", &n); V = dvec(prhs[2], "Varft", &nv); W = dvec(prhs[3], "Wnmf", NULL);
  M = mxGetM(prhs[1]); D = mxGetM(prhs[3]); N = D ? mxGetNumberOfElements(prhs[3]) / D : 0;
  if (!E || !V || !W || n != nv || M != D + N) mexErrMsgIdAndTxt("nagp:arg", "Eft, Varft must be (D+N) x T for Wnmf of D x N");
  T = n / M;
  gx = dvec(prhs[6], "gh_x", &ngx); gw = dvec(prhs[7], "gh_w", &ngw);
  if (ngx != ngw) mexErrMsgIdAndTxt("nagp:arg", "gh_x and gh_w must have the same length");
  dev = nrhs > 10 ? (int32_t)mxGetScalar(prhs[10]) : 0;
  o[0] = mxCreateDoubleMatrix(1, T, mxREAL); o[1] = mxCreateDoubleMatrix(1, T, mxREAL);
  o[2] = mxCreateDoubleMatrix(N, T, mxREAL); o[3] = mxCreateDoubleMatrix(N, T, mxREAL);
  fail_if(nagp_reconstruct((int32_t)D, (int32_t)N, (int64_t)T, E, V, W, (int32_t)mxGetScalar(prhs[4]), mxGetScalar(prhs[5]), (int32_t)ngx, gx, gw,
                           (int32_t)mxGetScalar(prhs[8]), (uint64_t)mxGetScalar(prhs[9]), mxGetPr(o[0]), mxGetPr(o[1]), mxGetPr(o[2]), mxGetPr(o[3]), dev));
  plhs[0] = o[0];
  for (i = 1; i < 4; ++i) if (nlhs > i) plhs[i] = o[i];
}

static void cmd_reconstruct_sources(int nlhs, mxArray* plhs[], int nrhs, const mxArray* prhs[]) {
  /* ('reconstruct_sources', Eft, Varft, Wnmf, ropts) -> [Esig,Vsig,Esrc,Vsrc,Eenv,Eft_mod,Varft_mod]  (source_sep_piano.m:165-244, noise_reduction_speech.m:142);
     only the outputs asked for are computed (the others stay NULL in nagp_recon_out) */
  size_t n, nv, ng, nw, nx, D, N, M, T, J = 1; const double *E, *V, *W; const mxArray* f; nagp_recon_opts o; nagp_recon_out r; double* p[7]; int i;
  if (nrhs != 5 || nlhs > 7) mexErrMsgIdAndTxt("nagp:arg", "usage: [Esig,Vsig,Esrc,Vsrc,Eenv,Eft_mod,Varft_mod] = nagp_mex('reconstruct_sources',Eft,Varft,Wnmf,ropts)");
  E = dvec(prhs[1], "Eft", &n); V = dvec(prhs[2], "Varft", &nv); W = dvec(prhs[3], "Wnmf", NULL);
  M = mxGetM(prhs[1]); D = mxGetM(prhs[3]); N = D ? mxGetNumberOfElements(prhs[3]) / D : 0;
  if (!E || !V || !W || n != nv || M != D + N) mexErrMsgIdAndTxt("nagp:arg", "Eft, Varft must be (D+N) x T for Wnmf of D x N");
  T = n / M;
  memset(&o, 0, sizeof o); memset(&r, 0, sizeof r);
  o.amp_kind = (int32_t)scalar_or(prhs[4], "amp_kind", NAGP_AMP_SQRT);
  o.link_kind = (int32_t)scalar_or(prhs[4], "link_kind", NAGP_LINK_SOFTPLUS);
  o.link_shift = scalar_or(prhs[4], "link_shift", 0.0);
  f = field(prhs[4], "source_offsets", 0);
  if (f && !mxIsEmpty(f)) {
    if (!mxIsInt32(f) || mxGetNumberOfElements(f) < 2) mexErrMsgIdAndTxt("nagp:arg", "source_offsets must be int32 with J+1 entries");
    J = mxGetNumberOfElements(f) - 1; o.source_offsets = (const int32_t*)mxGetData(f);
  }
  o.n_sources = (int32_t)J;
  o.n_samples = (int32_t)scalar_or(prhs[4], "n_samples", 0); o.seed = (uint64_t)scalar_or(prhs[4], "seed", 0);
  o.gh_x = doubles(prhs[4], "gh_x", 0, &ng); o.gh_w = doubles(prhs[4], "gh_w", 0, &nw);
  if (ng != nw) mexErrMsgIdAndTxt("nagp:arg", "gh_x and gh_w must have the same length");
  o.n_gh = (int32_t)ng;
  o.wn = doubles(prhs[4], "wn", 0, &nw); o.xn_unscaled = doubles(prhs[4], "xn_unscaled", 0, &nx);
  if (nx != nw * N) mexErrMsgIdAndTxt("nagp:arg", "xn_unscaled must be N x numel(wn)");
  o.n_pts = (int32_t)nw;
  o.device = (int32_t)scalar_or(prhs[4], "device", 0);
  for (i = 0; i < (nlhs > 1 ? nlhs : 1); ++i) {
    plhs[i] = mxCreateDoubleMatrix(i < 2 ? 1 : (i < 4 ? J : (i == 4 ? D : N)), T, mxREAL); p[i] = mxGetPr(plhs[i]);
  }
  for (; i < 7; ++i) p[i] = NULL;
  r.Esig = p[0]; r.Vsig = p[1]; r.Esrc = p[2]; r.Vsrc = p[3]; r.Eenv = p[4]; r.Eft_mod = p[5]; r.Varft_mod = p[6];
  fail_if(nagp_reconstruct_sources((int32_t)D, (int32_t)N, (int64_t)T, E, V, W, &o, &r));
}

static void cmd_batch(int nlhs, mxArray* plhs[], int nrhs, const mxArray* prhs[]) {
  /* ('batch', models {cell}, ys {cell}, opts, n_gpus [, tables {cell}]) -> [nlZ_total, Eft {cell}, Varft {cell}, nlZ {cell}]
     segments / objective replicas spread over the GPUs of the node, nlZ all-reduced with RCCL (nagp_batch_run) */
  size_t B, T = 0, q; nagp_model* ms; nagp_ihgp_tables* ts = NULL; const double** ys; nagp_out* outs; nagp_opts o; int32_t ng;
  mxArray *cE, *cV, *cZ;
  if (nrhs < 5 || nrhs > 6 || !mxIsCell(prhs[1]) || !mxIsCell(prhs[2])) mexErrMsgIdAndTxt("nagp:arg", "usage: [nlZ_total,Eft,Varft,nlZ] = nagp_mex('batch',models,ys,opts,n_gpus[,tables])");
  B = mxGetNumberOfElements(prhs[1]);
  if (B < 1 || mxGetNumberOfElements(prhs[2]) != B || (nrhs > 5 && (!mxIsCell(prhs[5]) || mxGetNumberOfElements(prhs[5]) != B)))
    mexErrMsgIdAndTxt("nagp:arg", "models, ys (and tables) must be cell arrays of the same length");
  /* mxCalloc: MATLAB frees these when an argument error below leaves the MEX function through mexErrMsgIdAndTxt (a longjmp) */
  ms = (nagp_model*)mxCalloc(B, sizeof *ms); ys = (const double**)mxCalloc(B, sizeof *ys); outs = (nagp_out*)mxCalloc(B, sizeof *outs);
  if (nrhs > 5) ts = (nagp_ihgp_tables*)mxCalloc(B, sizeof *ts);
  for (q = 0; q < B; ++q) {
    size_t n;
    read_model(mxGetCell(prhs[1], q), &ms[q]);
    ys[q] = dvec(mxGetCell(prhs[2], q), "y", &n);
    if (q == 0) T = n;
    if (!ys[q] || n != T) mexErrMsgIdAndTxt("nagp:arg", "every y must be a real double vector of the same length");
    if (ts) read_tables(mxGetCell(prhs[5], q), &ts[q], ms[q].M);
  }
  read_opts(prhs[3], &o, ms[0].M, T);
  if (o.ttau0 || o.tnu0) mexErrMsgIdAndTxt("nagp:arg", "the batch call takes no warm-start sites");
  ng = (int32_t)mxGetScalar(prhs[4]);
  plhs[0] = mxCreateDoubleMatrix(1, o.ep_itts, mxREAL);
  cE = mxCreateCellMatrix(1, B); cV = mxCreateCellMatrix(1, B); cZ = mxCreateCellMatrix(1, B);
  for (q = 0; q < B; ++q) {
    mxArray* e = mxCreateDoubleMatrix(ms[q].M, T, mxREAL); mxArray* v = mxCreateDoubleMatrix(ms[q].M, T, mxREAL); mxArray* z = mxCreateDoubleMatrix(1, o.ep_itts, mxREAL);
    outs[q].Eft = mxGetPr(e); outs[q].Varft = mxGetPr(v); outs[q].nlZ = mxGetPr(z);
    mxSetCell(cE, q, e); mxSetCell(cV, q, v); mxSetCell(cZ, q, z);
  }
  { const int st = nagp_batch_run((int32_t)B, ms, ts, ys, (int64_t)T, &o, outs, ng, mxGetPr(plhs[0]));
    mxFree(ms); mxFree((void*)ys); mxFree(outs); if (ts) mxFree(ts);
    fail_if(st); }
  if (nlhs > 1) plhs[1] = cE;
  if (nlhs > 2) plhs[2] = cV;
  if (nlhs > 3) plhs[3] = cZ;
}

void mexFunction(int nlhs, mxArray* plhs[], int nrhs, const mxArray* prhs[]) {
  nagp_model m;
  nagp_opts o;
  nagp_out out;
  nagp_ihgp_tables tb;
  size_t T;
  int st;
  mwSize dims3[3];

  if (nrhs >= 1 && mxIsChar(prhs[0])) {
    char cmd[32];
    if (mxGetString(prhs[0], cmd, sizeof cmd)) mexErrMsgIdAndTxt("nagp:arg", "command string too long");
    if (!strcmp(cmd, "iekf_update1")) cmd_iekf_update1(nlhs, plhs, nrhs, prhs);
    else if (!strcmp(cmd, "fastfb")) cmd_fastfb(nlhs, plhs, nrhs, prhs);
    else if (!strcmp(cmd, "fastfb_sample")) cmd_fastfb_sample(nlhs, plhs, nrhs, prhs);
    else if (!strcmp(cmd, "ep_sample")) cmd_ep_sample(nlhs, plhs, nrhs, prhs);
    else if (!strcmp(cmd, "slowfb")) cmd_slowfb(nlhs, plhs, nrhs, prhs);
    else if (!strcmp(cmd, "nmf_fp")) cmd_nmf_fp(nlhs, plhs, nrhs, prhs);
    else if (!strcmp(cmd, "pstft_obj")) cmd_pstft_obj(nlhs, plhs, nrhs, prhs);
    else if (!strcmp(cmd, "segp_obj")) cmd_segp_obj(nlhs, plhs, nrhs, prhs);
    else if (!strcmp(cmd, "gppad_obj")) cmd_gppad_obj(nlhs, plhs, nrhs, prhs);
    else if (!strcmp(cmd, "gppad_cas_obj")) cmd_gppad_cas_obj(nlhs, plhs, nrhs, prhs);
    else if (!strcmp(cmd, "nmf_temp_obj")) cmd_nmf_temp_obj(nlhs, plhs, nrhs, prhs);
    else if (!strcmp(cmd, "tnmf_obj")) cmd_tnmf_obj(nlhs, plhs, nrhs, prhs);
    else if (!strcmp(cmd, "sebf_fit_obj")) cmd_sebf_fit_obj(nlhs, plhs, nrhs, prhs);
    else if (!strcmp(cmd, "sebf_conv")) cmd_sebf_conv(nlhs, plhs, nrhs, prhs);
    else if (!strcmp(cmd, "reconstruct")) cmd_reconstruct(nlhs, plhs, nrhs, prhs);
    else if (!strcmp(cmd, "reconstruct_sources")) cmd_reconstruct_sources(nlhs, plhs, nrhs, prhs);
    else if (!strcmp(cmd, "batch")) cmd_batch(nlhs, plhs, nrhs, prhs);
    else if (!strcmp(cmd, "giekf_grad")) cmd_giekf_grad(nlhs, plhs, nrhs, prhs);
    else mexErrMsgIdAndTxt("nagp:arg", "unknown command '%s'", cmd);
    return;
  }
  if (nrhs < 3 || nrhs > 4) mexErrMsgIdAndTxt("nagp:arg", "usage: [...] = nagp_mex(model, y, opts [, tables])");
  if (nlhs > 12) mexErrMsgIdAndTxt("nagp:arg", "at most 12 outputs");
  memset(&out, 0, sizeof out); memset(&tb, 0, sizeof tb);
  read_model(prhs[0], &m);

  /* ---- observations */
  if (!mxIsDouble(prhs[1]) || mxIsComplex(prhs[1])) mexErrMsgIdAndTxt("nagp:arg", "y must be real double");
  T = mxGetNumberOfElements(prhs[1]);
  read_opts(prhs[2], &o, m.M, T);
  if (nlhs > 11) o.flags |= NAGP_FLAG_WANT_PS;

  /* ---- outputs (column-major M x T etc.: exactly the library's layout) */
  /* MATLAB guarantees max(nlhs, 1) slots in plhs and no more: only those are touched */
  plhs[0] = mxCreateDoubleMatrix(m.M, T, mxREAL); out.Eft = mxGetPr(plhs[0]);
  if (nlhs > 1) { plhs[1] = mxCreateDoubleMatrix(m.M, T, mxREAL); out.Varft = mxGetPr(plhs[1]); }
  if (nlhs > 2) { plhs[2] = mxCreateDoubleMatrix(m.M, T, mxREAL); out.ttau = mxGetPr(plhs[2]); }
  if (nlhs > 3) { plhs[3] = mxCreateDoubleMatrix(m.M, T, mxREAL); out.tnu = mxGetPr(plhs[3]); }
  if (nlhs > 4) { plhs[4] = mxCreateDoubleMatrix(m.M, T, mxREAL); out.R = mxGetPr(plhs[4]); }
  if (nlhs > 5) { plhs[5] = mxCreateDoubleMatrix(1, T, mxREAL); out.lZ = mxGetPr(plhs[5]); }
  if (nlhs > 6) { plhs[6] = mxCreateDoubleMatrix(1, o.ep_itts, mxREAL); out.nlZ = mxGetPr(plhs[6]); }
  if (nlhs > 7) { plhs[7] = mxCreateDoubleMatrix(1, o.ep_itts, mxREAL); out.maxDiffM = mxGetPr(plhs[7]); }
  if (nlhs > 8) { plhs[8] = mxCreateDoubleMatrix(1, o.ep_itts, mxREAL); out.maxDiffP = mxGetPr(plhs[8]); }
  if (nlhs > 9) { plhs[9] = mxCreateNumericMatrix(1, NAGP_N_COUNTERS, mxINT64_CLASS, mxREAL); out.counters = (int64_t*)mxGetData(plhs[9]); }
  if (nlhs > 10) { plhs[10] = mxCreateDoubleMatrix(m.S, T, mxREAL); out.MS = mxGetPr(plhs[10]); }
  if (nlhs > 11) {
    dims3[0] = (mwSize)m.S; dims3[1] = (mwSize)m.S; dims3[2] = (mwSize)T;
    plhs[11] = mxCreateNumericArray(3, dims3, mxDOUBLE_CLASS, mxREAL); out.PS = mxGetPr(plhs[11]);
  }

  /* ---- the call */
  if (o.kind == NAGP_KIND_IHGP) {
    if (nrhs < 4) mexErrMsgIdAndTxt("nagp:arg", "the infinite-horizon kind needs the look-up tables");
    read_tables(prhs[3], &tb, m.M);
    st = nagp_ihgp_run(&m, &tb, mxGetPr(prhs[1]), (int64_t)T, &o, &out);
  } else if (o.kind == NAGP_KIND_GIEKF) {
    st = nagp_giekf_run(&m, mxGetPr(prhs[1]), (int64_t)T, &o, &out);
  } else if (scalar_or(prhs[2], "windows", 0.0) > 1.0) {
    /* optional field `windows` of the options (nagp_opts.m): the fixed-site filter of the sweeps >= 2 in that many windows at the same time
     * (nagp_plan_set_windows; fields window_overlap / window_tol, defaults 8000 steps / 1e-10) -- the steps of nagp_ep_run on a plan of one problem */
    nagp_plan* pl = NULL;
    const double* ys[1]; const double* t0[1]; const double* n0[1];
    ys[0] = mxGetPr(prhs[1]); t0[0] = o.ttau0; n0[0] = o.tnu0;
    if (out.PS) o.flags |= NAGP_FLAG_WANT_PS;
    st = nagp_plan_create(&pl, 1, &m, NULL, (int64_t)T, &o);
    if (st == NAGP_OK) st = nagp_plan_set_windows(pl, (int32_t)scalar_or(prhs[2], "windows", 0.0), (int32_t)scalar_or(prhs[2], "window_overlap", 8000.0),
                                                  scalar_or(prhs[2], "window_tol", 1e-10));
    if (st == NAGP_OK) st = nagp_plan_upload_y(pl, ys);
    if (st == NAGP_OK && (o.ttau0 || o.tnu0)) st = nagp_plan_upload_sites(pl, t0, n0);
    if (st == NAGP_OK) st = nagp_plan_execute(pl);
    if (st == NAGP_OK) st = nagp_plan_download(pl, &out);
    nagp_plan_destroy(pl);
  } else {      /* (no `windows` field, or <= 1: today's path) */
    st = nagp_ep_run(&m, mxGetPr(prhs[1]), (int64_t)T, &o, &out);
  }
  fail_if(st);
}
