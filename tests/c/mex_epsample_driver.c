/* mex_epsample_driver.c -- drives the 'ep_sample' command of matlab/nagp_mex.c (compiled against the mock mex.h of this directory)
 * with the argument list matlab/gf_ep_sample.m builds, on dumped matrices: output sizes, values bit for bit those of the dumped results
 * of the Python call; a call with one output gives the same Fdraw.
 *   mex_epsample_driver <dump dir>        exit 0 = sizes right and every value equal */
#include "dump.h"
#include "mex.h"

static mxArray* dbl(const char* d, const char* name, size_t rows) {
  size_t n; double* p = (double*)dump_load(d, name, 8, &n);
  mxArray* a = mock_numeric(mxDOUBLE_CLASS, rows ? rows : n, rows ? n / rows : 1, p);
  free(p); return a;
}

int main(int argc, char** argv) {
  const char* d = argc > 1 ? argv[1] : ".";
  static const char* names[4] = {"Fdraw", "Xdraw", "Sdraw", "MS"};
  const size_t S = (size_t)dump_scalar(d, "S"), nd = (size_t)dump_scalar(d, "n_draws"), D = (size_t)dump_scalar(d, "D");
  size_t T, M, n, want[4], i;
  mxArray *model = mock_struct(), *sig = mock_struct();
  const mxArray* prhs[11]; mxArray **plhs, **plhs1;
  int32_t* bo = (int32_t*)dump_load(d, "block_offsets", 4, &n);
  M = n - 1;
  mock_set(model, "A", dbl(d, "A", S)); mock_set(model, "Q", dbl(d, "Q", S)); mock_set(model, "Pinf", dbl(d, "Pinf", S));
  mock_set(model, "block_offsets", mock_numeric(mxINT32_CLASS, 1, n, bo));
  mock_set(model, "h_val", dbl(d, "h_val", 0));
  mock_set(model, "Wnmf", dbl(d, "Wnmf", D));
  mock_set(model, "D", mock_scalar((double)D)); mock_set(model, "N", mock_scalar(dump_scalar(d, "N")));
  mock_set(model, "lik_param", mock_scalar(dump_scalar(d, "lik_param")));
  mock_set(sig, "Wnmf", dbl(d, "Wnmf", D)); mock_set(sig, "amp_kind", mock_scalar(dump_scalar(d, "amp_kind")));
  mock_set(sig, "link_kind", mock_scalar(dump_scalar(d, "link_kind"))); mock_set(sig, "link_shift", mock_scalar(dump_scalar(d, "link_shift")));
  prhs[0] = mock_string("ep_sample"); prhs[1] = model; prhs[2] = dbl(d, "ttau", M); prhs[3] = dbl(d, "tnu", M); prhs[4] = dbl(d, "y", 0);
  prhs[5] = mock_scalar(0); prhs[6] = mock_scalar((double)nd); prhs[7] = mock_scalar(dump_scalar(d, "seed"));
  prhs[8] = mxCreateDoubleMatrix(0, 0, mxREAL); prhs[9] = sig; prhs[10] = mock_scalar(0);
  T = mxGetNumberOfElements(prhs[4]);
  /* plhs has EXACTLY nlhs slots (heap, so that a sanitizer build sees a gateway that writes past them) */
  plhs = (mxArray**)malloc(5 * sizeof *plhs);
  mexFunction(5, plhs, 11, prhs);
  want[0] = M * T * nd; want[1] = S * T * nd; want[2] = T * nd; want[3] = S * T;
  if (mxGetM(plhs[0]) != M || mxGetM(plhs[1]) != S || mxGetM(plhs[2]) != T || mxGetM(plhs[3]) != S || mxGetNumberOfElements(plhs[4]) != 2) { printf("wrong sizes\n"); return 1; }
  for (i = 0; i < 4; ++i) {
    double* e;
    if (mxGetNumberOfElements(plhs[i]) != want[i]) { printf("%s: wrong size\n", names[i]); return 1; }
    e = (double*)dump_load(d, names[i], 8, &n);
    if (n != want[i]) { printf("%s: dump has %zu entries\n", names[i], n); return 1; }
    if (memcmp(mxGetPr(plhs[i]), e, n * sizeof(double))) { printf("%s: differs from the Python call (%.3e)\n", names[i], rel_diff(mxGetPr(plhs[i]), e, n, names[i])); return 1; }
    free(e);
  }
  if (mxGetPr(plhs[4])[0] != 0.0 || mxGetPr(plhs[4])[1] != 0.0) { printf("counters not zero\n"); return 1; }
  plhs1 = (mxArray**)malloc(1 * sizeof *plhs1);           /* Fdraw = nagp_mex(...), 10 arguments (default device) */
  mexFunction(1, plhs1, 10, prhs);
  if (mxGetNumberOfElements(plhs1[0]) != want[0] || memcmp(mxGetPr(plhs1[0]), mxGetPr(plhs[0]), want[0] * sizeof(double))) {
    printf("nlhs=1 call: Fdraw differs from the nlhs=5 call\n"); return 1; }
  printf("S %zu M %zu T %zu n_draws %zu: bit for bit\n", S, M, T, nd);
  return 0;
}
