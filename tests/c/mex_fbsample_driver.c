/* mex_fbsample_driver.c -- drives the 'fastfb_sample' command of matlab/nagp_mex.c (compiled against the mock mex.h of this
 * directory) with the argument list matlab/kernel_ss_sampleFastFB.m builds, on dumped matrices: output sizes, values against the dumped
 * results of the Python call; a call with one output gives the same Ydraw.
 *   mex_fbsample_driver <dump dir>        exit 0 = sizes right and values within 1e-12 */
#include "dump.h"
#include "mex.h"

static mxArray* dbl(const char* d, const char* name, size_t rows) {
  size_t n; double* p = (double*)dump_load(d, name, 8, &n);
  mxArray* a = mock_numeric(mxDOUBLE_CLASS, rows ? rows : n, rows ? n / rows : 1, p);
  free(p); return a;
}

int main(int argc, char** argv) {
  const char* d = argc > 1 ? argv[1] : ".";
  static const char* names[3] = {"Ydraw", "Xdraw", "MS"};
  const size_t S = (size_t)dump_scalar(d, "S"), nd = (size_t)dump_scalar(d, "n_draws");
  size_t T, n, want[3], i; double worst = 0.0, r;
  const mxArray* prhs[14]; mxArray **plhs, **plhs1;
  prhs[0] = mock_string("fastfb_sample");
  prhs[1] = dbl(d, "A", S); prhs[2] = dbl(d, "AKHA", S); prhs[3] = dbl(d, "HA", 0); prhs[4] = dbl(d, "K", 0); prhs[5] = dbl(d, "G", S);
  prhs[6] = dbl(d, "H", 0); prhs[7] = mock_scalar(dump_scalar(d, "R")); prhs[8] = dbl(d, "Lp", S); prhs[9] = dbl(d, "Lq", S);
  prhs[10] = dbl(d, "y", 0); prhs[11] = mock_scalar((double)nd); prhs[12] = mock_scalar(dump_scalar(d, "seed")); prhs[13] = mock_scalar(0);
  T = mxGetNumberOfElements(prhs[10]);
  /* plhs has EXACTLY nlhs slots (heap, so that a sanitizer build sees a gateway that writes past them) */
  plhs = (mxArray**)malloc(3 * sizeof *plhs);
  mexFunction(3, plhs, 14, prhs);
  want[0] = T * nd; want[1] = S * T * nd; want[2] = S * T;
  if (mxGetM(plhs[0]) != T || mxGetM(plhs[1]) != S || mxGetM(plhs[2]) != S) { printf("wrong leading sizes\n"); return 1; }
  for (i = 0; i < 3; ++i) {
    double* e;
    if (mxGetNumberOfElements(plhs[i]) != want[i]) { printf("%s: wrong size\n", names[i]); return 1; }
    e = (double*)dump_load(d, names[i], 8, &n);
    if (n != want[i]) { printf("%s: dump has %zu entries\n", names[i], n); return 1; }
    r = rel_diff(mxGetPr(plhs[i]), e, n, names[i]); if (r > worst) worst = r;
    free(e);
  }
  plhs1 = (mxArray**)malloc(1 * sizeof *plhs1);           /* Ydraw = nagp_mex(...), 13 arguments (default device) */
  mexFunction(1, plhs1, 13, prhs);
  if (mxGetNumberOfElements(plhs1[0]) != want[0] || memcmp(mxGetPr(plhs1[0]), mxGetPr(plhs[0]), want[0] * sizeof(double))) {
    printf("nlhs=1 call: Ydraw differs from the nlhs=3 call\n"); return 1; }
  printf("S %zu T %zu n_draws %zu worst %.3e\n", S, T, nd, worst);
  return worst < 1e-12 ? 0 : 1;
}
