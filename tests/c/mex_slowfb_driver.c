/* mex_slowfb_driver.c -- drives the 'slowfb' command of matlab/nagp_mex.c (compiled against the mock mex.h of this directory) with
 * the argument list matlab/kernel_ss_kalmanSlowFB.m builds, on dumped matrices: output sizes, and lik / MS / Psub bit for bit
 * against the dumped results of the Python call; a call with one output gives the same lik.
 *   mex_slowfb_driver <dump dir>        exit 0 = sizes right and every value bit-equal */
#include "dump.h"
#include "mex.h"

static mxArray* dbl(const char* d, const char* name, size_t rows) {
  size_t n; double* p = (double*)dump_load(d, name, 8, &n);
  mxArray* a = mock_numeric(mxDOUBLE_CLASS, rows ? rows : n, rows ? n / rows : 1, p);
  free(p); return a;
}

int main(int argc, char** argv) {
  const char* d = argc > 1 ? argv[1] : ".";
  static const char* names[3] = {"lik", "MS", "Psub"};
  const size_t S = (size_t)dump_scalar(d, "S");
  size_t T, n, nsub, want[3], i; int32_t* sub; double* sd;
  const mxArray* prhs[12]; mxArray **plhs, **plhs1;
  prhs[0] = mock_string("slowfb");
  prhs[1] = dbl(d, "A", S); prhs[2] = dbl(d, "Q", S); prhs[3] = dbl(d, "H", 0); prhs[4] = dbl(d, "P0", S);
  prhs[5] = mock_scalar(dump_scalar(d, "block")); prhs[6] = dbl(d, "y", 0); prhs[7] = dbl(d, "vary", 0);
  prhs[8] = mock_scalar(0); prhs[9] = mock_scalar(2);
  sd = (double*)dump_load(d, "sub_idx", 8, &nsub);
  sub = (int32_t*)malloc(nsub * sizeof *sub);
  for (i = 0; i < nsub; ++i) sub[i] = (int32_t)sd[i];
  prhs[10] = mock_numeric(mxINT32_CLASS, nsub, 1, sub); prhs[11] = mock_scalar(0);
  free(sd); free(sub);
  T = mxGetNumberOfElements(prhs[6]);
  /* plhs has EXACTLY nlhs slots (heap, so that a sanitizer build sees a gateway that writes past them) */
  plhs = (mxArray**)malloc(3 * sizeof *plhs);
  mexFunction(3, plhs, 12, prhs);
  want[0] = 1; want[1] = S * T; want[2] = nsub * nsub * T;
  if (mxGetM(plhs[0]) != 1 || mxGetM(plhs[1]) != S || mxGetM(plhs[2]) != nsub) { printf("wrong leading sizes\n"); return 1; }
  for (i = 0; i < 3; ++i) {
    double* e;
    if (mxGetNumberOfElements(plhs[i]) != want[i]) { printf("%s: wrong size\n", names[i]); return 1; }
    e = (double*)dump_load(d, names[i], 8, &n);
    if (n != want[i]) { printf("%s: dump has %zu entries\n", names[i], n); return 1; }
    if (rel_diff(mxGetPr(plhs[i]), e, n, names[i]) != 0.0 || memcmp(mxGetPr(plhs[i]), e, n * sizeof(double))) { printf("%s: not bit-equal to the Python call\n", names[i]); return 1; }
    free(e);
  }
  plhs1 = (mxArray**)malloc(1 * sizeof *plhs1);           /* lik = nagp_mex(...), 11 arguments (default device) */
  mexFunction(1, plhs1, 11, prhs);
  if (mxGetNumberOfElements(plhs1[0]) != 1 || memcmp(mxGetPr(plhs1[0]), mxGetPr(plhs[0]), sizeof(double))) {
    printf("nlhs=1 call: lik differs from the nlhs=3 call\n"); return 1; }
  printf("S %zu T %zu n_sub %zu bit-equal\n", S, T, nsub);
  return 0;
}
