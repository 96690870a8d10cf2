/* mex_nmf_driver.c -- drives the 'nmf_fp' command of matlab/nagp_mex.c (compiled against the mock mex.h of this directory) with the
 * argument list matlab/nmf_fp.m and matlab/nmf_inf_fp.m build, on dumped matrices: output sizes, and W / H / Obj bit for bit against
 * the dumped results of the Python call; a call with one output and the default device gives the same W.
 *   mex_nmf_driver <dump dir>        exit 0 = sizes right and every value bit-equal */
#include "dump.h"
#include "mex.h"

static mxArray* dbl(const char* d, const char* name, size_t rows) {
  size_t n; double* p = (double*)dump_load(d, name, 8, &n);
  mxArray* a = mock_numeric(mxDOUBLE_CLASS, rows, n / rows, p);
  free(p); return a;
}

int main(int argc, char** argv) {
  const char* d = argc > 1 ? argv[1] : ".";
  static const char* names[3] = {"W", "H", "Obj"};
  const size_t T = (size_t)dump_scalar(d, "T"), K = (size_t)dump_scalar(d, "K");
  const int its = (int)dump_scalar(d, "its"), uw = (int)dump_scalar(d, "update_w");
  size_t n, nw, P, D, want[3], lead[3], i;
  const mxArray* prhs[8]; mxArray **plhs, **plhs1;
  prhs[0] = mock_string("nmf_fp");
  prhs[1] = dbl(d, "A", T);
  prhs[2] = dump_count(d, "vary") ? dbl(d, "vary", T) : mxCreateDoubleMatrix(0, 0, mxREAL);
  prhs[3] = dbl(d, "W0", K); prhs[4] = dbl(d, "H0", T);
  prhs[5] = mock_scalar(its); prhs[6] = mock_scalar(uw); prhs[7] = mock_scalar(0);
  D = mxGetNumberOfElements(prhs[1]) / T; nw = mxGetNumberOfElements(prhs[3]); P = nw / (K * D);
  /* plhs has EXACTLY nlhs slots (heap, so that a sanitizer build sees a gateway that writes past them) */
  plhs = (mxArray**)malloc(3 * sizeof *plhs);
  mexFunction(3, plhs, 8, prhs);
  want[0] = K * D * P; want[1] = T * K * P; want[2] = (size_t)(uw ? 2 : 1) * (size_t)its * P;
  lead[0] = K; lead[1] = T; lead[2] = (size_t)(uw ? 2 : 1) * (size_t)its;
  for (i = 0; i < 3; ++i) {
    double* e;
    if (mxGetNumberOfElements(plhs[i]) != want[i] || mxGetM(plhs[i]) != lead[i]) { printf("%s: wrong size\n", names[i]); return 1; }
    e = (double*)dump_load(d, names[i], 8, &n);
    if (n != want[i]) { printf("%s: dump has %zu entries\n", names[i], n); return 1; }
    if (rel_diff(mxGetPr(plhs[i]), e, n, names[i]) != 0.0 || memcmp(mxGetPr(plhs[i]), e, n * sizeof(double))) { printf("%s: not bit-equal to the Python call\n", names[i]); return 1; }
    free(e);
  }
  plhs1 = (mxArray**)malloc(1 * sizeof *plhs1);           /* W = nagp_mex(...), 7 arguments (default device) */
  mexFunction(1, plhs1, 7, prhs);
  if (mxGetNumberOfElements(plhs1[0]) != want[0] || memcmp(mxGetPr(plhs1[0]), mxGetPr(plhs[0]), want[0] * sizeof(double))) {
    printf("nlhs=1 call: W differs from the nlhs=3 call\n"); return 1; }
  printf("T %zu D %zu K %zu P %zu bit-equal\n", T, D, K, P);
  return 0;
}
