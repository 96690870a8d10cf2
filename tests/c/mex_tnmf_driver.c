/* mex_tnmf_driver.c -- drives the 'tnmf_obj', 'sebf_fit_obj' and 'sebf_conv' commands of matlab/nagp_mex.c (compiled against the mock mex.h of
 * this directory) with the argument lists matlab/getObj_nmf_log_norm.m, getObj_nmf_log_norm_inf.m, getObj_fitSE_basis_func.m and basis2SEGP.m
 * build, on dumped arrays: output sizes, and Obj / dObj (Y) bit for bit against the dumped results of the Python call; a call with one
 * output and the default device gives the same Obj.  An array dumped with no entries is passed as [].  The dumped scalar `mode` picks the
 * command: 0 tnmf_obj, 1 sebf_fit_obj, 2 sebf_conv.
 *   mex_tnmf_driver <dump dir>        exit 0 = sizes right and every value bit-equal */
#include "dump.h"
#include "mex.h"

static mxArray* dbl(const char* d, const char* name, size_t rows) {
  size_t n; double* p;
  mxArray* a;
  if (!dump_count(d, name) || !rows) return mock_numeric(mxDOUBLE_CLASS, 0, 0, NULL);
  p = (double*)dump_load(d, name, 8, &n);
  a = mock_numeric(mxDOUBLE_CLASS, rows, n / rows, p);
  free(p); return a;
}

static int same(const char* d, const char* name, const mxArray* got, size_t rows, size_t cols) {
  size_t n; double* e;
  if (mxGetNumberOfElements(got) != rows * cols || mxGetM(got) != rows) { printf("%s: wrong size\n", name); return 0; }
  e = (double*)dump_load(d, name, 8, &n);
  if (n != rows * cols || rel_diff(mxGetPr(got), e, n, name) != 0.0 || memcmp(mxGetPr(got), e, n * sizeof(double))) { printf("%s: not bit-equal to the Python call\n", name); return 0; }
  free(e);
  return 1;
}

int main(int argc, char** argv) {
  const char* d = argc > 1 ? argv[1] : ".";
  const int mode = (int)dump_scalar(d, "mode");
  const size_t X = (size_t)dump_scalar(d, "X"), T = (size_t)dump_scalar(d, "T"), K = (size_t)dump_scalar(d, "K"), P = (size_t)dump_scalar(d, "P");
  const mxArray* prhs[10]; mxArray **plhs, **plhs1;
  int nrhs;
  if (mode == 0) {
    prhs[0] = mock_string("tnmf_obj");
    prhs[1] = dbl(d, "x", X); prhs[2] = dbl(d, "A", T); prhs[3] = dbl(d, "vary", T); prhs[4] = dbl(d, "W", K);
    prhs[5] = dbl(d, "lenx", 1); prhs[6] = dbl(d, "mux", 1); prhs[7] = dbl(d, "varx", 1); prhs[8] = dbl(d, "tol", 1);
    prhs[9] = mock_scalar(0); nrhs = 10;
  } else if (mode == 1) {
    prhs[0] = mock_string("sebf_fit_obj");
    prhs[1] = dbl(d, "x", X); prhs[2] = dbl(d, "y", T); prhs[3] = dbl(d, "lenx", 1); prhs[4] = dbl(d, "varx", 1); prhs[5] = dbl(d, "tol", 1);
    prhs[6] = mock_scalar(0); nrhs = 7;
  } else {
    prhs[0] = mock_string("sebf_conv");
    prhs[1] = dbl(d, "x", X); prhs[2] = dbl(d, "lenx", 1); prhs[3] = dbl(d, "varx", 1); prhs[4] = dbl(d, "tol", 1);
    prhs[5] = mock_scalar(0); nrhs = 6;
  }
  if (mode == 2) {                                          /* Y = nagp_mex('sebf_conv', ...): one output, T x P */
    plhs = (mxArray**)malloc(1 * sizeof *plhs);
    mexFunction(1, plhs, nrhs, prhs);
    if (!same(d, "Y", plhs[0], X, P)) return 1;
    plhs1 = (mxArray**)malloc(1 * sizeof *plhs1);
    mexFunction(1, plhs1, nrhs - 1, prhs);                  /* the default device */
    if (memcmp(mxGetPr(plhs1[0]), mxGetPr(plhs[0]), X * P * sizeof(double))) { printf("default device: Y differs\n"); return 1; }
    printf("mode 2 T %zu K %zu bit-equal\n", X, P);
    return 0;
  }
  /* plhs has EXACTLY nlhs slots (heap, so that a sanitizer build sees a gateway that writes past them) */
  plhs = (mxArray**)malloc(2 * sizeof *plhs);
  mexFunction(2, plhs, nrhs, prhs);
  if (!same(d, "Obj", plhs[0], P, 1) || !same(d, "dObj", plhs[1], X, P)) return 1;
  plhs1 = (mxArray**)malloc(1 * sizeof *plhs1);             /* Obj = nagp_mex(...), the default device */
  mexFunction(1, plhs1, nrhs - 1, prhs);
  if (mxGetNumberOfElements(plhs1[0]) != P || memcmp(mxGetPr(plhs1[0]), mxGetPr(plhs[0]), P * sizeof(double))) {
    printf("nlhs=1 call: Obj differs from the nlhs=2 call\n"); return 1; }
  printf("mode %d X %zu T %zu P %zu bit-equal\n", mode, X, T, P);
  return 0;
}
