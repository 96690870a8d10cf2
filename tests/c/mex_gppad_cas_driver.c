/* mex_gppad_cas_driver.c -- drives the 'gppad_cas_obj' command of matlab/nagp_mex.c (compiled against the mock mex.h of this directory)
 * with the argument list matlab/GetObjCasGPFAST.m builds, on dumped arrays: output sizes, and Obj / dObj bit for bit against the dumped
 * results of the Python call; a call with one output and the default device gives the same Obj.
 *   mex_gppad_cas_driver <dump dir>        exit 0 = sizes right and every value bit-equal */
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
  const size_t M = (size_t)dump_scalar(d, "M"), T = (size_t)dump_scalar(d, "T"), Tx = (size_t)dump_scalar(d, "Tx"), P = (size_t)dump_scalar(d, "P");
  const size_t vrows = (size_t)dump_scalar(d, "vrows");
  const mxArray* prhs[8]; mxArray **plhs, **plhs1;
  prhs[0] = mock_string("gppad_cas_obj");
  prhs[1] = dbl(d, "x", M * Tx); prhs[2] = dbl(d, "y", T); prhs[3] = dbl(d, "fftCovs", Tx);
  prhs[4] = dbl(d, "varx", vrows); prhs[5] = dbl(d, "mux", vrows); prhs[6] = dbl(d, "varc", 1); prhs[7] = mock_scalar(0);
  /* plhs has EXACTLY nlhs slots (heap, so that a sanitizer build sees a gateway that writes past them) */
  plhs = (mxArray**)malloc(2 * sizeof *plhs);
  mexFunction(2, plhs, 8, prhs);
  if (!same(d, "Obj", plhs[0], P, 1) || !same(d, "dObj", plhs[1], M * Tx, P)) return 1;
  plhs1 = (mxArray**)malloc(1 * sizeof *plhs1);             /* Obj = nagp_mex(...), the default device */
  mexFunction(1, plhs1, 7, prhs);
  if (mxGetNumberOfElements(plhs1[0]) != P || memcmp(mxGetPr(plhs1[0]), mxGetPr(plhs[0]), P * sizeof(double))) {
    printf("nlhs=1 call: Obj differs from the nlhs=2 call\n"); return 1; }
  printf("M %zu T %zu Tx %zu P %zu bit-equal\n", M, T, Tx, P);
  return 0;
}
