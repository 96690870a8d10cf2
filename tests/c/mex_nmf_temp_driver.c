/* mex_nmf_temp_driver.c -- drives the 'nmf_temp_obj' command of matlab/nagp_mex.c (compiled against the mock mex.h of this directory)
 * with the argument list matlab/getObj_nmf_temp.m and getObj_nmf_temp_inf.m build, on dumped arrays: output sizes, and Obj / dObj bit
 * for bit against the dumped results of the Python call; a call with one output and the default device gives the same Obj.  An array
 * dumped with no entries is passed as [].
 *   mex_nmf_temp_driver <dump dir>        exit 0 = sizes right and every value bit-equal */
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

int main(int argc, char** argv) {
  const char* d = argc > 1 ? argv[1] : ".";
  const size_t X = (size_t)dump_scalar(d, "X"), T = (size_t)dump_scalar(d, "T"), K = (size_t)dump_scalar(d, "K"), P = (size_t)dump_scalar(d, "P");
  size_t n; double* e;
  const mxArray* prhs[9]; mxArray **plhs, **plhs1;
  prhs[0] = mock_string("nmf_temp_obj");
  prhs[1] = dbl(d, "x", X);
  prhs[2] = dbl(d, "A", T);
  prhs[3] = dbl(d, "vary", T);
  prhs[4] = dbl(d, "W", K);
  prhs[5] = dbl(d, "muinf", 1);
  prhs[6] = dbl(d, "varinf", 1);
  prhs[7] = dbl(d, "lam", 1);
  prhs[8] = mock_scalar(0);
  /* plhs has EXACTLY nlhs slots (heap, so that a sanitizer build sees a gateway that writes past them) */
  plhs = (mxArray**)malloc(2 * sizeof *plhs);
  mexFunction(2, plhs, 9, prhs);
  if (mxGetNumberOfElements(plhs[0]) != P || mxGetM(plhs[0]) != P) { printf("Obj: wrong size\n"); return 1; }
  if (mxGetNumberOfElements(plhs[1]) != X * P || mxGetM(plhs[1]) != X) { printf("dObj: wrong size\n"); return 1; }
  e = (double*)dump_load(d, "Obj", 8, &n);
  if (n != P || rel_diff(mxGetPr(plhs[0]), e, n, "Obj") != 0.0 || memcmp(mxGetPr(plhs[0]), e, n * sizeof(double))) { printf("Obj: not bit-equal to the Python call\n"); return 1; }
  free(e);
  e = (double*)dump_load(d, "dObj", 8, &n);
  if (n != X * P || rel_diff(mxGetPr(plhs[1]), e, n, "dObj") != 0.0 || memcmp(mxGetPr(plhs[1]), e, n * sizeof(double))) { printf("dObj: not bit-equal to the Python call\n"); return 1; }
  free(e);
  plhs1 = (mxArray**)malloc(1 * sizeof *plhs1);           /* Obj = nagp_mex(...), 8 arguments (default device) */
  mexFunction(1, plhs1, 8, prhs);
  if (mxGetNumberOfElements(plhs1[0]) != P || memcmp(mxGetPr(plhs1[0]), mxGetPr(plhs[0]), P * sizeof(double))) {
    printf("nlhs=1 call: Obj differs from the nlhs=2 call\n"); return 1; }
  printf("X %zu T %zu P %zu bit-equal\n", X, T, P);
  return 0;
}
