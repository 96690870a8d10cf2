/* mex_pstft_driver.c -- drives the 'pstft_obj' command of matlab/nagp_mex.c (compiled against the mock mex.h of this directory) with
 * the argument list matlab/get_Obj_pSTFT_*.m build, on dumped arrays: output sizes, and Obj / dObj bit for bit against the dumped
 * results of the Python call; a call with one output and the default device gives the same Obj.
 *   mex_pstft_driver <dump dir>        exit 0 = sizes right and every value bit-equal */
#include "dump.h"
#include "mex.h"

static mxArray* dbl(const char* d, const char* name, size_t rows) {
  size_t n; double* p = (double*)dump_load(d, name, 8, &n);
  mxArray* a = mock_numeric(mxDOUBLE_CLASS, rows, n / rows, p);
  free(p); return a;
}

int main(int argc, char** argv) {
  static const char* kernels[4] = {"exp", "matern32", "matern52", "matern72"};
  const char* d = argc > 1 ? argv[1] : ".";
  const size_t D = (size_t)dump_scalar(d, "D"), N = (size_t)dump_scalar(d, "N"), P = (size_t)dump_scalar(d, "P");
  const int kernel = (int)dump_scalar(d, "kernel"), form = (int)dump_scalar(d, "form");
  size_t n; double* e;
  const mxArray* prhs[11]; mxArray **plhs, **plhs1;
  prhs[0] = mock_string("pstft_obj");
  prhs[1] = mock_string(kernel >= 0 && kernel < 4 ? kernels[kernel] : "se");
  prhs[2] = mock_scalar(form);
  prhs[3] = dbl(d, "theta", 3 * D);
  prhs[4] = dbl(d, "vary", dump_count(d, "vary"));
  prhs[5] = dbl(d, "specTar", N);
  prhs[6] = dbl(d, "minVar", D);
  prhs[7] = dbl(d, "limOm", D); prhs[8] = dbl(d, "limLam", D);
  prhs[9] = dbl(d, "bet", dump_count(d, "bet"));
  prhs[10] = mock_scalar(0);
  /* plhs has EXACTLY nlhs slots (heap, so that a sanitizer build sees a gateway that writes past them) */
  plhs = (mxArray**)malloc(2 * sizeof *plhs);
  mexFunction(2, plhs, 11, prhs);
  if (mxGetNumberOfElements(plhs[0]) != P || mxGetM(plhs[0]) != P) { printf("Obj: wrong size\n"); return 1; }
  if (mxGetNumberOfElements(plhs[1]) != 3 * D * P || mxGetM(plhs[1]) != 3 * D) { printf("dObj: wrong size\n"); return 1; }
  e = (double*)dump_load(d, "Obj", 8, &n);
  if (n != P || rel_diff(mxGetPr(plhs[0]), e, n, "Obj") != 0.0 || memcmp(mxGetPr(plhs[0]), e, n * sizeof(double))) { printf("Obj: not bit-equal to the Python call\n"); return 1; }
  free(e);
  e = (double*)dump_load(d, "dObj", 8, &n);
  if (n != 3 * D * P || rel_diff(mxGetPr(plhs[1]), e, n, "dObj") != 0.0 || memcmp(mxGetPr(plhs[1]), e, n * sizeof(double))) { printf("dObj: not bit-equal to the Python call\n"); return 1; }
  free(e);
  plhs1 = (mxArray**)malloc(1 * sizeof *plhs1);           /* Obj = nagp_mex(...), 10 arguments (default device) */
  mexFunction(1, plhs1, 10, prhs);
  if (mxGetNumberOfElements(plhs1[0]) != P || memcmp(mxGetPr(plhs1[0]), mxGetPr(plhs[0]), P * sizeof(double))) {
    printf("nlhs=1 call: Obj differs from the nlhs=2 call\n"); return 1; }
  printf("D %zu N %zu P %zu bit-equal\n", D, N, P);
  return 0;
}
