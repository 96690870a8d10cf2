/* mex_grad_driver.c -- drives the 'giekf_grad' command of matlab/nagp_mex.c (compiled against the mock mex.h of this directory) with
 * the argument list matlab/gf_giekf_modulator_nmf_constraints.m builds, on dumped inputs: output sizes, values against the dumped
 * results of the Python call; a call with one output (and the default device) gives the same energy.
 *   mex_grad_driver <dump dir>        exit 0 = sizes right and values within 1e-12 */
#include "dump.h"
#include "mex.h"

static mxArray* dbl(const char* d, const char* name, size_t rows) {
  size_t n; double* p = (double*)dump_load(d, name, 8, &n);
  mxArray* a = mock_numeric(mxDOUBLE_CLASS, rows ? rows : 1, rows ? n / rows : n, p);
  free(p); return a;
}
static mxArray* i32(const char* d, const char* name) {
  size_t n; int32_t* p = (int32_t*)dump_load(d, name, 4, &n);
  mxArray* a = mock_numeric(mxINT32_CLASS, 1, n, p);
  free(p); return a;
}

int main(int argc, char** argv) {
  const char* d = argc > 1 ? argv[1] : ".";
  const size_t S = (size_t)dump_scalar(d, "S"), D = (size_t)dump_scalar(d, "D");
  size_t n, np_; double worst, r, *e, *g;
  mxArray* model = mock_struct(); const mxArray* prhs[11]; mxArray **plhs, **plhs1;
  mock_set(model, "A", dbl(d, "A", S)); mock_set(model, "Q", dbl(d, "Q", S)); mock_set(model, "Pinf", dbl(d, "Pinf", S));
  mock_set(model, "h_val", dbl(d, "h_val", 0)); mock_set(model, "block_offsets", i32(d, "block_offsets"));
  mock_set(model, "Wnmf", dbl(d, "Wnmf", D)); mock_set(model, "D", mock_scalar((double)D)); mock_set(model, "N", mock_scalar(dump_scalar(d, "N")));
  mock_set(model, "lik_param", mock_scalar(dump_scalar(d, "lik_param")));
  prhs[0] = mock_string("giekf_grad"); prhs[1] = model; prhs[2] = dbl(d, "y", 0);
  prhs[3] = dbl(d, "dA", S); prhs[4] = dbl(d, "dQ", S); prhs[5] = dbl(d, "dPinf", S); prhs[6] = dbl(d, "dR", 0);
  prhs[7] = i32(d, "hess"); prhs[8] = i32(d, "w_index"); prhs[9] = i32(d, "w_direct"); prhs[10] = mock_scalar(0);
  np_ = mxGetNumberOfElements(prhs[6]);
  /* plhs has EXACTLY nlhs slots (heap, so that a sanitizer build sees a gateway that writes past them) */
  plhs = (mxArray**)malloc(2 * sizeof *plhs);
  mexFunction(2, plhs, 11, prhs);
  if (mxGetNumberOfElements(plhs[0]) != 1 || mxGetM(plhs[1]) != 1 || mxGetNumberOfElements(plhs[1]) != np_) { printf("wrong output sizes\n"); return 1; }
  e = (double*)dump_load(d, "e", 8, &n); if (n != 1) { printf("e: dump has %zu entries\n", n); return 1; }
  g = (double*)dump_load(d, "g", 8, &n); if (n != np_) { printf("g: dump has %zu entries\n", n); return 1; }
  worst = rel_diff(mxGetPr(plhs[0]), e, 1, "e");
  r = rel_diff(mxGetPr(plhs[1]), g, np_, "g"); if (r > worst) worst = r;
  plhs1 = (mxArray**)malloc(1 * sizeof *plhs1);           /* e = nagp_mex(...), 10 arguments (default device) */
  mexFunction(1, plhs1, 10, prhs);
  if (mxGetNumberOfElements(plhs1[0]) != 1 || memcmp(mxGetPr(plhs1[0]), mxGetPr(plhs[0]), sizeof(double))) {
    printf("nlhs=1 call: e differs from the nlhs=2 call\n"); return 1; }
  printf("S %zu n_param %zu worst %.3e\n", S, np_, worst);
  free(e); free(g);
  return worst < 1e-12 ? 0 : 1;
}
