/* mex_recon_driver.c -- drives the 'reconstruct_sources' command of matlab/nagp_mex.c (compiled against the mock mex.h of this
 * directory) on dumped marginals: the options struct matlab/nagp_reconstruct_sources.m builds, output sizes, values against the dumped
 * results of the Python call; a call with fewer outputs gives the same leading outputs.
 *   mex_recon_driver <dump dir>        exit 0 = sizes right and values within 1e-12 */
#include "dump.h"
#include "mex.h"

static mxArray* dbl(const char* d, const char* name, size_t rows) {
  size_t n; double* p = (double*)dump_load(d, name, 8, &n);
  mxArray* a = mock_numeric(mxDOUBLE_CLASS, rows ? rows : 1, rows ? n / rows : n, p);
  free(p); return a;
}

int main(int argc, char** argv) {
  const char* d = argc > 1 ? argv[1] : ".";
  static const char* names[7] = {"Esig", "Vsig", "Esrc", "Vsrc", "Eenv", "Eft_mod", "Varft_mod"};
  const size_t D = (size_t)dump_scalar(d, "D"), N = (size_t)dump_scalar(d, "N");
  size_t n, J, T, rows[7], i; double worst = 0.0, r;
  int32_t* off = (int32_t*)dump_load(d, "source_offsets", 4, &n);
  mxArray* o = mock_struct(); const mxArray* prhs[5]; mxArray **plhs, **plhs3;
  J = n - 1;
  prhs[0] = mock_string("reconstruct_sources"); prhs[1] = dbl(d, "Eft", D + N); prhs[2] = dbl(d, "Varft", D + N); prhs[3] = dbl(d, "Wnmf", D); prhs[4] = o;
  T = mxGetNumberOfElements(prhs[1]) / (D + N);
  mock_set(o, "amp_kind", mock_scalar(dump_scalar(d, "amp_kind"))); mock_set(o, "link_kind", mock_scalar(dump_scalar(d, "link_kind")));
  mock_set(o, "link_shift", mock_scalar(dump_scalar(d, "link_shift")));
  mock_set(o, "source_offsets", mock_numeric(mxINT32_CLASS, 1, n, off));
  mock_set(o, "n_samples", mock_scalar(dump_scalar(d, "n_samples"))); mock_set(o, "seed", mock_scalar(dump_scalar(d, "seed")));
  mock_set(o, "device", mock_scalar(0));
  if (dump_scalar(d, "n_samples") == 0) {
    mock_set(o, "gh_x", dbl(d, "gh_x", 0)); mock_set(o, "gh_w", dbl(d, "gh_w", 0));
    mock_set(o, "wn", dbl(d, "wn", 0)); mock_set(o, "xn_unscaled", dbl(d, "xn_unscaled", N));
  }
  /* plhs has EXACTLY nlhs slots (heap, so that a sanitizer build sees a gateway that writes past them) */
  plhs = (mxArray**)malloc(7 * sizeof *plhs);
  mexFunction(7, plhs, 5, prhs);
  rows[0] = rows[1] = 1; rows[2] = rows[3] = J; rows[4] = D; rows[5] = rows[6] = N;
  for (i = 0; i < 7; ++i) {
    double* e;
    if (mxGetM(plhs[i]) != rows[i] || mxGetNumberOfElements(plhs[i]) != rows[i] * T) { printf("%s: wrong size\n", names[i]); return 1; }
    e = (double*)dump_load(d, names[i], 8, &n);
    if (n != rows[i] * T) { printf("%s: dump has %zu entries\n", names[i], n); return 1; }
    r = rel_diff(mxGetPr(plhs[i]), e, n, names[i]); if (r > worst) worst = r;
    free(e);
  }
  plhs3 = (mxArray**)malloc(3 * sizeof *plhs3);           /* [Esig, Vsig, Esrc] = nagp_mex(...) */
  mexFunction(3, plhs3, 5, prhs);
  for (i = 0; i < 3; ++i)
    if (mxGetNumberOfElements(plhs3[i]) != rows[i] * T || memcmp(mxGetPr(plhs3[i]), mxGetPr(plhs[i]), rows[i] * T * sizeof(double))) {
      printf("nlhs=3 call: %s differs from the nlhs=7 call\n", names[i]); return 1; }
  printf("D %zu N %zu J %zu T %zu worst %.3e\n", D, N, J, T, worst);
  return worst < 1e-12 ? 0 : 1;
}
