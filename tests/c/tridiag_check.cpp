// tridiag_check.cpp -- the symmetric tridiagonal eigen-solver of csrc/nagp_tridiag.hpp (implicit QL) as a stand-alone program under the
// host sanitizers.  argv[1]: a raw float64 file  n | d (n) | e (n, e[0] unused);  argv[2]: the output  eigenvalues (n) | last row of the
// eigenvector matrix from the one-row run (n) | the eigenvector matrix from the full run (n x n, row-major).  Besides, for the same n,
// the (2, -1) matrix against its closed form 2 - 2 cos(k pi / (n + 1)): the largest error is printed and must stay below 1e-14 n.
// Built and run by tests/test_gppad_lap_host.py, which compares the output with numpy.linalg.eigh.
#include "nagp_tridiag.hpp"
#include <cstdio>
using namespace nagp;

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  FILE* fi = fopen(argv[1], "rb"); if (!fi) return 2;
  double nd; if (fread(&nd, 8, 1, fi) != 1) return 2;
  const int n = (int)nd;
  std::vector<double> d(n), e(n);
  if (fread(d.data(), 8, n, fi) != (size_t)n || fread(e.data(), 8, n, fi) != (size_t)n) return 2;
  fclose(fi);
  std::vector<double> d1 = d, e1 = e, last(n, 0.0), d2 = d, e2 = e, Z((size_t)n * n, 0.0);
  last[n - 1] = 1.0;
  for (int i = 0; i < n; ++i) Z[(size_t)i * n + i] = 1.0;
  if (!tridiag_ql(n, d1.data(), e1.data(), last.data(), 1) || !tridiag_ql(n, d2.data(), e2.data(), Z.data(), n)) { printf("no convergence\n"); return 1; }
  for (int i = 0; i < n; ++i) if (d1[i] != d2[i]) { printf("the one-row run and the full run differ at %d\n", i); return 1; }
  FILE* fo = fopen(argv[2], "wb"); if (!fo) return 2;
  fwrite(d1.data(), 8, n, fo); fwrite(last.data(), 8, n, fo); fwrite(Z.data(), 8, (size_t)n * n, fo);
  fclose(fo);
  std::vector<double> td(n, 2.0), te(n, -1.0), none(1);
  if (!tridiag_ql(n, td.data(), te.data(), none.data(), 0)) { printf("no convergence\n"); return 1; }
  const long double pi = 3.14159265358979323846264338327950288L;
  double worst = 0.0;
  for (int k = 1; k <= n; ++k) worst = std::max(worst, (double)fabsl((long double)td[k - 1] - (2 - 2 * cosl(k * pi / (n + 1)))));
  printf("n %d toeplitz error %.3e\n", n, worst);
  if (!(worst < 1e-14 * n)) return 1;
  double bad[3] = {1.0, NAN, 2.0}, be[3] = {0.0, 0.5, 0.5};
  if (tridiag_ql(3, bad, be, none.data(), 0)) { printf("a NaN entry was not refused\n"); return 1; }
  printf("ok\n");
  return 0;
}
