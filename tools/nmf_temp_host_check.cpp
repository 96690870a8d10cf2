// nmf_temp_host_check.cpp -- the host-side checks of nagp_nmf_temp_create (csrc/nagp_nmf_temp_check.hpp: every NAGP_EINVAL /
// NAGP_EUNSUPPORTED line of include/nagp.h and the byte rule of the budget) as a stand-alone program on exactly-sized heap blocks, so
// that the host sanitizers see a read past an argument.  No device, no HIP runtime, nothing loaded into Python.  From the repository root:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -I nonstationary-audio-gp_amd/csrc \
//       -o /tmp/nmf_temp_host_check tools/nmf_temp_host_check.cpp && /tmp/nmf_temp_host_check
// (tests/test_nmf_temp_host.py builds and runs it.)
#include "nagp_nmf_temp_check.hpp"

#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

using namespace nagp;

static int bad = 0;
static char msg[512];

struct Args {
  int n = 2, D = 3, K = 2, prior = 2;
  int64_t T = 5;
  std::vector<double> A, vary, W, mu, vi, la;
  bool has_A = true, has_vary = true, has_W = false, has_mu = true, has_vi = true, has_la = true;
  size_t budget = (size_t)1 << 30;
  Args() { fill(); }
  void fill() {
    A.assign((size_t)T * D, 1.5); vary.assign((size_t)T * D, 0.2); W.assign((size_t)n * K * D, 0.3);
    mu.assign(K, 0.25); vi.assign(K, 0.0625); la.assign(K, 0.1);
  }
  int run(NmftShape* sh = nullptr) const {
    NmftShape local;
    // exactly-sized copies on the heap: a read past an argument is a heap-buffer-overflow
    auto copy = [](const std::vector<double>& v) { double* p = new double[v.size()]; std::memcpy(p, v.data(), v.size() * sizeof(double)); return p; };
    double *a = copy(A), *v = copy(vary), *w = copy(W), *m = copy(mu), *s = copy(vi), *l = copy(la);
    const int st = nmft_host_check(n, T, D, K, prior, has_A ? a : nullptr, has_vary ? v : nullptr, has_W ? w : nullptr, has_mu ? m : nullptr,
                                   has_vi ? s : nullptr, has_la ? l : nullptr, budget, sh ? sh : &local, msg, sizeof msg);
    delete[] a; delete[] v; delete[] w; delete[] m; delete[] s; delete[] l;
    return st;
  }
};

static void expect(const char* what, int got, int want) {
  if (got != want) { std::fprintf(stderr, "%s -> %d (%s), expected %d\n", what, got, msg, want); ++bad; }
}
#define EXPECT(mod, code) do { Args a; mod; expect(#mod, a.run(), code); } while (0)

int main() {
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  EXPECT((void)0, NMFT_OK);
  EXPECT(a.has_W = true, NMFT_OK);
  EXPECT((a.prior = 0, a.has_mu = a.has_vi = a.has_la = false), NMFT_OK);                 // no prior reads no parameter array
  EXPECT((a.prior = 1, a.has_mu = false), NMFT_OK);                                      // TG does not read muinf
  EXPECT(a.has_vary = false, NMFT_OK);
  EXPECT((a.prior = 1, a.la[1] = -3.0), NMFT_OK);                                        // lam is bounded for IG only
  EXPECT((a.la[0] = 0.0, a.la[1] = 1.0), NMFT_OK);
  EXPECT(a.has_A = false, NMFT_EINVAL);
  EXPECT(a.n = 0, NMFT_EINVAL); EXPECT(a.D = 0, NMFT_EINVAL); EXPECT(a.K = 0, NMFT_EINVAL); EXPECT(a.T = 0, NMFT_EINVAL);
  EXPECT(a.T = 1, NMFT_EINVAL);                                                          // a prior needs H(2,:)
  EXPECT((a.T = 1, a.prior = 0), NMFT_OK);
  EXPECT(a.prior = 3, NMFT_EINVAL); EXPECT(a.prior = -1, NMFT_EINVAL);
  EXPECT(a.D = 65, NMFT_EUNSUPPORTED); EXPECT(a.K = 17, NMFT_EUNSUPPORTED);              // decided on the sizes: the (too small) arrays are not read
  EXPECT(a.has_vi = false, NMFT_EINVAL); EXPECT(a.has_la = false, NMFT_EINVAL); EXPECT(a.has_mu = false, NMFT_EINVAL);
  EXPECT((a.prior = 1, a.has_vi = false), NMFT_EINVAL);
  for (double b : {nan, inf, -inf, -1e-9}) {
    EXPECT(a.A.back() = b, NMFT_EINVAL); EXPECT(a.vary.back() = b, NMFT_EINVAL);
    EXPECT((a.has_W = true, a.W.back() = b), NMFT_EINVAL);
  }
  for (double b : {nan, inf, -inf, 0.0, -1.0}) { EXPECT(a.vi.back() = b, NMFT_EINVAL); EXPECT(a.mu.back() = b, NMFT_EINVAL); }
  for (double b : {nan, inf, -inf, -1e-9, 1.0 + 1e-9}) EXPECT(a.la.back() = b, NMFT_EINVAL);
  EXPECT((a.prior = 1, a.la.back() = nan), NMFT_EINVAL);
  EXPECT((a.has_W = true, a.W[6 + 1] = a.W[6 + 3] = a.W[6 + 5] = 0.0), NMFT_EINVAL);     // row 1 of the second problem's W all zero
  EXPECT((a.has_W = true, a.W[6 + 1] = a.W[6 + 3] = 0.0), NMFT_OK);
  // the shape arithmetic and the byte rule: T = 1999, D = 16, K = 3, IG, learning form: nx = 6045, 8 workgroups, 16 sums each
  {
    Args a; a.T = 1999; a.D = 16; a.K = 3; a.n = 12; a.fill();
    NmftShape sh;
    expect("drivers' shape", a.run(&sh), NMFT_OK);
    if (sh.learn != 1 || sh.nwg != 8 || sh.n_po != 16 || sh.nx != 6045 || sh.per_problem != 8 * (2 * 6045 + 8 * (48 + 16) + 1)) { std::fprintf(stderr, "shape arithmetic\n"); ++bad; }
    a.has_W = true;
    expect("inference form", a.run(&sh), NMFT_OK);
    if (sh.learn != 0 || sh.nx != 5997 || sh.per_problem != 8 * (2 * 5997 + 8 * 16 + 1)) { std::fprintf(stderr, "shape arithmetic (inference form)\n"); ++bad; }
    a.budget = sh.per_problem; expect("exactly the budget", a.run(&sh), NMFT_OK);
    a.budget = sh.per_problem - 1; expect("one byte over", a.run(&sh), NMFT_EUNSUPPORTED);
  }
  if (bad) { std::fprintf(stderr, "%d unexpected statuses\n", bad); return 1; }
  std::printf("all host checks returned their status\n");
  return 0;
}
