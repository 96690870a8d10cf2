// gppad_host_check.cpp -- runs the kernel bodies of csrc/nagp_gppad.hpp on the CPU, one "thread" per workgroup (barriers and the wave
// butterfly fall away), for Tx = 2^1 .. 2^14 and 2^17 with two problems each (entries 800, 501, -31, -40 among x, per-sample vary, len = 0.7
// and Tx / 8), against a long double radix-2 FFT: the index arithmetic of the LDS passes, of the four-step split and of the permuted 1 / c
// without a device.  The "LDS" is a heap block of exactly the size the kernels ask for, so a host AddressSanitizer build sees an index
// past it.  Not part of the test suite (the compile takes half a minute); from the repository root:
//   hipcc -x hip --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address -fsanitize=address \
//         -I nonstationary-audio-gp_amd/csrc -o /tmp/gppad_host_check tools/gppad_host_check.cpp && /tmp/gppad_host_check
#include "nagp_gppad.hpp"
#include <vector>
#include <complex>
#include <cstdio>
#include <cmath>
#include <random>
using namespace nagp;
typedef std::complex<long double> cl;
static void fftl(std::vector<cl>& a, int dir) {
  size_t n = a.size(); if (n == 1) return;
  std::vector<cl> e(n / 2), o(n / 2);
  for (size_t i = 0; i < n / 2; ++i) { e[i] = a[2 * i]; o[i] = a[2 * i + 1]; }
  fftl(e, dir); fftl(o, dir);
  const long double pi = 3.14159265358979323846264338327950288L;
  for (size_t k = 0; k < n / 2; ++k) { cl w = std::polar(1.0L, -dir * 2 * pi * k / n) * o[k]; a[k] = e[k] + w; a[k + n / 2] = e[k] - w; }
}
int main() {
  const long double pi = 3.14159265358979323846264338327950288L;
  int bad = 0;
  for (int l = 1; l <= 20; ++l) {
    if (l > 14 && l != 17) continue;
    const int64_t Tx = (int64_t)1 << l, T = std::max<int64_t>(1, (int64_t)(0.64 * Tx));
    const int np = 2;
    std::mt19937_64 g(l);
    std::normal_distribution<double> nd;
    std::vector<double> x(np * Tx), y(np * T), vary(np * T), len = {0.7, (double)Tx / 8}, varx = {1.3, 0.4}, mux = {-0.3, 0.2}, varc = {0.9, 2.0};
    for (auto& v : x) v = nd(g); for (auto& v : y) v = nd(g); for (auto& v : vary) v = std::fabs(nd(g));
    x[0] = 800; if (Tx > 4) { x[1] = -40; x[Tx + 2] = 501; x[Tx + 3] = -31; }
    std::vector<double2> tw(Tx);
    for (int64_t m = 0; m < Tx; ++m) tw[m] = make_double2((double)cosl(2 * pi * m / Tx), (double)-sinl(2 * pi * m / Tx));
    GppadPar p{};
    p.T = T; p.Tx = Tx;
    if (Tx > GPPAD_TILE) { p.N2 = GPPAD_TILE; p.N1 = (int)(Tx / GPPAD_TILE); p.lcb = GPPAD_LOG_TILE - gp_log2(p.N1); p.nwg = p.N1; }
    else { p.N1 = 1; p.N2 = (int)Tx; p.nwg = 1; }
    std::vector<double> ic(np * Tx), dObj(np * Tx), part(np * p.nwg * 2), Obj(np);
    std::vector<double2> work(np * Tx);
    std::vector<double2> lds(gppad_lds_points(Tx));
    double red[16];
    p.grad = 1; p.x = x.data(); p.y = y.data(); p.vary = vary.data(); p.vary_stride = T; p.ic = ic.data(); p.ic_stride = Tx;
    p.varx = varx.data(); p.mux = mux.data(); p.varc = varc.data(); p.tw = tw.data(); p.work = work.data(); p.part = part.data();
    p.Obj = Obj.data(); p.dObj = dObj.data(); p.len = len.data(); p.ic_out = ic.data();
    for (int q = 0; q < np; ++q) {
      for (int64_t e = 0; e < Tx; ++e) gppad_cov_item(p, q, e);
      if (p.N1 == 1) gppad_lds_body(p, q, 0, 1, lds.data(), red);
      else {
        for (int b = 0; b < p.N1; ++b) gppad_colf_body(p, q, b, 0, 1, lds.data());
        for (int b = 0; b < p.N1; ++b) gppad_row_body(p, q, b, 0, 1, lds.data());
        for (int b = 0; b < p.N1; ++b) gppad_coli_body(p, q, b, 0, 1, lds.data(), red);
      }
      gppad_finish_item(p, q);
      // reference
      std::vector<cl> a(Tx);
      for (int64_t e = 0; e < Tx; ++e) a[e] = (long double)x[q * Tx + e] - (long double)mux[q];
      fftl(a, 1);
      for (int64_t k = 0; k < Tx; ++k) {
        long double f = k <= Tx / 2 ? k : k - Tx, om = 2 * pi * f / Tx, L = len[q];
        a[k] /= sqrtl(2 * pi * L * L) * expl(-om * om * L * L / 2) + 1e-6L;
      }
      fftl(a, -1);
      long double oa = 0, ob = 0, md = 0, mr = 0;
      for (int64_t e = 0; e < Tx; ++e) {
        long double u = a[e].real() / Tx, xx = x[q * Tx + e];
        ob += u * (xx - mux[q]);
        long double gd = u / varx[q];
        if (e < T) {
          long double am = xx > 500 ? xx : (xx < -30 ? expl(xx) : logl(1 + expl(xx))), s = 1 / (1 + expl(-xx));
          long double v = am * am * varc[q] + vary[q * T + e] + 1e-5L, yy = y[q * T + e];
          oa += 0.5L * logl(v) + 0.5L * yy * yy / v;
          gd += s * am / v * (1 - yy * yy / v) * varc[q];
        }
        md = std::max(md, fabsl(gd - dObj[q * Tx + e])); mr = std::max(mr, fabsl(gd));
      }
      long double O = oa + ob / (2 * varx[q]);
      double eo = (double)(fabsl(O - Obj[q]) / fabsl(O)), ed = (double)(md / mr);
      printf("Tx=2^%d prob %d  Obj %.17g  err Obj %.2e dObj %.2e\n", l, q, Obj[q], eo, ed);
      if (!(eo < 1e-12) || !(ed < 1e-12)) ++bad;
    }
  }
  printf(bad ? "FAILED %d\n" : "ok\n", bad);
  return bad != 0;
}
