// gppad_cas_host_check.cpp -- runs the kernel bodies of the cascade form of csrc/nagp_gppad.hpp (gppad_cas_pre_body, the V = 1 transform
// bodies, gppad_cas_finish_item) on the CPU, one "thread" per workgroup (barriers and the wave butterfly fall away), at the shapes of the
// fixture of tests/gppad_cas_ref.py, two cascades each (the second with the spectra shared, ic_stride = 0, on the 'given' shape), against
// plain long double loops around a radix-2 FFT: the index arithmetic of cascade / column / sample, of D and partA and of the shared
// spectra without a device.  Every buffer is a heap block of exactly the size the entry points allocate, so the host AddressSanitizer
// sees an index past it.  Built with -Xarch_host -fsanitize=address,undefined and run by tests/test_gppad_cas_host.py.
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
static long double ampl(long double x) { return x > 500 ? x : (x < -30 ? expl(x) : logl(1 + expl(x))); }

struct Shape { int M; int64_t T, Tx; bool shared, specials; };

int main() {
  const long double pi = 3.14159265358979323846264338327950288L;
  const Shape shapes[] = {{1, 1, 2, false, false}, {2, 64, 64, false, false}, {3, 40, 64, false, false}, {8, 100, 128, false, false},
                          {2, 3000, 4096, false, false}, {3, 5000, 8192, false, false}, {3, 200, 256, true, false}, {2, 100, 128, false, true}};
  int bad = 0;
  for (const Shape& sh : shapes) {
    const int M = sh.M, nc = 2, nq = nc * M;
    const int64_t T = sh.T, Tx = sh.Tx;
    std::mt19937_64 g((unsigned)(M * 131 + Tx));
    std::normal_distribution<double> nd;
    std::vector<double> x((size_t)nq * Tx), y((size_t)nc * T), len(nq), varx(nq), mux(nq), varc = {0.8, 1.7};
    for (auto& v : x) v = 0.3 + nd(g);
    for (auto& v : y) v = nd(g);
    for (int q = 0; q < nq; ++q) { len[q] = sh.shared ? 2.0 * (1 << (3 * (q % M))) : 0.7 + (double)Tx / 16 * (q % M) / M + 0.1 * (q / M); varx[q] = 1.2 - 0.05 * q; mux[q] = 0.4 - 0.1 * q; }
    if (sh.specials) { x[5] = -35; y[5] = 0; x[Tx + 17] = 0; x[40] = 600; x[(size_t)(M + 1) * Tx + 41] = 600; }
    std::vector<double2> tw(Tx);
    for (int64_t m = 0; m < Tx; ++m) tw[m] = make_double2((double)cosl(2 * pi * m / Tx), (double)-sinl(2 * pi * m / Tx));
    GppadPar p{};
    p.T = T; p.Tx = Tx; p.M = M;
    if (Tx > GPPAD_TILE) { p.N2 = GPPAD_TILE; p.N1 = (int)(Tx / GPPAD_TILE); p.lcb = GPPAD_LOG_TILE - gp_log2(p.N1); p.nwg = p.N1; }
    else { p.N1 = 1; p.N2 = (int)Tx; p.nwg = 1; }
    p.nwgA = gppad_cas_nwg(T);
    const size_t n_ic = (size_t)(sh.shared ? M : nq) * Tx;
    std::vector<double> ic((size_t)nq * Tx), dObj((size_t)nq * Tx), part((size_t)nq * p.nwg * 2), Obj(nc), D((size_t)nc * T), partA((size_t)nc * p.nwgA * 2);
    std::vector<double2> work(p.N1 > 1 ? (size_t)nq * Tx : 0);
    std::vector<double2> lds(gppad_lds_points(Tx));
    double red[16];
    p.grad = 1; p.x = x.data(); p.y = y.data(); p.ic_stride = Tx; p.varx = varx.data(); p.mux = mux.data(); p.varc = varc.data(); p.tw = tw.data();
    p.work = work.data(); p.part = part.data(); p.Obj = Obj.data(); p.dObj = dObj.data(); p.len = len.data(); p.ic_out = ic.data(); p.D = D.data(); p.partA = partA.data();
    for (int q = 0; q < nq; ++q) for (int64_t e = 0; e < Tx; ++e) gppad_cov_item(p, q, e);
    std::vector<double> ics(ic.begin(), ic.begin() + (long)n_ic);      // shared: the M spectra of the first cascade, exactly M x Tx
    p.ic = ics.data(); p.ic_stride = sh.shared ? 0 : Tx;
    for (int c = 0; c < nc; ++c) for (int b = 0; b < p.nwgA; ++b) gppad_cas_pre_body(p, c, b, 0, 1, red);
    for (int q = 0; q < nq; ++q) {
      if (p.N1 == 1) gppad_lds_body<1>(p, q, 0, 1, lds.data(), red);
      else {
        for (int b = 0; b < p.N1; ++b) gppad_colf_body(p, q, b, 0, 1, lds.data());
        for (int b = 0; b < p.N1; ++b) gppad_row_body<1>(p, q, b, 0, 1, lds.data());
        for (int b = 0; b < p.N1; ++b) gppad_coli_body<1>(p, q, b, 0, 1, lds.data(), red);
      }
    }
    for (int c = 0; c < nc; ++c) gppad_cas_finish_item(p, c);
    // reference: plain loops
    for (int c = 0; c < nc; ++c) {
      long double O = 0, quad = 0, md = 0, mr = 0;
      std::vector<long double> Dl(T);
      for (int64_t t = 0; t < T; ++t) {
        long double P = 1;
        for (int m = 0; m < M; ++m) { const long double a = ampl(x[(size_t)(c * M + m) * Tx + t]); P *= a; O += logl(a); }
        const long double yy = y[(size_t)c * T + t];
        quad += yy * yy / (P * P) / 2; Dl[t] = 1 - yy * yy / (varc[c] * P * P);
      }
      O += quad / varc[c];
      {   // x is white, so ObjB and u dominate Obj and dObj: the likelihood's own pieces, ObjA from partA and D, are compared by themselves
        double sl = 0, sq = 0; long double mD = 0, rD = 0;
        for (int w = 0; w < p.nwgA; ++w) { sl += partA[((size_t)c * p.nwgA + w) * 2]; sq += partA[((size_t)c * p.nwgA + w) * 2 + 1]; }
        for (int64_t t = 0; t < T; ++t) { mD = std::max(mD, fabsl(Dl[t] - D[(size_t)c * T + t])); rD = std::max(rD, fabsl(Dl[t])); }
        const double ea = (double)(fabsl(O - (sl + sq / varc[c])) / fabsl(O)), eD = (double)(mD / rD);
        printf("M=%d T=%lld Tx=%lld cascade %d  err ObjA %.2e D %.2e\n", M, (long long)T, (long long)Tx, c, ea, eD);
        if (!(ea < 1e-13) || !(eD < 1e-13)) ++bad;
      }
      for (int m = 0; m < M; ++m) {
        const int q = c * M + m;
        const long double L = len[sh.shared ? m : q];
        std::vector<cl> a(Tx);
        for (int64_t e = 0; e < Tx; ++e) a[e] = (long double)x[(size_t)q * Tx + e] - (long double)mux[q];
        fftl(a, 1);
        for (int64_t k = 0; k < Tx; ++k) {
          long double f = k <= Tx / 2 ? k : k - Tx, om = 2 * pi * f / Tx;
          a[k] /= sqrtl(2 * pi * L * L) * expl(-om * om * L * L / 2) + 1e-6L;
        }
        fftl(a, -1);
        long double ob = 0;
        for (int64_t e = 0; e < Tx; ++e) {
          const long double u = a[e].real() / Tx, xx = x[(size_t)q * Tx + e];
          ob += u * (xx - mux[q]);
          long double gd = u / varx[q];
          if (e < T) gd += 1 / (1 + expl(-xx)) / ampl(xx) * Dl[e];
          md = std::max(md, fabsl(gd - dObj[(size_t)q * Tx + e])); mr = std::max(mr, fabsl(gd));
        }
        O += ob / (2 * varx[q]);
      }
      const double eo = (double)(fabsl(O - Obj[c]) / fabsl(O)), ed = (double)(md / mr);
      printf("M=%d T=%lld Tx=%lld cascade %d  Obj %.17g  err Obj %.2e dObj %.2e\n", M, (long long)T, (long long)Tx, c, Obj[c], eo, ed);
      if (!(eo < 1e-11) || !(ed < 1e-11)) ++bad;
    }
  }
  printf(bad ? "FAILED %d\n" : "ok\n", bad);
  return bad != 0;
}
