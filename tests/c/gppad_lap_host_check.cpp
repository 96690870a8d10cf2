// gppad_lap_host_check.cpp -- runs the kernel bodies of csrc/nagp_gppad_lap.hpp on the CPU, one "thread" per workgroup (barriers and the
// wave butterfly fall away), in the sequence nagp_gppad_lap_hess / _apply / _eig / _varx launch them, with the Lanczos control of
// csrc/nagp_tridiag.hpp: a device batch of two problems (the case, and the same model started from the reversed vstart with nev - 1, so
// that the two stop at different steps and the mask is used).  Every buffer is a heap block of exactly the size the entry points
// allocate, so the host AddressSanitizer sees an index past it.  Input (argv[1]) and output (argv[2]) are raw float64 files:
//   in:  T Tx nev jmax len varx mux varc vary | x (Tx) | y (T) | vstart (Tx)
//   out: per problem: steps reorths nconv status anorm | lmb (jmax) | then for problem 0: d (T) | A vstart (Tx) | Varx (Tx) | xv (nconv x Tx)
// Built with -Xarch_host -fsanitize=address,undefined and run by tests/test_gppad_lap_host.py, which compares with tests/gppad_lap_ref.py.
#include "nagp_gppad_lap.hpp"
#include "nagp_tridiag.hpp"
#include "nagp_api_layout.hpp"
#include <cstdio>
#include <vector>
using namespace nagp;

struct Host {
  int nb, N1, N2, lcb, nwe, np, jmax; int64_t T, Tx;
  std::vector<double> g, d, x, y, vary, varx, varc, len, zeros, flag, part, al, be, sc, h1, S, lam, V, XV, r, tmp, Varx;
  std::vector<double2> tw, work, lds;
  double red[16];
  LapPar par() {
    LapPar p{};
    p.T = T; p.Tx = Tx; p.N1 = N1; p.N2 = N2; p.lcb = lcb; p.nb = nb; p.jmax = jmax; p.np = 1; p.ss = 1; p.lev = 1.0;
    p.flag = flag.data(); p.g = g.data(); p.tw = tw.data(); p.work = work.data(); p.d = d.data(); p.part = part.data(); p.h1 = h1.data(); p.S = S.data();
    p.q = V.data(); p.x = x.data(); p.y = y.data(); p.vary = vary.data(); p.varx = varx.data(); p.varc = varc.data(); p.len = len.data();
    return p;
  }
  template <int E> void sandwich(const LapPar& p) {
    if (N1 == 1) { for (int q = 0; q < nb; ++q) lap_lds_body<E>(p, q, 0, 1, lds.data(), red); return; }
    GppadPar gp{};
    gp.T = T; gp.Tx = Tx; gp.N1 = N1; gp.N2 = N2; gp.lcb = lcb; gp.nwg = N1; gp.tw = tw.data(); gp.x = p.in; gp.mux = zeros.data(); gp.ic = p.g; gp.ic_stride = Tx; gp.work = work.data();
    for (int q = 0; q < nb; ++q) for (int b = 0; b < N1; ++b) gppad_colf_body(gp, q, b, 0, 1, lds.data());
    for (int q = 0; q < nb; ++q) for (int b = 0; b < N1; ++b) gppad_row_body<0>(gp, q, b, 0, 1, lds.data());
    for (int q = 0; q < nb; ++q) for (int b = 0; b < N1; ++b) lap_coli_body<E>(p, q, b, 0, 1, lds.data(), red);
  }
  void update(LapPar p) { p.out = r.data(); p.np = nwe; for (int q = 0; q < nb; ++q) for (int b = 0; b < nwe; ++b) lap_update_body(p, q, b, 0, 1, red); }
  void norm_of_r(LapPar p) { update(p); p.np = nwe; p.root = 1; p.res = be.data(); for (int q = 0; q < nb; ++q) lap_finish_item(p, q); }
};

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  FILE* fi = fopen(argv[1], "rb"); if (!fi) return 2;
  double hd[9]; if (fread(hd, 8, 9, fi) != 9) return 2;
  Host H;
  const int64_t T = (int64_t)hd[0], Tx = (int64_t)hd[1]; const int nev = (int)hd[2], jmax = (int)hd[3], nb = 2;
  H.nb = nb; H.T = T; H.Tx = Tx; H.jmax = jmax;
  if (Tx > GPPAD_TILE) { H.N2 = GPPAD_TILE; H.N1 = (int)(Tx / GPPAD_TILE); H.lcb = GPPAD_LOG_TILE - gp_log2(H.N1); } else { H.N1 = 1; H.N2 = (int)Tx; H.lcb = 0; }
  H.nwe = lap_nwe(Tx); H.np = std::max(H.nwe, H.N1);
  const size_t Txz = (size_t)Tx, Tz = (size_t)T, jz = (size_t)jmax, slot = (size_t)nb * Txz;
  const LapBat lb = lap_bat(Txz, jz, H.N1 > 1, (size_t)H.np, (size_t)nb);
  std::vector<double> x0(Txz), y0(Tz), v0(Txz);
  if (fread(x0.data(), 8, Txz, fi) != Txz || fread(y0.data(), 8, Tz, fi) != Tz || fread(v0.data(), 8, Txz, fi) != Txz) return 2;
  fclose(fi);
  H.x.resize(slot); H.y.resize(nb * Tz); H.r.resize(slot); H.tmp.resize(slot); H.g.resize(slot); H.d.resize(nb * Tz); H.Varx.resize(slot);
  H.V.resize(jz * slot); H.XV.resize(jz * slot); H.work.resize(H.N1 > 1 ? slot : 0); H.lds.resize(gppad_lds_points(Tx));
  H.part.resize(lb.al - lb.pt); H.al.resize(nb); H.be.resize(nb); H.sc.resize(2 * nb); H.h1.resize(lb.S - lb.h1); H.S.assign(lb.lam - lb.S, 0.0); H.lam.resize(lb.ob - lb.lam);
  H.flag.assign(nb, 1.0); H.zeros.assign(nb, 0.0);
  H.vary.assign(nb, hd[8]); H.varx.assign(nb, hd[5]); H.varc.assign(nb, hd[7]); H.len.assign(nb, hd[4]);
  for (int q = 0; q < nb; ++q) {
    std::copy(x0.begin(), x0.end(), H.x.begin() + q * Txz); std::copy(y0.begin(), y0.end(), H.y.begin() + q * Tz);
    for (size_t e = 0; e < Txz; ++e) H.r[q * Txz + e] = q ? v0[Txz - 1 - e] : v0[e];
  }
  const long double pi = 3.14159265358979323846264338327950288L;
  H.tw.resize(Txz);
  for (int64_t m = 0; m < Tx; ++m) H.tw[m] = make_double2((double)cosl(2 * pi * m / Tx), (double)-sinl(2 * pi * m / Tx));
  { LapPar p = H.par(); p.out = H.g.data(); for (int q = 0; q < nb; ++q) for (int64_t e = 0; e < Tx; ++e) lap_spec_item(p, q, e); }
  { LapPar p = H.par(); p.out = H.d.data(); for (int q = 0; q < nb; ++q) for (int64_t t = 0; t < T; ++t) lap_hess_item(p, q, t); }
  // A vstart (nagp_gppad_lap_apply), left in tmp2
  std::vector<double> Av(slot);
  { LapPar p = H.par(); p.in = H.r.data(); p.out = H.tmp.data(); H.sandwich<1>(p); p.in = H.tmp.data(); p.out = Av.data(); H.sandwich<0>(p); }
  // nagp_gppad_lap_eig
  std::vector<LanczosControl> ctl(nb);
  { LapPar p = H.par(); p.j = -1; H.norm_of_r(p); }
  for (int q = 0; q < nb; ++q) ctl[q].start(q ? std::max(1, nev - 1) : nev, jmax, 1e-12, 1e-8, H.be[q]);
  for (int step = 0; step < jmax; ++step) {
    double* const vj = H.V.data() + (size_t)step * slot;
    LapPar p = H.par();
    p.in = H.r.data(); p.out = vj; p.sc = H.be.data();
    for (int q = 0; q < nb; ++q) for (int64_t e = 0; e < Tx; ++e) lap_scale_item(p, q, e);
    p.in = vj; p.out = H.tmp.data(); H.sandwich<1>(p);
    p.in = H.tmp.data(); p.out = H.r.data(); p.j = step; p.va = vj; p.vb = step ? vj - slot : vj; H.sandwich<2>(p);
    p.np = H.N1; p.root = 0; p.res = H.al.data();
    for (int q = 0; q < nb; ++q) lap_finish_item(p, q);
    p.sc = H.al.data(); H.norm_of_r(p);
    bool any = false;
    for (int q = 0; q < nb; ++q) if (H.flag[q] >= 1.0 && ctl[q].step(H.al[q], H.be[q])) { H.flag[q] = 2.0; any = true; }
    if (any) {
      LapPar rp = H.par();
      rp.j = step; rp.va = vj; rp.in = H.r.data(); rp.out = H.r.data(); rp.res = H.h1.data(); rp.lev = 2.0;
      if (step > 0) {
        for (int pass = 0; pass < 2; ++pass) {
          for (int q = 0; q < nb; ++q) for (int i = 0; i < step; ++i) lap_h1_body(rp, q, i, 0, 1, H.red);
          for (int q = 0; q < nb; ++q) for (int64_t e = 0; e < Tx; ++e) lap_sub_item(rp, q, e);
          bool again = false;
          for (int q = 0; q < nb && !pass; ++q)
            if (H.flag[q] == 2.0 && norm2_two_columns(H.h1.data() + (size_t)q * jz * 2, step) > 10.0 * std::sqrt(2.220446049250313e-16)) { H.flag[q] = 3.0; again = true; }
          if (!again) break;
          rp.lev = 3.0;
        }
        rp.lev = 2.0;
      }
      rp.q = vj; rp.jmax = 1; rp.res = H.sc.data();
      for (int q = 0; q < nb; ++q) lap_h1_body(rp, q, 0, 0, 1, H.red);
      rp.sc = H.sc.data() + 1; rp.ss = 2; H.update(rp);
      for (int q = 0; q < nb; ++q) if (H.flag[q] >= 2.0) { ctl[q].after_reorth(); H.flag[q] = 1.0; }
    }
    bool left = false;
    for (int q = 0; q < nb; ++q) {
      if (H.flag[q] < 1.0) continue;
      ctl[q].finish_step();
      if (ctl[q].done) H.flag[q] = 0.0; else left = true;
    }
    if (!left) break;
  }
  std::vector<std::vector<double>> lmb(nb);
  std::vector<double> steps(nb);
  int K = 0;
  for (int q = 0; q < nb; ++q) {
    if (!ctl[q].ritz(lmb[q], H.S.data() + (size_t)q * jz * jz, jmax)) { ctl[q].status = LAP_NO_QL; lmb[q].clear(); }
    H.flag[q] = (double)lmb[q].size(); steps[q] = ctl[q].j; K = std::max(K, (int)lmb[q].size());
  }
  { LapPar p = H.par(); p.sc = steps.data(); p.out = H.XV.data();
    for (int q = 0; q < nb; ++q) for (int kt = 0; kt < (K + LAP_KT - 1) / LAP_KT; ++kt) for (int64_t e = 0; e < Tx; ++e) lap_ritz_item(p, q, kt, e); }
  for (int q = 0; q < nb; ++q) for (size_t e = 0; e < Txz; ++e) H.Varx[q * Txz + e] = H.varx[q];
  std::vector<double> lam((size_t)std::max(K, 1) * nb, NAN);
  for (int q = 0; q < nb; ++q) for (size_t k = 0; k < lmb[q].size(); ++k) lam[k * nb + q] = std::max(lmb[q][k], 0.0);
  for (int k = 0; k < K; ++k) { LapPar p = H.par(); p.in = H.XV.data() + (size_t)k * slot; p.out = H.Varx.data(); p.sc = lam.data() + (size_t)k * nb; H.sandwich<3>(p); }
  FILE* fo = fopen(argv[2], "wb"); if (!fo) return 2;
  for (int q = 0; q < nb; ++q) {
    const double inf[5] = {(double)ctl[q].j, (double)ctl[q].reorths, (double)lmb[q].size(), (double)ctl[q].status, ctl[q].anorm};
    std::vector<double> l(jz, NAN); std::copy(lmb[q].begin(), lmb[q].end(), l.begin());
    fwrite(inf, 8, 5, fo); fwrite(l.data(), 8, jz, fo);
    printf("problem %d: steps %d reorths %d nconv %zu status %d anorm %.6g\n", q, ctl[q].j, ctl[q].reorths, lmb[q].size(), ctl[q].status, ctl[q].anorm);
  }
  fwrite(H.d.data(), 8, Tz, fo); fwrite(Av.data(), 8, Txz, fo); fwrite(H.Varx.data(), 8, Txz, fo);
  for (size_t k = 0; k < lmb[0].size(); ++k) fwrite(H.XV.data() + k * slot, 8, Txz, fo);
  fclose(fo);
  printf("ok\n");
  return 0;
}
