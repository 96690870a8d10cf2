// batch_layout_check.cpp -- csrc/nagp_api_layout.hpp with its own main, on the CPU under -fsanitize=address,undefined (built and run by
// tests/test_batch_layout_host.py): batch_plan and budget_bytes against the rule written out, and the device block of every batched
// entry point against the hand-chained offsets the entry points computed before they shared this header (copied here as the
// expectation), at the smallest shapes where an optional part switches on or off.
#include "nagp_api_layout.hpp"

#include <cstdio>
#include <initializer_list>

using namespace nagp;

static int bad = 0;
#define CHECK(x) do { if (!(x)) { fprintf(stderr, "line %d: %s\n", __LINE__, #x); ++bad; } } while (0)
#define SAME(got, want) do { const size_t g_ = (got), w_ = (want); if (g_ != w_) { fprintf(stderr, "line %d: %s = %zu, expected %zu\n", __LINE__, #got, g_, w_); ++bad; } } while (0)

static size_t min3(size_t a, size_t b, size_t c) { return a < b ? (a < c ? a : c) : (b < c ? b : c); }

static void plan_case(size_t n, size_t budget, size_t fixed, size_t per_item) {
  const BatchPlan p = batch_plan(n, budget, fixed, per_item);
  CHECK(p.ok == (fixed + per_item <= budget));
  if (p.ok) { SAME(p.nb, min3(n, (budget - fixed) / per_item, 32768)); CHECK(p.nb >= 1 && p.nb <= n); }
}

static void plans() {
  const size_t MB = (size_t)1 << 20;
  SAME(budget_bytes(0, 8 * MB), 8 * MB);                     // the switch not set: the entry point's constant
  SAME(budget_bytes(1, 8 * MB), MB);
  SAME(budget_bytes(3, 8 * MB), 3 * MB);
  const size_t fixed = 4096 + 800, per = 1000, fit = (MB - fixed) / per;      // 1043 items fit
  plan_case(1, MB, fixed, per);
  for (size_t n : {fit - 1, fit, fit + 1, 5 * fit}) plan_case(n, MB, fixed, per);
  SAME(batch_plan(fit + 1, MB, fixed, per).nb, fit);
  SAME(batch_plan(fit - 1, MB, fixed, per).nb, fit - 1);
  for (size_t n : {(size_t)32767, (size_t)32768, (size_t)32769, (size_t)100000}) plan_case(n, (size_t)48 << 30, fixed, 8);      // the cap
  SAME(batch_plan(100000, (size_t)48 << 30, fixed, 8).nb, 32768);
  for (size_t per_item : {MB - fixed - 1, MB - fixed, MB - fixed + 1}) plan_case(3, MB, fixed, per_item);      // one byte under, equal, one over
  CHECK(batch_plan(3, MB, fixed, MB - fixed).ok && batch_plan(3, MB, fixed, MB - fixed).nb == 1);
  CHECK(!batch_plan(3, MB, fixed, MB - fixed + 1).ok);
  CHECK(batch_plan(3, MB, 0, MB).ok && !batch_plan(3, MB, 0, MB + 1).ok);      // the handles: nothing fixed
  plan_case(7, budget_bytes(0, 8 * MB), fixed, 3 * MB);      // switch_mb = 0 against 1: two items fit, or none
  plan_case(7, budget_bytes(1, 8 * MB), fixed, 3 * MB);
  SAME(batch_plan(7, budget_bytes(0, 8 * MB), fixed, 3 * MB).nb, 2);
  CHECK(!batch_plan(7, budget_bytes(1, 8 * MB), fixed, 3 * MB).ok);
}

static void fastfb_sample() {
  for (size_t ns : {(size_t)1, (size_t)16})
    for (size_t nb : {(size_t)1, (size_t)3}) {
      const size_t S = 5, T = ns == 1 ? 7 : 2048, SS = S * S, SP = S + 4, TS = T * S;
      const size_t o_A = 0, o_B = o_A + SS, o_G = o_B + SS, o_lq = o_G + SS, o_lp = o_lq + SS, o_k = o_lp + SS, o_h = o_k + S, o_ha = o_h + S,
                   o_y = o_ha + S, o_phf = o_y + T, o_pha = o_phf + (size_t)ns * S * SP, o_phg = o_pha + S * SP, o_phl = o_phg + S * SP,
                   o_xs = o_phl + S * SP + 8, o_ms = o_xs + (size_t)nb * TS, o_d = o_ms + (size_t)nb * TS, o_yd = o_d + (size_t)nb * T,
                   o_c = o_yd + (size_t)nb * T, o_st = o_c + (size_t)nb * ns * S, total = o_st + (size_t)nb * ns * S;
      const FbsBlock o = fbs_block(S, T, ns, nb);
      SAME(o.A, o_A); SAME(o.B, o_B); SAME(o.G, o_G); SAME(o.lq, o_lq); SAME(o.lp, o_lp); SAME(o.k, o_k); SAME(o.h, o_h); SAME(o.ha, o_ha); SAME(o.y, o_y);
      SAME(o.phf, o_phf); SAME(o.pha, o_pha); SAME(o.phg, o_phg); SAME(o.phl, o_phl); SAME(o.xs, o_xs); SAME(o.ms, o_ms); SAME(o.d, o_d); SAME(o.yd, o_yd);
      SAME(o.c, o_c); SAME(o.st, o_st); SAME(o.total, total);
      // the budget rule of the entry point covers the block
      const size_t fixed = (5 * SS + 3 * S + T + (ns + 3) * S * SP + 8) * sizeof(double), per_draw = (2 * TS + 2 * T + 2 * ns * S) * sizeof(double);
      CHECK(o.total * sizeof(double) <= fixed + nb * per_draw);
    }
}

static void slowfb() {
  for (int fo = 0; fo <= 1; ++fo)
    for (int Pdiag = 0; Pdiag <= 1; ++Pdiag)
      for (size_t n_sub : {(size_t)0, (size_t)1, (size_t)2, (size_t)3})      // Psub absent or present; an even and an odd count of ints
        for (size_t nb : {(size_t)1, (size_t)2, (size_t)3}) {
          const size_t S = 4, block = 2, T = 3, SS = S * S, ns2 = n_sub * n_sub;
          const size_t TS = (size_t)T * S, TSS = (size_t)T * SS, nbz = (size_t)nb;
          const size_t o_ab = 0, o_qb = o_ab + (size_t)S * block, o_p0 = o_qb + (size_t)S * block, o_h = o_p0 + SS, o_sub = o_h + S,
                       o_y = o_sub + (size_t)n_sub / 2 + 1, o_vr = o_y + nbz * T, o_lik = o_vr + nbz * T, o_fl = o_lik + nbz, o_pm = o_fl + nbz / 2 + 1,
                       o_pP = o_pm + nbz * TS, o_v = o_pP + nbz * TSS, o_si = o_v + (fo ? 0 : nbz * T), o_K = o_si + (fo ? 0 : nbz * T),
                       o_r = o_K + (fo ? 0 : nbz * TS), o_N = o_r + (fo ? 0 : nbz * TS), o_ms = o_N + (fo ? 0 : nbz * TSS),
                       o_pd = o_ms + nbz * TS, o_ps = o_pd + (Pdiag ? nbz * TS : 0), total = o_ps + nbz * ns2 * T + 2;
          const SfbBlock o = sfb_block(S, block, T, n_sub, fo != 0, Pdiag != 0, nb);
          SAME(o.ab, o_ab); SAME(o.qb, o_qb); SAME(o.p0, o_p0); SAME(o.h, o_h); SAME(o.sub, o_sub); SAME(o.y, o_y); SAME(o.vr, o_vr); SAME(o.lik, o_lik);
          SAME(o.fl, o_fl); SAME(o.pm, o_pm); SAME(o.pP, o_pP); SAME(o.v, o_v); SAME(o.si, o_si); SAME(o.K, o_K); SAME(o.r, o_r); SAME(o.N, o_N);
          SAME(o.ms, o_ms); SAME(o.pd, o_pd); SAME(o.ps, o_ps); SAME(o.total, total);
          CHECK((o.y - o.sub) * 8 >= n_sub * 4 && (o.pm - o.fl) * 8 >= nb * 4);      // the int slots hold their ints
          const size_t per_series = 8 * (size_t)T * ((fo ? SS + S : 2 * SS + 3 * (size_t)S + 2) + 2 + S + (Pdiag ? S : 0) + ns2);
          const size_t fixed = 8 * (2 * SS + 2 * (size_t)S * block + S) + 4 * (size_t)n_sub + 4096;
          CHECK(o.total * 8 <= fixed + nb * per_series);
        }
}

static void nmf() {
  for (int vary = 0; vary <= 1; ++vary)
    for (size_t nb : {(size_t)1, (size_t)2}) {
      const size_t T = 300, D = 3, K = 2, nwg = 2, n_obj = 4, TD = T * D, TK = T * K, KD = K * D, nbz = nb;
      const size_t o_a = 0, o_v = o_a + TD, o_w = o_v + (vary ? TD : 0), o_h = o_w + nbz * KD, o_pw = o_h + nbz * TK,
                   o_po = o_pw + nbz * nwg * 2 * KD, o_ob = o_po + nbz * nwg * 2, total = o_ob + nbz * n_obj + 2;
      const NmfBlock o = nmf_block(T, D, K, nwg, n_obj, vary != 0, nb);
      SAME(o.a, o_a); SAME(o.v, o_v); SAME(o.w, o_w); SAME(o.h, o_h); SAME(o.pw, o_pw); SAME(o.po, o_po); SAME(o.ob, o_ob); SAME(o.total, total);
      CHECK(o.total * 8 <= 8 * (vary ? 2 : 1) * TD + 4096 + nb * 8 * (TK + KD + nwg * (2 * KD + 2) + n_obj));
    }
}

static void pstft() {
  for (size_t spec_stride : {(size_t)0, (size_t)9})
    for (size_t n_out : {(size_t)2, (size_t)8})              // without and with the gradient (3 D + 2)
      for (size_t nb : {(size_t)1, (size_t)3}) {
        const size_t Dz = 2, Nz = 9, nwg = 1, nbz = nb;
        const size_t o_mv = 0, o_lo = o_mv + Dz, o_ll = o_lo + 2 * Dz, o_ss = o_ll + 2 * Dz, o_th = o_ss + (spec_stride ? 0 : Nz), o_vy = o_th + nbz * 3 * Dz,
                     o_bt = o_vy + nbz, o_sp = o_bt + nbz, o_pt = o_sp + (spec_stride ? nbz * Nz : 0), o_ob = o_pt + nbz * nwg * n_out, o_dg = o_ob + nbz,
                     total = o_dg + nbz * 3 * Dz + 2;
        const PstftBlock o = pstft_block(Dz, Nz, spec_stride != 0, nwg, n_out, nb);
        SAME(o.mv, o_mv); SAME(o.lo, o_lo); SAME(o.ll, o_ll); SAME(o.ss, o_ss); SAME(o.th, o_th); SAME(o.vy, o_vy); SAME(o.bt, o_bt); SAME(o.sp, o_sp);
        SAME(o.pt, o_pt); SAME(o.ob, o_ob); SAME(o.dg, o_dg); SAME(o.total, total);
        CHECK(o.total * 8 <= 8 * ((spec_stride ? 0 : Nz) + 5 * Dz) + 4096 + nb * 8 * ((spec_stride ? Nz : 0) + nwg * n_out + 6 * Dz + 3));
      }
}

static void segp() {
  for (size_t spec_stride : {(size_t)0, (size_t)5})
    for (size_t np : {(size_t)1, (size_t)2, (size_t)3})
      for (size_t nb : {(size_t)1, (size_t)3}) {
        const size_t Tz = 5, nwg = 1, n_out = 2 + np, nbz = nb;
        const size_t o_ss = 0, o_pa = o_ss + (spec_stride ? 0 : Tz), o_vy = o_pa + nbz * np, o_vx = o_vy + nbz, o_sp = o_vx + nbz,
                     o_pt = o_sp + (spec_stride ? nbz * Tz : 0), o_ob = o_pt + nbz * nwg * n_out, o_dg = o_ob + nbz, total = o_dg + nbz * np + 2;
        const SegpBlock o = segp_block(np, Tz, spec_stride != 0, nwg, n_out, nb);
        SAME(o.ss, o_ss); SAME(o.pa, o_pa); SAME(o.vy, o_vy); SAME(o.vx, o_vx); SAME(o.sp, o_sp); SAME(o.pt, o_pt); SAME(o.ob, o_ob); SAME(o.dg, o_dg);
        SAME(o.total, total);
        CHECK(o.total * 8 <= 8 * (spec_stride ? 0 : Tz) + 4096 + nb * 8 * ((spec_stride ? Tz : 0) + nwg * n_out + 2 * np + 3));
      }
}

static void gppad() {
  const size_t GPPAD_TILE = 4096;                            // nagp_gppad.hpp: Tx above it runs the four-step form, N1 = Tx / GPPAD_TILE workgroups
  for (size_t Txz : {GPPAD_TILE, 2 * GPPAD_TILE})
    for (size_t vary_stride : {(size_t)0, (size_t)100})
      for (size_t ic_stride : {(size_t)0, Txz})
        for (size_t nb : {(size_t)1, (size_t)2}) {
          const size_t nz = 3, Tz = 100, nbz = nb;
          const bool four = Txz > GPPAD_TILE;
          const size_t h_nwg = four ? Txz / GPPAD_TILE : 1;
          const size_t n_vy = vary_stride ? nz * Tz : nz, n_ic = ic_stride ? nz * Txz : Txz;
          const size_t h_o_vy = nz * Tz, h_o_ic = h_o_vy + n_vy, h_o_vx = h_o_ic + n_ic, h_o_mu = h_o_vx + nz, h_o_vc = h_o_mu + nz;
          const size_t res_total = h_o_vc + nz + 2;
          const size_t h_o_dg = nbz * Txz, h_o_wk = h_o_dg + nbz * Txz, h_o_pt = h_o_wk + (four ? 2 * nbz * Txz : 0), h_o_ob = h_o_pt + 2 * nbz * h_nwg;
          const size_t bat_total = h_o_ob + nbz + 2;
          const GppadRes r = gppad_res(nz, Tz, Txz, vary_stride != 0, ic_stride != 0);
          const GppadBat b = gppad_bat(Txz, four, h_nwg, nb);
          SAME(r.y, 0); SAME(r.vy, h_o_vy); SAME(r.ic, h_o_ic); SAME(r.vx, h_o_vx); SAME(r.mu, h_o_mu); SAME(r.vc, h_o_vc); SAME(r.total, res_total);
          SAME(b.x, 0); SAME(b.dg, h_o_dg); SAME(b.wk, h_o_wk); SAME(b.pt, h_o_pt); SAME(b.ob, h_o_ob); SAME(b.total, bat_total);
          CHECK(b.total * 8 <= nb * 8 * (2 * Txz + (four ? 2 * Txz : 0) + 2 * h_nwg + 1) + 16);      // the budget rule, and the pad of two doubles
        }
}

static void nmf_temp() {
  for (int learn = 0; learn <= 1; ++learn)
    for (int vary = 0; vary <= 1; ++vary)
      for (size_t nb : {(size_t)1, (size_t)2}) {
        const size_t nz = 3, T = 300, D = 3, K = 2, TD = T * D, KD = K * D, h_nwg = 2, h_n_po = 1 + 4 * K, nbz = nb;
        const bool W = !learn;
        const size_t h_nx = T * K + (learn ? KD : 0);
        const size_t h_o_vy = TD, h_o_w = h_o_vy + (vary ? TD : 0), h_o_pr = h_o_w + (W ? nz * KD : 0);
        const size_t res_total = h_o_pr + 3 * (size_t)K + 2;
        const size_t h_o_dg = nbz * h_nx, h_o_pw = h_o_dg + nbz * h_nx, h_o_po = h_o_pw + (learn ? nbz * h_nwg * KD : 0), h_o_ob = h_o_po + nbz * h_nwg * h_n_po;
        const size_t bat_total = h_o_ob + nbz + 2;
        const NmftRes r = nmft_res(nz, T, D, K, vary != 0, W);
        const NmftBat b = nmft_bat(h_nx, D, K, learn != 0, h_nwg, h_n_po, nb);
        SAME(r.a, 0); SAME(r.vy, h_o_vy); SAME(r.w, h_o_w); SAME(r.pr, h_o_pr); SAME(r.total, res_total);
        SAME(b.x, 0); SAME(b.dg, h_o_dg); SAME(b.pw, h_o_pw); SAME(b.po, h_o_po); SAME(b.ob, h_o_ob); SAME(b.total, bat_total);
        CHECK(b.total * 8 <= nb * 8 * (2 * h_nx + h_nwg * ((learn ? KD : 0) + h_n_po) + 1) + 16);
      }
}

int main() {
  plans();
  fastfb_sample(); slowfb(); nmf(); pstft(); segp(); gppad(); nmf_temp();
  if (bad) { fprintf(stderr, "%d layout checks failed\n", bad); return 1; }
  printf("all batch plans and block layouts are as written out\n");
  return 0;
}
