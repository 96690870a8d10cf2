// nagp_api_layout.hpp -- part of the host translation unit nagp_api.hip: the arithmetic of the batched entry points ("Batched
// entry points") -- the budget, the size of a device batch and the offsets inside "one device block of doubles" of every entry point.
// Plain C++ without the HIP runtime, so that tests/c/batch_layout_check.cpp can run all of it under the host sanitizers.
#pragma once
#include <algorithm>
#include <cstddef>

namespace nagp {
constexpr size_t BATCH_MAX = 32768;      // items of one device batch at the most (the y extent of a grid stays far below 65535)
// the device-memory budget of one call: the developer switch in MiB when it is set, the entry point's constant otherwise
inline size_t budget_bytes(int switch_mb, size_t default_bytes) { return switch_mb ? (size_t)switch_mb << 20 : default_bytes; }

// n items in device batches of nb under `budget` bytes: `fixed` bytes once, `per_item` bytes for every item of a batch.  !ok: one item
// does not fit (the caller refuses with its own status and text)
struct BatchPlan { bool ok; size_t nb; };
inline BatchPlan batch_plan(size_t n, size_t budget, size_t fixed, size_t per_item) {
  return fixed + per_item > budget ? BatchPlan{false, 0} : BatchPlan{true, std::min({n, (budget - fixed) / per_item, BATCH_MAX})};
}

// one device block of doubles, stated as a sequence of parts: take(n) gives the offset of the next n doubles, total(pad) closes the block
struct Layout {
  size_t at = 0;
  size_t take(size_t n_doubles) { const size_t o = at; at += n_doubles; return o; }
  size_t total(size_t pad) const { return at + pad; }
};

// ---- the blocks of the entry points, nb items per device batch (a braced list is evaluated left to right: the parts lie in the order written)
// nagp_fastfb_sample: A | AKHA | G | Lq | Lp | K | H | HA | y | span matrices: filter, A^L, G^L, G^last (+ 8) | per batch: x* | ms | d | yd | c | starts
struct FbsBlock { size_t A, B, G, lq, lp, k, h, ha, y, phf, pha, phg, phl, xs, ms, d, yd, c, st, total; };
inline FbsBlock fbs_block(size_t S, size_t T, size_t ns, size_t nb) {
  const size_t SS = S * S, SSP = S * (S + 4), TS = T * S;
  Layout l; return {l.take(SS), l.take(SS), l.take(SS), l.take(SS), l.take(SS), l.take(S), l.take(S), l.take(S), l.take(T), l.take(ns * SSP), l.take(SSP), l.take(SSP),
          l.take(SSP + 8), l.take(nb * TS), l.take(nb * TS), l.take(nb * T), l.take(nb * T), l.take(nb * ns * S), l.take(nb * ns * S), l.total(0)};
}
// nagp_ep_sample: A | Q | P0 | Ab | Qb | h_val | off, boff, blk (int) | W | ttau | tnu | y | MF | PF / G | Lc | MS | counters | per batch: z | X | F | Sdraw
// (z with the caller's normals, X / F / Sdraw when asked for; F also behind Sdraw)
struct EpsBlock { size_t A, Q, p0, ab, qb, h, idx, w, tt, tn, y, mf, pg, lc, ms, cnt, z, x, f, sd, total; };
inline size_t eps_fixed_bytes(size_t S, size_t M, size_t T, size_t nb2, size_t DN) {
  return 8 * (T * (2 * S * S + 2 * S + 2 * M + 1) + 3 * S * S + 2 * nb2 + M + DN + 8) + 4 * (2 * M + 2 + S) + 4096;
}
inline size_t eps_draw_bytes(size_t S, size_t M, size_t T, bool z, bool x, bool f, bool sd) {
  return std::max<size_t>(8, 8 * T * ((z ? S : 0) + (x ? S : 0) + (f || sd ? M : 0) + (sd ? 1 : 0)));
}
inline EpsBlock eps_block(size_t S, size_t M, size_t T, size_t nb2, size_t DN, bool z, bool x, bool f, bool sd, size_t nb) {
  const size_t SS = S * S;
  Layout l; return {l.take(SS), l.take(SS), l.take(SS), l.take(nb2), l.take(nb2), l.take(M), l.take((2 * M + 2 + S) / 2 + 1), l.take(DN), l.take(T * M), l.take(T * M), l.take(T),
          l.take(T * S), l.take(T * SS), l.take(T * SS), l.take(T * S), l.take(4), l.take(z ? nb * T * S : 0), l.take(x ? nb * T * S : 0), l.take(f || sd ? nb * T * M : 0),
          l.take(sd ? nb * T : 0), l.total(2)};
}
// nagp_slowfb_run: Ab | Qb | P0 | H | sub (int) | per batch: y | vary | lik | flag (int) | pm | pP | v | 1/s | K | r | N | MS | Pdiag | Psub
// (v .. N only for the smoother, Pdiag when asked for; n ints lie in n / 2 + 1 doubles)
struct SfbBlock { size_t ab, qb, p0, h, sub, y, vr, lik, fl, pm, pP, v, si, K, r, N, ms, pd, ps, total; };
inline SfbBlock sfb_block(size_t S, size_t block, size_t T, size_t n_sub, bool filter_only, bool pdiag, size_t nb) {
  const size_t SS = S * S, TS = T * S, TSS = T * SS, sm = filter_only ? 0 : nb;
  Layout l; return {l.take(S * block), l.take(S * block), l.take(SS), l.take(S), l.take(n_sub / 2 + 1), l.take(nb * T), l.take(nb * T), l.take(nb), l.take(nb / 2 + 1),
          l.take(nb * TS), l.take(nb * TSS), l.take(sm * T), l.take(sm * T), l.take(sm * TS), l.take(sm * TS), l.take(sm * TSS), l.take(nb * TS),
          l.take(pdiag ? nb * TS : 0), l.take(nb * n_sub * n_sub * T), l.total(2)};
}
// nagp_nmf_fp: A | vary | per batch: W | H | pw | po | Obj
struct NmfBlock { size_t a, v, w, h, pw, po, ob, total; };
inline NmfBlock nmf_block(size_t T, size_t D, size_t K, size_t nwg, size_t n_obj, bool vary, size_t nb) {
  Layout l; return {l.take(T * D), l.take(vary ? T * D : 0), l.take(nb * K * D), l.take(nb * T * K), l.take(nb * nwg * 2 * K * D), l.take(nb * nwg * 2), l.take(nb * n_obj), l.total(2)};
}
// nagp_pstft_obj: minVar | limOm | limLam | specTar (shared) | per batch: theta | vary | bet | specTar | part | Obj | dObj
struct PstftBlock { size_t mv, lo, ll, ss, th, vy, bt, sp, pt, ob, dg, total; };
inline PstftBlock pstft_block(size_t D, size_t N, bool per_problem_spec, size_t nwg, size_t n_out, size_t nb) {
  Layout l; return {l.take(D), l.take(2 * D), l.take(2 * D), l.take(per_problem_spec ? 0 : N), l.take(nb * 3 * D), l.take(nb), l.take(nb), l.take(per_problem_spec ? nb * N : 0),
          l.take(nb * nwg * n_out), l.take(nb), l.take(nb * 3 * D), l.total(2)};
}
// nagp_segp_obj: specy (shared) | per batch: param | vary | varx | specy | part | Obj | dObj
struct SegpBlock { size_t ss, pa, vy, vx, sp, pt, ob, dg, total; };
inline SegpBlock segp_block(size_t n_param, size_t T, bool per_problem_spec, size_t nwg, size_t n_out, size_t nb) {
  Layout l; return {l.take(per_problem_spec ? 0 : T), l.take(nb * n_param), l.take(nb), l.take(nb), l.take(per_problem_spec ? nb * T : 0), l.take(nb * nwg * n_out), l.take(nb),
          l.take(nb * n_param), l.total(2)};
}
// nagp_gppad handle, resident: y | vary | ic | varx | mux | varc;  per device batch: x | dObj | work (four-step form) | part | Obj
struct GppadRes { size_t y, vy, ic, vx, mu, vc, total; };
inline GppadRes gppad_res(size_t n, size_t T, size_t Tx, bool vary_per_sample, bool ic_per_problem) {
  Layout l; return {l.take(n * T), l.take(vary_per_sample ? n * T : n), l.take(ic_per_problem ? n * Tx : Tx), l.take(n), l.take(n), l.take(n), l.total(2)};
}
struct GppadBat { size_t x, dg, wk, pt, ob, total; };
inline GppadBat gppad_bat(size_t Tx, bool four_step, size_t nwg, size_t nb) {
  Layout l; return {l.take(nb * Tx), l.take(nb * Tx), l.take(four_step ? 2 * nb * Tx : 0), l.take(2 * nb * nwg), l.take(nb), l.total(2)};
}
// nagp_gppad_cas handle (n cascades of M columns), resident: y | ic | varx | mux | varc;  per device batch: x | dObj | work (four-step
// form) | part | D | partA | Obj
struct GppadCasRes { size_t y, ic, vx, mu, vc, total; };
inline GppadCasRes gppad_cas_res(size_t n, size_t M, size_t T, size_t Tx, bool ic_per_cascade) {
  Layout l; return {l.take(n * T), l.take(ic_per_cascade ? n * M * Tx : M * Tx), l.take(n * M), l.take(n * M), l.take(n), l.total(2)};
}
struct GppadCasBat { size_t x, dg, wk, pt, d, pa, ob, total; };
inline GppadCasBat gppad_cas_bat(size_t M, size_t T, size_t Tx, bool four_step, size_t nwg, size_t nwgA, size_t nb) {
  Layout l; return {l.take(nb * M * Tx), l.take(nb * M * Tx), l.take(four_step ? 2 * nb * M * Tx : 0), l.take(2 * nb * M * nwg), l.take(nb * T), l.take(2 * nb * nwgA),
          l.take(nb), l.total(2)};
}
// nagp_gppad_lap handle, resident: y | vary | g | ic | varx | mux | varc | zeros | x | d | Varx;  per device batch (slot-major vectors, nb Tx
// each): V (jmax slots) | xv (jmax slots) | r | tmp | work (four-step form) | part | alpha | beta | flag | sc | h1 | S | lambda | Obj
struct LapRes { size_t y, vy, g, ic, vx, mu, vc, ze, x, d, var, total; };
inline LapRes lap_res(size_t n, size_t T, size_t Tx, bool vary_per_sample) {
  Layout l; return {l.take(n * T), l.take(vary_per_sample ? n * T : n), l.take(n * Tx), l.take(n * Tx), l.take(n), l.take(n), l.take(n), l.take(n), l.take(n * Tx), l.take(n * T),
          l.take(n * Tx), l.total(2)};
}
struct LapBat { size_t V, xv, r, tmp, wk, pt, al, be, fl, sc, h1, S, lam, ob, total; };
inline size_t lap_bat_per_problem(size_t Tx, size_t jmax, bool four_step, size_t np) {
  return (2 * jmax + 2 + (four_step ? 2 : 0)) * Tx + 2 * np + 5 + 2 * jmax + jmax * jmax + jmax + 3;
}
inline LapBat lap_bat(size_t Tx, size_t jmax, bool four_step, size_t np, size_t nb) {
  Layout l; return {l.take(jmax * nb * Tx), l.take(jmax * nb * Tx), l.take(nb * Tx), l.take(nb * Tx), l.take(four_step ? 2 * nb * Tx : 0), l.take(2 * nb * np), l.take(nb), l.take(nb),
          l.take(nb), l.take(2 * nb), l.take(2 * nb * jmax), l.take(nb * jmax * jmax), l.take(jmax * nb), l.take(3 * nb), l.total(2)};
}
// nagp_nmf_temp handle, resident: A | vary | W (inference form) | muinf, varinf, lam;  per device batch: x | dObj | pw (learning form) | po | Obj
struct NmftRes { size_t a, vy, w, pr, total; };
inline NmftRes nmft_res(size_t n, size_t T, size_t D, size_t K, bool vary, bool given_W) {
  Layout l; return {l.take(T * D), l.take(vary ? T * D : 0), l.take(given_W ? n * K * D : 0), l.take(3 * K), l.total(2)};
}
struct NmftBat { size_t x, dg, pw, po, ob, total; };
inline NmftBat nmft_bat(size_t nx, size_t D, size_t K, bool learn, size_t nwg, size_t n_po, size_t nb) {
  Layout l; return {l.take(nb * nx), l.take(nb * nx), l.take(learn ? nb * nwg * K * D : 0), l.take(nb * nwg * n_po), l.take(nb), l.total(2)};
}
// the squared-exponential basis of a nagp_sebf_fit / nagp_tnmf handle or a nagp_sebf_conv call, resident: taps | first tap of every tap
// column (int64) | tau (int) | mux | the targets of the fit
struct SebfRes { size_t tp, of, ta, c, e, total; };
inline SebfRes sebf_res(size_t n_taps, size_t n_tc, size_t n_targets) {
  Layout l; return {l.take(n_taps), l.take(n_tc), l.take(n_tc / 2 + 1), l.take(n_tc), l.take(n_targets), l.total(2)};
}
// per device batch.  nagp_sebf_conv: Z | Y;  nagp_sebf_fit: z | dx | dObj | Obj;  nagp_tnmf: x | logH (and log W) | the row kernel's gradient |
// dObj | pw (learning form) | po | Obj
struct SebfBat { size_t x, lh, dg, out, pw, po, ob, total; };
inline SebfBat sebf_conv_bat(size_t T, size_t nb) { Layout l; return {l.take(nb * T), 0, 0, l.take(nb * T), 0, 0, 0, l.total(2)}; }
inline SebfBat sebf_fit_bat(size_t T, size_t nb) { Layout l; return {l.take(nb * T), l.take(nb * T), 0, l.take(nb * T), 0, 0, l.take(nb), l.total(2)}; }
inline SebfBat tnmf_bat(size_t nx, size_t D, size_t K, bool learn, size_t nwg, size_t nb) {
  Layout l; return {l.take(nb * nx), l.take(nb * nx), l.take(nb * nx), l.take(nb * nx), l.take(learn ? nb * nwg * K * D : 0), l.take(nb * nwg), l.take(nb), l.total(2)};
}
}  // namespace nagp
