// nagp_api_kernels.hpp -- part of the ONE translation unit nagp_api.hip (included there ahead of the plan struct and the three parts).
// Which instantiation of a templated kernel a plan runs is decided once, at plan creation: a picker maps the plan's integers to the host
// handle of an instantiation, set_kernel raises its dynamic-LDS limit and stores (handle, bytes) in the plan's table (nagp_plan::k), and
// the launch sites of nagp_api_sweep.hpp launch through that table.  Every ladder over template arguments is written here and nowhere
// else (tests/test_host.py holds the other parts to that).  A new instantiation needs its line in nagp_inst.hpp and its arm in a picker.
#pragma once
#include <type_traits>

using GfFn = void (*)(Shape, Bufs, MomCfg, FilterPar);
using GainFn = void (*)(Shape, Bufs, GainPar);
using SpanFn = void (*)(Shape, Bufs, SpanPar);
using MfmaFn = void (*)(Shape, Bufs, MfmaPar);
using EpFn = void (*)(Shape, Bufs, MomCfg, EpPar);
using MomFn = void (*)(MomCfg, MomPar);
using IhFn = void (*)(Shape, Bufs, MomCfg, IhgpTabs, IhgpPar);                // NAGP_SIG_IH
using IhaFn = void (*)(Shape, Bufs, MomCfg, MomSp, IhgpTabs, IhgpPar);        // NAGP_SIG_IHA
using AffFn = void (*)(Shape, Bufs, IhgpTabs, AffPar);
using AffBndFn = void (*)(Shape, Bufs, AffPar, int);
using IhScanFn = void (*)(Shape, Bufs, IhgpTabs, double*);

// one launchable role of a plan: the instantiation and the dynamic LDS it was set up with (fn == nullptr: the plan cannot reach it)
template <typename Fn> struct Kern { Fn fn = nullptr; size_t lds = 0; };

enum SpanPass { SPAN_COMPOSE = 0, SPAN_BOUNDARY = 1, SPAN_APPLY = 2 };
enum MomForm { FORM_GENERAL = 0, FORM_SP = 1, FORM_SQ = 2 };      // mom as a whole / sparse-point (nagp_momsp.hpp) / staged sqrt (nagp_momsq.hpp)

struct PlanKernels {
  Kern<GfFn> adf, adf8, fixed, fixed_win, ekf;      // gf filter: ADF launch, role-specialised sweep 1, fixed-site launch and its windowed twin, EKF
  Kern<GainFn> gain, gain_mfma;                     // rts_gain_kernel (VALU, (G, Delta) as tiles) / rts_gain_mfma_kernel (dense)
  Kern<SpanFn> span[3];                             // [SpanPass], VALU passes
  Kern<MfmaFn> span_m[3], big_phi;                  // [SpanPass], MFMA passes or (plans with big_sp) the column-owner ones with their Phi pass
  Kern<EpFn> site;                                  // site refresh
  Kern<IhFn> ih_filter;                             // IHGP: the general ADF filter
  Kern<IhaFn> ih_adf;                               // ... and the sparse-point / role-specialised / staged-sqrt sweep that replaces it
  Kern<AffFn> aff_compose[2], aff_apply[2];         // [AffPar::mode]
  Kern<AffBndFn> aff_boundary[2];
  Kern<IhScanFn> ih_scan;
};

// The dynamic-LDS limit of a kernel is a per-process attribute: it is raised to the full 160 KiB once and never lowered, so that
// plans with different LDS needs can be alive at the same time (a later, smaller plan must not shrink it under a live one).
template <typename K>
static int set_lds(K kernel, size_t bytes) {
  if (bytes > 160 * 1024) FAIL(NAGP_EUNSUPPORTED, "kernel needs %zu B of LDS (> 160 KiB)", bytes);
  if (bytes > 48 * 1024)
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  return NAGP_OK;
}

// the one place a plan's role is filled
template <typename Fn>
static int set_kernel(Kern<Fn>& k, Fn fn, size_t bytes) {
  const int st = set_lds(fn, bytes);
  if (st == NAGP_OK) { k.fn = fn; k.lds = bytes; }
  return st;
}

// f(std::integral_constant<int, V>) for the V among V0, Vs... that equals v.  Any other v takes the LAST value: the `default:` arm of a
// switch ladder, which catches the values below the listed ones as well as those above.
template <int V0, int... Vs, typename F>
static auto pick_of(int v, F f) {
  if constexpr (sizeof...(Vs) == 0) return f(std::integral_constant<int, V0>{});
  else return v == V0 ? f(std::integral_constant<int, V0>{}) : pick_of<Vs...>(v, f);
}
// ... for the V of LO .. HI; any other v takes HI
template <int LO, int HI, typename F>
static auto pick_in(int v, F f) {
  if constexpr (LO == HI) return f(std::integral_constant<int, HI>{});
  else return v == LO ? f(std::integral_constant<int, LO>{}) : pick_in<LO + 1, HI>(v, f);
}
#define NAGP_V(X) decltype(X)::value      // (the template argument behind a pick_of / pick_in callback's parameter; undefined at the end of this file)

// ---- gf filter.  mv: mom variant (0 = POWER, 1 .. 9 = NMF cubature dimension; the sparse-point form exists for 1 .. 7, the staged sqrt
// form for 1 .. 6).  ADF launches: split blocks (cpl) run <1 | 2 | 4, 0, mv, 512, 0, true>; else 1 .. 4 tiles per thread under the
// 256-thread bound, or (lb == 512) four under the 512-thread bound.
static GfFn pick_gf_adf(int tpt, int lb, int mv, MomForm form, bool cpl) {
  if (cpl) return pick_of<1, 2, 4>(tpt, [&](auto TP) { return pick_in<0, 9>(mv, [](auto V) -> GfFn { return gf_filter_kernel<NAGP_V(TP), 0, NAGP_V(V), 512, 0, true>; }); });
  if (form == FORM_SQ) return pick_in<1, 4>(tpt, [&](auto TP) { return pick_in<1, 6>(mv, [](auto V) -> GfFn { return gf_filter_kernel<NAGP_V(TP), 0, NAGP_V(V), 256, 2>; }); });
  if (form == FORM_SP) return pick_in<1, 4>(tpt, [&](auto TP) { return pick_in<1, 7>(mv, [](auto V) -> GfFn { return gf_filter_kernel<NAGP_V(TP), 0, NAGP_V(V), 256, 1>; }); });
  if (lb == 512) return pick_in<0, 9>(mv, [](auto V) -> GfFn { return gf_filter_kernel<4, 0, NAGP_V(V), 512>; });
  return pick_in<1, 4>(tpt, [&](auto TP) { return pick_in<0, 9>(mv, [](auto V) -> GfFn { return gf_filter_kernel<NAGP_V(TP), 0, NAGP_V(V), 256>; }); });
}
// sweep 1 with role-specialised waves: one or two lower tiles per thread on the worker waves, or (st) two on all eight waves
static GfFn pick_gf_adf8(int tpt, int cd, bool st) {
  return pick_in<1, 7>(cd, [&](auto V) -> GfFn {
    if (st) return gf_adf8_kernel<2, NAGP_V(V), true>;
    if (tpt == 1) return gf_adf8_kernel<1, NAGP_V(V), false>;
    return gf_adf8_kernel<2, NAGP_V(V), false>;
  });
}
// fixed-site launches (no step calls mom): lb = 768 / 1024 are the wide forms (one tile per thread), anything else the 512-thread bound
// with 1 | 2 | 4 tiles per thread; win: the time-parallel twin (nagp_plan_set_windows)
static GfFn pick_gf_fixed(int tpt, int lb, bool cpl, bool win) {
  return pick_of<0, 1>(cpl, [&](auto C) { return pick_of<0, 1>(win, [&](auto W) -> GfFn {
    constexpr bool c = NAGP_V(C) != 0, w = NAGP_V(W) != 0;
    if (lb == 768) return gf_filter_kernel<1, 0, -1, 768, 0, c, w>;
    if (lb == 1024) return gf_filter_kernel<1, 0, -1, 1024, 0, c, w>;
    return pick_of<1, 2, 4>(tpt, [](auto TP) -> GfFn { return gf_filter_kernel<NAGP_V(TP), 0, -1, 512, 0, c, w>; });
  }); });
}
static GfFn pick_gf_ekf(int tpt, bool cpl) {
  return pick_of<1, 2, 4>(tpt, [&](auto TP) -> GfFn {
    if (cpl) return gf_filter_kernel<NAGP_V(TP), 1, 0, 512, 0, true>;
    return gf_filter_kernel<NAGP_V(TP), 1, 0>;
  });
}

// ---- RTS gain.  Tiles per thread 1 .. 4, anything else 8 (46 .. 64 tile rows: tiles in scratch)
enum GainForm { GAIN_PLAIN = 0, GAIN_CPL = 1, GAIN_768 = 2 };      // GAIN_CPL: split blocks (cross tiles); GAIN_768: rts_gain_kernel<2, 768>
static GainFn pick_gain(int tpt, GainForm form) {
  if (form == GAIN_768) return rts_gain_kernel<2, 768>;
  return pick_of<1, 2, 3, 4, 8>(tpt, [&](auto TP) -> GainFn {
    if (form == GAIN_CPL) return rts_gain_kernel<NAGP_V(TP), 512, true>;
    return rts_gain_kernel<NAGP_V(TP)>;
  });
}
static GainFn pick_gain_mfma(int ntl, bool inv) {
  return pick_in<1, 10>(ntl, [&](auto N) -> GainFn {
    if (inv) return rts_gain_mfma_kernel<NAGP_V(N), true>;
    return rts_gain_mfma_kernel<NAGP_V(N), false>;
  });
}

// ---- span passes of the smoother: VALU (tiles per thread as for the gain), MFMA (Sp / 16 = 1 .. 6), column owners (Sp / 16 = 5 .. 10)
static SpanFn pick_span(SpanPass pass, int tpt) {
  return pick_of<1, 2, 3, 4, 8>(tpt, [&](auto TP) -> SpanFn {
    if (pass == SPAN_COMPOSE) return rts_compose_kernel<NAGP_V(TP)>;
    if (pass == SPAN_BOUNDARY) return rts_boundary_kernel<NAGP_V(TP)>;
    return rts_apply_kernel<NAGP_V(TP)>;
  });
}
static MfmaFn pick_span_mfma(SpanPass pass, int ntl) {
  return pick_in<1, 6>(ntl, [&](auto N) -> MfmaFn {
    if (pass == SPAN_COMPOSE) return rts_compose_mfma_kernel<NAGP_V(N)>;
    if (pass == SPAN_BOUNDARY) return rts_boundary_mfma_kernel<NAGP_V(N)>;
    return rts_apply_mfma_kernel<NAGP_V(N)>;
  });
}
static MfmaFn pick_span_big(SpanPass pass, int ntl) {
  return pick_in<5, 10>(ntl, [&](auto N) -> MfmaFn {
    if (pass == SPAN_COMPOSE) return rts_big_kernel<NAGP_V(N), 0>;
    if (pass == SPAN_BOUNDARY) return rts_big_kernel<NAGP_V(N), 1>;
    return rts_big_kernel<NAGP_V(N), 2>;
  });
}
static MfmaFn pick_big_phi(int ntl) {
  return pick_in<5, 10>(ntl, [](auto N) -> MfmaFn { return rts_big_phi_kernel<NAGP_V(N)>; });
}

// ---- site refresh and mom on its own.  v: the mom variant (FORM_GENERAL) or the cubature dimension (FORM_SP: 1 .. 7, FORM_SQ: 1 .. 6)
static EpFn pick_ep_site(MomForm form, int v) {
  if (form == FORM_SQ) return pick_in<1, 6>(v, [](auto V) -> EpFn { return ep_site_sq_kernel<NAGP_V(V)>; });
  if (form == FORM_SP) return pick_in<1, 7>(v, [](auto V) -> EpFn { return ep_site_sp_kernel<NAGP_V(V)>; });
  return pick_in<0, 9>(v, [](auto V) -> EpFn { return ep_site_kernel<NAGP_V(V)>; });
}
static MomFn pick_mom(int mv) {
  return pick_in<0, 9>(mv, [](auto V) -> MomFn { return mom_kernel<NAGP_V(V)>; });
}

// ---- IHGP.  The general filter: blocks of 5 .. 8 states (bs8) come before the block-structured mom (src)
static IhFn pick_ih_filter(int mv, bool src, bool bs8) {
  return pick_in<0, 9>(mv, [&](auto V) -> IhFn {
    if (bs8) return ihgp_filter_kernel<NAGP_V(V), false, 8>;
    if (src) return ihgp_filter_kernel<NAGP_V(V), true>;
    return ihgp_filter_kernel<NAGP_V(V), false>;
  });
}
// FORM_SP: ihgp_adf_kernel, or with roles ihgp_adf8_kernel<cd> (the three-barrier schedule: direct form, cd = 1 .. 6) and
// ihgp_adf8b_kernel<cd, tab> (barrier B1: cd = 7, and the table form at cd = 1 .. 7); FORM_SQ: ihgp_adf8sq_kernel (1 .. 6).  stamps (NAGP_STAMPS):
// the three-barrier schedule has its stamps in instantiations of their own; every other kernel tests the pointer.
// qf (nagp_qform.hpp, qform_pick of the plan's D): the form of Q / 2Q / v on wave 0 of that schedule; every other kernel ignores it
static IhaFn pick_ih_adf(MomForm form, int cd, bool roles, bool tab, bool stamps, int qf) {
  if (form == FORM_SQ) return pick_in<1, 6>(cd, [](auto V) -> IhaFn { return ihgp_adf8sq_kernel<NAGP_V(V)>; });
  return pick_in<1, 7>(cd, [&](auto V) -> IhaFn {
    if (!roles) return ihgp_adf_kernel<NAGP_V(V)>;
    if (tab) return ihgp_adf8b_kernel<NAGP_V(V), true>;
    if constexpr (NAGP_V(V) <= 6) {
      return pick_of<QF_K4, QF_K8, QF_K16P, QF_RUNTIME>(qf, [&](auto F) -> IhaFn {
        if (stamps) return ihgp_adf8_kernel<NAGP_V(V), true, NAGP_V(F)>;
        return ihgp_adf8_kernel<NAGP_V(V), false, NAGP_V(F)>;
      });
    } else return ihgp_adf8b_kernel<NAGP_V(V), false>;
  });
}
// the affine scans and the sequential scan: block stride 8 for plans with a block of 5 .. 8 states, else 4; mode as AffPar::mode (0, else 1)
static AffFn pick_aff_compose(int mode, int bs) {
  return pick_of<8, 4>(bs, [&](auto BSV) { return pick_of<0, 1>(mode, [](auto MO) -> AffFn { return ihgp_aff_compose_kernel<NAGP_V(MO), NAGP_V(BSV)>; }); });
}
static AffBndFn pick_aff_boundary(int mode, int bs) {
  return pick_of<8, 4>(bs, [&](auto BSV) { return pick_of<0, 1>(mode, [](auto MO) -> AffBndFn { return ihgp_aff_boundary_kernel<NAGP_V(MO), NAGP_V(BSV)>; }); });
}
static AffFn pick_aff_apply(int mode, int bs) {
  return pick_of<8, 4>(bs, [&](auto BSV) { return pick_of<0, 1>(mode, [](auto MO) -> AffFn { return ihgp_aff_apply_kernel<NAGP_V(MO), NAGP_V(BSV)>; }); });
}
static IhScanFn pick_ih_scan(int bs) {
  return pick_of<8, 4>(bs, [](auto BSV) -> IhScanFn { return ihgp_scan_kernel<NAGP_V(BSV)>; });
}
#undef NAGP_V
