// nagp_msr_desc.hpp -- the LDS layout of the cubature workspace and the member / term lists of the role layout's cubature sums
// (nagp_momsp.hpp: msr_sums, msr_reduce).  Plain C++: plan creation, the kernels and tests/c/msr_desc_host.cpp read the same lines.
#pragma once
#include <algorithm>
#include <vector>

#include "nagp_qform.hpp"

namespace nagp {

constexpr int MSP_NW = 4;
constexpr int MSP_NST = 20;   // MFMA steps per wave in stage 2 (4 points each)
constexpr int MSP_TS = 64;    // stride of the (dimension, coordinate) tables: CD*nd <= 63, entry 63 of e / t1 / ve stays zero
constexpr int MSP_CS = 4 * MSP_NW * MSP_NST + 1;   // stride of c0 / c1 / c2: every point an MFMA step can address, zero beyond n_pts

// LDS workspace (offsets in doubles).  Tables lk | xg | xg2 | e | t1 | ve, MSP_TS entries each.
struct MspLay { int lk, xg, xg2, e, t1, ve, one, zero, Q, Q2, v, q0, s0, c0, c1, c2, part, acc, marg, wwt, total; };
// LAY 0: the 256-thread layout (four waves share every stage); LAY 1: the role layout of 512 threads (nagp_ihgp.hpp:
// two serial waves, six worker waves; `part` holds the results of the bin sums, msr_sums)
constexpr int MSR_NWK = 6;     // worker waves of the role layout
constexpr int MSR_NMEM = 16;   // members of a bin sum per lane (bins of up to 64 members span 2 or 4 lanes)
constexpr int MSR_NMARG = 32;  // marginal sums (non-centre (dimension, coordinate) pairs) of nagp_momsq.hpp
constexpr int MSR_CS = 64 * MSR_NWK + 1;      // one weight per worker lane
NAGP_QF_HD inline MspLay msp_layout(int CD, int D, int LAY = 0) {
  MspLay l;
  const int cs = LAY ? MSR_CS : MSP_CS, nparts = LAY ? MSR_NWK : MSP_NW;
  l.lk = 0; l.xg = MSP_TS; l.xg2 = 2 * MSP_TS; l.e = 3 * MSP_TS; l.t1 = 4 * MSP_TS; l.ve = 5 * MSP_TS;
  l.zero = l.e + MSP_TS - 1;                     // e[63] (t1[63], ve[63] are zero as well)
  l.one = 6 * MSP_TS;
  l.Q = l.one + 1; l.Q2 = l.Q + CD * CD; l.v = l.Q2 + CD * CD; l.q0 = l.v + CD; l.s0 = l.q0 + 1;
  int o = (l.s0 + 2) & ~1;
  l.c0 = o; l.c1 = o + cs; l.c2 = o + 2 * cs;
  o = (o + 3 * cs + 1) & ~1;
  l.part = o; o += nparts * 256;
  l.acc = o; o += 128;
  l.marg = o; o += LAY ? MSR_NMARG : 0;
  l.wwt = o; o += msp_qterms(D) * 192;            // static W products of stage A, [q][lane of waves 1..3], zero for sub-bands >= D
  l.total = o;
  return l;
}
NAGP_QF_HD inline int msp_nacc(int CD) { return CD + CD * (CD + 1) / 2 + 2 * CD + 1; }   // u, R (upper), g1, g2, Z

constexpr int MSR_KT = 4;      // level-2 terms per lane (outputs with more span an aligned group of 2 or 4 lanes)
constexpr int MSR_DW = MSR_NMEM + 1 + 3 * MSR_KT + 1;   // descriptor ints per worker lane: members | group flags | terms | group flags
constexpr int MSR_RW = 8;      // descriptor ints per lane of msr_reduce: p, a, b, c, d, s, f, g  ->  p + c d + a b + s f g
constexpr int MSR_NL = 64 * MSR_NWK;                    // worker lanes; level-1 results at part + L, level-2 results at part + MSR_NL + L
constexpr int MSR_MONE = 2 * MSR_NL;                    // part + MSR_MONE: the constant -1
NAGP_QF_HD inline int msr_desc_ints() { return MSR_NL * MSR_DW + 64 * MSR_RW; }
// The descriptor holds the lists twice.  [0, msr_desc_ints()): the first-fit placement in the order the chunks come, which msr_sums' other
// users read (ihgp_adf8b_kernel, ihgp_adf8sq_kernel's reduction, gf_adf8_kernel).  [msr_desc_w_base(), + msr_desc_ints()): the same bins,
// chunks and terms placed for few LDS bank conflicts in the member reads; the three-barrier ihgp_adf8_kernel reads this copy.
NAGP_QF_HD inline int msr_desc_w_base() { return msr_desc_ints(); }
NAGP_QF_HD inline int msr_desc_w_ints() { return 2 * msr_desc_ints(); }

// LDS cycles of one ds_read_b64 of a wave whose lanes read the doubles addr[0..63] (offsets in doubles): the two halves of the wave are
// served one after the other, a half in as many cycles as the busiest pair of banks holds DIFFERENT addresses (equal addresses are one
// broadcast); 64 banks of 4 bytes: the pair of a double is its offset mod 32.
inline int msr_read_cycles(const int* addr) {
  int total = 0;
  for (int h = 0; h < 2; ++h) {
    int cnt[32] = {0}, seen[32][32], mx = 0;
    for (int i = 32 * h; i < 32 * h + 32; ++i) {
      const int a = addr[i], bk = a & 31;
      bool dup = false;
      for (int u = 0; u < cnt[bk]; ++u) dup = dup || seen[bk][u] == a;
      if (!dup) { seen[bk][cnt[bk]++] = a; mx = std::max(mx, cnt[bk]); }
    }
    total += mx;
  }
  return total;
}
// the same over the MSR_NMEM member reads of the worker waves of one copy of the lists (D0: its first word)
inline int msr_member_cycles(const int* D0) {
  int total = 0;
  for (int w = 0; w < MSR_NWK; ++w)
    for (int s = 0; s < MSR_NMEM; ++s) {
      int addr[64];
      for (int i = 0; i < 64; ++i) addr[i] = D0[(size_t)(w * 64 + i) * MSR_DW + s];
      total += msr_read_cycles(addr);
    }
  return total;
}

// ---------------------------------------------------------------------------------------------
// Member and term lists of the role layout's cubature sums, built once per plan from the static cubature codes.  Bins: S_k (k = 0, 1, 2),
// Ck(j,c), C2(j,c; j',c'), each cut into chunks of <= 64 members on an aligned group of 1, 2 or 4 lanes.  Level-2 outputs: U_j, E_j, P_jj,
// g1_j, G2_j, P_jj', S_k, each <= 4 MSR_KT terms bin * table * table.  The bins of a dimension (and its outputs), of a dimension pair and of
// a total go to ONE worker wave (their level 2 reads its own bins), first fit by decreasing size.  Returns false when the rule does not fit
// the six worker waves.
// The second copy (msr_desc_w_base()).  The stage that reads the lists is bound by the LDS: six waves issue their 16 member reads at once,
// and with the chunks in the order they come a read takes 6 cycles on average where 2 is the floor -- c0 / c1 / c2 lie 385 doubles apart,
// one pair of banks, so the three bins of a (dimension, coordinate) collide, and the chunks of a total lie 64 doubles apart, the same
// banks.  What a sum adds, and in which order, is fixed by the chunk (member i on lane i % G, slot i / G); WHERE in its wave a chunk sits
// is free.  So, for this copy: one total per wave where the rule still fits that way (else the packing of the first copy), and within a
// wave chunks of one group size trade places while that lowers msr_member_cycles.  Of the two packings the one with fewer cycles is taken:
// the second copy never costs more cycles than the first, and a rule fits both copies or neither.
inline bool msr_build_desc(int CD, int nd, int c0, int npt, const std::vector<unsigned char>& code, std::vector<int>& dsc) {
  const MspLay l = msp_layout(CD, 1, 1);      // (the offsets used here do not depend on D)
  const int zero = l.zero, one = l.one, mone = l.part + MSR_MONE;
  struct Bin { int k; std::vector<int> pts; std::vector<int> slot; };      // slot: level-1 result of each chunk
  struct Term { int bin, fa, fb; };
  struct Out { std::vector<Term> t; int slot = -1; };
  struct Grp { std::vector<int> bins, outs; int n1 = 0, n2 = 0; };
  std::vector<Bin> bins; std::vector<Out> outs; std::vector<Grp> grps;
  auto pw2 = [](int n) { return n <= 1 ? 1 : (n <= 2 ? 2 : 4); };
  auto chunks = [](const Bin& b) { return std::max(1, ((int)b.pts.size() + 63) / 64); };
  auto chunk_lanes = [&](const Bin& b, int q) { const int n = std::min(64, (int)b.pts.size() - 64 * q); return pw2((n + MSR_NMEM - 1) / MSR_NMEM); };
  auto nterms = [&](const Out& o) { int n = 0; for (const Term& t : o.t) n += chunks(bins[t.bin]); return n; };
  auto add_bin = [&](int k, std::vector<int> pts) { bins.push_back({k, std::move(pts), {}}); return (int)bins.size() - 1; };
  auto add_out = [&](Grp& g) { outs.push_back(Out{}); g.outs.push_back((int)outs.size() - 1); return (int)outs.size() - 1; };
  auto cd = [&](int p, int j) { return (int)code[(size_t)p * CD + j]; };
  const int lk = l.lk, e = l.e;
  std::vector<int> oU(CD, -1), oE(CD, -1), oPd(CD, -1), oG1(CD, -1), oG2(CD, -1), oS(3, -1);
  std::vector<std::vector<int>> oP(CD, std::vector<int>(CD, -1));
  for (int j = 0; j < CD; ++j) {      // dimension j: C0, C1, C2 (j, c) and the outputs U, E, P_jj, g1, G2
    Grp g;
    oU[j] = add_out(g); oE[j] = add_out(g); oPd[j] = add_out(g); oG1[j] = add_out(g); oG2[j] = add_out(g);
    for (int c = 0; c < nd; ++c) {
      if (c == c0) continue;
      std::vector<int> pts;
      for (int p = 0; p < npt; ++p) if (cd(p, j) == c) pts.push_back(p);
      if (pts.empty()) continue;
      const int t = j * nd + c;
      const int b0 = add_bin(0, pts), b1 = add_bin(1, pts), b2 = add_bin(2, pts);
      g.bins.insert(g.bins.end(), {b0, b1, b2});
      outs[oU[j]].t.push_back({b1, e + t, one});
      outs[oE[j]].t.push_back({b2, e + t, one});
      outs[oPd[j]].t.push_back({b2, e + t, e + t});
      outs[oG1[j]].t.push_back({b0, l.xg + t, one});
      outs[oG2[j]].t.push_back({b0, l.xg2 + t, one});
      outs[oG2[j]].t.push_back({b0, l.xg2 + j * nd + c0, mone});
    }
    grps.push_back(g);
  }
  for (int j = 0; j < CD; ++j)        // dimension pair j < j2: C2 (j, c; j2, c2) and P_jj2
    for (int j2 = j + 1; j2 < CD; ++j2) {
      Grp g;
      oP[j][j2] = add_out(g);
      for (int c = 0; c < nd; ++c)
        for (int cc = 0; cc < nd; ++cc) {
          if (c == c0 || cc == c0) continue;
          std::vector<int> pts;
          for (int p = 0; p < npt; ++p) if (cd(p, j) == c && cd(p, j2) == cc) pts.push_back(p);
          if (pts.empty()) continue;
          const int b = add_bin(2, pts);
          g.bins.push_back(b);
          outs[oP[j][j2]].t.push_back({b, e + j * nd + c, e + j2 * nd + cc});
        }
      grps.push_back(g);
    }
  for (int k = 0; k < 3; ++k) {       // totals
    Grp g;
    std::vector<int> pts(npt);
    for (int p = 0; p < npt; ++p) pts[p] = p;
    const int b = add_bin(k, pts);
    g.bins.push_back(b);
    oS[k] = add_out(g);
    outs[oS[k]].t.push_back({b, one, one});
    grps.push_back(g);
  }
  for (Grp& g : grps) {
    for (int b : g.bins) for (int q = 0; q < chunks(bins[b]); ++q) g.n1 += chunk_lanes(bins[b], q);
    for (int o : g.outs) {
      const int n = nterms(outs[o]);
      if (n > 4 * MSR_KT) return false;
      g.n2 += pw2((n + MSR_KT - 1) / MSR_KT);
    }
  }
  // first fit by decreasing level-1 lanes
  std::vector<int> order(grps.size());
  for (size_t i = 0; i < order.size(); ++i) order[i] = (int)i;
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return grps[a].n1 > grps[b].n1; });
  std::vector<std::vector<int>> wg(MSR_NWK);
  int used1[MSR_NWK] = {0}, used2[MSR_NWK] = {0};
  for (int gi : order) {
    int w = 0;
    while (w < MSR_NWK && (used1[w] + grps[gi].n1 > 64 || used2[w] + grps[gi].n2 > 64)) ++w;
    if (w == MSR_NWK) return false;
    wg[w].push_back(gi); used1[w] += grps[gi].n1; used2[w] += grps[gi].n2;
  }
  // the first-fit packing with one total per wave (the totals are the last three groups)
  std::vector<std::vector<int>> wg1(MSR_NWK);
  bool spread = true;
  {
    int u1[MSR_NWK] = {0}, u2[MSR_NWK] = {0};
    const int ng = (int)grps.size();
    for (int k = 0; k < 3; ++k) { const int gi = ng - 3 + k; wg1[k].push_back(gi); u1[k] += grps[gi].n1; u2[k] += grps[gi].n2; }
    for (int gi : order) {
      if (gi >= ng - 3) continue;
      int w = 0;
      while (w < MSR_NWK && (u1[w] + grps[gi].n1 > 64 || u2[w] + grps[gi].n2 > 64)) ++w;
      if (w == MSR_NWK) { spread = false; break; }
      wg1[w].push_back(gi); u1[w] += grps[gi].n1; u2[w] += grps[gi].n2;
    }
  }
  const int grp_flags[5] = {0, 0, 1, 0, 3};      // by group size
  const int nq = CD * (CD + 1) / 2;
  struct Ch { int b, q, G; };
  // one copy of the lists at D0 from a packing; tidy: chunks of one group size trade places while that lowers the cycles of the member reads
  auto emit = [&](int* D0, const std::vector<std::vector<int>>& pack, bool tidy) {
    std::fill(D0, D0 + msr_desc_ints(), zero);
    for (int L = 0; L < MSR_NL; ++L) { D0[(size_t)L * MSR_DW + MSR_NMEM] = 0; D0[(size_t)L * MSR_DW + MSR_NMEM + 1 + 3 * MSR_KT] = 0; }
    for (Bin& b : bins) b.slot.clear();
    for (int w = 0; w < MSR_NWK; ++w) {
      // level 1: chunks by decreasing group size (aligned groups)
      std::vector<Ch> ch;
      for (int gi : pack[w]) for (int b : grps[gi].bins) for (int q = 0; q < chunks(bins[b]); ++q) ch.push_back({b, q, chunk_lanes(bins[b], q)});
      std::stable_sort(ch.begin(), ch.end(), [](const Ch& a, const Ch& b) { return a.G > b.G; });
      auto member = [&](const Ch& c, int i) {      // member i of the chunk: lane i % G, slot i / G
        const Bin& b = bins[c.b];
        const int n = std::min(64, (int)b.pts.size() - 64 * c.q);
        return i < n ? (b.k == 0 ? l.c0 : (b.k == 1 ? l.c1 : l.c2)) + b.pts[64 * c.q + i] : zero;
      };
      if (tidy) {
        auto cost = [&]() {
          int addr[MSR_NMEM][64], total = 0, lane = 0;
          for (int s = 0; s < MSR_NMEM; ++s) for (int i = 0; i < 64; ++i) addr[s][i] = zero;
          for (const Ch& c : ch) { for (int i = 0; i < c.G * MSR_NMEM; ++i) addr[i / c.G][lane + i % c.G] = member(c, i); lane += c.G; }
          for (int s = 0; s < MSR_NMEM; ++s) total += msr_read_cycles(addr[s]);
          return total;
        };
        int best = cost();
        for (bool moved = true; moved;) {
          moved = false;
          for (size_t i = 0; i < ch.size(); ++i)
            for (size_t j = i + 1; j < ch.size() && ch[j].G == ch[i].G; ++j) {
              std::swap(ch[i], ch[j]);
              const int c2 = cost();
              if (c2 < best) { best = c2; moved = true; } else std::swap(ch[i], ch[j]);
            }
        }
      }
      int lane = 0;
      for (const Ch& c : ch) {
        Bin& b = bins[c.b];
        for (int i = 0; i < c.G * MSR_NMEM; ++i) D0[(size_t)(w * 64 + lane + i % c.G) * MSR_DW + i / c.G] = member(c, i);
        for (int i = 0; i < c.G; ++i) D0[(size_t)(w * 64 + lane + i) * MSR_DW + MSR_NMEM] = grp_flags[c.G];
        if ((int)b.slot.size() <= c.q) b.slot.resize(c.q + 1, -1);
        b.slot[c.q] = l.part + w * 64 + lane;
        lane += c.G;
      }
      // level 2: outputs by decreasing group size
      struct Oc { int o, G; };
      std::vector<Oc> oc;
      for (int gi : pack[w]) for (int o : grps[gi].outs) oc.push_back({o, pw2((nterms(outs[o]) + MSR_KT - 1) / MSR_KT)});
      std::stable_sort(oc.begin(), oc.end(), [](const Oc& a, const Oc& b) { return a.G > b.G; });
      lane = 0;
      for (const Oc& c : oc) {
        std::vector<Term> ts;      // chunks expanded
        for (const Term& t : outs[c.o].t)
          for (int q = 0; q < chunks(bins[t.bin]); ++q) ts.push_back({bins[t.bin].slot[q], t.fa, t.fb});
        for (size_t i = 0; i < ts.size(); ++i) {
          int* d = &D0[(size_t)(w * 64 + lane + (int)i / MSR_KT) * MSR_DW + MSR_NMEM + 1 + 3 * ((int)i % MSR_KT)];
          d[0] = ts[i].bin; d[1] = ts[i].fa; d[2] = ts[i].fb;
        }
        for (int i = 0; i < c.G; ++i) D0[(size_t)(w * 64 + lane + i) * MSR_DW + MSR_NMEM + 1 + 3 * MSR_KT] = grp_flags[c.G];
        outs[c.o].slot = l.part + MSR_NL + w * 64 + lane;
        lane += c.G;
      }
    }
    // msr_reduce: acc[o] = p + c d + a b + s f g
    auto L2 = [&](int o) { return (o >= 0 && !outs[o].t.empty()) ? outs[o].slot : zero; };
    auto l0 = [&](int j) { return lk + j * nd + c0; };
    for (int o = 0; o < msp_nacc(CD); ++o) {
      int* r = &D0[(size_t)MSR_NL * MSR_DW + (size_t)o * MSR_RW];      // p, a, b, c, d, s, f, g (zero word by default)
      if (o < CD) { r[0] = L2(oU[o]); r[5] = L2(oS[1]); r[6] = l0(o); r[7] = one; }
      else if (o < CD + nq) {
        int q = o - CD, j = 0;
        while (q >= CD - j) { q -= CD - j; ++j; }
        const int j2 = j + q;
        r[0] = (j == j2) ? L2(oPd[j]) : L2(oP[j][j2]);
        r[1] = l0(j2); r[2] = L2(oE[j]); r[3] = l0(j); r[4] = L2(oE[j2]);
        r[5] = L2(oS[2]); r[6] = l0(j); r[7] = l0(j2);
      } else if (o < 2 * CD + nq) r[0] = L2(oG1[o - CD - nq]);
      else if (o < 3 * CD + nq) { const int j = o - 2 * CD - nq; r[0] = L2(oG2[j]); r[5] = L2(oS[0]); r[6] = l.xg2 + j * nd + c0; r[7] = one; }
      else r[0] = L2(oS[0]);
    }
  };
  dsc.assign((size_t)msr_desc_w_ints(), zero);
  emit(dsc.data(), wg, false);
  int* const D1 = dsc.data() + msr_desc_w_base();
  emit(D1, wg, true);
  if (spread) {
    std::vector<int> alt((size_t)msr_desc_ints());
    emit(alt.data(), wg1, true);
    if (msr_member_cycles(alt.data()) < msr_member_cycles(D1)) std::copy(alt.begin(), alt.end(), D1);
  }
  return true;
}

// ---------------------------------------------------------------------------------------------
// The placed copy.  What still collides in the second copy is WHERE a point's three weights sit inside c0 / c1 / c2: point p at offset p in
// all three, so the three bins of a (dimension, coordinate) read the same points one pair of banks apart, and the five chunks of a total
// read points 64 doubles apart, on the same banks.  The writer of the weights (msr_stage1b_direct) stores through a per-lane address and
// the readers (msr_sums) load through per-lane member addresses, so a position table per kind of weight, pos[k][p] in [0, MSR_NL), moves
// the weights without moving anything else: MspLay, MSR_CS and the lists' lanes, slots, terms and flags stay.  Which number is added to
// which, and in which order, does not change.
//   [msr_desc_p_base(), + msr_desc_ints())       the second copy with every member c_k + p rewritten to c_k + pos[k][p]
//   [msr_desc_pos_base(), + 3 MSR_NL)            pos[0] | pos[1] | pos[2], each a permutation of [0, MSR_NL) (beyond the points: the slots left over)
// both behind the two copies of msr_build_desc in the plan's buffer; msr_place_weights returns them as one vector of msr_placed_ints().
NAGP_QF_HD inline int msr_desc_p_base() { return msr_desc_w_ints(); }
NAGP_QF_HD inline int msr_desc_pos_base() { return msr_desc_p_base() + msr_desc_ints(); }
NAGP_QF_HD inline int msr_placed_ints() { return msr_desc_ints() + 3 * MSR_NL; }
NAGP_QF_HD inline int msr_desc_p_ints() { return msr_desc_w_ints() + msr_placed_ints(); }

// LDS cycles of the three weight stores (ds_write_b64, counted as a read is: per half of a wave, the most addresses on one pair of banks)
// of every worker wave that holds a point: lane = point - 64 wave, lanes without a point do not store.  pos: 3 x MSR_NL.
inline int msr_store_cycles(int CD, int npt, const int* pos) {
  const MspLay l = msp_layout(CD, 1, 1);
  int total = 0;
  for (int k = 0; k < 3; ++k)
    for (int h = 0; 32 * h < npt; ++h) {
      int cnt[32] = {0}, mx = 0;
      for (int p = 32 * h; p < std::min(npt, 32 * h + 32); ++p) mx = std::max(mx, ++cnt[(l.c0 + k * MSR_CS + pos[k * MSR_NL + p]) & 31]);
      total += mx;
    }
  return total;
}

constexpr int MSR_PLACE_MOVES = 24000;   // proposals of the search: about 2 ms of plan creation, once per rule and process
constexpr int MSR_PLACE_STORE_W = 1;     // weight of a store cycle against a read cycle in the search's cost

// Position tables and placed copy for the lists dsc_in (msr_build_desc's vector).  A hill-climb over swaps of two positions of one kind of
// weight, from the identity; the cost is msr_member_cycles of the placed copy plus MSR_PLACE_STORE_W * msr_store_cycles, evaluated
// incrementally: per read or store and half of a wave a count per pair of banks (the members of one half are different addresses but for
// the zero word, so a count is a number of addresses), and a swap touches only the halves that hold one of the two points.  Integer
// arithmetic and a generator of its own: the same tables on every host.  Where the search does not lower the cost, the placed copy is the
// second copy and the positions are the identity.  Returns the cost's two parts through cyc (before: reads, stores; after: reads, stores).
inline void msr_place_weights(int CD, int npt, const std::vector<int>& dsc_in, std::vector<int>& placed, int cyc[4] = nullptr,
                              int moves = MSR_PLACE_MOVES, int store_w = MSR_PLACE_STORE_W) {
  const MspLay l = msp_layout(CD, 1, 1);
  const int* D1 = dsc_in.data() + msr_desc_w_base();
  placed.assign((size_t)msr_placed_ints(), 0);
  std::copy(D1, D1 + msr_desc_ints(), placed.begin());
  int* const pos = placed.data() + msr_desc_ints();
  for (int k = 0; k < 3; ++k) for (int i = 0; i < MSR_NL; ++i) pos[k * MSR_NL + i] = i;
  const int reads0 = msr_member_cycles(D1), stores0 = msr_store_cycles(CD, npt, pos);
  if (cyc) { cyc[0] = cyc[2] = reads0; cyc[1] = cyc[3] = stores0; }
  // halves: the reads (wave, slot, half), then the stores (kind, wave, half)
  constexpr int NRH = MSR_NWK * MSR_NMEM * 2, NH = NRH + 3 * MSR_NWK * 2;
  struct Half { unsigned char cnt[32]; int mx, wt; };
  std::vector<Half> hv(NH);
  for (int i = 0; i < NH; ++i) { std::fill(hv[i].cnt, hv[i].cnt + 32, (unsigned char)0); hv[i].mx = 0; hv[i].wt = i < NRH ? 1 : store_w; }
  std::vector<std::vector<int>> in(3 * MSR_NL);            // item (k, p) -> the halves that hold it
  auto bank = [&](int k, int slot) { return (l.c0 + k * MSR_CS + slot) & 31; };
  for (int w = 0; w < MSR_NWK; ++w)
    for (int s = 0; s < MSR_NMEM; ++s)
      for (int i = 0; i < 64; ++i) {
        const int a = D1[(size_t)(w * 64 + i) * MSR_DW + s], hid = (w * MSR_NMEM + s) * 2 + i / 32;
        if (a == l.zero) { hv[hid].cnt[a & 31] = 1; continue; }      // (one address however many lanes read it)
        std::vector<int>& v = in[(a - l.c0) / MSR_CS * MSR_NL + (a - l.c0) % MSR_CS];
        if (std::find(v.begin(), v.end(), hid) == v.end()) { v.push_back(hid); ++hv[hid].cnt[a & 31]; }
      }
  for (int k = 0; k < 3; ++k)
    for (int p = 0; p < npt; ++p) { const int hid = NRH + (k * MSR_NWK + p / 64) * 2 + (p % 64) / 32; in[k * MSR_NL + p].push_back(hid); ++hv[hid].cnt[bank(k, p)]; }
  auto hmax = [](const Half& h) { int m = 0; for (int b = 0; b < 32; ++b) m = std::max(m, (int)h.cnt[b]); return m; };
  for (Half& h : hv) h.mx = hmax(h);
  std::vector<int> inv(3 * MSR_NL, -1);                    // (k, slot) -> the point there
  for (int k = 0; k < 3; ++k) for (int p = 0; p < npt; ++p) inv[k * MSR_NL + p] = p;
  std::vector<int> mark(NH, -1), touched, nmx;
  unsigned long long rng = 0x9E3779B97F4A7C15ull;
  auto rnd = [&](int n) { rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17; return (int)((rng >> 16) % (unsigned)n); };
  std::vector<std::vector<int>> held(NH);                  // half -> its items
  for (int i = 0; i < 3 * MSR_NL; ++i) for (int hid : in[i]) held[hid].push_back(i);
  for (int it = 0; it < moves; ++it) {
    // the point to move: one of a busiest pair of banks of a half drawn at random (every other proposal), or any point
    int k = rnd(3), p = rnd(npt);
    if (it & 1) {
      const int hid = rnd(NH), n = (int)held[hid].size();
      if (n == 0 || hv[hid].mx < 2) continue;
      const int i0 = rnd(n);
      int found = -1;
      for (int i = 0; i < n && found < 0; ++i) {
        const int item = held[hid][(i0 + i) % n], kk = item / MSR_NL;
        if (hv[hid].cnt[bank(kk, pos[item])] == hv[hid].mx) found = item;
      }
      if (found < 0) continue;      // (the busiest pair holds the zero word and one point less)
      k = found / MSR_NL; p = found % MSR_NL;
    }
    const int b = rnd(MSR_NL), a = pos[k * MSR_NL + p], q = inv[k * MSR_NL + b];
    const int ba = bank(k, a), bb = bank(k, b);
    if (ba == bb) continue;
    touched.clear();
    int d2 = 0;      // the same move's change of the sum of squared counts: what ranks two moves that leave every busiest pair as busy
    auto shift = [&](int pt, int from, int to) {
      for (int hid : in[k * MSR_NL + pt]) {
        d2 += hv[hid].wt * (2 * ((int)hv[hid].cnt[to] - (int)hv[hid].cnt[from]) + 2);
        --hv[hid].cnt[from]; ++hv[hid].cnt[to];
        if (mark[hid] != it) { mark[hid] = it; touched.push_back(hid); }
      }
    };
    shift(p, ba, bb);
    if (q >= 0) shift(q, bb, ba);
    int delta = 0;
    nmx.clear();
    for (int hid : touched) { nmx.push_back(hmax(hv[hid])); delta += hv[hid].wt * (nmx.back() - hv[hid].mx); }
    if (delta < 0 || (delta == 0 && d2 <= 0)) {
      for (size_t i = 0; i < touched.size(); ++i) hv[touched[i]].mx = nmx[i];
      pos[k * MSR_NL + p] = b; inv[k * MSR_NL + b] = p; inv[k * MSR_NL + a] = q;
      if (q >= 0) pos[k * MSR_NL + q] = a;
    } else {
      for (int hid : in[k * MSR_NL + p]) { ++hv[hid].cnt[ba]; --hv[hid].cnt[bb]; }
      if (q >= 0) for (int hid : in[k * MSR_NL + q]) { ++hv[hid].cnt[bb]; --hv[hid].cnt[ba]; }
    }
  }
  // positions beyond the points: the slots no point took, in rising order (each table stays a permutation of [0, MSR_NL))
  for (int k = 0; k < 3; ++k) {
    int p = npt;
    for (int s = 0; s < MSR_NL; ++s) if (inv[k * MSR_NL + s] < 0) pos[k * MSR_NL + p++] = s;
  }
  for (int L = 0; L < MSR_NL; ++L)
    for (int s = 0; s < MSR_NMEM; ++s) {
      int& a = placed[(size_t)L * MSR_DW + s];
      if (a != l.zero) { const int k = (a - l.c0) / MSR_CS; a = l.c0 + k * MSR_CS + pos[k * MSR_NL + (a - l.c0) % MSR_CS]; }
    }
  const int reads1 = msr_member_cycles(placed.data()), stores1 = msr_store_cycles(CD, npt, pos);
  if (reads1 + store_w * stores1 >= reads0 + store_w * stores0) {
    std::copy(D1, D1 + msr_desc_ints(), placed.begin());
    for (int k = 0; k < 3; ++k) for (int i = 0; i < MSR_NL; ++i) pos[k * MSR_NL + i] = i;
  } else if (cyc) { cyc[2] = reads1; cyc[3] = stores1; }
}

}  // namespace nagp
