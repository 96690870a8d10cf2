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

}  // namespace nagp
