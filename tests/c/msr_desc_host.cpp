// The member / term lists of the role layout's cubature sums (csrc/nagp_msr_desc.hpp, msr_build_desc) for every rule handed in: both
// copies of the lists (the chunks as they come; the chunks placed for few LDS bank conflicts, which the three-barrier ihgp_adf8_kernel reads)
// are checked structurally and by an exact evaluation in integers against the dense sums.  Stand-alone, host only.
//   usage: msr_desc_host RULES      RULES: text, per rule "p CD npt" and npt * CD coordinates (point-major), as the plan receives them
//   prints one line per rule, "rule p=<p> CD=<CD> npt=<n>: fits, member reads <c0> -> <c1> LDS cycles | does not fit", and a last line
//   "checked <n> rules".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <map>
#include <set>
#include <vector>

#include "nagp_msr_desc.hpp"

using namespace nagp;

static int fail(const char* what, int p, int CD, int a = 0, int b = 0) {
  std::printf("FAILED: p=%d CD=%d: %s (%d, %d)\n", p, CD, what, a, b);
  return 1;
}

typedef __int128 wide;

// one copy of the lists, evaluated as the kernels evaluate it, in integers: ws[] holds the tables and the weights
static void evaluate(const int* D0, const MspLay& l, std::vector<wide>& ws, int CD, std::vector<wide>& acc) {
  for (int w = 0; w < MSR_NWK; ++w) {
    wide s[64];
    for (int ln = 0; ln < 64; ++ln) {
      const int* d = D0 + (size_t)(w * 64 + ln) * MSR_DW;
      s[ln] = 0;
      for (int k = 0; k < MSR_NMEM; ++k) s[ln] += ws[d[k]];
    }
    for (int step = 1; step <= 2; ++step) {
      wide n[64];
      for (int ln = 0; ln < 64; ++ln) n[ln] = s[ln ^ step];
      for (int ln = 0; ln < 64; ++ln) if (D0[(size_t)(w * 64 + ln) * MSR_DW + MSR_NMEM] & step) s[ln] += n[ln];
    }
    for (int ln = 0; ln < 64; ++ln) ws[l.part + w * 64 + ln] = s[ln];
    for (int ln = 0; ln < 64; ++ln) {
      const int* d = D0 + (size_t)(w * 64 + ln) * MSR_DW + MSR_NMEM + 1;
      s[ln] = 0;
      for (int t = 0; t < MSR_KT; ++t) s[ln] += ws[d[3 * t]] * ws[d[3 * t + 1]] * ws[d[3 * t + 2]];
    }
    for (int step = 1; step <= 2; ++step) {
      wide n[64];
      for (int ln = 0; ln < 64; ++ln) n[ln] = s[ln ^ step];
      for (int ln = 0; ln < 64; ++ln) if (D0[(size_t)(w * 64 + ln) * MSR_DW + MSR_NMEM + 1 + 3 * MSR_KT] & step) s[ln] += n[ln];
    }
    for (int ln = 0; ln < 64; ++ln) ws[l.part + MSR_NL + w * 64 + ln] = s[ln];
  }
  acc.assign(msp_nacc(CD), 0);
  for (int o = 0; o < msp_nacc(CD); ++o) {
    const int* r = D0 + (size_t)MSR_NL * MSR_DW + (size_t)o * MSR_RW;
    acc[o] = ws[r[0]] + ws[r[3]] * ws[r[4]] + ws[r[1]] * ws[r[2]] + ws[r[5]] * ws[r[6]] * ws[r[7]];
  }
}

// LDS cycles of the member reads of one copy, restated: per read and half of a wave, the most different addresses on one pair of banks
static int member_cycles(const int* D0) {
  int total = 0;
  for (int w = 0; w < MSR_NWK; ++w)
    for (int s = 0; s < MSR_NMEM; ++s)
      for (int h = 0; h < 2; ++h) {
        std::map<int, std::set<int>> on;
        for (int i = 32 * h; i < 32 * h + 32; ++i) { const int a = D0[(size_t)(w * 64 + i) * MSR_DW + s]; on[a % 32].insert(a); }
        size_t mx = 0;
        for (auto& kv : on) mx = std::max(mx, kv.second.size());
        total += (int)mx;
      }
  return total;
}

static int check_rule(int p, int CD, int npt, const std::vector<double>& xn, bool& fits, int cyc[2]) {
  // distinct coordinates and byte codes, as plan creation forms them
  std::vector<double> xd;
  std::vector<unsigned char> code((size_t)npt * CD);
  for (int pt = 0; pt < npt; ++pt)
    for (int j = 0; j < CD; ++j) {
      const double v = xn[(size_t)pt * CD + j];
      size_t ci = 0;
      while (ci < xd.size() && xd[ci] != v) ++ci;
      if (ci == xd.size()) xd.push_back(v);
      code[(size_t)pt * CD + j] = (unsigned char)ci;
    }
  const int nd = (int)xd.size();
  int c0 = -1;
  for (int ci = 0; ci < nd; ++ci) if (xd[ci] == 0.0) c0 = ci;
  if (c0 < 0 || nd * CD > MSP_TS - 1 || npt > 64 * MSR_NWK) return fail("the rule is outside the role layout", p, CD, nd, npt);
  std::vector<int> dsc;
  fits = msr_build_desc(CD, nd, c0, npt, code, dsc);
  if (!fits) return 0;
  if ((int)dsc.size() != msr_desc_w_ints()) return fail("descriptor size", p, CD, (int)dsc.size(), msr_desc_w_ints());
  const MspLay l = msp_layout(CD, 1, 1);
  for (int copy = 0; copy < 2; ++copy) {
    const int* D0 = dsc.data() + (copy ? msr_desc_w_base() : 0);
    // ---- every word addresses the workspace
    for (int L = 0; L < MSR_NL; ++L) {
      const int* d = D0 + (size_t)L * MSR_DW;
      for (int k = 0; k < MSR_NMEM; ++k)
        if (d[k] != l.zero && !(d[k] >= l.c0 && d[k] < l.c0 + 3 * MSR_CS)) return fail("a member is neither a weight nor the zero word", p, CD, L, d[k]);
      if ((d[MSR_NMEM] & ~3) || d[MSR_NMEM] == 2 || (d[MSR_NMEM + 1 + 3 * MSR_KT] & ~3) || d[MSR_NMEM + 1 + 3 * MSR_KT] == 2) return fail("group flags", p, CD, L);
    }
    // ---- bins: members of the group that starts at a level-1 slot
    auto members = [&](int slot, std::multiset<int>& m, int& k) {
      const int L = slot - l.part, g = D0[(size_t)L * MSR_DW + MSR_NMEM], G = g == 3 ? 4 : (g == 1 ? 2 : 1);
      k = -1;
      for (int i = 0; i < G; ++i) {
        const int* d = D0 + (size_t)(L + i) * MSR_DW;
        if (d[MSR_NMEM] != g) return false;
        for (int q = 0; q < MSR_NMEM; ++q) {
          if (d[q] == l.zero) continue;
          const int kk = (d[q] - l.c0) / MSR_CS, pt = (d[q] - l.c0) % MSR_CS;
          if (k >= 0 && kk != k) return false;
          k = kk; m.insert(pt);
        }
      }
      return (L % G) == 0;
    };
    // ---- outputs: per output (aligned lane group of level 2), the terms by their table factors
    for (int w = 0; w < MSR_NWK; ++w) {
      for (int ln = 0; ln < 64; ++ln) {
        const int* d = D0 + (size_t)(w * 64 + ln) * MSR_DW;
        for (int t = 0; t < MSR_KT; ++t) {
          const int slot = d[MSR_NMEM + 1 + 3 * t];
          if (slot == l.zero) {
            if (d[MSR_NMEM + 2 + 3 * t] != l.zero || d[MSR_NMEM + 3 + 3 * t] != l.zero) return fail("a term without a bin has a table factor", p, CD, w, ln);
            continue;
          }
          if (slot < l.part + 64 * w || slot >= l.part + 64 * w + 64) return fail("a level-2 term names a slot of another wave", p, CD, w, ln);
        }
      }
      for (int ln = 0; ln < 64;) {
        const int g = D0[(size_t)(w * 64 + ln) * MSR_DW + MSR_NMEM + 1 + 3 * MSR_KT], G = g == 3 ? 4 : (g == 1 ? 2 : 1);
        if (ln % G) return fail("a level-2 group is not aligned", p, CD, w, ln);
        std::map<std::pair<int, int>, std::multiset<int>> byfac;
        std::map<std::pair<int, int>, int> kof;
        for (int i = 0; i < G; ++i) {
          const int* d = D0 + (size_t)(w * 64 + ln + i) * MSR_DW;
          if (d[MSR_NMEM + 1 + 3 * MSR_KT] != g) return fail("level-2 group flags differ inside a group", p, CD, w, ln);
          for (int t = 0; t < MSR_KT; ++t) {
            const int slot = d[MSR_NMEM + 1 + 3 * t];
            if (slot == l.zero) continue;
            int k;
            const std::pair<int, int> f(d[MSR_NMEM + 2 + 3 * t], d[MSR_NMEM + 3 + 3 * t]);
            if (!members(slot, byfac[f], k)) return fail("a level-2 term names no aligned level-1 group of one kind of weight", p, CD, w, ln);
            if (kof.count(f) && kof[f] != k) return fail("chunks of one bin differ in their kind of weight", p, CD, w, ln);
            kof[f] = k;
          }
        }
        // the bin behind (fa, fb): all points (one, one); coordinate (j, c) from a table entry; two coordinates from two e entries
        for (auto& it : byfac) {
          const int fa = it.first.first, fb = it.first.second;
          auto jc = [&](int off, int& j, int& c) {
            if (off < 0 || off >= 6 * MSP_TS) return false;
            const int t = off % MSP_TS; j = t / nd; c = t % nd; return j < CD;
          };
          std::multiset<int> want;
          int j = -1, c = -1, j2 = -1, c2 = -1;
          if (fa == l.one && fb == l.one) { for (int pt = 0; pt < npt; ++pt) want.insert(pt); }
          else if (jc(fa, j, c) && fa / MSP_TS == 3 && jc(fb, j2, c2) && fb / MSP_TS == 3 && j2 != j) {
            for (int pt = 0; pt < npt; ++pt) if (code[(size_t)pt * CD + j] == c && code[(size_t)pt * CD + j2] == c2) want.insert(pt);
          } else if (fb == l.part + MSR_MONE && jc(fa, j, c) && c == c0) {      // G2's centre term: the bins of dimension j, every c
            // (one term per non-centre coordinate shares this pair of factors: all points off the centre in dimension j)
            for (int pt = 0; pt < npt; ++pt) if (code[(size_t)pt * CD + j] != c0) want.insert(pt);
          } else if (jc(fa, j, c)) {
            for (int pt = 0; pt < npt; ++pt) if (code[(size_t)pt * CD + j] == c) want.insert(pt);
          } else return fail("a term's factors name no bin", p, CD, fa, fb);
          if (it.second != want) return fail("a bin does not hold each of its points exactly once", p, CD, fa, fb);
        }
        ln += G;
      }
    }
    // ---- exact evaluation: integer weights and tables, the kernels' formula against the dense sums
    std::vector<wide> ws((size_t)l.total + 1, 0);
    uint64_t rng = 0x9E3779B97F4A7C15ull + (uint64_t)(p * 16 + CD);
    auto rnd = [&]() { rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17; return (long)(rng % 2001) - 1000; };
    ws[l.one] = 1; ws[l.part + MSR_MONE] = -1;
    for (int j = 0; j < CD; ++j)
      for (int c = 0; c < nd; ++c) {
        const int t = j * nd + c;
        ws[l.lk + t] = rnd(); ws[l.xg + t] = (c == c0) ? 0 : rnd(); ws[l.xg2 + t] = rnd();
      }
    for (int j = 0; j < CD; ++j) for (int c = 0; c < nd; ++c) ws[l.e + j * nd + c] = ws[l.lk + j * nd + c] - ws[l.lk + j * nd + c0];
    for (int k = 0; k < 3; ++k) for (int pt = 0; pt < npt; ++pt) ws[l.c0 + k * MSR_CS + pt] = rnd();
    std::vector<wide> acc;
    evaluate(D0, l, ws, CD, acc);
    auto LK = [&](int pt, int j) { return ws[l.lk + j * nd + code[(size_t)pt * CD + j]]; };
    auto C = [&](int k, int pt) { return ws[l.c0 + k * MSR_CS + pt]; };
    const int nq = CD * (CD + 1) / 2;
    for (int o = 0; o < msp_nacc(CD); ++o) {
      wide want = 0;
      if (o < CD) { for (int pt = 0; pt < npt; ++pt) want += C(1, pt) * LK(pt, o); }
      else if (o < CD + nq) {
        int q = o - CD, j = 0;
        while (q >= CD - j) { q -= CD - j; ++j; }
        for (int pt = 0; pt < npt; ++pt) want += C(2, pt) * LK(pt, j) * LK(pt, j + q);
      } else if (o < 2 * CD + nq) { const int j = o - CD - nq; for (int pt = 0; pt < npt; ++pt) want += C(0, pt) * ws[l.xg + j * nd + code[(size_t)pt * CD + j]]; }
      else if (o < 3 * CD + nq) { const int j = o - 2 * CD - nq; for (int pt = 0; pt < npt; ++pt) want += C(0, pt) * ws[l.xg2 + j * nd + code[(size_t)pt * CD + j]]; }
      else { for (int pt = 0; pt < npt; ++pt) want += C(0, pt); }
      if (acc[o] != want) return fail("a sum differs from the dense sum in exact arithmetic", p, CD, copy, o);
    }
  }
  // the second copy holds the lanes of the first, elsewhere: a lane's member list (what it adds, in which order) and its group flag,
  // each list as often as in the first copy -- and its member reads cost no more LDS cycles
  std::multiset<std::vector<int>> lanes[2];
  for (int copy = 0; copy < 2; ++copy)
    for (int L = 0; L < MSR_NL; ++L) {
      const int* d = dsc.data() + (copy ? msr_desc_w_base() : 0) + (size_t)L * MSR_DW;
      lanes[copy].insert(std::vector<int>(d, d + MSR_NMEM + 1));
    }
  if (lanes[0] != lanes[1]) return fail("the second copy does not hold the lanes of the first", p, CD);
  cyc[0] = member_cycles(dsc.data()); cyc[1] = member_cycles(dsc.data() + msr_desc_w_base());
  if (cyc[0] != msr_member_cycles(dsc.data()) || cyc[1] != msr_member_cycles(dsc.data() + msr_desc_w_base())) return fail("msr_member_cycles", p, CD, cyc[0], cyc[1]);
  if (cyc[1] > cyc[0]) return fail("the second copy's member reads cost more LDS cycles than the first's", p, CD, cyc[0], cyc[1]);
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 2) { std::printf("usage: msr_desc_host RULES\n"); return 2; }
  std::FILE* f = std::fopen(argv[1], "r");
  if (!f) { std::printf("cannot open %s\n", argv[1]); return 2; }
  int p, CD, npt, n = 0;
  while (std::fscanf(f, "%d %d %d", &p, &CD, &npt) == 3) {
    if (CD < 1 || CD > 7 || npt < 1 || npt > 4096) { std::printf("bad rule header\n"); std::fclose(f); return 2; }
    std::vector<double> xn((size_t)npt * CD);
    for (double& v : xn) if (std::fscanf(f, "%lf", &v) != 1) { std::printf("short rule\n"); std::fclose(f); return 2; }
    bool fits = false;
    int cyc[2] = {0, 0};
    if (check_rule(p, CD, npt, xn, fits, cyc)) { std::fclose(f); return 1; }
    if (fits) std::printf("rule p=%d CD=%d npt=%d: fits, member reads %d -> %d LDS cycles\n", p, CD, npt, cyc[0], cyc[1]);
    else std::printf("rule p=%d CD=%d npt=%d: does not fit\n", p, CD, npt);
    ++n;
  }
  std::fclose(f);
  std::printf("checked %d rules\n", n);
  return 0;
}
