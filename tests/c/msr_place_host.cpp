// The placed copy of the role layout's lists and its position tables (csrc/nagp_msr_desc.hpp, msr_place_weights) for every rule handed in:
// where in c0 / c1 / c2 a point's three weights sit, chosen for few LDS bank conflicts in the bin sums' member reads and in the weight stores
// of the three-barrier ihgp_adf8_kernel.  Checked: the tables are injections, the placed copy is the second copy of msr_build_desc seen
// through them, the sums are the dense sums in exact integer arithmetic with the weights stored at their positions, the search gives the
// same tables twice, and the modelled cycles do not rise.  Stand-alone, host only.
//   usage: msr_place_host RULES      RULES: text, per rule "p CD npt" and npt * CD coordinates (point-major), as the plan receives them
//   prints per rule that fits "rule p=<p> CD=<CD> npt=<n>: reads <r0> stores <s0> -> reads <r1> stores <s1> LDS cycles | per wave <six> -> <six>"
//   and a last line "checked <n> rules".
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

// LDS cycles of one access of a wave, restated: per half, the most different addresses on one pair of banks; a lane with addr < 0 is idle
static int access_cycles(const int* addr) {
  int total = 0;
  for (int h = 0; h < 2; ++h) {
    std::map<int, std::set<int>> on;
    for (int i = 32 * h; i < 32 * h + 32; ++i) if (addr[i] >= 0) on[addr[i] % 32].insert(addr[i]);
    size_t mx = 0;
    for (auto& kv : on) mx = std::max(mx, kv.second.size());
    total += (int)mx;
  }
  return total;
}
// the 16 member reads of worker wave w of one copy
static int wave_read_cycles(const int* D0, int w) {
  int total = 0;
  for (int s = 0; s < MSR_NMEM; ++s) {
    int addr[64];
    for (int i = 0; i < 64; ++i) addr[i] = D0[(size_t)(w * 64 + i) * MSR_DW + s];
    total += access_cycles(addr);
  }
  return total;
}
// the three weight stores of every wave: lane = point - 64 wave, lanes without a point do not store
static int store_cycles(const MspLay& l, int npt, const int* pos) {
  int total = 0;
  for (int k = 0; k < 3; ++k)
    for (int w = 0; w < MSR_NWK; ++w) {
      int addr[64];
      for (int i = 0; i < 64; ++i) addr[i] = (w * 64 + i < npt) ? l.c0 + k * MSR_CS + pos[k * MSR_NL + w * 64 + i] : -1;
      total += access_cycles(addr);
    }
  return total;
}

static int check_rule(int p, int CD, int npt, const std::vector<double>& xn, bool& fits, int cyc[4], int wave[2][MSR_NWK]) {
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
  const std::vector<int> dsc_before = dsc;
  std::vector<int> placed, again;
  int got[4] = {-1, -1, -1, -1};
  msr_place_weights(CD, npt, dsc, placed, got);
  msr_place_weights(CD, npt, dsc, again);
  if (dsc != dsc_before) return fail("msr_place_weights changed the lists handed in", p, CD);
  if ((int)placed.size() != msr_placed_ints() || msr_desc_p_ints() != msr_desc_w_ints() + msr_placed_ints() ||
      msr_desc_pos_base() != msr_desc_p_base() + msr_desc_ints() || msr_desc_p_base() != (int)dsc.size())
    return fail("sizes of the placed copy", p, CD, (int)placed.size(), msr_placed_ints());
  if (placed != again) return fail("two calls return different tables", p, CD);
  const MspLay l = msp_layout(CD, 1, 1);
  const int* D1 = dsc.data() + msr_desc_w_base();
  const int* DP = placed.data();
  const int* pos = placed.data() + msr_desc_ints();
  // ---- each table is an injection of the points into [0, 64 MSR_NWK), the present extent of c0 / c1 / c2 (entry MSR_CS - 1 stays zero)
  std::vector<int> inv(3 * MSR_NL, -1);
  for (int k = 0; k < 3; ++k)
    for (int pt = 0; pt < MSR_NL; ++pt) {
      const int s = pos[k * MSR_NL + pt];
      if (s < 0 || s >= 64 * MSR_NWK) return fail("a position lies outside its region", p, CD, k, pt);
      if (inv[k * MSR_NL + s] >= 0) return fail("two points share a position", p, CD, k, pt);
      inv[k * MSR_NL + s] = pt;
    }
  // ---- the placed copy through the inverse positions is the second copy, word for word
  for (int i = 0; i < msr_desc_ints(); ++i) {
    int a = DP[i];
    const bool member = i < MSR_NL * MSR_DW && (i % MSR_DW) < MSR_NMEM;
    if (member && a != l.zero) {
      if (a < l.c0 || a >= l.c0 + 3 * MSR_CS || (a - l.c0) % MSR_CS >= MSR_NL) return fail("a member is neither a weight nor the zero word", p, CD, i, a);
      const int k = (a - l.c0) / MSR_CS, pt = inv[k * MSR_NL + (a - l.c0) % MSR_CS];
      if (pt >= npt) return fail("a member names a position no point holds", p, CD, i, a);
      a = l.c0 + k * MSR_CS + pt;
    }
    if (a != D1[i]) return fail(member ? "a member of the placed copy is not the second copy's" : "a flag, term or reduce word differs from the second copy's", p, CD, i, a);
  }
  // ---- exact evaluation: integer weights stored at their positions, the kernels' formula against the dense sums
  {
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
    std::vector<wide> wt((size_t)3 * npt);
    for (int k = 0; k < 3; ++k) for (int pt = 0; pt < npt; ++pt) { wt[(size_t)k * npt + pt] = rnd(); ws[l.c0 + k * MSR_CS + pos[k * MSR_NL + pt]] = wt[(size_t)k * npt + pt]; }
    std::vector<wide> acc;
    evaluate(DP, l, ws, CD, acc);
    auto LK = [&](int pt, int j) { return ws[l.lk + j * nd + code[(size_t)pt * CD + j]]; };
    auto C = [&](int k, int pt) { return wt[(size_t)k * npt + pt]; };
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
      if (acc[o] != want) return fail("a sum differs from the dense sum in exact arithmetic", p, CD, o);
    }
  }
  // ---- the modelled cycles, counted here: member reads of the six waves + the three stores of every wave that holds a point
  std::vector<int> ident(3 * MSR_NL);
  for (int k = 0; k < 3; ++k) for (int i = 0; i < MSR_NL; ++i) ident[k * MSR_NL + i] = i;
  cyc[0] = cyc[2] = 0;
  for (int w = 0; w < MSR_NWK; ++w) { wave[0][w] = wave_read_cycles(D1, w); wave[1][w] = wave_read_cycles(DP, w); cyc[0] += wave[0][w]; cyc[2] += wave[1][w]; }
  cyc[1] = store_cycles(l, npt, ident.data()); cyc[3] = store_cycles(l, npt, pos);
  for (int i = 0; i < 4; ++i) if (got[i] != cyc[i]) return fail("the cycles msr_place_weights reports are not the cycles counted here", p, CD, got[i], cyc[i]);
  if (cyc[2] + cyc[3] > cyc[0] + cyc[1]) return fail("the placed copy costs more LDS cycles than the second copy at identity positions", p, CD, cyc[2] + cyc[3], cyc[0] + cyc[1]);
  // ---- no search: the second copy and identity positions
  std::vector<int> none;
  msr_place_weights(CD, npt, dsc, none, nullptr, 0);
  if (!std::equal(none.begin(), none.begin() + msr_desc_ints(), D1) || !std::equal(ident.begin(), ident.end(), none.begin() + msr_desc_ints()))
    return fail("without a search the placed copy is not the second copy at identity positions", p, CD);
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 2) { std::printf("usage: msr_place_host RULES\n"); return 2; }
  std::FILE* f = std::fopen(argv[1], "r");
  if (!f) { std::printf("cannot open %s\n", argv[1]); return 2; }
  int p, CD, npt, n = 0;
  while (std::fscanf(f, "%d %d %d", &p, &CD, &npt) == 3) {
    if (CD < 1 || CD > 7 || npt < 1 || npt > 4096) { std::printf("bad rule header\n"); std::fclose(f); return 2; }
    std::vector<double> xn((size_t)npt * CD);
    for (double& v : xn) if (std::fscanf(f, "%lf", &v) != 1) { std::printf("short rule\n"); std::fclose(f); return 2; }
    bool fits = false;
    int cyc[4] = {0, 0, 0, 0}, wave[2][MSR_NWK];
    if (check_rule(p, CD, npt, xn, fits, cyc, wave)) { std::fclose(f); return 1; }
    if (fits) {
      std::printf("rule p=%d CD=%d npt=%d: reads %d stores %d -> reads %d stores %d LDS cycles | per wave", p, CD, npt, cyc[0], cyc[1], cyc[2], cyc[3]);
      for (int c = 0; c < 2; ++c) { for (int w = 0; w < MSR_NWK; ++w) std::printf(" %d", wave[c][w]); if (!c) std::printf(" ->"); }
      std::printf("\n");
    } else std::printf("rule p=%d CD=%d npt=%d: does not fit\n", p, CD, npt);
    ++n;
  }
  std::fclose(f);
  std::printf("checked %d rules\n", n);
  return 0;
}
