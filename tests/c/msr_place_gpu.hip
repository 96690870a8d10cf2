// msr_sums + msr_reduce (csrc/nagp_momsp.hpp) on the placed copy of one rule's lists, the weights stored through the position tables
// (csrc/nagp_msr_desc.hpp: msr_place_weights), against the second copy with the weights at identity positions, bit pattern by bit pattern.
// One 512-thread workgroup fills the tables with seeded values of both signs and clears c0 / c1 / c2; worker lane p stores the three weights
// of point p -- at c_k + p, then at c_k + pos[k][p] -- runs the bin sums and the reduction, and the host compares every level-2 result the
// reduction names (operands p, b, d, s of each of its sums) and the sums themselves.  Stand-alone.
//   usage: msr_place_gpu RULES      RULES: text, per rule "p CD npt" and npt * CD coordinates (point-major)
//   prints per rule "rule p=<p> CD=<CD> npt=<n>: <m> values, <d> differ | moved <points whose position is not the identity, per kind> x 3"
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "nagp_momsp.hpp"

using namespace nagp;

constexpr int NSEED = 3;                        // value sets per rule: seeded; seeded with signed zeros among the weights; every weight -0.0
constexpr int NOUT = MSR_NL + 64;               // per form: the level-2 results, the reduced sums

template <int CD>
__device__ void reduce_setup(MsrS<CD>& x, const int* bdesc, int dbase, const MspLay& l, double* ws) {
  const int lane = threadIdx.x & 63;
  const int* d = bdesc + dbase + (size_t)MSR_NL * MSR_DW + (size_t)lane * MSR_RW;
  for (int i = 0; i < MSR_RW; ++i) x.r_p[i] = (msp_rp)(ws + d[i]);
  x.r_dst = (msp_wp)(ws + l.acc + lane);
}

// in: the workspace with c0 / c1 / c2 zero; wt: [3][npt] the weights by kind and point
template <int CD>
__global__ void __launch_bounds__(MSR_NT) place_kernel(const int* bdesc, const double* in, const double* wt, double* out, int total, int npt) {
  extern __shared__ __attribute__((aligned(16))) double ws[];
  const int tid = threadIdx.x, wave = tid >> 6;
  const MspLay l = msp_layout(CD, 4, 1);
  for (int form = 0; form < 2; ++form) {
    const int dbase = form ? msr_desc_p_base() : msr_desc_w_base();
    for (int i = tid; i < total; i += MSR_NT) ws[i] = in[i];
    __syncthreads();
    if (wave >= MSR_W0) {
      const int p = tid - 64 * MSR_W0;
      if (p < npt)
        for (int k = 0; k < 3; ++k) {
          const int at = form ? bdesc[msr_desc_pos_base() + k * MSR_NL + p] : p;
          if (at >= 0 && at < MSR_NL) ws[l.c0 + k * MSR_CS + at] = wt[k * npt + p];
        }
    }
    __syncthreads();
    if (wave >= MSR_W0) {
      MsrW<CD> x;
      msr_setup_sums(x, bdesc, dbase, l, ws);
      msr_sums(x);
    }
    __syncthreads();
    if (wave == 0) {
      MsrS<CD> x;
      reduce_setup<CD>(x, bdesc, dbase, l, ws);
      msr_reduce<CD>(x);
    }
    __syncthreads();
    for (int i = tid; i < MSR_NL; i += MSR_NT) out[form * NOUT + i] = ws[l.part + MSR_NL + i];
    if (tid < 64) out[form * NOUT + MSR_NL + tid] = (tid < msp_nacc(CD)) ? ws[l.acc + tid] : 0.0;
    __syncthreads();
  }
}

#define TRY(e) do { hipError_t s_ = (e); if (s_ != hipSuccess) { std::printf("HIP error %s at line %d\n", hipGetErrorString(s_), __LINE__); return 2; } } while (0)

static uint64_t g_rng;
static double rnd() {      // both signs, magnitudes over a dozen binades
  g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17;
  const double m = 1.0 + (double)(g_rng >> 12) / 4503599627370496.0;
  const int e = (int)((g_rng >> 3) % 13) - 6;
  return ((g_rng & 1) ? -m : m) * std::ldexp(1.0, e);
}

template <int CD>
static int launch(const int* d_desc, const double* d_in, const double* d_wt, double* d_out, int total, int npt) {
  hipLaunchKernelGGL(place_kernel<CD>, dim3(1), dim3(MSR_NT), (size_t)total * sizeof(double), 0, d_desc, d_in, d_wt, d_out, total, npt);
  TRY(hipGetLastError());
  TRY(hipDeviceSynchronize());
  return 0;
}

static int run_rule(int p, int CD, int npt, const std::vector<double>& xn) {
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
  std::vector<int> dsc, placed;
  if (c0 < 0 || nd * CD > MSP_TS - 1 || npt > MSR_NL || !msr_build_desc(CD, nd, c0, npt, code, dsc)) { std::printf("rule p=%d CD=%d: does not fit\n", p, CD); return 1; }
  msr_place_weights(CD, npt, dsc, placed);
  dsc.insert(dsc.end(), placed.begin(), placed.end());
  if ((int)dsc.size() != msr_desc_p_ints()) { std::printf("rule p=%d CD=%d: size of the lists\n", p, CD); return 1; }
  const MspLay l = msp_layout(CD, 4, 1);
  const int total = l.total;
  // every word of the two copies read here addresses the workspace, every position its region (the kernel reads and writes nothing else)
  for (int copy = 1; copy < 3; ++copy)
    for (int i = 0; i < msr_desc_ints(); ++i) {
      const int w = i % MSR_DW, L = i / MSR_DW, v = dsc[(size_t)copy * msr_desc_ints() + i];
      const bool flag = L < MSR_NL && (w == MSR_NMEM || w == MSR_NMEM + 1 + 3 * MSR_KT);
      if (!flag && (v < 0 || v >= total)) { std::printf("rule p=%d CD=%d: descriptor word %d of copy %d outside the workspace\n", p, CD, i, copy); return 1; }
    }
  int moved[3] = {0, 0, 0};
  for (int k = 0; k < 3; ++k)
    for (int pt = 0; pt < MSR_NL; ++pt) {
      const int at = dsc[(size_t)msr_desc_pos_base() + k * MSR_NL + pt];
      if (at < 0 || at >= MSR_NL) { std::printf("rule p=%d CD=%d: position %d of kind %d outside its region\n", p, CD, pt, k); return 1; }
      if (pt < npt && at != pt) ++moved[k];
    }
  int* d_desc = nullptr; double* d_in = nullptr; double* d_wt = nullptr; double* d_out = nullptr;
  TRY(hipMalloc(&d_desc, dsc.size() * sizeof(int)));
  TRY(hipMalloc(&d_in, (size_t)total * sizeof(double)));
  TRY(hipMalloc(&d_wt, (size_t)3 * npt * sizeof(double)));
  TRY(hipMalloc(&d_out, 2 * NOUT * sizeof(double)));
  TRY(hipMemcpy(d_desc, dsc.data(), dsc.size() * sizeof(int), hipMemcpyHostToDevice));
  long nval = 0, ndiff = 0;
  for (int seed = 0; seed < NSEED; ++seed) {
    g_rng = 0x9E3779B97F4A7C15ull ^ ((uint64_t)(p * 64 + CD * 8 + seed) * 0x100000001B3ull);
    std::vector<double> in((size_t)total, 0.0), wt((size_t)3 * npt);
    in[l.one] = 1.0; in[l.part + MSR_MONE] = -1.0;
    for (int j = 0; j < CD; ++j)
      for (int c = 0; c < nd; ++c) {
        const int t = j * nd + c;
        in[l.lk + t] = rnd(); in[l.xg + t] = (c == c0) ? 0.0 : rnd(); in[l.xg2 + t] = rnd();
      }
    for (int j = 0; j < CD; ++j) for (int c = 0; c < nd; ++c) in[l.e + j * nd + c] = in[l.lk + j * nd + c] - in[l.lk + j * nd + c0];
    for (int k = 0; k < 3; ++k)
      for (int pt = 0; pt < npt; ++pt) {
        double v = rnd();
        if (seed == 1 && (g_rng >> 40) % 4 == 0) v = ((g_rng >> 50) & 1) ? -0.0 : 0.0;
        if (seed == 2) v = -0.0;
        wt[(size_t)k * npt + pt] = v;
      }
    TRY(hipMemcpy(d_in, in.data(), in.size() * sizeof(double), hipMemcpyHostToDevice));
    TRY(hipMemcpy(d_wt, wt.data(), wt.size() * sizeof(double), hipMemcpyHostToDevice));
    TRY(hipMemset(d_out, 0xFF, 2 * NOUT * sizeof(double)));
    int st = 0;
    switch (CD) {
      case 1: st = launch<1>(d_desc, d_in, d_wt, d_out, total, npt); break;
      case 2: st = launch<2>(d_desc, d_in, d_wt, d_out, total, npt); break;
      case 3: st = launch<3>(d_desc, d_in, d_wt, d_out, total, npt); break;
      case 4: st = launch<4>(d_desc, d_in, d_wt, d_out, total, npt); break;
      case 5: st = launch<5>(d_desc, d_in, d_wt, d_out, total, npt); break;
      default: st = launch<6>(d_desc, d_in, d_wt, d_out, total, npt); break;
    }
    if (st) return st;
    std::vector<double> out(2 * NOUT);
    TRY(hipMemcpy(out.data(), d_out, out.size() * sizeof(double), hipMemcpyDeviceToHost));
    auto bits = [](double v) { uint64_t b; std::memcpy(&b, &v, 8); return b; };
    bool nonzero = false;
    for (int o = 0; o < msp_nacc(CD); ++o) {
      const int* r0 = &dsc[(size_t)msr_desc_w_base() + (size_t)MSR_NL * MSR_DW + (size_t)o * MSR_RW];
      const int* r1 = &dsc[(size_t)msr_desc_p_base() + (size_t)MSR_NL * MSR_DW + (size_t)o * MSR_RW];
      for (int i : {0, 2, 4, 5}) {      // the level-2 results among the operands (or the zero word, in both copies)
        if (r0[i] != r1[i]) { std::printf("rule p=%d CD=%d: sum %d, operand %d: the reduce words of the two copies differ\n", p, CD, o, i); return 1; }
        if (r0[i] == l.zero) continue;
        ++nval;
        if (bits(out[r0[i] - l.part - MSR_NL]) != bits(out[NOUT + r1[i] - l.part - MSR_NL])) ++ndiff;
      }
      ++nval;
      if (bits(out[MSR_NL + o]) != bits(out[NOUT + MSR_NL + o])) ++ndiff;
      if (out[MSR_NL + o] != 0.0) nonzero = true;
    }
    if (seed == 0 && !nonzero) { std::printf("rule p=%d CD=%d: every sum is zero\n", p, CD); return 1; }
  }
  TRY(hipFree(d_desc)); TRY(hipFree(d_in)); TRY(hipFree(d_wt)); TRY(hipFree(d_out));
  std::printf("rule p=%d CD=%d npt=%d: %ld values, %ld differ | moved %d %d %d\n", p, CD, npt, nval, ndiff, moved[0], moved[1], moved[2]);
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 2) { std::printf("usage: msr_place_gpu RULES\n"); return 2; }
  std::FILE* f = std::fopen(argv[1], "r");
  if (!f) { std::printf("cannot open %s\n", argv[1]); return 2; }
  int p, CD, npt;
  while (std::fscanf(f, "%d %d %d", &p, &CD, &npt) == 3) {
    if (CD < 1 || CD > 6 || npt < 1 || npt > MSR_NL) { std::printf("bad rule header\n"); std::fclose(f); return 2; }
    std::vector<double> xn((size_t)npt * CD);
    for (double& v : xn) if (std::fscanf(f, "%lf", &v) != 1) { std::printf("short rule\n"); std::fclose(f); return 2; }
    const int st = run_rule(p, CD, npt, xn);
    if (st) { std::fclose(f); return st; }
  }
  std::fclose(f);
  return 0;
}
