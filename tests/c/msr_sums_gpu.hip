// msr_sums + msr_reduce (csrc/nagp_momsp.hpp) on the two copies of one rule's lists (csrc/nagp_msr_desc.hpp: the chunks as they come, and
// placed for few LDS bank conflicts), bit pattern by bit pattern.  One 512-thread workgroup fills the workspace with seeded values of both
// signs (the tables, c0 / c1 / c2), runs the bin sums and the reduction on the first copy, clears the results and runs them on the second;
// the host compares every level-2 result the reduction names (operands p, b, d, s of each of its sums) and the sums themselves.  Stand-alone.
//   usage: msr_sums_gpu RULES      RULES: text, per rule "p CD npt" and npt * CD coordinates (point-major)
//   prints per rule "rule p=<p> CD=<CD> npt=<n>: <m> values, <d> differ | lanes <used by the first copy> x 6 | <by the second> x 6"
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

template <int CD>
__global__ void __launch_bounds__(MSR_NT) sums_kernel(const int* bdesc, const double* in, double* out, int total) {
  extern __shared__ __attribute__((aligned(16))) double ws[];
  const int tid = threadIdx.x, wave = tid >> 6;
  const MspLay l = msp_layout(CD, 4, 1);
  for (int form = 0; form < 2; ++form) {
    for (int i = tid; i < total; i += MSR_NT) ws[i] = in[i];
    __syncthreads();
    if (wave >= MSR_W0) {
      MsrW<CD> x;
      msr_setup_sums(x, bdesc, form ? msr_desc_w_base() : 0, l, ws);
      msr_sums(x);
    }
    __syncthreads();
    if (wave == 0) {
      MsrS<CD> x;
      reduce_setup<CD>(x, bdesc, form ? msr_desc_w_base() : 0, l, ws);
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
static int launch(const int* d_desc, const double* d_in, double* d_out, int total) {
  hipLaunchKernelGGL(sums_kernel<CD>, dim3(1), dim3(MSR_NT), (size_t)total * sizeof(double), 0, d_desc, d_in, d_out, total);
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
  std::vector<int> dsc;
  if (c0 < 0 || nd * CD > MSP_TS - 1 || npt > MSR_NL || !msr_build_desc(CD, nd, c0, npt, code, dsc)) { std::printf("rule p=%d CD=%d: does not fit\n", p, CD); return 1; }
  const MspLay l = msp_layout(CD, 4, 1);
  const int total = l.total;
  // every word of both copies addresses the workspace (the kernel reads and writes nothing else)
  for (size_t i = 0; i < (size_t)2 * msr_desc_ints(); ++i) {
    const int w = (int)(i % msr_desc_ints()) % MSR_DW, L = (int)(i % msr_desc_ints()) / MSR_DW;
    const bool flag = L < MSR_NL && (w == MSR_NMEM || w == MSR_NMEM + 1 + 3 * MSR_KT);
    if (!flag && (dsc[i] < 0 || dsc[i] >= total)) { std::printf("rule p=%d CD=%d: descriptor word %zu outside the workspace\n", p, CD, i); return 1; }
  }
  int* d_desc = nullptr; double* d_in = nullptr; double* d_out = nullptr;
  TRY(hipMalloc(&d_desc, dsc.size() * sizeof(int)));
  TRY(hipMalloc(&d_in, (size_t)total * sizeof(double)));
  TRY(hipMalloc(&d_out, 2 * NOUT * sizeof(double)));
  TRY(hipMemcpy(d_desc, dsc.data(), dsc.size() * sizeof(int), hipMemcpyHostToDevice));
  long nval = 0, ndiff = 0;
  for (int seed = 0; seed < NSEED; ++seed) {
    g_rng = 0x9E3779B97F4A7C15ull ^ ((uint64_t)(p * 64 + CD * 8 + seed) * 0x100000001B3ull);
    std::vector<double> in((size_t)total, 0.0);
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
        in[l.c0 + k * MSR_CS + pt] = v;
      }
    TRY(hipMemcpy(d_in, in.data(), in.size() * sizeof(double), hipMemcpyHostToDevice));
    TRY(hipMemset(d_out, 0xFF, 2 * NOUT * sizeof(double)));
    int st = 0;
    switch (CD) {
      case 1: st = launch<1>(d_desc, d_in, d_out, total); break;
      case 2: st = launch<2>(d_desc, d_in, d_out, total); break;
      case 3: st = launch<3>(d_desc, d_in, d_out, total); break;
      case 4: st = launch<4>(d_desc, d_in, d_out, total); break;
      case 5: st = launch<5>(d_desc, d_in, d_out, total); break;
      default: st = launch<6>(d_desc, d_in, d_out, total); break;
    }
    if (st) return st;
    std::vector<double> out(2 * NOUT);
    TRY(hipMemcpy(out.data(), d_out, out.size() * sizeof(double), hipMemcpyDeviceToHost));
    auto bits = [](double v) { uint64_t b; std::memcpy(&b, &v, 8); return b; };
    bool nonzero = false;
    for (int o = 0; o < msp_nacc(CD); ++o) {
      const int* r0 = &dsc[(size_t)MSR_NL * MSR_DW + (size_t)o * MSR_RW];
      const int* r1 = r0 + msr_desc_w_base();
      for (int i : {0, 2, 4, 5}) {      // the level-2 results among the operands (or the zero word, in both copies)
        if ((r0[i] == l.zero) != (r1[i] == l.zero)) { std::printf("rule p=%d CD=%d: sum %d, operand %d: a result in one copy, the zero word in the other\n", p, CD, o, i); return 1; }
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
  TRY(hipFree(d_desc)); TRY(hipFree(d_in)); TRY(hipFree(d_out));
  std::printf("rule p=%d CD=%d npt=%d: %ld values, %ld differ", p, CD, npt, nval, ndiff);
  for (int copy = 0; copy < 2; ++copy) {
    std::printf(" | lanes");
    for (int w = 0; w < MSR_NWK; ++w) {
      int used = 0;
      for (int ln = 0; ln < 64; ++ln) if (dsc[(copy ? msr_desc_w_base() : 0) + (size_t)(w * 64 + ln) * MSR_DW] != l.zero) ++used;
      std::printf(" %d", used);
    }
  }
  std::printf("\n");
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 2) { std::printf("usage: msr_sums_gpu RULES\n"); return 2; }
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
