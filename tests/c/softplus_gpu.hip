// softplus_short, log1p_01 and exp_le0 of csrc/nagp_explog.hpp: what the device computes against what the host computes from the same
// text, bit pattern by bit pattern (two NaNs count as equal whatever their payloads).  Stand-alone: prints one line per function,
// "<name>: <arguments> arguments, <n> differ[, first at <bits of the argument>]".
//   softplus_short  2^21 arguments over [-750, 750], 2^21 over [-40, 40], 2^20 over [-2^-10, 2^-10], |z| = 2^(-1074 + 2097 i / 2^19) of
//                   both signs (2^20), the special values and the edges of tests/c/softplus_host.cpp
//   log1p_01        2^21 arguments over [0, 1], 2^20 over [0.5 - 2^-12, 0.5 + 2^-12] (the split), t = 2^(-1074 i / 2^20) (2^20), 0, 1, NaN
//   exp_le0         the arguments -|z| of the first list
#include <hip/hip_runtime.h>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "nagp_explog.hpp"

using namespace nagp;

enum Fn { SOFTPLUS = 0, LOG1P = 1, EXPLE0 = 2, NFN = 3 };

template <int FN>
__host__ __device__ inline double eval(double z) {
  if (FN == SOFTPLUS) return softplus_short(z);
  if (FN == LOG1P) return log1p_01(z);
  return exp_le0(-__builtin_fabs(z));
}
template <int FN>
__global__ void eval_kernel(const double* z, double* out, long n) {
  const long stride = (long)gridDim.x * blockDim.x;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) out[i] = eval<FN>(z[i]);
}

#define TRY(e) do { hipError_t s_ = (e); if (s_ != hipSuccess) { std::printf("HIP error %s at line %d\n", hipGetErrorString(s_), __LINE__); return 2; } } while (0)

static uint64_t bits(double v) { uint64_t u; std::memcpy(&u, &v, 8); return u; }

template <int FN>
static int run(const char* name, const std::vector<double>& z) {
  const long n = (long)z.size();
  double *d_z = nullptr, *d_o = nullptr;
  std::vector<double> got(n);
  TRY(hipMalloc(&d_z, n * sizeof(double)));
  TRY(hipMalloc(&d_o, n * sizeof(double)));
  TRY(hipMemcpy(d_z, z.data(), n * sizeof(double), hipMemcpyHostToDevice));
  TRY(hipMemset(d_o, 0xFF, n * sizeof(double)));
  hipLaunchKernelGGL(eval_kernel<FN>, dim3(512), dim3(256), 0, 0, d_z, d_o, n);
  TRY(hipGetLastError());
  TRY(hipDeviceSynchronize());
  TRY(hipMemcpy(got.data(), d_o, n * sizeof(double), hipMemcpyDeviceToHost));
  TRY(hipFree(d_z));
  TRY(hipFree(d_o));
  long differ = 0;
  uint64_t first = 0;
  for (long i = 0; i < n; ++i) {
    const double want = eval<FN>(z[i]);
    if (std::isnan(want) && std::isnan(got[i])) continue;
    if (bits(want) != bits(got[i])) { if (!differ) first = bits(z[i]); ++differ; }
  }
  std::printf("%s: %ld arguments, %ld differ", name, n, differ);
  if (differ) std::printf(", first at %016llx", (unsigned long long)first);
  std::printf("\n");
  return 0;
}

int main() {
  const double inf = HUGE_VAL, nan1 = std::nan(""), nan2 = -std::nan("0x1234");
  std::vector<double> z, t;
  const long N21 = 1L << 21, N20 = 1L << 20, N19 = 1L << 19;
  for (long i = 0; i < N21; ++i) z.push_back(-750.0 + 1500.0 * ((double)i / (double)(N21 - 1)));
  for (long i = 0; i < N21; ++i) z.push_back(-40.0 + 80.0 * ((double)i / (double)(N21 - 1)));
  for (long i = 0; i < N20; ++i) z.push_back(ldexp((double)(i - N19), -29));
  for (long i = 0; i < N19; ++i) { const double m = exp2(-1074.0 + 2097.0 * ((double)i / (double)(N19 - 1))); z.push_back(m); z.push_back(-m); }
  const double sp[] = {inf, -inf, nan1, nan2, 0.0, -0.0, DBL_MAX, -DBL_MAX, DBL_MIN, -DBL_MIN, 4.9e-324, -4.9e-324, -0.6931471805599453, -0.69314718055994529,
                       -0.6931471805599454, 0.6931471805599453, -36.7368005696771, -708.3964185322641, -745.13321910194122, -745.2, -746.0, -1074.0,
                       -1075.0, -1076.0, 709.782712893384, 710.0, 1024.0, 1e300, -1e300, 1.0, -1.0};
  for (double v : sp) z.push_back(v);
  for (long i = 0; i < N21; ++i) t.push_back((double)i / (double)(N21 - 1));
  for (long i = 0; i < N20; ++i) t.push_back(0.5 + ldexp((double)(i - N19), -31));
  for (long i = 0; i < N20; ++i) t.push_back(exp2(-1074.0 * ((double)i / (double)(N20 - 1))));
  const double tsp[] = {0.0, 1.0, nan1, 0.5, 0.49999999999999994, 0.5000000000000001, 4.9e-324, DBL_MIN, 0x1p-53, 0x1p-52, 0x1.fffffffffffffp-1};
  for (double v : tsp) t.push_back(v);
  int st = run<SOFTPLUS>("softplus_short", z);
  if (st) return st;
  st = run<LOG1P>("log1p_01", t);
  if (st) return st;
  return run<EXPLE0>("exp_le0", z);
}
