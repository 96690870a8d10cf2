// exp_le0, exp_any and log_ge1 of csrc/nagp_explog.hpp against the device library's exp and log, bit pattern by bit pattern, on the
// domain each is written for.  Stand-alone: prints one line per function, "<name>: <arguments> arguments, <n> differ[, largest at <bits of the argument>]".
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "nagp_explog.hpp"

using namespace nagp;

constexpr long NDENSE = 1 << 21;      // arguments of a dense sweep
constexpr int NSPEC = 16;             // special arguments per function (padded with repeats)
enum Fn { EXP_LE0 = 0, EXP_ANY = 1, LOG_GE1 = 2, NFN = 3 };

struct Spec { double x[NFN][NSPEC]; };

__device__ inline unsigned long long bits(double v) { return (unsigned long long)__double_as_longlong(v); }

// argument i of function fn: dense sweeps first, then the neighbours of an edge, then the specials
__device__ double arg_of(int fn, long i, const Spec& sp, long n) {
  if (i >= n - NSPEC) return sp.x[fn][i - (n - NSPEC)];
  if (fn == EXP_LE0) {
    if (i < NDENSE) return -746.0 * ((double)i / (double)(NDENSE - 1));                         // [-746, 0]
    return -708.0 - 38.0 * ((double)(i - NDENSE) / (double)(NDENSE - 1));                       // [-746, -708]: denormal results, the underflow edge
  }
  if (fn == EXP_ANY) {
    if (i < NDENSE) return -746.0 + 1456.0 * ((double)i / (double)(NDENSE - 1));                // [-746, 710]
    return 709.0 + ((double)(i - NDENSE) / (double)(NDENSE - 1));                               // [709, 710]: the overflow edge
  }
  if (i < NDENSE) return exp2(1023.0 * ((double)i / (double)(NDENSE - 1)));                     // [1, 2^1023], log-uniform
  if (i < NDENSE + 1001) return __longlong_as_double(0x3FF0000000000000LL + (i - NDENSE));      // 1 and the 1 000 doubles above it
  return 1.0 + 1.0 * ((double)(i - NDENSE - 1001) / (double)(NDENSE - 1));                      // [1, 2): every exponent of the reduction's split
}

__host__ __device__ inline long count_of(int fn) { return fn == LOG_GE1 ? 2 * NDENSE + 1001 + NSPEC : 2 * NDENSE + NSPEC; }

__global__ void check_kernel(Spec sp, unsigned long long* out /* [NFN][3]: differing, bits of the largest differing argument, evaluated */) {
  const long stride = (long)gridDim.x * blockDim.x;
  for (int fn = 0; fn < NFN; ++fn) {
    const long n = count_of(fn);
    unsigned long long nd = 0, nev = 0, worst = 0;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
      const double x = arg_of(fn, i, sp, n);
      double got, want;
      if (fn == EXP_LE0) { got = exp_le0(x); want = exp(x); }
      else if (fn == EXP_ANY) { got = exp_any(x); want = exp(x); }
      else { got = log_ge1(x); want = log(x); }
      ++nev;
      if (bits(got) != bits(want)) { ++nd; if (bits(x) > worst) worst = bits(x); }
    }
    if (nd) { atomicAdd(&out[3 * fn], nd); atomicMax(&out[3 * fn + 1], worst); }
    atomicAdd(&out[3 * fn + 2], nev);
  }
}

#define TRY(e) do { hipError_t s_ = (e); if (s_ != hipSuccess) { std::printf("HIP error %s at line %d\n", hipGetErrorString(s_), __LINE__); return 2; } } while (0)

int main() {
  Spec sp;
  const double inf = __builtin_inf(), nan1 = __builtin_nan(""), nan2 = -__builtin_nan("0x1234");
  const double le0[NSPEC] = {-0.0, 0.0, -inf, nan1, nan2, -1075.0, -1075.5, -1074.5, -745.2, -745.13321910194122, -1e300, -4.9e-324, -2.2250738585072014e-308, -1e-17, -708.3964185322641, -746.0};
  const double any[NSPEC] = {inf, -inf, nan1, nan2, 1024.0, 1024.5, 1023.9, 709.782712893384, 709.7827128933841, 710.0, 1e300, -1e300, 0.0, -0.0, 4.9e-324, -1075.5};
  const double ge1[NSPEC] = {inf, nan1, nan2, 1.0, 1.7976931348623157e308, 8.98846567431158e307, 1.3333333333333333, 1.3333333333333335, 1.3333333333333330, 2.0, 1.9999999999999998, 4.0, 2.6666666666666665, 2.666666666666667, 1e300, 3.0};
  std::memcpy(sp.x[EXP_LE0], le0, sizeof le0); std::memcpy(sp.x[EXP_ANY], any, sizeof any); std::memcpy(sp.x[LOG_GE1], ge1, sizeof ge1);
  unsigned long long* d_out = nullptr;
  unsigned long long h_out[3 * NFN];
  TRY(hipMalloc(&d_out, sizeof h_out));
  TRY(hipMemset(d_out, 0, sizeof h_out));
  hipLaunchKernelGGL(check_kernel, dim3(512), dim3(256), 0, 0, sp, d_out);
  TRY(hipGetLastError());
  TRY(hipDeviceSynchronize());
  TRY(hipMemcpy(h_out, d_out, sizeof h_out, hipMemcpyDeviceToHost));
  TRY(hipFree(d_out));
  const char* names[NFN] = {"exp_le0", "exp_any", "log_ge1"};
  for (int fn = 0; fn < NFN; ++fn) {
    if (h_out[3 * fn + 2] != (unsigned long long)count_of(fn)) { std::printf("%s: evaluated %llu of %ld arguments\n", names[fn], h_out[3 * fn + 2], count_of(fn)); return 3; }
    std::printf("%s: %ld arguments, %llu differ", names[fn], count_of(fn), h_out[3 * fn]);
    if (h_out[3 * fn]) std::printf(", largest at %016llx", h_out[3 * fn + 1]);
    std::printf("\n");
  }
  return 0;
}
