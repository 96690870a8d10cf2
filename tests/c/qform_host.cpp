// The plain-C++ piece that decides which form of Q / 2Q / v a plan's three-barrier ihgp_adf8_kernel is instantiated with
// (csrc/nagp_qform.hpp), against the rule written out, for every D in 1 .. 63.  Stand-alone: no device, no library.
#include <cstdio>
#include <cstdlib>

#include "nagp_qform.hpp"

using namespace nagp;

static int fails = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++fails; std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

int main() {
  int count[QF_COUNT] = {0, 0, 0, 0};
  for (int D = 1; D <= 63; ++D) {
    // the rule, written out: K is the next of 4, 8, 16 with 4 K >= D; PAD = 4 K > D
    int K = 4;
    while (4 * K < D) K *= 2;
    const bool pad = 4 * K > D;
    CHECK(K == 4 || K == 8 || K == 16, "D = %d: K = %d", D, K);
    CHECK(msp_qterms(D) == K, "D = %d: msp_qterms %d, expected %d", D, msp_qterms(D), K);
    const int qf = qform_pick(D, false);
    int want = QF_RUNTIME;
    if (D == 16) want = QF_K4;
    else if (D == 32) want = QF_K8;
    else if (D > 32) want = QF_K16P;
    CHECK(qf == want, "D = %d: form %d, expected %d", D, qf, want);
    CHECK(qf >= 0 && qf < QF_COUNT, "D = %d: form %d out of range", D, qf);
    ++count[qf];
    // a fixed form carries exactly the (K, PAD) of its D; the run-time form carries none
    if (qf != QF_RUNTIME) {
      CHECK(qform_terms(qf) == K, "D = %d: form %d has K = %d, the shape %d", D, qf, qform_terms(qf), K);
      CHECK(qform_pad(qf) == pad, "D = %d: form %d has PAD = %d, the shape %d", D, qf, (int)qform_pad(qf), (int)pad);
    } else {
      CHECK(pad && K < 16, "D = %d takes the run-time form although its shape (K = %d, PAD = %d) has one of its own", D, K, (int)pad);
      CHECK(qform_terms(qf) == 0, "the run-time form names no K");
    }
    // which forms may run D: the picked one and the run-time one, no other
    for (int f = 0; f < QF_COUNT; ++f)
      CHECK(qform_serves(f, D) == (f == QF_RUNTIME || f == qf), "D = %d: qform_serves(%d) = %d", D, f, (int)qform_serves(f, D));
    // the developer switch: the run-time form for every D
    CHECK(qform_pick(D, true) == QF_RUNTIME, "D = %d: the fallback is not the run-time form", D);
    CHECK(qform_name(qf) != nullptr && qform_name(qf)[0] != 0, "D = %d: no name", D);
  }
  CHECK(count[QF_K4] == 1 && count[QF_K8] == 1 && count[QF_K16P] == 31 && count[QF_RUNTIME] == 30, "counts %d %d %d %d", count[QF_RUNTIME],
        count[QF_K4], count[QF_K8], count[QF_K16P]);
  // outside the range the kernels serve: the run-time form is picked, and nothing serves it
  const int outside[] = {-5, 0, 64, 65, 1000};
  for (int D : outside) {
    CHECK(qform_pick(D, false) == QF_RUNTIME, "D = %d outside 1 .. 63 picked a fixed form", D);
    for (int f = 0; f < QF_COUNT; ++f) CHECK(!qform_serves(f, D), "form %d serves D = %d", f, D);
  }
  if (fails) { std::printf("%d checks failed\n", fails); return 1; }
  std::printf("every D in 1 .. 63 takes the form written out\n");
  return 0;
}
