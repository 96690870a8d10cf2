// nagp_qform.hpp -- how many terms a partial sum of Q / 2Q / v takes (msp_qterms) and which form of msr_qv_serial (nagp_momsp.hpp) a plan's
// three-barrier ihgp_adf8_kernel is instantiated with.  Plain C++: the host's picker, the kernels and tests/c/qform_host.cpp read the same lines.
#pragma once

#if defined(__HIPCC__)
#define NAGP_QF_HD __host__ __device__
#else
#define NAGP_QF_HD
#endif

namespace nagp {

// terms per partial sum: the sub-bands d = sub + 4 q, q < K, cover D <= 4 K
NAGP_QF_HD inline int msp_qterms(int D) { return D <= 16 ? 4 : (D <= 32 ? 8 : 16); }

// Forms of msr_qv_serial.  QF_RUNTIME reads K and PAD = (4 K != D) from the kernel's arguments every step and serves every D; the three
// others fix them at compile time and serve the D they are named for: 4 K = D without padding (D = 16, D = 32), and K = 16, which always
// pads (D + N <= 64 sites, so D < 64).  The remaining padded shapes (D < 16, 16 < D < 32) share QF_RUNTIME.
enum QForm { QF_RUNTIME = 0, QF_K4 = 1, QF_K8 = 2, QF_K16P = 3, QF_COUNT = 4 };

NAGP_QF_HD inline int qform_terms(int qf) { return qf == QF_K4 ? 4 : (qf == QF_K8 ? 8 : (qf == QF_K16P ? 16 : 0)); }
NAGP_QF_HD inline bool qform_pad(int qf) { return qf == QF_K16P; }
// may a kernel of form qf run D sub-bands?
NAGP_QF_HD inline bool qform_serves(int qf, int D) {
  if (D < 1 || D > 63) return false;
  if (qf == QF_RUNTIME) return true;
  return qform_terms(qf) == msp_qterms(D) && qform_pad(qf) == (4 * msp_qterms(D) != D);
}
// the form a plan takes (fallback: the developer switch NAGP_IH_QFORM=0)
NAGP_QF_HD inline int qform_pick(int D, bool fallback) {
  if (fallback || D < 1 || D > 63) return QF_RUNTIME;
  const int K = msp_qterms(D);
  const bool pad = 4 * K != D;
  if (K == 16) return pad ? QF_K16P : QF_RUNTIME;
  if (pad) return QF_RUNTIME;
  return K == 4 ? QF_K4 : QF_K8;
}
inline const char* qform_name(int qf) {
  return qf == QF_K4 ? "K4" : (qf == QF_K8 ? "K8" : (qf == QF_K16P ? "K16-pad" : "run-time"));
}

}  // namespace nagp
