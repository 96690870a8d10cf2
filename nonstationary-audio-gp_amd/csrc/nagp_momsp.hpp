// nagp_momsp.hpp -- likModulatorNMFPower (matlab/likModulatorNMFPower.m:28-87) for fully symmetric sigma-point sets,
// laid out for the sequential ADF step: one wave per SIMD, every LDS address static and register resident.
//
// The sigma points of ut3/5/7/9_ws (matlab/symmetric-cubature-rules) are the centre plus points with at most four
// non-centre coordinates.  With lk_p = l0 + dev_p (l0 = link at the centre of every modulator, dev_p non-zero in the
// non-centre dimensions only) the per-point quantities of likModulatorNMFPower.m:44-47 become
//   sum_d a_d mu_d   = s0 + sum_r ve[j_r][c_r]                      s0 = v.l0,     ve[j][c] = v_j e_j(c)
//   sum_d a_d^2 s2_d = q0 + sum_r t1[j_r][c_r] + sum_{r<s} 2 Q(j_r,j_s) e_r e_s    q0 = l0'Q l0,  t1 = e (2 (Q l0)_j + Q_jj e)
// with Q = W' diag(s2_z) W, v = W' mu_z (the N x N forms of mom_quad) and e_j(c) = link(xn_{j,c}) - l0_j: a dozen table
// reads per sigma point instead of an N x N quadratic form.  The weighted sums over the points (:59-80) are one 16x16
// block of A'B on v_mfma_f64_16x16x4 exactly as in mom_quad, but every lane's operand addresses are computed ONCE per
// kernel (they depend on the static cubature codes only), so a step of the accumulation is three LDS reads, one multiply
// and the MFMA.  Same arithmetic as the reference up to summation order.
//
// Stages (256 threads = 4 waves; a workgroup barrier between stages):
//   A   wave 0, lane (j,c): link, xg, xg2 tables            | waves 1-3: Q, 2Q, v by 4-lane groups (static W products in LDS)
//   B   wave 0, lane (j,c): e, t1, ve tables                | wave 1: q0, s0
//   1b  one lane per sigma point (<= MSP_NPS per lane): Gaussian weight -> c0, c1, c2
//   2   every wave: its share of the MFMA steps -> 16x16 partial in LDS
//   3   (caller's choice of lanes, after a barrier) fixed-order sum of the partials, outputs d lZ, d2 lZ, Z
#pragma once
#include "nagp_dev.hpp"
#include "nagp_qform.hpp"
#include "nagp_msr_desc.hpp"

namespace nagp {

constexpr int MSP_NT = 256;   // threads per workgroup the stages are written for
constexpr int MSP_NPS = 2;    // sigma points per lane in stage 1b
constexpr int MSP_DT = 16;    // sub-bands per lane of a 4-lane group in stage A (D <= 64)
constexpr int MSP_MAXCD = 7;  // 2*CD + 2 <= 16 rows of the MFMA block

typedef const double __attribute__((address_space(3))) * msp_rp;   // LDS read pointer (32-bit, register resident)
typedef double __attribute__((address_space(3))) * msp_wp;

// terms per lane of the 4-lane groups that form Q and v (stage A): the next of 4, 8, 16 that covers D sub-bands -- msp_qterms, nagp_qform.hpp

// LDS workspace: MspLay, msp_layout and the constants of the role layout (LAY = 1), nagp_msr_desc.hpp
__host__ __device__ inline size_t msp_lds_doubles(int CD, int D, int LAY = 0) { return (size_t)msp_layout(CD, D, LAY).total; }

// 1/x by the hardware estimate and two Newton steps (~1 ulp)
// (x = 0, inf or of underflow size: the refinement is NaN -- callers on such values branch to true divisions)
__device__ __forceinline__ double rcp_nr(double x) {
  double r = __builtin_amdgcn_rcp(x);
  double e = fma(-x, r, 1.0); r = fma(r, e, r);
  e = fma(-x, r, 1.0); r = fma(r, e, r);
  return r;
}
// a zero the compiler cannot see through: added to a wave-uniform LDS address it keeps the address in ONE vector register
// (uniform addresses are otherwise materialised one scalar register per constant offset, and spilled)
__device__ __forceinline__ int opaque_zero() { int z = 0; asm volatile("" : "+v"(z)); return z; }

// Register-resident state of one thread.  Everything here is computed once per kernel.
template <int CD>
struct MspCtx {
  static constexpr int NPS = MSP_NPS, NST = MSP_NST, WSTR = 4 * MSP_NW, NPART = MSP_NW, CS = MSP_CS;
  int lw, qw;          // wave that evaluates the link tables / wave that forms q0, s0 (wave-uniform)
  // stage A / B, wave lw: lane t = j*nd + c
  double xdc; msp_rp a_mu, a_s2, a_l0[CD], a_l0own, a_qrow, a_qjj, a_v; msp_wp a_out;   // a_out[k*MSP_TS]: lk, xg, xg2, e, t1, ve
  // stage B, wave 1: lane L < CD*CD: Q(j,j') l0_j l0_j' ; next CD lanes: v_j l0_j
  int b_kind; msp_rp b_p0, b_p1, b_p2;
  // stage A, waves 1-3: 4-lane group -> one entry of Q (and 2Q) or v
  int q_kind;          // 0: none, 1: Q(j,j'), 2: v(j)
  msp_rp q_ww, q_src;  // products at q_ww[192*q] (zero for sub-bands >= D), operands at q_src[4*q]
  msp_wp q_out0, q_out1, q_out2, q_out3;
  // stage 1b
  msp_rp p_e[MSP_NPS][MSP_NZ], p_q[MSP_NPS][6];   // e at p_e[0], t1 at [MSP_TS], ve at [2*MSP_TS]
  msp_wp p_c[MSP_NPS];
  double p_wn[MSP_NPS];
  bool p_ok[MSP_NPS];
  int p_any[MSP_NPS];  // wave-uniform: some lane of this wave owns a point in the slot
  // stage 2
  msp_rp m_a[MSP_NST], m_b[MSP_NST], m_w0;   // weight of step s at m_w0[WSTR*s]
  msp_wp m_part;       // this wave's 16x16 partial block, + lane
  int nst, m_on;       // steps of this wave; the wave takes part in stage 2 (wave-uniform)
  // partial-sum reduction: lane o < nacc of the reducing wave
  msp_rp r_src; msp_wp r_dst;
  msp_rp accp;         // reduced sums (one vector register, immediate offsets)
};

template <int CD>
__device__ __forceinline__ void msp_setup(MspCtx<CD>& x, const MomCfg& c, const MomSp& sp, const double* Wl /* LDS D x CD */,
                                           const double* fmu, const double* HPH, double* ws, int LW = 0) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nd = c.nd, D = c.D, TN = CD * nd, npt = c.n_pts;
  const MspLay l = msp_layout(CD, D);
  const int oz = opaque_zero();
  // roles: the link tables on wave LW (0: the wave that owns the sites; 1: a kernel that gives the modulator sites to wave 1
  // lets their link evaluation run beside the sub-band sites' serial work), Q / v on the three other waves, q0 / s0 on wave qw
  x.lw = LW; x.qw = (LW == 1) ? 2 : 1;
  const int tl = tid - 64 * LW;                                  // lane index on the link wave
  const int wq = (wave < LW) ? wave : wave - 1;                  // rank among the Q / v waves
  const int Lq = (wave != LW && wave < MSP_NW) ? wq * 64 + lane : -1;   // 0 .. 191
  // constants, zero entries of the tables, zero weights beyond the points
  for (int i = tid; i < 6 * MSP_TS; i += MSP_NT) ws[i] = 0.0;
  if (tid == 0) ws[l.one] = 1.0;
  for (int i = tid; i < 3 * MSP_CS; i += MSP_NT) ws[l.c0 + i] = 0.0;
  // ---- stage A / B of wave 0
  {
    const int t = (tl >= 0 && tl < TN) ? tl : 0;
    const int j = t / nd, cc = t - j * nd;
    x.xdc = c.xd[cc];
    x.a_mu = (msp_rp)(fmu + D + j); x.a_s2 = (msp_rp)(HPH + D + j);
#pragma unroll
    for (int j2 = 0; j2 < CD; ++j2) x.a_l0[j2] = (msp_rp)(ws + l.lk + j2 * nd + sp.c0) + oz;
    x.a_l0own = (msp_rp)(ws + l.lk + j * nd + sp.c0);
    x.a_qrow = (msp_rp)(ws + l.Q + j * CD);
    x.a_qjj = (msp_rp)(ws + l.Q + j * CD + j);
    x.a_v = (msp_rp)(ws + l.v + j);
    x.a_out = (msp_wp)(ws + t);
  }
  // ---- stage B: q0, s0 on wave qw
  {
    const int L = tid - 64 * x.qw;
    x.b_kind = 0; x.b_p0 = x.b_p1 = x.b_p2 = (msp_rp)(ws + l.zero);
    if (L >= 0 && L < CD * CD) {
      const int j = L / CD, j2 = L - j * CD;
      x.b_kind = 1; x.b_p0 = (msp_rp)(ws + l.Q + L); x.b_p1 = (msp_rp)(ws + l.lk + j * nd + sp.c0); x.b_p2 = (msp_rp)(ws + l.lk + j2 * nd + sp.c0);
    } else if (L >= CD * CD && L < CD * CD + CD) {
      const int j = L - CD * CD;
      x.b_kind = 2; x.b_p0 = (msp_rp)(ws + l.v + j); x.b_p1 = (msp_rp)(ws + l.lk + j * nd + sp.c0); x.b_p2 = (msp_rp)(ws + l.one);
    }
  }
  // ---- stage A of waves 1..3
  {
    x.q_kind = 0;
    x.q_out0 = x.q_out1 = x.q_out2 = x.q_out3 = (msp_wp)(ws + l.acc + 127);   // scratch slot
    x.q_ww = x.q_src = (msp_rp)(ws + l.zero);
    const int L = Lq;
    if (L >= 0 && L < 192) {      // the three waves beside the link wave (a larger workgroup's further waves take no part in the cubature)
      const int g = L >> 2, sub = L & 3;
      const int nq = CD * (CD + 1) / 2;
      int j = 0, j2 = 0;
      if (g < nq) {          // upper-triangular pair (j, j2), j <= j2
        int r = g; j = 0;
        while (r >= CD - j) { r -= CD - j; ++j; }
        j2 = j + r;
        x.q_kind = 1;
        x.q_out0 = (msp_wp)(ws + l.Q + j * CD + j2); x.q_out1 = (msp_wp)(ws + l.Q + j2 * CD + j);
        x.q_out2 = (msp_wp)(ws + l.Q2 + j * CD + j2); x.q_out3 = (msp_wp)(ws + l.Q2 + j2 * CD + j);
      } else if (g < nq + CD) {
        j = g - nq; x.q_kind = 2;
        x.q_out0 = (msp_wp)(ws + l.v + j);
      }
      // zero weights for sub-bands >= D: the operand read there (a modulator's entry, or the zero padding of fmu / HPH) is multiplied by 0
      for (int q = 0; q < msp_qterms(D); ++q) {
        const int d = sub + 4 * q;
        double v = 0.0;
        if (x.q_kind && d < D) v = (x.q_kind == 1) ? Wl[d * CD + j] * Wl[d * CD + j2] : Wl[d * CD + j];
        ws[l.wwt + q * 192 + L] = v;
      }
      x.q_ww = (msp_rp)(ws + l.wwt + L);
      x.q_src = (msp_rp)(((x.q_kind == 1) ? HPH : fmu) + sub);
    }
  }
  // ---- stage 1b: slot 0 = point tid; slot 1 = points 256.. on the LAST wave (wave 0 carries the serial stages)
  {
    const msp_rp zero = (msp_rp)(ws + l.zero);
#pragma unroll
    for (int u = 0; u < MSP_NPS; ++u) {
      int p = (u == 0) ? tid : (MSP_NT * u + (tid - (MSP_NT - 64)));
      const bool ok = (tid < MSP_NT) && ((u == 0) ? (p < npt) : (tid >= MSP_NT - 64 && p < npt));
      x.p_ok[u] = ok;
      x.p_any[u] = (__builtin_amdgcn_ballot_w64(ok) != 0) ? 1 : 0;
      if (!ok) p = 0;
      int tj[MSP_NZ];
#pragma unroll
      for (int r = 0; r < MSP_NZ; ++r) {
        tj[r] = ok ? sp.pdesc[(size_t)p * MSP_NZ + r] : -1;
        if (tj[r] >= 0) tj[r] = (tj[r] / nd) * 64 + (tj[r] % nd);      // (j, c) packed as j*64 + c
      }
#pragma unroll
      for (int r = 0; r < MSP_NZ; ++r) x.p_e[u][r] = (tj[r] >= 0) ? (msp_rp)(ws + l.e + (tj[r] >> 6) * nd + (tj[r] & 63)) : zero;
      int pi = 0;
#pragma unroll
      for (int r = 0; r < MSP_NZ; ++r)
#pragma unroll
        for (int s = r + 1; s < MSP_NZ; ++s) {
          x.p_q[u][pi] = (tj[r] >= 0 && tj[s] >= 0) ? (msp_rp)(ws + l.Q2 + (tj[r] >> 6) * CD + (tj[s] >> 6)) : zero;
          ++pi;
        }
      x.p_c[u] = (msp_wp)(ws + l.c0 + p);
      x.p_wn[u] = ok ? c.wn[p] : 0.0;
    }
  }
  // ---- stage 2: wave w takes the steps w', w'+4, ... ; lane (i = lane & 15, kq = lane >> 4) feeds row/col i with point 4*step+kq
  //   A_p = [c2 lk_0..lk_{N-1} | c1 | c0 xg2_0..xg2_{N-1} | c0]      B_p = [lk_0..lk_{N-1} | xg_0..xg_{N-1} | 1]
  {
    const int i = lane & 15, kq = lane >> 4;
    const int nstep = (npt + 3) >> 2;
    // wave 0 goes on to the serial part of the step: it takes the short share
    const int wv = (wave + MSP_NW - 1) % MSP_NW;
    x.nst = (nstep - wv + MSP_NW - 1) / MSP_NW;
    if (x.nst < 0 || wave >= MSP_NW) x.nst = 0;
    int wbase = l.c0;                                // rows without a weight multiply a zero operand
    if (i < CD) wbase = l.c2; else if (i == CD) wbase = l.c1;
    x.m_w0 = (msp_rp)(ws + wbase + 4 * wv + kq);     // point of step s: 4*(wv + 4s) + kq
    x.m_part = (msp_wp)(ws + l.part + ((wave < MSP_NW) ? wave : 0) * 256 + kq * 16 + i);
    x.m_on = (wave < MSP_NW) ? 1 : 0;
#pragma unroll
    for (int s = 0; s < MSP_NST; ++s) {
      const int p = 4 * (wv + MSP_NW * s) + kq;
      const bool ok = (s < x.nst) && (p < npt) && (wave < MSP_NW);
      int offA = l.zero, offB = l.zero;             // beyond the points: zero operands (their weights are zero too)
      if (ok) {
        const unsigned char* cp = c.code + (size_t)p * CD;
        if (i < CD) offA = l.lk + i * nd + cp[i];
        else if (i == CD) offA = l.one;
        else if (i <= 2 * CD) offA = l.xg2 + (i - CD - 1) * nd + cp[i - CD - 1];
        else if (i == 2 * CD + 1) offA = l.one;
        if (i < CD) offB = l.lk + i * nd + cp[i];
        else if (i < 2 * CD) offB = l.xg + (i - CD) * nd + cp[i - CD];
        else if (i == 2 * CD) offB = l.one;
      }
      x.m_a[s] = (msp_rp)(ws + offA); x.m_b[s] = (msp_rp)(ws + offB);
    }
  }
  // ---- reduction of the four 16x16 partials: lane o -> (row, col) of the block
  {
    const int o = lane, nq = CD * (CD + 1) / 2;
    int row = 0, col = 0;
    if (o < CD) { row = CD; col = o; }                                        // u_j
    else if (o < CD + nq) { int r = o - CD, j = 0; while (r >= CD - j) { r -= CD - j; ++j; } row = j; col = j + r; }   // R(j,j'), j <= j'
    else if (o < 2 * CD + nq) { row = 2 * CD + 1; col = CD + (o - CD - nq); }    // g1_j
    else if (o < 3 * CD + nq) { row = CD + 1 + (o - 2 * CD - nq); col = 2 * CD; } // g2_j
    else { row = 2 * CD + 1; col = 2 * CD; }                                      // Z
    x.r_src = (msp_rp)(ws + l.part + row * 16 + col);
    const int ab = (wave == 1) ? 64 : 0;                           // waves 0 and 1 may both reduce: own buffers
    x.r_dst = (msp_wp)(ws + l.acc + ab + o);
    x.accp = (msp_rp)(ws + l.acc + ab) + oz;
  }
}

template <int K>
__device__ __forceinline__ void msp_qsum(msp_rp ww, msp_rp src, double& a0, double& a1) {
  double w[K], v[K];
#pragma unroll
  for (int q = 0; q < K; ++q) { w[q] = ww[192 * q]; v[q] = src[4 * q]; }
#pragma unroll
  for (int q = 0; q < K; q += 2) { a0 = fma(w[q], v[q], a0); a1 = fma(w[q + 1], v[q + 1], a1); }
}

// stage A, link part (wave lw): needs fmu / HPH of the MODULATOR sites; no barrier
template <int CD, class X>
__device__ __forceinline__ void msp_link(const X& x, const MomCfg& c) {
  const int tl = (int)threadIdx.x - 64 * x.lw, TN = CD * c.nd;
  if (tl >= 0 && tl < TN) {
    const double mu = *x.a_mu, s2 = *x.a_s2;
    // sqrt(s2) and 1/s2 through one reciprocal square root -- inside the range where its Newton steps are exact to an ulp; a cavity
    // variance of 1e200 or 1e-200 (the site refresh of an ill-conditioned sweep produces them) takes the square root and the division
    double sg, inv;
    if (s2 > 1e-150 && s2 < 1e150) { const double rs = rsqrt_nr(s2); sg = s2 * rs; inv = rs * rs; }
    else { sg = sqrt(s2); inv = 1.0 / s2; }
    const double xn = mu + sg * x.xdc;                                   // likModulatorNMFPower.m:34
    const double lk = link_eval(c.link_kind, c.link_shift, xn);
    const double xg = (xn - mu) * inv;                                   // (xn - mu_g)./s2_g  (:72)
    x.a_out[0] = lk; x.a_out[MSP_TS] = xg; x.a_out[2 * MSP_TS] = xg * xg - inv;   // :79
  }
}
// msp_link on serial wave 1 of the three-barrier schedule of ihgp_adf8_kernel, with the link's kind a constant of the loop's copy (LK),
// its shift and the lane's part in the tables (on = its lane index < CD nd) in registers set ahead of the loop -- the chain reads no
// kernel argument, whose scalar load would wait for every LDS operation in flight.  The exp link is msp_link's operation for operation
// (exp_any, nagp_explog.hpp: the same bits).  The softplus is softplus_short: max(x, 0) + log1p(exp(-|x|)), which never rounds
// 1 + exp(x) -- about forty instructions fewer than the library's double-double log behind an exp, and closer to the true value than
// link_eval's log(1 + exp(x)), whose bits it therefore is not (the ADF results are held by the multi-precision fixture instead).
template <int CD, int LK, class X>
__device__ __forceinline__ void msr_link_serial(const X& x, bool on, double shift) {
  static_assert(LK == 0 || LK == 1, "softplus or exp");
  if (on) {
    const double mu = *x.a_mu, s2 = *x.a_s2;
    double sg, inv;
    if (s2 > 1e-150 && s2 < 1e150) { const double rs = rsqrt_nr(s2); sg = s2 * rs; inv = rs * rs; }
    else { sg = sqrt(s2); inv = 1.0 / s2; }
    const double xn = mu + sg * x.xdc;                                   // likModulatorNMFPower.m:34
    const double lk = (LK == 0) ? softplus_short(xn - shift) : exp_any(xn);              // link_eval
    const double xg = (xn - mu) * inv;                                   // (xn - mu_g)./s2_g  (:72)
    x.a_out[0] = lk; x.a_out[MSP_TS] = xg; x.a_out[2 * MSP_TS] = xg * xg - inv;   // :79
  }
}
// stage A, Q / 2Q / v part (the three other waves): needs fmu / HPH of the SUB-BAND sites; no barrier
template <int CD, class X>
__device__ __forceinline__ void msp_qv(const X& x, const MomCfg& c) {
  if (x.q_kind) {
    const int K = __builtin_amdgcn_readfirstlane(msp_qterms(c.D));
    double a0 = 0.0, a1 = 0.0;
    if (K == 4) msp_qsum<4>(x.q_ww, x.q_src, a0, a1);
    else if (K == 8) msp_qsum<8>(x.q_ww, x.q_src, a0, a1);
    else msp_qsum<16>(x.q_ww, x.q_src, a0, a1);
    double a = a0 + a1;
    a += dpp_mov<0xB1>(a);
    a += dpp_mov<0x4E>(a);
    if ((threadIdx.x & 3) == 0) {
      if (x.q_kind == 1) { *x.q_out0 = a; *x.q_out1 = a; *x.q_out2 = 2.0 * a; *x.q_out3 = 2.0 * a; }
      else *x.q_out0 = a;
    }
  }
}
// stage A.  Needs fmu / HPH of all sites visible; ends WITHOUT a barrier (the caller places it).
template <int CD>
__device__ __forceinline__ void msp_stageA(const MspCtx<CD>& x, const MomCfg& c) {
  const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  if (wave >= MSP_NW) return;
  if (wave == __builtin_amdgcn_readfirstlane(x.lw)) msp_link<CD>(x, c); else msp_qv<CD>(x, c);
}

// stage B, table part (lanes t < CD*nd of the link wave): e, t1, ve from lk, Q, v
template <int CD, class X>
__device__ __forceinline__ void msp_tables(const X& x, const MomCfg& c) {
  const int TN = CD * c.nd;
  if (((int)threadIdx.x & 63) < TN) {
    // every operand first -- ONE LDS round trip (left to itself the compiler reads a pair, waits, multiplies, reads the next pair: a dozen
    // round trips of ~100 cycles on a wave that has its SIMD to itself) -- then arithmetic, then the three stores
    double lk = ((msp_rp)x.a_out)[0], l0o = *x.a_l0own, qjj = *x.a_qjj, vv = *x.a_v;
    double qr[CD], l0v[CD];
#pragma unroll
    for (int j2 = 0; j2 < CD; ++j2) { qr[j2] = x.a_qrow[j2]; l0v[j2] = *x.a_l0[j2]; }
#pragma unroll
    for (int j2 = 0; j2 < CD; ++j2) asm volatile("" : "+v"(qr[j2]), "+v"(l0v[j2]));
    asm volatile("" : "+v"(lk), "+v"(l0o), "+v"(qjj), "+v"(vv));
    double ql0 = 0.0, ql1 = 0.0;
#pragma unroll
    for (int j2 = 0; j2 < CD; ++j2) { if (j2 & 1) ql1 = fma(qr[j2], l0v[j2], ql1); else ql0 = fma(qr[j2], l0v[j2], ql0); }
    const double ql = ql0 + ql1;
    const double e = lk - l0o;
    x.a_out[3 * MSP_TS] = e;
    x.a_out[4 * MSP_TS] = e * fma(qjj, e, 2.0 * ql);
    x.a_out[5 * MSP_TS] = vv * e;
  }
}
// the e table alone (direct form of the role layout, msr_stage1b_direct: t1, ve, q0, s0 have no reader there); e = lk - l0 is read by
// level 2 of msr_sums, behind the barrier that follows the weights
template <int CD, class X>
__device__ __forceinline__ void msr_etable(const X& x, const MomCfg& c) {
  const int TN = CD * c.nd;
  if (((int)threadIdx.x & 63) < TN) {
    const double lk = ((msp_rp)x.a_out)[0], l0o = *x.a_l0own;
    x.a_out[3 * MSP_TS] = lk - l0o;
  }
}
// stage B, q0 = l0' Q l0 and s0 = v' l0 (one wave)
template <class X>
__device__ __forceinline__ void msp_q0s0(const X& x, double* q0, double* s0) {
  const double t = (*x.b_p0) * (*x.b_p1) * (*x.b_p2);      // unused lanes: zero * ...
  double tq = (x.b_kind == 1) ? t : 0.0, tsv = (x.b_kind == 2) ? t : 0.0;
  tq = wave_sum(tq);
  tsv = wave_sum(tsv);
  if (((int)threadIdx.x & 63) == 0) { *q0 = tq; *s0 = tsv; }
}
// the same, one sum per wave (role layout): the wave holding the Q terms writes q0, the wave holding the v terms writes s0
template <class X>
__device__ __forceinline__ void msr_q0_or_s0(const X& x, bool is_q0, double* q0, double* s0) {
  const double t = (*x.b_p0) * (*x.b_p1) * (*x.b_p2);      // unused lanes: zero * ...
  const double sum = wave_sum(t);
  if (((int)threadIdx.x & 63) == 0) { if (is_q0) *q0 = sum; else *s0 = sum; }
}
// stage B.  After a barrier behind stage A; ends without a barrier.
template <int CD>
__device__ __forceinline__ void msp_stageB(const MspCtx<CD>& x, const MomCfg& c, double* ws) {
  const MspLay l = msp_layout(CD, c.D);
  const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  if (wave == __builtin_amdgcn_readfirstlane(x.lw)) msp_tables<CD>(x, c);
  else if (wave == __builtin_amdgcn_readfirstlane(x.qw)) msp_q0s0(x, ws + l.q0, ws + l.s0);
}

// stage 1b.  After a barrier behind stage B; ends without a barrier.
template <int CD, class X>
__device__ __forceinline__ void msp_stage1b_qs(const X& x, const MomCfg& c, const MomSp& sp, double sn2a, double y, double q0, double s0);
template <int CD, class X>
__device__ __forceinline__ void msp_stage1b(const X& x, const MomCfg& c, const MomSp& sp, double sn2a, double y, const double* ws) {
  const MspLay l = msp_layout(CD, c.D);      // q0, s0 sit at the same offsets in both layouts
  msp_stage1b_qs<CD>(x, c, sp, sn2a, y, ws[l.q0], ws[l.s0]);
}
template <int CD, class X>
__device__ __forceinline__ void msp_stage1b_qs(const X& x, const MomCfg& c, const MomSp& sp, double sn2a, double y, double q0, double s0) {
  const bool four = __builtin_amdgcn_readfirstlane(sp.nzmax > 3 ? 1 : 0) != 0;
  const bool three = __builtin_amdgcn_readfirstlane(sp.nzmax > 2 ? 1 : 0) != 0;
#pragma unroll
  for (int u = 0; u < X::NPS; ++u) {
    if (__builtin_amdgcn_readfirstlane(x.p_any[u]) == 0) continue;   // wave-uniform skip
    // all table entries of the point first (one LDS round trip; the entries of components a point does not have are reads of the zero
    // word), then arithmetic in the order of the reference form
    double ev[MSP_NZ], tv[MSP_NZ], vv[MSP_NZ], qv[6];
#pragma unroll
    for (int r = 0; r < MSP_NZ; ++r) {
      const bool on = r < 2 || (r == 2 && three) || (r == 3 && four);
      ev[r] = tv[r] = vv[r] = 0.0;
      if (on) { ev[r] = x.p_e[u][r][0]; tv[r] = x.p_e[u][r][MSP_TS]; vv[r] = x.p_e[u][r][2 * MSP_TS]; }
    }
    qv[0] = *x.p_q[u][0];
    qv[1] = qv[2] = qv[3] = qv[4] = qv[5] = 0.0;
    if (three) { qv[1] = *x.p_q[u][1]; qv[3] = *x.p_q[u][3]; }
    if (four) { qv[2] = *x.p_q[u][2]; qv[4] = *x.p_q[u][4]; qv[5] = *x.p_q[u][5]; }
#pragma unroll
    for (int r = 0; r < MSP_NZ; ++r) asm volatile("" : "+v"(ev[r]), "+v"(tv[r]), "+v"(vv[r]));
#pragma unroll
    for (int r = 0; r < 6; ++r) asm volatile("" : "+v"(qv[r]));
    const double e0 = ev[0], e1 = ev[1];
    double sam = (s0 + vv[0]) + vv[1];
    double sa2 = (q0 + tv[0]) + tv[1];
    double cr = qv[0] * e0 * e1;
    if (three) {
      const double e2 = ev[2];
      sam += vv[2]; sa2 += tv[2];
      cr = fma(qv[1] * e0, e2, cr);
      cr = fma(qv[3] * e1, e2, cr);
      if (four) {
        const double e3 = ev[3];
        sam += vv[3]; sa2 += tv[3];
        cr = fma(qv[2] * e0, e3, cr);
        cr = fma(qv[4] * e1, e3, cr);
        cr = fma(qv[5] * e2, e3, cr);
      }
    }
    sa2 += cr;
    double pdf, q, inv;
    gauss_terms(y, sam, sn2a + sa2, pdf, q, inv);
    const double w0 = x.p_wn[u] * pdf;
    if (x.p_ok[u]) {
      x.p_c[u][0] = w0;
      x.p_c[u][X::CS] = w0 * q;
      x.p_c[u][2 * X::CS] = w0 * (q * q - inv);
    }
  }
}

// stage 1b of the role layout in the DIRECT form (likModulatorNMFPower.m:44-47 as written): with Q = W' diag(s2) W and v = W' mu
// behind the barrier that follows msp_qv,
//   sum_d a_d mu_d = v . lk_p,      sum_d a_d^2 s2_d = lk_p' Q lk_p = sum_j lk_j (Q_jj lk_j + sum_{j2 > j} 2 Q_jj2 lk_j2)
// with lk_pj = link table[j][c_pj]: CD reads at static per-lane addresses, Q (diagonal) / 2Q (above it) / v at wave-uniform addresses
// (broadcast reads), all issued before the first FMA; CD independent chains, no cross-lane operation.  Needs nothing of stage B: no
// e / t1 / ve tables, no q0 / s0, no barrier between msp_qv's and this stage's.  Every term is positive for W >= 0, lk > 0 (no
// cancellation, where the centre + deviation form of msp_stage1b_qs adds terms of both signs).  Lanes without a point read the zero word.
// LE0: the weights' exp as exp_le0 (nagp_explog.hpp; the three-barrier schedule of ihgp_adf8_kernel)
template <int CD, bool LE0 = false, class X>
__device__ __forceinline__ void msr_stage1b_direct(const X& x, double sn2a, double y) {
  if (__builtin_amdgcn_readfirstlane(x.p_any[0]) == 0) return;   // wave-uniform skip
  constexpr int NO = CD * (CD - 1) / 2;
  double lk[CD], qd[CD], vv[CD], qo[NO + 1];
#pragma unroll
  for (int j = 0; j < CD; ++j) { lk[j] = *x.d_lk[j]; qd[j] = x.d_qv[j * CD + j]; vv[j] = x.d_qv[2 * CD * CD + j]; }
  {
    int q = 0;
#pragma unroll
    for (int j = 0; j < CD; ++j)
#pragma unroll
      for (int j2 = j + 1; j2 < CD; ++j2) { qo[q] = x.d_qv[CD * CD + j * CD + j2]; ++q; }
  }
#pragma unroll
  for (int j = 0; j < CD; ++j) asm volatile("" : "+v"(lk[j]), "+v"(qd[j]), "+v"(vv[j]));
#pragma unroll
  for (int q = 0; q < NO; ++q) asm volatile("" : "+v"(qo[q]));
  double a0 = 0.0, a1 = 0.0;
#pragma unroll
  for (int j = 0; j < CD; ++j) { if (j & 1) a1 = fma(vv[j], lk[j], a1); else a0 = fma(vv[j], lk[j], a0); }
  const double sam = a0 + a1;
  // the rows' chains are independent (row j: CD - j operations); the two sums take the short rows first
  double t[CD];
  {
    int q = 0;
#pragma unroll
    for (int j = 0; j < CD; ++j) {
      t[j] = qd[j] * lk[j];
#pragma unroll
      for (int j2 = j + 1; j2 < CD; ++j2) { t[j] = fma(qo[q], lk[j2], t[j]); ++q; }
    }
  }
  double b0 = 0.0, b1 = 0.0;
#pragma unroll
  for (int j = CD - 1; j >= 0; --j) { if (j & 1) b1 = fma(lk[j], t[j], b1); else b0 = fma(lk[j], t[j], b0); }
  const double sa2 = b0 + b1;
  double pdf, q, inv;
  gauss_terms<LE0>(y, sam, sn2a + sa2, pdf, q, inv);
  const double w0 = x.p_wn[0] * pdf;
  if (x.p_ok[0]) {
    if constexpr (X::PLACED) {
      x.p_c[0][0] = w0;
      x.p_c1[0][0] = w0 * q;
      x.p_c2[0][0] = w0 * (q * q - inv);
    } else {
      x.p_c[0][0] = w0;
      x.p_c[0][X::CS] = w0 * q;
      x.p_c[0][2 * X::CS] = w0 * (q * q - inv);
    }
  }
}

// stage 2.  After a barrier behind stage 1b; leaves this wave's 16x16 partial in LDS, no barrier.
// Two accumulators (the dependent-accumulator latency of the f64 MFMA is longer than its issue time) and the operands of
// the next four steps in flight while the current four multiply.
template <int CD, class X>
__device__ __forceinline__ void msp_stage2(const X& x, const MomCfg& c, double* ws) {
  if (__builtin_amdgcn_readfirstlane(x.m_on) == 0) return;      // a wave outside the stage has no partial block
  const int nst = __builtin_amdgcn_readfirstlane(x.nst);
  constexpr int NST = X::NST, WS = X::WSTR;
  v4d acc0 = {0.0, 0.0, 0.0, 0.0}, acc1 = {0.0, 0.0, 0.0, 0.0};
  double a[4], bb[4], w[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) { a[u] = *x.m_a[u]; bb[u] = *x.m_b[u]; w[u] = x.m_w0[WS * u]; }
#pragma unroll
  for (int s0 = 0; s0 < NST; s0 += 4) {
    if (s0 < nst) {      // uniform; steps beyond nst inside the group of four carry zero operands
      double an[4], bn[4], wn_[4];
      if (s0 + 4 < NST) {
#pragma unroll
        for (int u = 0; u < 4; ++u) { an[u] = *x.m_a[s0 + 4 + u]; bn[u] = *x.m_b[s0 + 4 + u]; wn_[u] = x.m_w0[WS * (s0 + 4 + u)]; }
      }
      acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(a[0] * w[0], bb[0], acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(a[1] * w[1], bb[1], acc1, 0, 0, 0);
      acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(a[2] * w[2], bb[2], acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(a[3] * w[3], bb[3], acc1, 0, 0, 0);
      if (s0 + 4 < NST) {
#pragma unroll
        for (int u = 0; u < 4; ++u) { a[u] = an[u]; bb[u] = bn[u]; w[u] = wn_[u]; }
      }
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) x.m_part[64 * r] = acc0[r] + acc1[r];      // element (kq + 4r, i) of the block
}

// fixed-order sum of the partials: lanes o < msp_nacc(CD) of ONE wave; the same wave may read acc after msp_wave_fence()
template <int CD, class X>
__device__ __forceinline__ void msp_reduce(const X& x) {
  const int lane = threadIdx.x & 63;
  if (lane < msp_nacc(CD)) {
    double a = x.r_src[0];
#pragma unroll
    for (int w = 1; w < X::NPART; ++w) a += x.r_src[256 * w];
    *x.r_dst = a;
  }
}
// orders the LDS traffic of one wave (DS operations of a wave complete in issue order; no workgroup barrier)
__device__ __forceinline__ void msp_wave_fence() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

// acc layout: [u: CD][R upper, row-major: CD(CD+1)/2][g1: CD][g2: CD][Z]
// sub-band site (sub): s1 = W_n . u, s2 = W_n' R W_n ;  modulator site j: s1 = g1_j, s2 = g2_j
// returns d lZ and d2 lZ (likModulatorNMFPower.m:59-80); Z = pEP*max(sum, jitter) (:55)
template <int CD>
__device__ __forceinline__ void msp_outputs(msp_rp acc, bool sub, int jmod, const double* wrow, double pEP, double jitter,
                                            double& Z, double& d1, double& d2) {
  constexpr int nq = CD * (CD + 1) / 2;
  const double Zs = acc[3 * CD + nq];
  Z = pEP * ((Zs > jitter) ? Zs : jitter);          // max(NaN, jitter) = jitter
  const double Zinv = pEP * rcp_nr(Z);              // Z >= pEP*jitter > 0, finite (or inf: Zinv = NaN like inf/inf)
  double s1, s2;
  if (sub) {
    // all reads first (one LDS round trip), then arithmetic only
    double av[CD + nq];
#pragma unroll
    for (int q = 0; q < CD + nq; ++q) av[q] = acc[q];
#pragma unroll
    for (int q = 0; q < CD + nq; ++q) asm volatile("" : "+v"(av[q]));
    double a0 = 0.0, a1 = 0.0;
#pragma unroll
    for (int j = 0; j < CD; ++j) { if (j & 1) a1 = fma(wrow[j], av[j], a1); else a0 = fma(wrow[j], av[j], a0); }
    s1 = a0 + a1;
    // w'Rw = sum_j 2 w_j (R_jj w_j / 2 + sum_{j2 > j} R_jj2 w_j2): CD independent chains, then one
    double b0 = 0.0, b1 = 0.0;
    int q = 0;
#pragma unroll
    for (int j = 0; j < CD; ++j) {
      double t = 0.5 * av[CD + q] * wrow[j]; ++q;
#pragma unroll
      for (int j2 = j + 1; j2 < CD; ++j2) { t = fma(av[CD + q], wrow[j2], t); ++q; }
      if (j & 1) b1 = fma(2.0 * wrow[j], t, b1); else b0 = fma(2.0 * wrow[j], t, b0);
    }
    s2 = b0 + b1;
  } else {
    s1 = acc[CD + nq + jmod];
    s2 = acc[2 * CD + nq + jmod];
  }
  d1 = Zinv * s1;
  d2 = fma(-d1, d1, Zinv * s2);
}

// msp_outputs where the lane's kind is a constant of the caller's copy of the loop (the serial waves of the three-barrier schedule of
// ihgp_adf8_kernel): Z's sum and the lane's own sums -- 27 words at CD = 6 on a sub-band lane, two on a modulator lane -- leave in ONE batch
// of LDS reads ahead of any arithmetic.  A modulator lane's arithmetic is msp_outputs', operation for operation.  A sub-band lane forms
// w'Rw = sum_q P_q R_q from the lane's static products P (msp_wproducts: W_dj W_dj', doubled off the diagonal, in the order of R's upper
// triangle): one FMA per entry of R in two chains, where msp_outputs scales and multiplies by the W row twice -- the same sum in exact
// arithmetic, another order of roundings.  s1 = w'u is msp_outputs'.
template <int CD>
__device__ __forceinline__ void msp_wproducts(const double* wrow, bool plain_offdiag, double* pw /* [CD (CD + 1) / 2] */) {
  int q = 0;
#pragma unroll
  for (int j = 0; j < CD; ++j)
#pragma unroll
    for (int j2 = j; j2 < CD; ++j2) {
      // plain_offdiag: developer switch (bit 64 of NAGP_STAMP_WORKER) -- the off-diagonal entries NOT doubled, the wrong table a test shows to fail
      pw[q] = (j2 == j || plain_offdiag) ? wrow[j] * wrow[j2] : (2.0 * wrow[j]) * wrow[j2];
      ++q;
    }
}
template <int CD, bool SUB>
__device__ __forceinline__ void msp_outputs_b(msp_rp acc, int jmod, const double* wrow, const double* pw, double pEP, double jitter,
                                              double& Z, double& d1, double& d2) {
  constexpr int nq = CD * (CD + 1) / 2;
  constexpr int NR = SUB ? CD + nq : 2;
  double av[NR];
  double Zs = acc[3 * CD + nq];
  if constexpr (SUB) {
#pragma unroll
    for (int q = 0; q < NR; ++q) av[q] = acc[q];
  } else {
    av[0] = acc[CD + nq + jmod]; av[1] = acc[2 * CD + nq + jmod];
  }
  asm volatile("" : "+v"(Zs));
#pragma unroll
  for (int q = 0; q < NR; ++q) asm volatile("" : "+v"(av[q]));
  Z = pEP * __builtin_fmax(Zs, jitter);             // (Zs > jitter) ? Zs : jitter as the maximum instruction: max(NaN, jitter) = jitter
  const double Zinv = pEP * rcp_nr(Z);              // Z >= pEP*jitter > 0, finite (or inf: Zinv = NaN like inf/inf)
  double s1, s2;
  if constexpr (SUB) {
    double a0 = 0.0, a1 = 0.0;
#pragma unroll
    for (int j = 0; j < CD; ++j) { if (j & 1) a1 = fma(wrow[j], av[j], a1); else a0 = fma(wrow[j], av[j], a0); }
    s1 = a0 + a1;
    double b0 = 0.0, b1 = 0.0;
#pragma unroll
    for (int q = 0; q < nq; ++q) { if (q & 1) b1 = fma(pw[q], av[CD + q], b1); else b0 = fma(pw[q], av[CD + q], b0); }
    s2 = b0 + b1;
  } else {
    s1 = av[0]; s2 = av[1];
  }
  d1 = Zinv * s1;
  d2 = fma(-d1, d1, Zinv * s2);
}

// msp_outputs_b<CD, true> on both halves of wave 0 (D <= 32: lanes 32 .. 63 carry no sub-band of their own).  The CD + CD (CD + 1) / 2 terms
// of a sub-band -- w_j u_j, then P_q R_q in the order of the acc layout -- are split between lane d, which takes the first NL =
// msp_half_terms (all of s1 = w'u and the first NL - CD terms of s2), and lane d + 32, which takes the rest of s2.  Each lane reads only
// its own NL words (acc_lane = acc + NL on the upper half) against NL static coefficients (msp_half_coeffs; the lane's registers for pw
// hold them); the upper half's partial sum comes down with v_permlane32_swap_b32 and one addition follows.  s1 is msp_outputs_b's,
// operation for operation; s2 is the same sum in another order of roundings.  Every lane of the wave calls this (the swap reads the upper
// half); Z, d1, d2 mean something on lanes d < D only.
template <int CD>
__host__ __device__ constexpr int msp_half_terms() { return (CD + CD * (CD + 1) / 2 + 1) / 2; }
template <int CD>
__device__ __forceinline__ void msp_half_coeffs(const double* wrow, bool upper, double* pw /* [CD (CD + 1) / 2]: the products in, the lane's coefficients out */) {
  constexpr int nq = CD * (CD + 1) / 2, NT = CD + nq, NL = msp_half_terms<CD>();
  double c[NT];
#pragma unroll
  for (int j = 0; j < CD; ++j) c[j] = wrow[j];
#pragma unroll
  for (int q = 0; q < nq; ++q) c[CD + q] = pw[q];
#pragma unroll
  for (int i = 0; i < nq; ++i) pw[i] = (i < NL) ? (upper ? ((NL + i < NT) ? c[NL + i] : 0.0) : c[i]) : 0.0;
}
template <int CD>
__device__ __forceinline__ void msp_outputs_h(msp_rp acc, msp_rp acc_lane, const double* hc, bool upper, double pEP, double jitter, double& Z, double& d1, double& d2) {
  constexpr int nq = CD * (CD + 1) / 2, NT = CD + nq, NL = msp_half_terms<CD>();
  static_assert(NL >= CD && NL <= nq, "the lower half holds all of s1; the coefficients fit the registers of the products");
  double av[NL];
  double Zs = acc[3 * CD + nq];
#pragma unroll
  for (int i = 0; i < NL; ++i) av[i] = acc_lane[i];
  asm volatile("" : "+v"(Zs));
#pragma unroll
  for (int i = 0; i < NL; ++i) asm volatile("" : "+v"(av[i]));
  if constexpr ((NT & 1) != 0) av[NL - 1] = upper ? 0.0 : av[NL - 1];      // the upper half has one term less: its last word is not one of R's
  Z = pEP * __builtin_fmax(Zs, jitter);
  const double Zinv = pEP * rcp_nr(Z);
  double a0 = 0.0, a1 = 0.0;      // the first CD terms: s1 on the lower half
#pragma unroll
  for (int j = 0; j < CD; ++j) { if (j & 1) a1 = fma(hc[j], av[j], a1); else a0 = fma(hc[j], av[j], a0); }
  const double pa = a0 + a1;
  double b0 = 0.0, b1 = 0.0;      // the others: terms of s2 on both halves
#pragma unroll
  for (int i = CD; i < NL; ++i) { if (i & 1) b1 = fma(hc[i], av[i], b1); else b0 = fma(hc[i], av[i], b0); }
  const double pb = b0 + b1;
  const double t = pa + pb;       // the upper half's share of s2
  typedef unsigned int u2v __attribute__((ext_vector_type(2)));
  unsigned long long tb;
  __builtin_memcpy(&tb, &t, 8);
  const unsigned int tlo = (unsigned int)tb, thi = (unsigned int)(tb >> 32);
  // (the swap exchanges lanes 32 .. 63 of its first operand with lanes 0 .. 31 of its second: the second result holds, on lane l < 32, lane l + 32)
  const u2v slo = __builtin_amdgcn_permlane32_swap(tlo, tlo, false, false), shi = __builtin_amdgcn_permlane32_swap(thi, thi, false, false);
  const unsigned long long ub = ((unsigned long long)shi.y << 32) | slo.y;
  double tu;
  __builtin_memcpy(&tu, &ub, 8);
  const double s1 = pa, s2 = pb + tu;
  d1 = Zinv * s1;
  d2 = fma(-d1, d1, Zinv * s2);
}

// =====================================================================================================================
// Role layout (LAY = 1): 512 threads.  Waves 0 and 1 carry the serial stages of the caller (wave 1 also evaluates the link
// tables and e -- with t1 / ve in the table form of stage 1b); waves 2 .. 7 carry the parallel ones: Q / 2Q / v on waves 2..4 (three-barrier schedule of ihgp_adf8_kernel: on wave 0, msr_qv_serial),
// (table form: q0 / s0 on waves 5 / 6), one sigma point per lane of the six (<= 384 points), the cubature sums round the six.  The two roles run in separate loops of the
// kernel, so a wave holds the registers of its own role only: two waves per SIMD within 256 registers each.
//
// The cubature sums (likModulatorNMFPower.m:59-80) from BIN SUMS over static member lists, on the VALU.  Every sigma point
// differs from the centre in at most four coordinates, so with lk_pj = l0_j + e_j(c_pj) (e_j(centre) = 0) and
//   S_k = sum_p c_k,p  (k = 0, 1, 2),   Ck(j,c) = sum of c_k over the points whose coordinate j is the non-centre value c,
//   C2(j,c; j',c') = the same sum of c2 over the points that have both,
// the 40 sums of a step (msp_nacc) are
//   Z = S0,   u_j = S1 l0_j + U_j,   U_j = sum_c C1(j,c) e_j(c)
//   R_jj' = S2 l0_j l0_j' + l0_j' E_j + l0_j E_j' + P_jj',   E_j = sum_c C2(j,c) e_j(c),
//   P_jj' = sum_{c,c'} C2(j,c; j',c') e_j(c) e_j'(c')  (j != j'),   P_jj = sum_c C2(j,c) e_j(c)^2
//   g1_j = sum_c C0(j,c) xg_j(c)  (xg of the centre is zero),   g2_j = G2_j + S0 xg2_j(centre),
//   G2_j = sum_c C0(j,c) (xg2_j(c) - xg2_j(centre))  [the centre bin is S0 - sum_c C0(j,c)]
// In exact arithmetic these are the dense sums sum_p c_k,p lk_pj lk_pj' ...; only the order of summation differs, and every
// term is bounded by |c2| (|l0| + |e|)^2 -- the bound of the terms of the dense sum -- so the rounding error is of its size.
// Level 1: each worker lane adds <= MSR_NMEM weights of one bin (bins of up to 64 members span an aligned group of 2 or 4
// lanes, combined by DPP); level 2: each worker lane forms <= MSR_KT products bin * table * table of bins of ITS OWN wave
// (behind msp_wave_fence, no barrier) -- U, E, P, g1, G2, S; msr_reduce on the serial waves combines them as above.  The
// member and term lists are static: the host builds them once per plan (msr_build_desc, nagp_msr_desc.hpp) into MomSp::bdesc.
constexpr int MSR_NT = 512;
constexpr int MSR_W0 = 2;      // first worker wave
// (MSR_KT, MSR_DW, MSR_RW, MSR_NL, MSR_MONE, msr_desc_ints and the second copy of the lists: nagp_msr_desc.hpp)

template <int CD>
struct MsrS {
  int lw;
  double xdc; msp_rp a_mu, a_s2, a_l0[CD], a_l0own, a_qrow, a_qjj, a_v; msp_wp a_out;
  msp_rp r_p[MSR_RW]; msp_wp r_dst; msp_rp accp;
};
// PL: the point's three weights are stored through three addresses of their own, p_c / p_c1 / p_c2 (the placed copy of the lists and its
// position tables, nagp_msr_desc.hpp: msr_place_weights); otherwise at p_c + k CS, and p_c1 / p_c2 have no reader
template <int CD, bool PL = false>
struct MsrW {
  static constexpr int NPS = 1, CS = MSR_CS;
  static constexpr bool PLACED = PL;
  int q_kind; msp_rp q_ww, q_src; msp_wp q_out0, q_out1, q_out2, q_out3;
  int b_kind; msp_rp b_p0, b_p1, b_p2;
  msp_rp p_e[1][MSP_NZ], p_q[1][6]; msp_wp p_c[1], p_c1[1], p_c2[1]; double p_wn[1]; bool p_ok[1]; int p_any[1];   // (p_e, p_q: table form of stage 1b)
  msp_rp d_lk[CD], d_qv;                                              // direct form of stage 1b: this point's link entries; Q | 2Q | v (uniform)
  msp_rp s_mem[MSR_NMEM]; msp_wp s_out; int s_grp;                    // level 1: members, result slot, group flags (1: lane ^ 1, 2: lane ^ 2)
  msp_rp t_bin[MSR_KT], t_fa[MSR_KT], t_fb[MSR_KT]; msp_wp t_out; int t_grp;   // level 2
};

// constants, zero entries of the tables, zero weights beyond the points (every thread of the workgroup)
__device__ __forceinline__ void msr_init(int CD, int D, double* ws) {
  const MspLay l = msp_layout(CD, D, 1);
  for (int i = threadIdx.x; i < 6 * MSP_TS; i += MSR_NT) ws[i] = 0.0;
  if (threadIdx.x == 0) ws[l.one] = 1.0;
  for (int i = threadIdx.x; i < 3 * MSR_CS; i += MSR_NT) ws[l.c0 + i] = 0.0;
  for (int i = threadIdx.x; i <= MSR_MONE; i += MSR_NT) ws[l.part + i] = (i == MSR_MONE) ? -1.0 : 0.0;
}

template <int CD>
__device__ __forceinline__ void msr_setup_S(MsrS<CD>& x, const MomCfg& c, const MomSp& sp, const double* fmu, const double* HPH, double* ws,
                                             int dbase = 0 /* copy of the lists: 0 or msr_desc_w_base() */) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nd = c.nd, D = c.D, TN = CD * nd;
  const MspLay l = msp_layout(CD, D, 1);
  const int oz = opaque_zero();
  x.lw = 1;
  {
    const int tl = tid - 64;
    const int t = (tl >= 0 && tl < TN) ? tl : 0;
    const int j = t / nd, cc = t - j * nd;
    x.xdc = c.xd[cc];
    x.a_mu = (msp_rp)(fmu + D + j); x.a_s2 = (msp_rp)(HPH + D + j);
#pragma unroll
    for (int j2 = 0; j2 < CD; ++j2) x.a_l0[j2] = (msp_rp)(ws + l.lk + j2 * nd + sp.c0) + oz;
    x.a_l0own = (msp_rp)(ws + l.lk + j * nd + sp.c0);
    x.a_qrow = (msp_rp)(ws + l.Q + j * CD);
    x.a_qjj = (msp_rp)(ws + l.Q + j * CD + j);
    x.a_v = (msp_rp)(ws + l.v + j);
    x.a_out = (msp_wp)(ws + t);
  }
  {
    const int* d = sp.bdesc + dbase + (size_t)MSR_NL * MSR_DW + (size_t)lane * MSR_RW;
#pragma unroll
    for (int i = 0; i < MSR_RW; ++i) x.r_p[i] = (msp_rp)(ws + d[i]);
    const int ab = (wave == 1) ? 64 : 0;
    x.r_dst = (msp_wp)(ws + l.acc + ab + lane);
    x.accp = (msp_rp)(ws + l.acc + ab) + oz;
  }
}

// the cubature sums' part of a worker lane's state: its members and terms (host lists, msr_build_desc; offsets in doubles from ws, unused
// entries address the zero word).  dbase: the copy of the lists, 0 or msr_desc_w_base() (nagp_msr_desc.hpp)
template <class X>
__device__ __forceinline__ void msr_setup_sums(X& x, const int* bdesc, int dbase, const MspLay& l, double* ws) {
  const int lane = threadIdx.x & 63, wr = ((int)threadIdx.x >> 6) - MSR_W0;
  const bool worker = wr >= 0 && wr < MSR_NWK;
  const int L = worker ? wr * 64 + lane : 0;
  const int* d = bdesc + dbase + (size_t)L * MSR_DW;
#pragma unroll
  for (int k = 0; k < MSR_NMEM; ++k) x.s_mem[k] = (msp_rp)(ws + d[k]);
  x.s_grp = d[MSR_NMEM];
  x.s_out = (msp_wp)(ws + l.part + L);
#pragma unroll
  for (int t = 0; t < MSR_KT; ++t) {
    x.t_bin[t] = (msp_rp)(ws + d[MSR_NMEM + 1 + 3 * t]);
    x.t_fa[t] = (msp_rp)(ws + d[MSR_NMEM + 2 + 3 * t]);
    x.t_fb[t] = (msp_rp)(ws + d[MSR_NMEM + 3 + 3 * t]);
  }
  x.t_grp = d[MSR_NMEM + 1 + 3 * MSR_KT];
  x.t_out = (msp_wp)(ws + l.part + MSR_NL + L);
}

// qv = false: Q / 2Q / v are formed on serial wave 0 (msr_setup_Q, msr_qv_serial), which then owns the wwt region; no worker lane takes a part
// pos (PL only): the position tables of the copy at dbase, pos[k * MSR_NL + p] = where in c_k the weight k of point p sits
template <int CD, bool PL>
__device__ __forceinline__ void msr_setup_W(MsrW<CD, PL>& x, const MomCfg& c, const MomSp& sp, const double* Wl /* LDS D x CD */,
                                             const double* fmu, const double* HPH, double* ws, bool qv = true, int dbase = 0,
                                             const int* pos = nullptr) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wr = wave - MSR_W0;     // wr = 0 .. 5
  const int nd = c.nd, D = c.D, npt = c.n_pts;
  const MspLay l = msp_layout(CD, D, 1);
  // ---- table form of stage 1b: q0 on worker 3, s0 on worker 4 (one wave sum each, side by side between barriers B2 and B3)
  {
    const int L = tid - 64 * (MSR_W0 + 3), L2 = tid - 64 * (MSR_W0 + 4);
    x.b_kind = 0; x.b_p0 = x.b_p1 = x.b_p2 = (msp_rp)(ws + l.zero);
    if (L >= 0 && L < CD * CD) {
      const int j = L / CD, j2 = L - j * CD;
      x.b_kind = 1; x.b_p0 = (msp_rp)(ws + l.Q + L); x.b_p1 = (msp_rp)(ws + l.lk + j * nd + sp.c0); x.b_p2 = (msp_rp)(ws + l.lk + j2 * nd + sp.c0);
    } else if (L2 >= 0 && L2 < CD) {
      const int j = L2;
      x.b_kind = 2; x.b_p0 = (msp_rp)(ws + l.v + j); x.b_p1 = (msp_rp)(ws + l.lk + j * nd + sp.c0); x.b_p2 = (msp_rp)(ws + l.one);
    }
  }
  // ---- Q / 2Q / v on workers 0..2: 4-lane group -> one entry
  {
    x.q_kind = 0;
    x.q_out0 = x.q_out1 = x.q_out2 = x.q_out3 = (msp_wp)(ws + l.acc + 127);
    x.q_ww = x.q_src = (msp_rp)(ws + l.zero);
    const int L = (qv && wr >= 0 && wr < 3) ? wr * 64 + lane : -1;
    if (L >= 0) {
      const int g = L >> 2, sub = L & 3;
      const int nq = CD * (CD + 1) / 2;
      int j = 0, j2 = 0;
      if (g < nq) {
        int r = g; j = 0;
        while (r >= CD - j) { r -= CD - j; ++j; }
        j2 = j + r;
        x.q_kind = 1;
        x.q_out0 = (msp_wp)(ws + l.Q + j * CD + j2); x.q_out1 = (msp_wp)(ws + l.Q + j2 * CD + j);
        x.q_out2 = (msp_wp)(ws + l.Q2 + j * CD + j2); x.q_out3 = (msp_wp)(ws + l.Q2 + j2 * CD + j);
      } else if (g < nq + CD) {
        j = g - nq; x.q_kind = 2;
        x.q_out0 = (msp_wp)(ws + l.v + j);
      }
      for (int q = 0; q < msp_qterms(D); ++q) {
        const int d = sub + 4 * q;
        double v = 0.0;
        if (x.q_kind && d < D) v = (x.q_kind == 1) ? Wl[d * CD + j] * Wl[d * CD + j2] : Wl[d * CD + j];
        ws[l.wwt + q * 192 + L] = v;
      }
      x.q_ww = (msp_rp)(ws + l.wwt + L);
      x.q_src = (msp_rp)(((x.q_kind == 1) ? HPH : fmu) + sub);
    }
  }
  // ---- stage 1b: worker lane (tid - 128) = point
  {
    const msp_rp zero = (msp_rp)(ws + l.zero);
    int p = tid - 64 * MSR_W0;
    const bool ok = p >= 0 && p < npt;
    x.p_ok[0] = ok;
    x.p_any[0] = (__builtin_amdgcn_ballot_w64(ok) != 0) ? 1 : 0;
    if (!ok) p = 0;
    int tj[MSP_NZ];
#pragma unroll
    for (int r = 0; r < MSP_NZ; ++r) {
      tj[r] = ok ? sp.pdesc[(size_t)p * MSP_NZ + r] : -1;
      if (tj[r] >= 0) tj[r] = (tj[r] / nd) * 64 + (tj[r] % nd);
    }
#pragma unroll
    for (int r = 0; r < MSP_NZ; ++r) x.p_e[0][r] = (tj[r] >= 0) ? (msp_rp)(ws + l.e + (tj[r] >> 6) * nd + (tj[r] & 63)) : zero;
    int pi = 0;
#pragma unroll
    for (int r = 0; r < MSP_NZ; ++r)
#pragma unroll
      for (int s_ = r + 1; s_ < MSP_NZ; ++s_) {
        x.p_q[0][pi] = (tj[r] >= 0 && tj[s_] >= 0) ? (msp_rp)(ws + l.Q2 + (tj[r] >> 6) * CD + (tj[s_] >> 6)) : zero;
        ++pi;
      }
    if constexpr (PL) {
      x.p_c[0] = (msp_wp)(ws + l.c0 + pos[p]);
      x.p_c1[0] = (msp_wp)(ws + l.c1 + pos[MSR_NL + p]);
      x.p_c2[0] = (msp_wp)(ws + l.c2 + pos[2 * MSR_NL + p]);
    } else {
      x.p_c[0] = (msp_wp)(ws + l.c0 + p);
      x.p_c1[0] = x.p_c[0] + MSR_CS; x.p_c2[0] = x.p_c[0] + 2 * MSR_CS;
    }
    x.p_wn[0] = ok ? c.wn[p] : 0.0;
    // direct form: the link entry of every dimension at this point's coordinate code (the centre's code where pdesc names none)
#pragma unroll
    for (int j = 0; j < CD; ++j) x.d_lk[j] = ok ? (msp_rp)(ws + l.lk + j * nd + c.code[(size_t)p * CD + j]) : zero;
    x.d_qv = (msp_rp)(ws + l.Q) + opaque_zero();
  }
  // ---- cubature sums: this lane's members and terms
  msr_setup_sums(x, sp.bdesc, dbase, l, ws);
}

// ---- Q / 2Q / v on serial wave 0 (the three-barrier schedule of ihgp_adf8_kernel): the nq + CD outputs of msr_setup_W's 4-lane groups on
// aligned groups of TWO lanes, 2 (nq + CD) <= 64 lanes for CD <= 6.  Lane h of a pair carries the partial sums p_h and p_{h+2} of the 4-lane
// form (p_sub: sub-bands d = sub + 4q, q < K, even and odd q in two chains added at the end), so every addition of msp_qv has its counterpart
// here with the same operands in the same order: the results are the same bits.  Static products at ws[wwt + 64 t + lane], t = s K + q for
// the term d = h + 2s + 4q of partial s (the region the workers' products take in the other schedules; written and read by the same lane).
constexpr int MSR_QG = 4;       // terms per group of msr_qv_serial
// what a lane keeps for the stage: two read and two write addresses (2Q sits CD*CD doubles behind Q); its kind follows from the lane index
template <int CD>
struct MsrQ { msp_rp ww, src; msp_wp out0, out1; };
// kind of the output of lane pair g: 1: Q(j,j'), 2: v(j), 0: none
template <int CD>
__host__ __device__ inline int msr_qkind(int g) { return g < CD * (CD + 1) / 2 ? 1 : (g < CD * (CD + 1) / 2 + CD ? 2 : 0); }

template <int CD>
__device__ __forceinline__ void msr_setup_Q(MsrQ<CD>& x, const MomCfg& c, const double* Wl /* LDS D x CD */, const double* fmu, const double* HPH,
                                             double* ws) {
  constexpr int nq = CD * (CD + 1) / 2;
  static_assert(2 * (nq + CD) <= 64, "the pairs of msr_qv_serial fill one wave up to CD = 6");
  const int tid = threadIdx.x, D = c.D, K = msp_qterms(D);
  const MspLay l = msp_layout(CD, D, 1);
  x.out0 = x.out1 = (msp_wp)(ws + l.acc + 127);      // scratch slot
  x.ww = x.src = (msp_rp)(ws + l.zero);
  if (tid < 64) {
    const int g = tid >> 1, h = tid & 1, kind = msr_qkind<CD>(g);
    int j = 0, j2 = 0;
    if (kind == 1) {
      int r = g; j = 0;
      while (r >= CD - j) { r -= CD - j; ++j; }
      j2 = j + r;
      x.out0 = (msp_wp)(ws + l.Q + j * CD + j2); x.out1 = (msp_wp)(ws + l.Q + j2 * CD + j);
    } else if (kind == 2) {
      j = g - nq;
      x.out0 = (msp_wp)(ws + l.v + j);
    }
    for (int t = 0; t < 2 * K; ++t) {
      const int s = t / K, q = t - s * K, d = h + 2 * s + 4 * q;
      double v = 0.0;
      if (kind && d < D) v = (kind == 1) ? Wl[d * CD + j] * Wl[d * CD + j2] : Wl[d * CD + j];
      ws[l.wwt + t * 64 + tid] = v;
    }
    x.ww = (msp_rp)(ws + l.wwt + tid);
    x.src = (msp_rp)(((kind == 1) ? HPH : fmu) + h);
  }
}
typedef double msr_d2 __attribute__((ext_vector_type(2)));      // two terms of msr_qsum2 as one paired LDS read delivers them
// PAD (4K > D): the operands beyond the sub-bands -- the modulators' entries, which wave 1 may be writing at this moment, and the zero
// padding -- are replaced by zero before they are used (msp_qv multiplies them by a zero product: the same sum for finite entries)
// TIE = false (the forms with K and PAD fixed, msr_qv_serial): the same groups, reads and order of additions, with the pins on the
// two-term tuples the paired reads deliver instead of on single terms.  A pin on one double of a four-register read result makes the
// compiler copy it out of the tuple (a 64-bit register copy per term ahead of its FMA); a pin on the tuple leaves it where it is.
template <int K, bool PAD, bool TIE = true>
__device__ __forceinline__ void msr_qsum2(msp_rp ww, msp_rp src, int dlim, double& p, double& r) {
  // groups of MSR_QG terms, the reads of the next group in flight while a group multiplies: one LDS latency, then the rate of the reads,
  // with 2 MSR_QG terms in registers at a time (the serial role has few registers to spare beside its state).  The pins fix that order:
  // a group's reads are issued behind the FMAs of the group two ahead of it.
  constexpr int G = MSR_QG, NGR = 2 * K / G;
  double acc[4] = {0.0, 0.0, 0.0, 0.0};              // chain 2s + (q & 1): the even and the odd q of partial s, q ascending
  if constexpr (!TIE) {
    static_assert(G % 2 == 0 && K % 2 == 0, "terms t, t + 1 of a pair belong to one partial");
    constexpr int H = G / 2;
    msr_d2 w2[NGR][H], v2[NGR][H];
    auto reads = [&](int g) __attribute__((always_inline)) {
#pragma unroll
      for (int u = 0; u < H; ++u) {
        const int t = G * g + 2 * u, o = 2 * (t / K) + 4 * (t % K);
        w2[g][u] = msr_d2{ww[64 * t], ww[64 * (t + 1)]};
        v2[g][u] = msr_d2{src[o], src[o + 4]};
      }
    };
#pragma unroll
    for (int g = 0; g < 2 && g < NGR; ++g) reads(g);
#pragma unroll
    for (int g = 0; g < NGR; ++g) {
#pragma unroll
      for (int u = 0; u < H; ++u) asm volatile("" : "+v"(w2[g][u]), "+v"(v2[g][u]));
#pragma unroll
      for (int u = 0; u < H; ++u) {
        const int t = G * g + 2 * u, s = t / K, o = 2 * s + 4 * (t % K);
        double va = v2[g][u].x, vb = v2[g][u].y;
        if (PAD) { va = (o < dlim) ? va : 0.0; vb = (o + 4 < dlim) ? vb : 0.0; }
        const int ca = 2 * s + (t % K & 1), cb = 2 * s + ((t + 1) % K & 1);
        acc[ca] = fma(w2[g][u].x, va, acc[ca]);
        acc[cb] = fma(w2[g][u].y, vb, acc[cb]);
      }
      if (g + 2 < NGR) {
        // (the chains of the second partial are pinned once they hold a term: a pinned zero would be a register set for nothing)
        if ((G * g + G - 1) / K == 0) asm volatile("" : "+v"(ww), "+v"(src), "+v"(acc[0]), "+v"(acc[1]));
        else asm volatile("" : "+v"(ww), "+v"(src), "+v"(acc[0]), "+v"(acc[1]), "+v"(acc[2]), "+v"(acc[3]));
        reads(g + 2);
      }
    }
    p = acc[0] + acc[1]; r = acc[2] + acc[3];
    return;
  }
  double w[NGR][G], v[NGR][G];
#pragma unroll
  for (int g = 0; g < 2 && g < NGR; ++g)
#pragma unroll
    for (int u = 0; u < G; ++u) { const int t = G * g + u; w[g][u] = ww[64 * t]; v[g][u] = src[2 * (t / K) + 4 * (t % K)]; }
#pragma unroll
  for (int g = 0; g < NGR; ++g) {
#pragma unroll
    for (int u = 0; u < G; ++u) asm volatile("" : "+v"(w[g][u]), "+v"(v[g][u]));
    if (PAD) {
#pragma unroll
      for (int u = 0; u < G; ++u) { const int t = G * g + u; v[g][u] = (2 * (t / K) + 4 * (t % K) < dlim) ? v[g][u] : 0.0; }
    }
#pragma unroll
    for (int u = 0; u < G; ++u) { const int t = G * g + u, ch = 2 * (t / K) + (t % K & 1); acc[ch] = fma(w[g][u], v[g][u], acc[ch]); }
    if (g + 2 < NGR) {
      asm volatile("" : "+v"(ww), "+v"(src), "+v"(acc[0]), "+v"(acc[1]), "+v"(acc[2]), "+v"(acc[3]));
#pragma unroll
      for (int u = 0; u < G; ++u) { const int t = G * (g + 2) + u; w[g + 2][u] = ww[64 * t]; v[g + 2][u] = src[2 * (t / K) + 4 * (t % K)]; }
    }
  }
  p = acc[0] + acc[1]; r = acc[2] + acc[3];
}
// Q / 2Q / v of a step on wave 0, straight behind the head that wrote the sub-bands' fmu / HPH (the same lanes' stores: msp_wave_fence
// between them); no barrier.  Every lane of the wave executes it.
// QF (nagp_qform.hpp): K and PAD are constants of the instantiation -- one path, no branch nest walked every step, and the operands stay
// in the registers their reads delivered them in (msr_qsum2, TIE = false); QF_RUNTIME: the six paths behind the run-time nest, any D.
// dlim (PAD only) is D - (lane & 1), formed by the caller ahead of its loop.
template <int CD, int QF = QF_RUNTIME>
__device__ __forceinline__ void msr_qv_serial(const MsrQ<CD>& x, const MomCfg& c, int dlim_fixed = 0) {
  const int lane = threadIdx.x & 63, kind = msr_qkind<CD>(lane >> 1);
  if (kind) {
    double p = 0.0, r = 0.0;
    if constexpr (QF == QF_K4) msr_qsum2<4, false, false>(x.ww, x.src, 0, p, r);
    else if constexpr (QF == QF_K8) msr_qsum2<8, false, false>(x.ww, x.src, 0, p, r);
    else if constexpr (QF == QF_K16P) msr_qsum2<16, true, false>(x.ww, x.src, dlim_fixed, p, r);
    else {
      const int K = __builtin_amdgcn_readfirstlane(msp_qterms(c.D));
      const bool pad = __builtin_amdgcn_readfirstlane(4 * K != c.D ? 1 : 0) != 0;
      const int dlim = c.D - (lane & 1);             // operand 2s + 4q of this lane is a sub-band's while 2s + 4q < dlim
      if (K == 4) { if (pad) msr_qsum2<4, true>(x.ww, x.src, dlim, p, r); else msr_qsum2<4, false>(x.ww, x.src, dlim, p, r); }
      else if (K == 8) { if (pad) msr_qsum2<8, true>(x.ww, x.src, dlim, p, r); else msr_qsum2<8, false>(x.ww, x.src, dlim, p, r); }
      else { if (pad) msr_qsum2<16, true>(x.ww, x.src, dlim, p, r); else msr_qsum2<16, false>(x.ww, x.src, dlim, p, r); }
    }
    p += dpp_mov<0xB1>(p);                           // lane 0 of the pair: p0 + p1
    r += dpp_mov<0xB1>(r);                           //                     p2 + p3
    const double a = p + r;
    if ((lane & 1) == 0) {
      if (kind == 1) { x.out0[0] = a; x.out1[0] = a; x.out0[CD * CD] = 2.0 * a; x.out1[CD * CD] = 2.0 * a; }
      else x.out0[0] = a;
    }
  }
}

// sum over the lanes of an aligned group of 1, 2 or 4 (grp bit 0: lane ^ 1 belongs to it, bit 1: lane ^ 2); every lane of the wave executes it
__device__ __forceinline__ double msr_group_sum(double s, int grp) {
  const double n1 = dpp_mov<0xB1>(s);
  s = (grp & 1) ? s + n1 : s;
  const double n2 = dpp_mov<0x4E>(s);
  return (grp & 2) ? s + n2 : s;
}

// the cubature sums of one worker wave (after the barrier behind stage 1b; no barrier): level 1, then level 2 from this wave's own bins
template <class X>
__device__ __forceinline__ void msr_sums(const X& x) {
  // every read that does not depend on the bins first -- the members and the table factors of the terms: one LDS round trip
  double m[MSR_NMEM], fa[MSR_KT], fb[MSR_KT];
#pragma unroll
  for (int k = 0; k < MSR_NMEM; ++k) m[k] = *x.s_mem[k];
#pragma unroll
  for (int t = 0; t < MSR_KT; ++t) { fa[t] = *x.t_fa[t]; fb[t] = *x.t_fb[t]; }
#pragma unroll
  for (int k = 0; k < MSR_NMEM; ++k) asm volatile("" : "+v"(m[k]));
  double s0 = 0.0, s1 = 0.0;
#pragma unroll
  for (int k = 0; k < MSR_NMEM; k += 2) { s0 += m[k]; s1 += m[k + 1]; }
  *x.s_out = msr_group_sum(s0 + s1, x.s_grp);
  msp_wave_fence();
  double bv[MSR_KT];
#pragma unroll
  for (int t = 0; t < MSR_KT; ++t) bv[t] = *x.t_bin[t];
#pragma unroll
  for (int t = 0; t < MSR_KT; ++t) asm volatile("" : "+v"(bv[t]));
  double v0 = 0.0, v1 = 0.0;
#pragma unroll
  for (int t = 0; t < MSR_KT; t += 2) { v0 = fma(bv[t] * fa[t], fb[t], v0); v1 = fma(bv[t + 1] * fa[t + 1], fb[t + 1], v1); }
  *x.t_out = msr_group_sum(v0 + v1, x.t_grp);
}

// the 40 sums (acc layout of msp_outputs) from the level-2 results: lanes o < msp_nacc(CD) of ONE serial wave, after the barrier
// behind msr_sums; the same wave may read acc after msp_wave_fence().  p + c d + a b + s f g, every operand one LDS read.
template <int CD, class X>
__device__ __forceinline__ void msr_reduce(const X& x) {
  const int lane = threadIdx.x & 63;
  if (lane < msp_nacc(CD)) {
    double r[MSR_RW];
#pragma unroll
    for (int i = 0; i < MSR_RW; ++i) r[i] = *x.r_p[i];
#pragma unroll
    for (int i = 0; i < MSR_RW; ++i) asm volatile("" : "+v"(r[i]));
    *x.r_dst = fma(r[5] * r[6], r[7], fma(r[1], r[2], fma(r[3], r[4], r[0])));
  }
}

// msr_reduce in two parts (the three-barrier schedule of ihgp_adf8_kernel).  Of the eight operands the words a, c, f, g (1, 3, 6, 7) are
// link-table or constant words (l0_j, xg2_j(centre), one, zero) and p, b, d, s (0, 2, 4, 5) level-2 results or the zero word
// (msr_build_desc).  The table words are final from the barrier ahead of the weights on and are read AHEAD of the barrier behind the bin
// sums, so that wave 1 may overwrite the link tables as soon as that barrier has released; the level-2 results are read behind it.
struct MsrRT { double a, c, f, g; };
template <int CD, class X>
__device__ __forceinline__ void msr_reduce_tab(const X& x, MsrRT& t) {
  t.a = t.c = t.f = t.g = 0.0;
  if ((int)(threadIdx.x & 63) < msp_nacc(CD)) {
    t.a = *x.r_p[1]; t.c = *x.r_p[3]; t.f = *x.r_p[6]; t.g = *x.r_p[7];
  }
  asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(t.a), "+v"(t.c), "+v"(t.f), "+v"(t.g) :: "memory");      // in registers before the barrier
}
template <int CD, class X>
__device__ __forceinline__ void msr_reduce_bins(const X& x, const MsrRT& t) {
  const int lane = threadIdx.x & 63;
  if (lane < msp_nacc(CD)) {
    double p = *x.r_p[0], b = *x.r_p[2], d = *x.r_p[4], s = *x.r_p[5];
    asm volatile("" : "+v"(p), "+v"(b), "+v"(d), "+v"(s));
    *x.r_dst = fma(s * t.f, t.g, fma(t.a, b, fma(t.c, d, p)));
  }
}

}  // namespace nagp
