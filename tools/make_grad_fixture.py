"""Multi-precision fixture of the EKF energy with its gradient recursion: tests/golden/ekf_grad_multiprecision.npz.

nagp_giekf_nlml_grad (csrc/nagp_grad.hip: ekf_grad_kernel) and the f64 oracle (oracle/giekf.py:run_nlml_grad) restate the same lines,
gf_giekf_modulator_nmf_constraints.m:385-472 with GradObj = 'on'; the gradient is a sum over T steps of terms that cancel, so where the
two disagree in f64 neither is the reference.  This script holds two pins per case, in 320-bit fixed point (the arithmetic of
tools/make_smoother_fixture.py: a number x is the Python integer floor(x 2^PREC), matrices are NumPy object arrays; mpmath supplies exp,
log, expm and the rounding to f64, once, at the end):

  pin (a)  the recursion from the EXACT f64 inputs the C ABI is handed -- the model A, Q, Pinf, h_val, block_offsets, Wnmf, lik_param, y,
           the per-slice stacks dA, dQ, dPinf, dR and the three flag vectors hess, w_index, w_direct, all stored -- for the literal flags
           (the reference's statements as written, api.giekf_nlml_grad(consistent=False)) and for the consistent flags:
             prediction  dm_j = dA_j m + A dm_j;  dP_j = dA_j P A' + A dP_j A' + (dA_j P A')' + dQ_j;  m = A m;  P = A P A' + Q
                         (at every step, the first included)
             model       z = H_z m, g = H_g m, mu = z' W link(g), JH = [W link(g); (z' W) .* link'(g)]' H, link = softplus
             jitter      S = R + JH P JH';  S <= 0: S = S + 0.5 1e-4;  still S <= 0: every output of the problem is NaN
             per slice   dmdJH = [hess_j] dm_j' d2h + [w_index_j >= 0] dh(m; W_),  dmu = JH dm_j + [w_direct_j] h(m; W_)
                         (W_ the unit matrix at entry w_index_j of W(:)),  dS = dmdJH P JH' + JH dP_j JH' + JH P dmdJH' + dR_j,
                         g_j += dS/(2S) - dmu v/S - (v/S)^2 dS/2,  dK = (dP_j JH' + P dmdJH')/S - P JH' dS/S^2,
                         dm_j += dK v - K dmu,  dP_j -= dK K' S + K K' dS + K dK' S
             energy      e += log(2 pi)/2 + log(S)/2 + v^2/(2S);  m += K v;  P -= K K' S
           edata and every gdata[j] are stored.  This pin tests the kernel's arithmetic alone.
  pin (b)  the derivative itself, for the consistent form: the energy as a function of the natural parameters
           theta = [sigma2, sig1, len1, omega, sig2, len2, W(:)] -- closed-form F and Pinf of the kernels, the balancing as the stored
           power-of-two scalings t (F -> T\\F T, Pinf -> T\\Pinf/T', h = t_1), A = expm(F) block by block, Q = Pinf - A Pinf A', the same
           pass -- and central differences of it at the step 2^-101; the step 2^-100 gives the same gradient to trunc_b (asserted
           < 1e-20 of the entry: the truncation error is a quarter of that).  Independent of the derivation, of ss.kernel_block_derivs,
           of api._giekf_grad_slices and of both f64 restatements.

Both pins are computed again at 256 bits: pin (a) agrees to better than 1e-60, pin (b) to better than 1e-30 (of the largest entry: the
difference quotient divides the 2^-256 resolution of the coarser run by 2^-101, and the small entries of a balanced Pinf amplify it).
ab_diff is the largest difference between pin (b) and pin (a) with consistent flags: the effect of the f64 rounding of the host's A, Q,
Pinf, dA, dQ, dPinf, below which pin (b) cannot be asserted.

Cases (T = 40 unless noted; seeds fixed):
  a      matern32 / matern52 (blocks 4, 3)  D=3, N=2   balanced
  b      the same, NOT balanced (a BlockSS without tbal)
  c      exp / matern32      (blocks 2, 2)  D=4, N=3
  d      exp / exp           (blocks 2, 1)  D=3, N=2   one-state blocks
  e      matern32 / exp      (blocks 4, 1)  D=2, N=3
  t1,t2  as a, T = 1 and 2
  j_ok   as d, T = 1, the first sub-band's Pinf (and Q) scaled negative so that S of the first step is -2.5e-5: the jitter rescues it
  j_bad  the same with S = -1e-3: every output NaN                                         (both: pin (a) only)
err_oracle = [edata literal, gdata literal, edata consistent, gdata consistent] of oracle/giekf.py:run_nlml_grad against pin (a) and
err_oracle_b = its consistent gradient against pin (b); gradient measure max_j |g_j - ref_j| / max(|ref_j|, 1e-3 max|ref|), energy relative.

Run:  python tools/make_grad_fixture.py [--jobs 4]     (about two minutes of one core)
      python tools/make_grad_fixture.py --check        (recompute and compare with the committed file)
The output is bit-for-bit reproducible (fixed zip time stamps); the printed table is the one in DESIGN.md.
"""
import argparse
import math
import os
import sys
import time

import numpy as np
from mpmath import mp, mpf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'nonstationary-audio-gp_amd'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from nagp import api as napi, harness, ss as pss                           # noqa: E402
from make_smoother_fixture import Fx, write_npz                            # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden', 'ekf_grad_multiprecision.npz')
PREC, PREC_LOW = 320, 256
FD_SHIFT = 101                                   # central differences at 2^-101 (and 2^-100 for the truncation error)
FORMS = ('lit', 'con')
ERR_FIELDS = ('e_lit', 'g_lit', 'e_con', 'g_con')
T_GEN = 40

CASES = {
    'a': dict(D=3, N=2, T=40, seed=611, k1='matern32', k2='matern52', bal=True),
    'b': dict(D=3, N=2, T=40, seed=611, k1='matern32', k2='matern52', bal=False),
    'c': dict(D=4, N=3, T=40, seed=612, k1='exp', k2='matern32', bal=True),
    'd': dict(D=3, N=2, T=40, seed=613, k1='exp', k2='exp', bal=True),
    'e': dict(D=2, N=3, T=40, seed=614, k1='matern32', k2='exp', bal=True),
    't1': dict(D=3, N=2, T=1, seed=611, k1='matern32', k2='matern52', bal=True),
    't2': dict(D=3, N=2, T=2, seed=611, k1='matern32', k2='matern52', bal=True),
    'j_ok': dict(D=3, N=2, T=1, seed=613, k1='exp', k2='exp', bal=True, jitter_S=-2.5e-5),
    'j_bad': dict(D=3, N=2, T=1, seed=613, k1='exp', k2='exp', bal=True, jitter_S=-1e-3),
}


# ---------------------------------------------------------------------------------------------
# the f64 inputs, as the product forms them
def case_blocks(p1, p2, k1, k2, balanced):
    blk = pss.ss_blocks_nmf(p1, p2, k1, k2)
    return pss.balance_blocks(blk) if balanced else blk


def first_step_S(inp, D):
    """S of the first step in f64: m = 0, P = Pinf, so S = R + sum_d (h_d ln 2 sum_c W_dc)^2 Pinf_d[0, 0]."""
    o = inp['block_offsets']
    cd = inp['h_val'][:D] * math.log(2.0) * inp['Wnmf'].sum(axis=1)
    return math.exp(float(inp['lik_param'][0])) + float(np.sum(cd ** 2 * inp['Pinf'][o[:D], o[:D]])), cd


def case_inputs(c):
    D, N = c['D'], c['N']
    vf, lf, om, vs, ls, W = harness.nmf_params(D, N, c['seed'], 'demo_nmf')
    p1 = np.concatenate([vf, lf, om]); p2 = np.concatenate([vs, ls]); lik = np.array([math.log(1e-4)])
    y = harness.sample_prior(pss.ss_blocks_nmf(p1, p2, c['k1'], c['k2']), W, T_GEN, np.random.default_rng(c['seed'] + 7919))
    y = (y / np.std(y))[:c['T']].copy()
    blk = case_blocks(p1, p2, c['k1'], c['k2'], c['bal'])
    A, Q, P = (np.array(x) for x in pss.discretise(blk, stationary_Q=True))           # what api.giekf_nlml_grad hands over
    tb = getattr(blk, 'tbal', [np.ones(k) for k in blk.sizes])
    inp = dict(param1=p1, param2=p2, Wnmf=np.array(W), lik_param=lik, A=A, Q=Q, Pinf=P, h_val=np.array(blk.h_val, float),
               block_offsets=np.array(blk.offsets, np.int32), y=y, tbal=np.concatenate(tb))
    for form in FORMS:
        dA, dQ, dPi, dR, hess, widx, wdir = napi._giekf_grad_inputs(blk, p1, p2, c['k1'], c['k2'], form == 'con')
        inp.update({'dA_' + form: dA, 'dQ_' + form: dQ, 'dPinf_' + form: dPi, 'dR_' + form: dR, 'hess_' + form: hess,
                    'w_index_' + form: widx, 'w_direct_' + form: wdir})
    if 'jitter_S' in c:
        # plain data for the ABI: the first sub-band's block of Pinf times s < 0, Q and every dQ_j formed from that Pinf by their statements
        S0, cd = first_step_S(inp, D)
        o, e = inp['block_offsets'][0], inp['block_offsets'][1]
        s = 1.0 + (c['jitter_S'] - S0) / (cd[0] ** 2 * P[o, o])
        assert s < 0
        P[o:e, o:e] *= s
        inp['Pinf'] = P
        inp['Q'] = P - A @ P @ A.T
        for form in FORMS:
            dA, dPi = inp['dA_' + form], inp['dPinf_' + form]
            X = np.stack([a @ P @ A.T for a in dA])
            inp['dQ_' + form] = dPi - X - np.stack([A @ d @ A.T for d in dPi]) - np.transpose(X, (0, 2, 1))
    return inp


# ---------------------------------------------------------------------------------------------
# the pass in fixed point
def fx_model(fx, inp):
    off = [int(o) for o in inp['block_offsets']]; M = len(off) - 1
    return dict(off=off, Ab=[fx.of(inp['A'][off[n]:off[n + 1], off[n]:off[n + 1]]) for n in range(M)], Q=fx.of(inp['Q']),
                Pinf=fx.of(inp['Pinf']), hv=fx.of(inp['h_val']), W=fx.of(inp['Wnmf']), R=fx.from_mpf(mp.exp(mpf(float(inp['lik_param'][0])))))


def fx_slices(fx, inp, form):
    return dict(dA=[fx.of(a) for a in inp['dA_' + form]], dQ=[fx.of(a) for a in inp['dQ_' + form]], dPinf=[fx.of(a) for a in inp['dPinf_' + form]],
                dR=[int(v) for v in fx.of(inp['dR_' + form])], hess=[int(v) for v in inp['hess_' + form]],
                widx=[int(v) for v in inp['w_index_' + form]], wdir=[int(v) for v in inp['w_direct_' + form]])


def ekf_pass(fx, mdl, y, D, N, sl=None):
    """(edata, [gdata_j]) as fixed-point integers, or (None, None) where the innovation variance stays <= 0 with the jitter.
    `y` fixed point; `sl` the slices of fx_slices (None: the energy alone)."""
    p = fx.p; off = mdl['off']; M = D + N; S = off[-1]
    first = np.array(off[:M])
    Ab, Q, hv, W, R = mdl['Ab'], mdl['Q'], mdl['hv'], mdl['W'], mdl['R']
    n = 0 if sl is None else len(sl['dR'])
    m = np.zeros(S, dtype=object); P = mdl['Pinf'].copy()
    dm = [np.zeros(S, dtype=object) for _ in range(n)]; dP = [sl['dPinf'][j].copy() for j in range(n)]
    e = 0; g = [0] * n
    half_log_2pi = fx.from_mpf(mp.log(2 * mp.pi) / 2); jitter = fx.from_mpf(mpf(1) / 20000)
    Amul = lambda x: np.concatenate([np.dot(Ab[b], x[off[b]:off[b + 1]]) >> p for b in range(M)])
    APAt = lambda X: fx.bd_right_t(fx.bd_left(Ab, off, X), Ab, off)
    sdot = lambda a, b: int(np.dot(a, b)) >> p
    for k in range(len(y)):
        for j in range(n):                                   # the old m, P on the right-hand sides
            dm[j] = fx.dot(sl['dA'][j], m) + Amul(dm[j])
            X = fx.bd_right_t(fx.dot(sl['dA'][j], P), Ab, off)
            dP[j] = X + APAt(dP[j]) + X.T + sl['dQ'][j]
        m = Amul(m); P = APAt(P) + Q
        z = fx.mul(hv[:D], m[first[:D]]); gg = [fx.mpf(v) for v in fx.mul(hv[D:], m[first[D:]])]
        lg = np.array([fx.from_mpf(mp.log1p(mp.exp(x))) for x in gg], dtype=object)
        dl = np.array([fx.from_mpf(1 / (1 + mp.exp(-x))) for x in gg], dtype=object)
        d2 = fx.mul(dl, fx.one - dl)
        Wl = fx.dot(W, lg); zW = fx.dot(z, W)
        mu = sdot(z, Wl)
        JH = fx.mul(np.concatenate([Wl, fx.mul(zW, dl)]), hv)               # the Jacobian on the first state of every block
        Pc = P[:, first]
        PJ = fx.dot(Pc, JH)                                                  # P JH'
        Sx = R + sdot(JH, PJ[first])
        if not Sx > 0:
            Sx = Sx + jitter
            if not Sx > 0:
                return None, None
        v = int(y[k]) - mu; vtiS = fx.div(v, Sx); K = fx.div(PJ, Sx)
        Wd = fx.mul(W, dl[None, :])
        for j in range(n):
            dmc = fx.mul(hv, dm[j][first])                                   # H dm_j
            dJ = np.zeros(M, dtype=object)
            if sl['hess'][j]:                                                # dm_j' d2h, d2h = H' [0 Wd; Wd' diag((z' W) .* link'')] H
                dJ = fx.mul(np.concatenate([fx.dot(Wd, dmc[D:]), fx.dot(dmc[:D], Wd) + fx.mul(fx.mul(zW, d2), dmc[D:])]), hv)
            dmu = sdot(JH, dm[j][first])
            if sl['widx'][j] >= 0:                                           # dh(m; W_), h(m; W_): W_ = 1 at (wd, wj), column-major entry of W
                wd, wj = sl['widx'][j] % D, sl['widx'][j] // D
                dJ[wd] += fx.mul(lg[wj], hv[wd]); dJ[D + wj] += fx.mul(fx.mul(z[wd], dl[wj]), hv[D + wj])
                if sl['wdir'][j]:
                    dmu += fx.mul(z[wd], lg[wj])
            Pd = fx.dot(Pc, dJ); dPJ = fx.dot(dP[j][:, first], JH)           # P dmdJH', dP_j JH'
            dS = sdot(dJ, PJ[first]) + sdot(JH, dPJ[first]) + sdot(JH, Pd[first]) + sl['dR'][j]
            g[j] += (fx.div(dS, Sx) - 2 * fx.mul(dmu, vtiS) - fx.mul(fx.mul(vtiS, dS), vtiS)) >> 1
            dK = fx.div(dPJ + Pd, Sx) - fx.div(fx.mul(K, dS), Sx)
            dm[j] = dm[j] + fx.mul(dK, v) - fx.mul(K, dmu)
            dKSKt = fx.mul(np.outer(dK, K) >> p, Sx)
            dP[j] = dP[j] - dKSKt - fx.mul(np.outer(K, K) >> p, dS) - dKSKt.T
        e += half_log_2pi + fx.from_mpf(mp.log(fx.mpf(Sx)) / 2) + (fx.mul(vtiS, v) >> 1)
        m = m + fx.mul(K, v); P = P - fx.mul(np.outer(K, K) >> p, Sx)
    return e, g


# ---------------------------------------------------------------------------------------------
# pin (b): the energy as a function of the natural parameters, in multi-precision from the closed forms
def mp_kernel_block(kernel, s2, ell):
    """(F, Pinf) of one stationary kernel in companion form (cf_exp_to_ss.m, cf_matern32_to_ss.m, cf_matern52_to_ss.m), mpmath matrices."""
    if kernel == 'exp':
        return mp.matrix([[-1 / ell]]), mp.matrix([[s2]])
    if kernel == 'matern32':
        lam = mp.sqrt(3) / ell
        return mp.matrix([[0, 1], [-lam ** 2, -2 * lam]]), mp.matrix([[s2, 0], [0, 3 * s2 / ell ** 2]])
    assert kernel == 'matern52'
    lam = mp.sqrt(5) / ell; kap = mpf(5) / 3 * s2 / ell ** 2
    return (mp.matrix([[0, 1, 0], [0, 0, 1], [-lam ** 3, -3 * lam ** 2, -3 * lam]]),
            mp.matrix([[s2, 0, -kap], [0, kap, 0], [-kap, 0, 25 * s2 / ell ** 4]]))


def mp_exact_model(fx, theta, c, inp):
    """The fixed-point model of ekf_pass from theta = [sigma2, sig1, len1, omega, sig2, len2, W(:)] (mpf), balanced by the stored scalings."""
    D, N = c['D'], c['N']; off = [int(o) for o in inp['block_offsets']]
    s1, l1, om = theta[1:1 + D], theta[1 + D:1 + 2 * D], theta[1 + 2 * D:1 + 3 * D]
    s2, l2 = theta[1 + 3 * D:1 + 3 * D + N], theta[1 + 3 * D + N:1 + 3 * D + 2 * N]
    Wv = theta[1 + 3 * D + 2 * N:]
    S = off[-1]
    Ab, hv = [], []
    Pinf = np.zeros((S, S), dtype=object); Q = np.zeros((S, S), dtype=object)
    to_fx = lambda X: np.array([[fx.from_mpf(X[i, k]) for k in range(X.cols)] for i in range(X.rows)], dtype=object)
    for n in range(D + N):
        if n < D:
            F1, P1 = mp_kernel_block(c['k1'], s1[n], l1[n]); t1 = F1.rows
            F = mp.zeros(2 * t1); Pn = mp.zeros(2 * t1)
            for i in range(t1):
                for k in range(t1):
                    for a in range(2):
                        F[2 * i + a, 2 * k + a] = F1[i, k]; Pn[2 * i + a, 2 * k + a] = P1[i, k]
                F[2 * i, 2 * i + 1] -= om[n]; F[2 * i + 1, 2 * i] += om[n]
        else:
            F, Pn = mp_kernel_block(c['k2'], s2[n - D], l2[n - D])
        b = F.rows; t = [mpf(float(v)) for v in inp['tbal'][off[n]:off[n + 1]]]
        assert b == off[n + 1] - off[n]
        for i in range(b):
            for k in range(b):
                F[i, k] = F[i, k] * t[k] / t[i]; Pn[i, k] = Pn[i, k] / (t[i] * t[k])
        A = mp.expm(F)
        assert mp.norm(A * mp.expm(-F) - mp.eye(b), 'inf') < mpf(2) ** (20 - fx.p)
        Ab.append(to_fx(A)); hv.append(fx.from_mpf(t[0]))
        Pinf[off[n]:off[n + 1], off[n]:off[n + 1]] = to_fx(Pn); Q[off[n]:off[n + 1], off[n]:off[n + 1]] = to_fx(Pn - A * Pn * A.T)
    W = np.array([[fx.from_mpf(Wv[d + D * j]) for j in range(N)] for d in range(D)], dtype=object)
    return dict(off=off, Ab=Ab, Q=Q, Pinf=Pinf, hv=np.array(hv, dtype=object), W=W, R=fx.from_mpf(theta[0]))


def natural_parameters(inp):
    return np.concatenate([np.exp(inp['lik_param']), inp['param1'], inp['param2'], inp['Wnmf'].ravel(order='F')])


def fd_gradient(fx, c, inp, shift):
    """Central differences of the energy at the step 2^-shift, one per natural parameter: a list of mpf."""
    theta = [mpf(float(v)) for v in natural_parameters(inp)]
    yf = fx.of(inp['y']); h = mpf(2) ** -shift; g = []
    for j in range(len(theta)):
        ep = []
        for sgn in (1, -1):
            th = list(theta); th[j] = th[j] + sgn * h
            ep.append(ekf_pass(fx, mp_exact_model(fx, th, c, inp), yf, c['D'], c['N'])[0])
        g.append(fx.mpf(ep[0] - ep[1]) / (2 * h))
    return g


# ---------------------------------------------------------------------------------------------
def run_pins(c, inp, prec, with_b=True):
    """{'e_lit', 'g_lit', 'e_con', 'g_con'[, 'g_b', 'g_b_coarse']} as mpf / lists of mpf (None where the outputs are NaN) at `prec` bits."""
    mp.prec = prec + 64
    fx = Fx(prec); mdl = fx_model(fx, inp); yf = fx.of(inp['y']); out = {}
    for form in FORMS:
        e, g = ekf_pass(fx, mdl, yf, c['D'], c['N'], fx_slices(fx, inp, form))
        out['e_' + form] = None if e is None else fx.mpf(e)
        out['g_' + form] = None if e is None else [fx.mpf(v) for v in g]
    if with_b:
        out['g_b'] = fd_gradient(fx, c, inp, FD_SHIFT)
        out['g_b_coarse'] = fd_gradient(fx, c, inp, FD_SHIFT - 1)
    return out


def grad_err(g, ref):
    """max_j |g_j - ref_j| / max(|ref_j|, 1e-3 max|ref|); 0 where both are NaN everywhere."""
    g = np.asarray(g, float); ref = np.asarray(ref, float)
    if np.all(np.isnan(ref)):
        return 0.0 if np.all(np.isnan(g)) else float('inf')
    return float(np.max(np.abs(g - ref) / np.maximum(np.abs(ref), 1e-3 * np.abs(ref).max())))


def oracle_run(c, inp, consistent):
    """oracle/giekf.py:run_nlml_grad on the case (its own dense assembly from the stored parameters; the stored Pinf where the case scaled it)."""
    from oracle import gf_ep as ogf, giekf as oek
    D, N = c['D'], c['N']
    model = ogf.assemble(inp['lik_param'], inp['param1'], inp['param2'], inp['Wnmf'], c['k1'], c['k2'], c['bal'])
    if 'jitter_S' in c:
        model['Pinf'] = inp['Pinf']
    gs = oek.grad_setup(model, inp['param1'], inp['param2'], c['k1'], c['k2'], consistent=consistent)
    n_w = 1 + 3 * D + 2 * N + (D * N if consistent else 0)
    with np.errstate(all='ignore'):
        e, g = oek.run_nlml_grad(model, gs, inp['y'], D, N, n_w, consistent=consistent)
    return float(e), np.asarray(g, float)


def oracle_errors(c, inp, ref):
    """(err_oracle[4], err_oracle_b or None) of the f64 oracle against the stored (f64-rounded) pins."""
    err = []
    gcon = None
    for form in FORMS:
        e, g = oracle_run(c, inp, form == 'con')
        err += [grad_err([e], [ref['e_' + form]]), grad_err(g, ref['g_' + form])]
        gcon = g
    return np.array(err), (grad_err(gcon, ref['g_b']) if 'g_b' in ref else None)


def build_case(name, verbose=True):
    c = CASES[name]; t0 = time.time()
    inp = case_inputs(c)
    with_b = 'jitter_S' not in c
    hi = run_pins(c, inp, PREC, with_b); lo = run_pins(c, inp, PREC_LOW, with_b)
    mp.prec = PREC + 64
    nan = hi['e_lit'] is None
    if 'jitter_S' in c:
        S0, _ = first_step_S(inp, c['D'])
        assert (S0 < -5e-5) == nan and S0 <= 0 and (lo['e_lit'] is None) == nan, (name, S0)
    else:
        assert not nan
    ref = {}; agree_a = agree_b = trunc_b = 0.0
    if nan:
        for form in FORMS:
            ref['e_' + form] = np.array(np.nan); ref['g_' + form] = np.full(len(inp['dR_' + form]), np.nan)
    else:
        for form in FORMS:
            gmax = max(abs(v) for v in hi['g_' + form])
            agree_a = max([agree_a, float(abs(hi['e_' + form] - lo['e_' + form]) / abs(hi['e_' + form]))]
                          + [float(abs(a - b) / gmax) for a, b in zip(hi['g_' + form], lo['g_' + form])])
            ref['e_' + form] = np.array(float(hi['e_' + form])); ref['g_' + form] = np.array([float(v) for v in hi['g_' + form]])
        assert agree_a < 1e-60, (name, agree_a)
    if with_b:
        gmax = max(abs(v) for v in hi['g_b'])
        agree_b = max(float(abs(a - b) / gmax) for a, b in zip(hi['g_b'], lo['g_b']))
        # of the entry; an entry that vanishes (T = 1: the mean is 0, the modulators' parameters do not reach S) is held to the largest one
        trunc_b = max(float(abs(a - b) / (abs(a) if abs(a) > gmax * mpf(10) ** -30 else gmax)) for a, b in zip(hi['g_b'], hi['g_b_coarse']))
        assert agree_b < 1e-30 and trunc_b < 1e-20, (name, agree_b, trunc_b)
        ref['g_b'] = np.array([float(v) for v in hi['g_b']])
    err, err_b = oracle_errors(c, inp, ref)
    out = dict(inp)
    out.update(ref)
    out.update(D=np.array(c['D']), N=np.array(c['N']), balanced=np.array(c['bal']), kernel1=np.array(c['k1']), kernel2=np.array(c['k2']),
               err_oracle=err, prec_bits=np.array(PREC), agree_256_bits=np.array(agree_a))
    if with_b:
        out.update(err_oracle_b=np.array(err_b), agree_256_bits_b=np.array(agree_b), trunc_b=np.array(trunc_b), fd_shift=np.array(FD_SHIFT),
                   ab_diff=np.array(grad_err(ref['g_con'], ref['g_b'])))
    if verbose:
        print('%-6s S %2d  T %2d  %4.0f s  320 vs 256 bits %.1e (b %.1e)  trunc_b %.1e  ab_diff %.1e  err_oracle %s  b %s'
              % (name, inp['A'].shape[0], c['T'], time.time() - t0, agree_a, agree_b, trunc_b, float(out.get('ab_diff', np.nan)),
                 ' '.join('%s %.1e' % (f, v) for f, v in zip(ERR_FIELDS, err)), '%.1e' % err_b if with_b else '-'), flush=True)
    return {'%s__%s' % (name, k): v for k, v in out.items()}


def build(names, jobs=1):
    if jobs > 1:
        from multiprocessing import Pool
        with Pool(jobs) as pool:
            parts = pool.map(build_case, names, chunksize=1)
    else:
        parts = [build_case(n) for n in names]
    arrays = {'cases': np.array(names), 'err_fields': np.array(ERR_FIELDS)}
    for part in parts:
        arrays.update(part)
    print('\nerr_oracle (oracle/giekf.py:run_nlml_grad against the fixture; g_b: its consistent gradient against pin (b); ab_diff: pin (b) against pin (a))')
    print('| case | ' + ' | '.join(ERR_FIELDS) + ' | g_b | ab_diff |'); print('|---|' + '---|' * (len(ERR_FIELDS) + 2))
    for n in names:
        b = '%.1e | %.1e' % (arrays[n + '__err_oracle_b'], arrays[n + '__ab_diff']) if n + '__err_oracle_b' in arrays else '- | -'
        print('| %s | ' % n + ' | '.join('%.1e' % v for v in arrays[n + '__err_oracle']) + ' | ' + b + ' |')
    return arrays


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--jobs', type=int, default=1, help='cases in parallel processes')
    ap.add_argument('--only', default='', help='comma-separated case names (with --check or --out elsewhere)')
    ap.add_argument('--check', action='store_true', help='compare with the committed fixture instead of writing it')
    ap.add_argument('--out', default=OUT)
    a = ap.parse_args()
    names = [n for n in a.only.split(',') if n] or list(CASES)
    arrays = build(names, a.jobs)
    if a.check:
        g = np.load(a.out)
        keys = [k for k in arrays if k not in ('cases',)]
        bad = [k for k in keys if k not in g.files or not np.array_equal(np.asarray(arrays[k]), g[k], equal_nan=np.asarray(arrays[k]).dtype.kind == 'f')]
        if not a.only:
            bad += [k for k in g.files if k not in arrays]
        print('fixture matches' if not bad else 'differs in %s' % bad)
        sys.exit(1 if bad else 0)
    assert not a.only or a.out != OUT, 'a partial fixture is not written over the committed one'
    write_npz(a.out, arrays)
    print('wrote %s (%d bytes)' % (os.path.relpath(a.out, ROOT), os.path.getsize(a.out)))


if __name__ == '__main__':
    main()
