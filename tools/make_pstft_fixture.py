"""Writes tests/golden/pstft_multiprecision.npz: get_Obj_pSTFT_exp.m, _matern32.m, _matern52.m (form 0) and get_Obj_pSTFT_all.m
(form 1, with its 2 tau x 2 tau complex solves (F - i omega I) \\ . per component and frequency, cf_<kernel>_to_ss(mVar, len, 4) with
its dF and dQc) statement by statement in 60-digit arithmetic (mpmath), on the cases of tests/pstft_ref.py.  The float64 inputs of a
case are what the 60-digit run starts from; pi and every transform are formed at 60 digits.  Stored per case and form:
<case>_Obj_f<form>, <case>_dObj_f<form>, and <case>_theta, <case>_sumSpec so that a change of the case builder is noticed.

Asserted while generating:
  - on exp, matern32, matern52 the generic and the closed form agree to 50 digits (every case that stores both);
  - dObj equals a central difference of Obj taken at 60 digits (step 1e-20, agreement 1e-30 of the largest entry), for every form
    of every case with N <= 257 and D <= 3, the generic form up to N = 65 (each of its 6 D evaluations is N D solves);
Where one of these failed, each form would follow its own .m and the difference would be stored (<case>_formdiff), not repaired.

    python tools/make_pstft_fixture.py [case ...]
"""
import os
import sys

import mpmath as mp
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import pstft_ref as ref  # noqa: E402

mp.mp.dps = 60
F = mp.mpf
to_mp = np.frompyfunc(lambda x: mp.mpf(float(x)), 1, 1)
mlog = np.frompyfunc(mp.log, 1, 1)
SQ = {'exp': F(1), 'matern32': mp.sqrt(3), 'matern52': mp.sqrt(5), 'matern72': mp.sqrt(7)}


def omegas(N):
    h = -(-N // 2)
    om = [mp.pi * k / (h - 1) for k in range(h)]
    return np.array(om + [-om[k] for k in range(N // 2 - 1, -1, -1)], dtype=object)


def transforms(theta, c):
    D = c['D']
    minVar = to_mp(c['minVar']); limOm = to_mp(c['limOm']); limLam = to_mp(c['limLam'])
    dVar = np.array([mp.exp(t) for t in theta[:D]], dtype=object)
    sig = lambda lim, t: np.array([lim[d, 0] + (lim[d, 1] - lim[d, 0]) / (1 + mp.exp(-t[d])) for d in range(D)], dtype=object)
    return dVar, minVar + dVar, sig(limOm, theta[D:2 * D]), sig(limLam, theta[2 * D:]), minVar, limOm, limLam


def tail(theta, c, spec, dspec, grad):
    D, N = c['D'], c['N']
    dVar, mVar, om, lam, minVar, limOm, limLam = transforms(theta, c)
    specTar = to_mp(c['specTar']); bet = F(float(c['bet']))
    Obj = (mlog(spec).sum() + (specTar / spec).sum() + bet * mVar.sum()) / N
    if not grad:
        return Obj
    g = 1 / spec - specTar / spec ** 2
    out = [None] * (3 * D)
    for d in range(D):
        tv, to, tl = dspec(d)
        out[d] = ((g * tv).sum() + bet * dVar[d]) / N
        out[D + d] = (g * to).sum() * (limOm[d, 1] - limOm[d, 0]) / 4 / mp.cosh(theta[D + d] / 2) ** 2 / N
        out[2 * D + d] = (g * tl).sum() * (limLam[d, 1] - limLam[d, 0]) / 4 / mp.cosh(theta[2 * D + d] / 2) ** 2 / N
    return Obj, np.array(out, dtype=object)


def closed(theta, c, grad=True):
    kernel, D, N = c['kernel'], c['D'], c['N']
    dVar, mVar, om, lam, minVar, _, _ = transforms(theta, c)
    w = omegas(N); spec = np.array([F(float(c['vary']))] * N, dtype=object)
    p = ref.ORDER[kernel]; k0 = {1: F(1), 2: F(2), 3: F(8) / 3}[p]

    def alp(d):
        return lam[d] ** 2 + (w - om[d]) ** 2, lam[d] ** 2 + (w + om[d]) ** 2
    for d in range(D):
        a1, a2 = alp(d)
        spec = spec + k0 * mVar[d] * (1 - lam[d] ** 2) * lam[d] ** (2 * p - 1) * (a1 ** -p + a2 ** -p)

    def dspec(d):
        a1, a2 = alp(d); l = lam[d]; wm = w - om[d]; wp = w + om[d]; m = mVar[d]
        if p == 1:
            return ((m - minVar[d]) * (1 - l ** 2) * l * (a1 ** -1 + a2 ** -1), 2 * m * (1 - l ** 2) * l * (a1 ** -2 * wm - a2 ** -2 * wp),
                    m * ((1 - 3 * l ** 2) * (a1 ** -1 + a2 ** -1) - 2 * l ** 2 * (1 - l ** 2) * (a1 ** -2 + a2 ** -2)))
        if p == 2:
            return ((m - minVar[d]) * 2 * (1 - l ** 2) * l ** 3 * (a1 ** -2 + a2 ** -2), 8 * m * (1 - l ** 2) * l ** 3 * (a1 ** -3 * wm - a2 ** -3 * wp),
                    2 * m * l ** 2 * ((3 * (1 - l ** 2) - 2 * l ** 2) * (a1 ** -2 + a2 ** -2) - 4 * (1 - l ** 2) * l ** 2 * (a1 ** -3 + a2 ** -3)))
        return ((m - minVar[d]) * (F(8) / 3) * (1 - l ** 2) * l ** 5 * (a1 ** -3 + a2 ** -3), 16 * m * (1 - l ** 2) * l ** 5 * (a1 ** -4 * wm - a2 ** -4 * wp),
                (F(8) / 3) * m * l ** 4 * ((5 - 7 * l ** 2) * (a1 ** -3 + a2 ** -3) - 6 * (1 - l ** 2) * l ** 2 * (a1 ** -4 + a2 ** -4)))
    return tail(theta, c, spec, dspec, grad)


def cf_to_ss(kernel, s2, ell):
    """[F, L, Qc, H, dF(:,:,2), dQc(2)] of cf_<kernel>_to_ss.m: companion form, lambda = sqrt(2 nu) / ell"""
    p = ref.ORDER[kernel]; lamb = SQ[kernel] / ell
    binom = [mp.binomial(p, k) for k in range(p)]
    Fm = mp.zeros(p, p); dF = mp.zeros(p, p)
    for k in range(p - 1):
        Fm[k, k + 1] = 1
    for k in range(p):
        Fm[p - 1, k] = -binom[k] * lamb ** (p - k)
        dF[p - 1, k] = binom[k] * (p - k) * lamb ** (p - k) / ell          # d/d ell of -C lambda^(p-k), lambda = c / ell
    q = {1: F(2), 2: 12 * mp.sqrt(3), 3: 400 * mp.sqrt(5) / 3, 4: 10976 * mp.sqrt(7) / 5}[p]
    Qc = s2 * q / ell ** (2 * p - 1)
    return Fm, Qc, dF, Qc / s2, -(2 * p - 1) * Qc / ell


def generic(theta, c, grad=True):
    """get_Obj_pSTFT_all.m, every solve carried out"""
    kernel, D, N = c['kernel'], c['D'], c['N']
    p = ref.ORDER[kernel]; n = 2 * p
    dVar, mVar, om, lam, minVar, _, _ = transforms(theta, c)
    w = omegas(N)
    cl = {'exp': F(1), 'matern32': mp.sqrt(3)}.get(kernel, mp.sqrt(5))                 # _all.m:81-94
    spec = np.array([F(float(c['vary']))] * N, dtype=object)
    parts = []
    for d in range(D):
        ell = cl / lam[d]; dl_dlam = -cl / lam[d] ** 2
        F1, Qc, dF1, dQc_dvar, dQc_dl = cf_to_ss(kernel, mVar[d], ell)
        Fm = mp.zeros(n, n); dF_dl = mp.zeros(n, n); dF_dom = mp.zeros(n, n); L = mp.zeros(n, 2)
        for a in range(p):
            for b in range(p):
                for e in range(2):
                    Fm[2 * a + e, 2 * b + e] = F1[a, b]; dF_dl[2 * a + e, 2 * b + e] = dF1[a, b]
            Fm[2 * a, 2 * a + 1] += -om[d]; Fm[2 * a + 1, 2 * a] += om[d]
            dF_dom[2 * a, 2 * a + 1] = -1; dF_dom[2 * a + 1, 2 * a] = 1
        L[n - 2, 0] = 1; L[n - 1, 1] = 1
        B = L * L.T
        S = [None] * N; dvar = [None] * N; dom = [None] * N; dlam = [None] * N
        for i in range(N):
            G = Fm - mp.mpc(0, 1) * w[i] * mp.eye(n)
            Gi = mp.inverse(G)
            J = Gi[0, :]                                                     # H / G, H = e_1'
            JL = J * L
            s = mp.re((JL * JL.H)[0, 0])
            S[i] = Qc * s
            if grad:
                JJ = J.H * J; GB = Gi * B

                def tr(dF):
                    K = dF * GB
                    M = JJ * (K + K.H)
                    return mp.re(sum(M[k, k] for k in range(n)))
                dvar[i] = dQc_dvar * s                                       # dF_dvar = 0
                dlam[i] = (dQc_dl * s - Qc * tr(dF_dl)) * dl_dlam
                dom[i] = -Qc * tr(dF_dom)                                    # dQc_dom = 0
        S = np.array(S, dtype=object)
        spec = spec + (1 - lam[d] ** 2) * S
        if grad:
            parts.append(((mVar[d] - minVar[d]) * (1 - lam[d] ** 2) * np.array(dvar, dtype=object), (1 - lam[d] ** 2) * np.array(dom, dtype=object),
                          (1 - lam[d] ** 2) * np.array(dlam, dtype=object) - 2 * lam[d] * S))
    return tail(theta, c, spec, (lambda d: parts[d]), grad)


def central_difference(f, theta, c):
    h = F(10) ** -20
    out = []
    for j in range(theta.size):
        tp = theta.copy(); tm = theta.copy(); tp[j] = tp[j] + h; tm[j] = tm[j] - h
        out.append((f(tp, c, grad=False) - f(tm, c, grad=False)) / (2 * h))
    return np.array(out, dtype=object)


def relmax(a, b):
    return max(abs(x - y) for x, y in zip(a, b)) / max(abs(y) for y in b)


to_f = lambda v: np.array([float(x) for x in np.atleast_1d(v)])

if __name__ == '__main__':
    path = os.path.join(ROOT, 'tests', 'golden', 'pstft_multiprecision.npz')
    names = sys.argv[1:] or sorted(ref.CASES)
    out = dict(np.load(path)) if sys.argv[1:] and os.path.exists(path) else {}
    for name in names:
        c = ref.case(name); theta = to_mp(c['theta']); res = {}
        out[name + '_theta'] = c['theta']; out[name + '_sumSpec'] = np.array(c['specTar'].sum())
        for form in ref.forms(name):
            f = closed if form == 0 else generic
            Obj, dObj = f(theta, c)
            res[form] = (Obj, dObj)
            if c['N'] <= 257 and c['D'] <= 3 and not (form == 1 and c['N'] > 65):
                e = relmax(central_difference(f, theta, c), dObj)
                print(name, 'form', form, 'dObj against the central difference: %s' % mp.nstr(e, 3), flush=True)
                assert e < F(10) ** -30, (name, form, e)
            out['%s_Obj_f%d' % (name, form)] = to_f(Obj)[0:1].reshape(())
            out['%s_dObj_f%d' % (name, form)] = to_f(dObj)
            print(name, 'form', form, 'Obj', mp.nstr(Obj, 20), flush=True)
        if len(res) == 2:
            e = max(abs(res[0][0] - res[1][0]) / abs(res[0][0]), relmax(res[1][1], res[0][1]))
            print(name, 'generic against closed: %s' % mp.nstr(e, 3), flush=True)
            assert e < F(10) ** -50, (name, e)
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')
