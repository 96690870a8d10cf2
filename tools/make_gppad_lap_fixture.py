#!/usr/bin/env python
"""Writes tests/golden/gppad_lap_multiprecision.npz: the yardstick of the Laplace step of GPPAD (tests/gppad_lap_ref.py holds the cases).

1. The parts without decisions, in mpmath at 60 digits from the float64 inputs of every FIXED case, results only, rounded to float64:
   d (GetHessian.m), A v (SigDSigTimesV.m), Varx for the given pairs (GetErrorBarGPPAD.m; a zero and a negative lmb among them) and
   Obj0, Obj1, Obj2 (GetLaplaceObjGPPADOneChunk.m).  The transforms are a radix-2 FFT on mpmath numbers.
2. The Lanczos run as a whole, for every STABLE case: the float64 restatement's clean run (steps, reorthogonalisations, nconv, anorm, lmb,
   Varx) and four runs with every operator product multiplied by 1 + 1e-15 g, g standard normal.  The tool refuses a case whose
   perturbed runs do not give the clean run's counts; the largest distance (max|d| / max|ref| per array) between the clean and the
   perturbed lmb and Varx is stored as the case's self-deviation.

    python tools/make_gppad_lap_fixture.py
"""
import os
import sys

import numpy as np
from mpmath import mp, mpf, mpc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import gppad_lap_ref as ref  # noqa: E402

mp.dps = 60
N_PERTURBED = 4


def fft(a, sign):
    n = len(a)
    if n == 1:
        return list(a)
    e = fft(a[0::2], sign); o = fft(a[1::2], sign)
    out = [None] * n
    for k in range(n // 2):
        w = mp.expjpi(mpf(sign * 2 * k) / n) * o[k]
        out[k] = e[k] + w; out[k + n // 2] = e[k] - w
    return out


def ifft(a):
    n = len(a)
    return [z / n for z in fft(a, 1)]


def spectrum(ell, Tx):
    ell = mpf(ell)
    out = []
    for k in range(Tx):
        f = k if k <= Tx // 2 else k - Tx
        w = 2 * mp.pi * f / Tx
        out.append(mp.sqrt(2 * mp.pi * ell ** 2) * mp.exp(-w ** 2 * ell ** 2 / 2) + mpf('1e-6'))
    return out


def amp(x):
    return x if x > 500 else (mp.exp(x) if x < -30 else mp.log(1 + mp.exp(x)))


def sandwich(v, hs):
    return [z.real for z in ifft([h * z for h, z in zip(hs, fft([mpc(q) for q in v], -1))])]


def fixed(c):
    T, Tx = c['T'], c['Tx']
    x = [mpf(float(q)) for q in c['x']]; y = [mpf(float(q)) for q in c['y']]
    vary = [mpf(float(q)) for q in np.broadcast_to(np.asarray(c['vary'], float), (T,))]
    varx, mux, varc = mpf(c['varx']), mpf(c['mux']), mpf(c['varc'])
    d = []; obj1 = mpf(0)
    for t in range(T):
        a = amp(x[t]); s = 1 / (1 + mp.exp(-x[t])); c2 = mpf(1) / 4 / mp.cosh(x[t] / 2) ** 2
        v = a ** 2 * varc + vary[t] + mpf('1e-5'); dv = 2 * varc * a * s; w = 1 - y[t] ** 2 / v
        d.append((c2 * a + s ** 2) / v * w * varc - s * a / v ** 2 * w * varc * dv + s * a / v * y[t] ** 2 / v ** 2 * varc * dv)
        obj1 -= (mp.log(v) + y[t] ** 2 / v) / 2
    cov = spectrum(c['len'], Tx)
    hs = [mp.sqrt(q * varx) for q in cov]
    a = sandwich([mpf(float(q)) for q in c['v']], hs)
    Av = sandwich([d[t] * a[t] if t < T else mpf(0) for t in range(Tx)], hs)
    Varx = [varx] * Tx; obj0 = mpf(0)
    for k, l in enumerate(c['lmb']):
        l = max(mpf(float(l)), mpf(0))
        b = sandwich([mpf(float(q)) for q in c['xv'][k]], hs)
        Varx = [V - q ** 2 * l / (l + 1) for V, q in zip(Varx, b)]
        obj0 -= mp.log(abs(1 + l)) / 2
    xe = [q - mux for q in x]
    u = [z.real for z in ifft([z / q for z, q in zip(fft([mpc(q) for q in xe], -1), cov)])]
    obj2 = -sum(p * q for p, q in zip(u, xe)) / (2 * varx)
    f = lambda z: np.array([float(q) for q in z])
    return dict(d=f(d), Av=f(Av), Varx=f(Varx), Obj=f([obj0, obj1, obj2]))


def stable(name):
    c = ref.stable_case(name)
    clean = ref.solve(c)
    dl = dv = 0.0
    for k in range(N_PERTURBED):
        p = ref.solve(c, perturb=np.random.default_rng(7700 + k))
        if ref.counts(p) != ref.counts(clean):
            raise SystemExit('%s: a perturbed run gives %s against %s: not a stable case' % (name, ref.counts(p), ref.counts(clean)))
        if clean['nconv']:
            dl = max(dl, ref.dist(p['lmb'], clean['lmb'])); dv = max(dv, ref.dist(p['Varx'], clean['Varx']))
    return dict(counts=np.array(ref.counts(clean)), anorm=np.array(clean['anorm']), lmb=clean['lmb'], Varx=clean['Varx'], selfdev=np.array([dl, dv]))


def main():
    out = {}
    for name in sorted(ref.FIXED):
        for k, v in fixed(ref.fixed_case(name)).items():
            out['%s_%s' % (name, k)] = v
        print(name, 'done')
    for name in sorted(ref.STABLE):
        r = stable(name)
        for k, v in r.items():
            out['%s_%s' % (name, k)] = v
        print(name, 'counts', r['counts'], 'self-deviation lmb %.2e Varx %.2e' % tuple(r['selfdev']))
    path = os.path.join(ROOT, 'tests', 'golden', 'gppad_lap_multiprecision.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
