"""Writes tests/golden/gppad_cas_multiprecision.npz: the objective and gradient of the GPPAD cascade (GetObjCasGPFAST.m, the formulae of
include/nagp.h, nagp_gppad_cas_obj) in 60-digit arithmetic (mpmath), on the cases of tests/gppad_cas_ref.py.  The float64 inputs of a
case (x, y and the parameters; len where the spectra are formed from it, the float64 fftCovs where they are given) are what the
60-digit run starts from; pi, the twiddles, the spectra formed from len and everything after them are formed at 60 digits, with the
radix-2 transform of tools/make_gppad_fixture.py.  Stored per case: <case>_Obj and <case>_dObj (M x Tx) only: inputs are regenerated from
the seeds.

Printed per case: the distance of the float64 restatement from the 60-digit values, forward and reverse.

    python tools/make_gppad_cas_fixture.py [case ...]
"""
import os
import sys

import mpmath as mp
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import gppad_cas_ref as ref  # noqa: E402
from make_gppad_fixture import fft, twiddles  # noqa: E402  (sets mp.mp.dps = 60)

F = mp.mpf


def objective(c):
    M, T, Tx = c['M'], c['T'], c['Tx']
    varc = F(float(c['varc']))
    tw = twiddles(Tx)
    X = [[F(float(v)) for v in c['x'][m]] for m in range(M)]
    A = [[None] * T for _ in range(M)]; S = [[None] * T for _ in range(M)]
    ObjA = F(0); quad = F(0); D = [None] * T
    for t in range(T):
        P = F(1)
        for m in range(M):
            xt = X[m][t]
            a = xt if xt > 500 else (mp.exp(xt) if xt < -30 else mp.log(1 + mp.exp(xt)))
            A[m][t] = a; S[m][t] = 1 / (1 + mp.exp(-xt))
            P *= a; ObjA += mp.log(a)
        yy = F(float(c['y'][t])) ** 2
        quad += yy / (P * P) / 2
        D[t] = 1 - yy / (varc * P * P)
    Obj = ObjA + quad / varc
    d = []
    for m in range(M):
        varx, mux = F(float(c['varx'][m])), F(float(c['mux'][m]))
        if c['given']:
            cov = [F(float(v)) for v in c['fftCovs'][m]]
        else:
            ell = F(float(c['len'][m])); amp = mp.sqrt(2 * mp.pi * ell ** 2)
            cov = []
            for k in range(Tx):
                w = 2 * mp.pi * (k if k <= Tx // 2 else k - Tx) / Tx
                cov.append(amp * mp.exp(-w ** 2 * ell ** 2 / 2) + F('1e-6'))
        re = [v - mux for v in X[m]]; im = [F(0)] * Tx
        fft(re, im, tw)
        re = [a / b for a, b in zip(re, cov)]; im = [a / b for a, b in zip(im, cov)]
        fft(re, im, tw, inverse=True)
        u = [v / Tx for v in re]
        Obj += sum(a * (b - mux) for a, b in zip(u, X[m])) / (2 * varx)
        dm = [v / varx for v in u]
        for t in range(T):
            dm[t] += S[m][t] / A[m][t] * D[t]
        d.append(dm)
    return Obj, d


if __name__ == '__main__':
    path = os.path.join(ROOT, 'tests', 'golden', 'gppad_cas_multiprecision.npz')
    names = sys.argv[1:] or sorted(ref.CASES)
    out = dict(np.load(path)) if sys.argv[1:] and os.path.exists(path) else {}
    for name in names:
        c = ref.case(name)
        Obj, dObj = objective(c)
        out[name + '_Obj'] = np.array(float(Obj)); out[name + '_dObj'] = np.array([[float(v) for v in row] for row in dObj])
        for rev in (False, True):
            O, d = ref.objective(c, reverse=rev)
            print(name, 'reverse %d: the restatement against 60 digits: Obj %.2e dObj %.2e'
                  % (rev, ref.dist(O, out[name + '_Obj']), ref.dist(d, out[name + '_dObj'])), flush=True)
        print(name, 'Obj', mp.nstr(Obj, 20), flush=True)
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')
