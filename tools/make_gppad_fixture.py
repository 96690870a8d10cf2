"""Writes tests/golden/gppad_multiprecision.npz: the objective and gradient of the GPPAD envelope inference (GetGPObjFast.m, the formulae
of include/nagp.h, nagp_gppad_obj) in 60-digit arithmetic (mpmath), on the cases of tests/gppad_ref.py.  The float64 inputs of a case
(x, y, vary and the parameters; len where the spectrum is formed from it, the float64 fftCov where it is given) are what the 60-digit run
starts from; pi, the twiddles, the spectrum formed from len and everything after them are formed at 60 digits.  The transform is a
radix-2 decimation-in-time FFT written here on mpf pairs.  Stored per case: <case>_Obj, <case>_dObj, and <case>_sums (the sums of x and
of y) so that a change of the case builder is noticed: inputs are regenerated from the seeds, only results are kept.

Printed per case: the distance of the float64 restatement from the 60-digit values, forward and reverse.

    python tools/make_gppad_fixture.py [case ...]
"""
import os
import sys

import mpmath as mp
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import gppad_ref as ref  # noqa: E402

mp.mp.dps = 60
F = mp.mpf


def twiddles(n):
    """exp(-2 pi i m / n), m < n / 2"""
    return [(mp.cospi(F(2 * m) / n), -mp.sinpi(F(2 * m) / n)) for m in range(n // 2)]


def fft(re, im, tw, inverse=False):
    """in place on two lists of mpf, n a power of two; the inverse is not normalised"""
    n = len(re)
    j = 0
    for i in range(1, n):                                    # bit reversal
        bit = n >> 1
        while j & bit:
            j ^= bit; bit >>= 1
        j |= bit
        if i < j:
            re[i], re[j] = re[j], re[i]; im[i], im[j] = im[j], im[i]
    size = 2
    while size <= n:
        half, step = size // 2, n // size
        for start in range(0, n, size):
            for k in range(half):
                wr, wi = tw[k * step]
                if inverse:
                    wi = -wi
                a, b = start + k, start + k + half
                tr = re[b] * wr - im[b] * wi; ti = re[b] * wi + im[b] * wr
                re[b] = re[a] - tr; im[b] = im[a] - ti
                re[a] += tr; im[a] += ti
        size *= 2


def objective(c):
    T, Tx = c['T'], c['Tx']
    varx, mux, varc = F(float(c['varx'])), F(float(c['mux'])), F(float(c['varc']))
    x = [F(float(v)) for v in c['x']]
    vary = np.broadcast_to(np.asarray(c['vary'], float), (T,))
    if c['given']:
        cov = [F(float(v)) for v in c['fftCov']]
    else:
        ell = F(float(c['len'])); amp = mp.sqrt(2 * mp.pi * ell ** 2)
        cov = []
        for k in range(Tx):
            w = 2 * mp.pi * (k if k <= Tx // 2 else k - Tx) / Tx
            cov.append(amp * mp.exp(-w ** 2 * ell ** 2 / 2) + F('1e-6'))
    tw = twiddles(Tx)
    re = [v - mux for v in x]; im = [F(0)] * Tx
    fft(re, im, tw)
    re = [a / b for a, b in zip(re, cov)]; im = [a / b for a, b in zip(im, cov)]
    fft(re, im, tw, inverse=True)
    u = [v / Tx for v in re]
    ObjB = sum(a * (b - mux) for a, b in zip(u, x)) / (2 * varx)
    ObjA = F(0)
    d = [v / varx for v in u]
    for t in range(T):
        xt = x[t]
        a = xt if xt > 500 else (mp.exp(xt) if xt < -30 else mp.log(1 + mp.exp(xt)))
        s = 1 / (1 + mp.exp(-xt))
        v = a * a * varc + F(float(vary[t])) + F('1e-5')
        yy = F(float(c['y'][t])) ** 2
        ObjA += mp.log(v) / 2 + yy / v / 2
        d[t] += s * a / v * (1 - yy / v) * varc
    return ObjA + ObjB, d


if __name__ == '__main__':
    path = os.path.join(ROOT, 'tests', 'golden', 'gppad_multiprecision.npz')
    names = sys.argv[1:] or sorted(ref.CASES)
    out = dict(np.load(path)) if sys.argv[1:] and os.path.exists(path) else {}
    for name in names:
        c = ref.case(name)
        Obj, dObj = objective(c)
        out[name + '_sums'] = np.array([c['x'].sum(), c['y'].sum()])
        out[name + '_Obj'] = np.array(float(Obj)); out[name + '_dObj'] = np.array([float(v) for v in dObj])
        for rev in (False, True):
            O, d = ref.objective(c, reverse=rev)
            print(name, 'reverse %d: the restatement against 60 digits: Obj %.2e dObj %.2e'
                  % (rev, ref.dist(O, out[name + '_Obj']), ref.dist(d, out[name + '_dObj'])), flush=True)
        print(name, 'Obj', mp.nstr(Obj, 20), flush=True)
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')
