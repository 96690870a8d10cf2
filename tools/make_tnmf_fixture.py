#!/usr/bin/env python3
"""Writes tests/golden/tnmf_multiprecision.npz: for every case of tests/tnmf_ref.py the primitive Y = basis2SEGP(X) and Obj, dObj of the
three objectives (the fit of every column, the learning form, the inference form), computed with mpmath at 60 digits from the formulae of
include/nagp.h and stored in float64, with two checksums of the inputs per case.  Needs mpmath; runs on a CPU in a few minutes.

The taps, exp, log and the row arithmetic are mpmath numbers.  The convolution sums -- millions of products per case -- are formed
exactly on integers: every factor is rounded once to a multiple of 2^-400 (its 200-bit mantissa is kept whole for any magnitude above
2^-200), the products and their sum are exact, and the sum goes back to an mpmath number.

    python tools/make_tnmf_fixture.py            # writes the fixture and prints the restatement's distance to it, forward and reverse
"""
import operator
import os
import sys
import time

import mpmath as mp
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import tnmf_ref as ref  # noqa: E402

mp.mp.dps = 60
S = 400
ONE = 1 << S


def to_int(v):
    return int(mp.floor(mp.mpf(v) * ONE + mp.mpf(1) / 2))


def taps(lenx, varx, tol):
    lenx = mp.mpf(float(lenx)); varx = mp.mpf(float(varx))
    tau = int(mp.ceil(lenx / mp.sqrt(2) * mp.mpf(float(tol))))
    assert tau == ref.tau_of(float(lenx), float(tol)), 'tau is at a rounding edge: choose another lenx'
    bh = mp.sqrt(varx * mp.sqrt(2) / (lenx * mp.sqrt(mp.pi)))
    return tau, [to_int(bh * mp.exp(-(s * s) / lenx ** 2)) for s in range(-tau, tau + 1)]


def conv(z, tau, bas):
    """Y(t) = sum_s bas(s) z(t - s) over the samples that exist, exact on the integers"""
    T = len(z)
    zi = [to_int(v) for v in z]
    zr = zi[::-1]                                           # zr[T - 1 - g] = z[g]
    out = []
    for t in range(T):
        s_lo = max(-tau, t - (T - 1)); s_hi = min(tau, t)   # 0 <= t - s <= T - 1
        # s ascending meets g = t - s descending: zr from T - 1 - (t - s_lo) on
        a = bas[s_lo + tau:s_hi + tau + 1]; b = zr[T - 1 - (t - s_lo):T - (t - s_hi)]
        out.append(mp.mpf(sum(map(operator.mul, a, b))) / ONE / ONE)
    return out


def one_case(c):
    T, D, K = c['T'], c['D'], c['K']
    M = lambda a: [[mp.mpf(float(v)) for v in row] for row in np.asarray(a, float)]
    X = M(c['X']); A = M(c['A']); y = M(c['y'])
    vary = M(c['vary']) if c['vary'] is not None else [[mp.mpf(0)] * D for _ in range(T)]
    mux = [mp.mpf(float(v)) for v in c['mux']]
    bases = [taps(c['lenx'][k], c['varx'][k], c['tol']) for k in range(K)]
    col = lambda Mx, k: [Mx[t][k] for t in range(T)]
    cv = lambda v, k: conv(v, *bases[k])
    out = {}
    CX = [cv(col(X, k), k) for k in range(K)]               # [k][t]
    out['Y'] = np.array([[float(CX[k][t]) for k in range(K)] for t in range(T)])
    # the fit of every column
    fo, fd = [], []
    for k in range(K):
        z = col(X, k)
        dx = [CX[k][t] - y[t][k] for t in range(T)]
        fo.append(float((mp.fsum(v * v for v in dx) / 2 + mp.fsum(v * v for v in z) / 2) / T))
        g = cv(dx, k)
        fd.append([float((g[t] + z[t]) / T) for t in range(T)])
    out['fit_Obj'] = np.array(fo); out['fit_dObj'] = np.array(fd)
    # the two forms of the NMF objective
    H = [[mp.exp(CX[k][t] + mux[k]) for k in range(K)] for t in range(T)]
    obj2 = mp.fsum(X[t][k] ** 2 for t in range(T) for k in range(K)) / 2
    for form in 'li':
        if form == 'l':
            lw = c['x'][T * K:].reshape(K, D, order='F')
            W = [[mp.exp(mp.mpf(float(lw[k, d]))) for d in range(D)] for k in range(K)]
            W = [[W[k][d] / mp.fsum(W[k]) for d in range(D)] for k in range(K)]
        else:
            W = M(c['W'])
        Ahat = [[mp.fsum(H[t][k] * W[k][d] for k in range(K)) + vary[t][d] for d in range(D)] for t in range(T)]
        obj1 = mp.fsum(A[t][d] / Ahat[t][d] + mp.log(Ahat[t][d]) for t in range(T) for d in range(D))
        dA = [[(Ahat[t][d] - A[t][d]) / Ahat[t][d] ** 2 for d in range(D)] for t in range(T)]
        G = [[mp.fsum(dA[t][d] * W[k][d] for d in range(D)) * H[t][k] for k in range(K)] for t in range(T)]
        dX = [cv(col(G, k), k) for k in range(K)]
        grad = [(dX[k][t] + X[t][k]) / T for k in range(K) for t in range(T)]
        if form == 'l':
            dW = [[mp.fsum(H[t][k] * dA[t][d] for t in range(T)) for d in range(D)] for k in range(K)]
            dWW = [[dW[k][d] * W[k][d] for d in range(D)] for k in range(K)]
            rs = [mp.fsum(dWW[k]) for k in range(K)]
            grad += [(dWW[k][d] - rs[k] * W[k][d]) / T for d in range(D) for k in range(K)]
        out[form + '_Obj'] = np.array(float((obj1 + obj2) / T))
        out[form + '_dObj'] = np.array([float(v) for v in grad])
    out['sums'] = np.array([c['x'].sum(), c['A'].sum()])
    return out


def main():
    fx = {}
    for name in sorted(ref.CASES):
        t0 = time.time()
        c = ref.case(name)
        res = one_case(c)
        for k, v in res.items():
            fx['%s_%s' % (name, k)] = v
        for reverse in (False, True):
            fo = ref.fit_objective(c, reverse)
            e = [ref.dist(ref.basis2SEGP(c['X'], c['lenx'], c['varx'], c['tol'], reverse), res['Y']), ref.dist(fo[0], res['fit_Obj']), ref.dist(fo[1], res['fit_dObj'])]
            for form in 'li':
                O, d = ref.objective(c, form == 'l', reverse)
                e += [ref.dist(O, res[form + '_Obj']), ref.dist(d, res[form + '_dObj'])]
            print('%-8s reverse %d: Y %.2e  fit Obj %.2e dObj %.2e  learn Obj %.2e dObj %.2e  inf Obj %.2e dObj %.2e   (%.0f s)' % ((name, reverse) + tuple(e) + (time.time() - t0,)), flush=True)
    path = os.path.join(ROOT, 'tests', 'golden', 'tnmf_multiprecision.npz')
    np.savez_compressed(path + '.tmp.npz', **fx)
    os.replace(path + '.tmp.npz', path)
    print('wrote %s (%d B)' % (path, os.path.getsize(path)))


if __name__ == '__main__':
    main()
