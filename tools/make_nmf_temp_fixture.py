"""Writes tests/golden/nmf_temp_multiprecision.npz: the objective and gradient of the conjugate-gradient NMF with temporal priors
(getObj_nmf_temp.m and getObj_nmf_temp_inf.m, the formulae of include/nagp.h, nagp_nmf_temp_obj) in 60-digit arithmetic (mpmath), on
the cases of tests/nmf_temp_ref.py.  The float64 inputs of a case (x, A, vary, a given W, the prior parameters) are what the 60-digit
run starts from; every exp, log, sum and quotient after them is formed at 60 digits.  Stored per case: <case>_Obj, <case>_dObj (float64)
and <case>_sums (the sums of x and of A) so that a change of the case builder is noticed: inputs are regenerated from the seeds, only
results are kept.

Printed per case: the distance of the float64 restatement from the 60-digit values, forward and reverse.

    python tools/make_nmf_temp_fixture.py [case ...]
"""
import os
import sys

import mpmath as mp
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import nmf_temp_ref as ref  # noqa: E402

mp.mp.dps = 60
F = mp.mpf


def objective(c):
    T, D, K = c['T'], c['D'], c['K']
    x = [F(float(v)) for v in c['x']]
    logH = [[x[t + k * T] for k in range(K)] for t in range(T)]
    H = [[mp.exp(v) for v in row] for row in logH]
    if c['learn']:
        W = [[mp.exp(x[T * K + k + d * K]) for d in range(D)] for k in range(K)]
        W = [[w / sum(row) for w in row] for row in W]
    else:
        W = [[F(float(c['W'][k, d])) for d in range(D)] for k in range(K)]
    A = [[F(float(v)) for v in row] for row in c['A']]
    vary = [[F(float(v)) for v in row] for row in c['vary']] if c['vary'] is not None else [[F(0)] * D for _ in range(T)]
    obj1 = F(0)
    dH = [[F(0)] * K for _ in range(T)]
    dW = [[F(0)] * D for _ in range(K)]
    for t in range(T):
        for d in range(D):
            ah = sum(H[t][k] * W[k][d] for k in range(K)) + vary[t][d]
            obj1 += A[t][d] / ah + mp.log(ah)
            da = (ah - A[t][d]) / ah ** 2
            for k in range(K):
                dH[t][k] += da * W[k][d]
                dW[k][d] += H[t][k] * da
    obj2 = F(0)
    d2 = [[F(0)] * K for _ in range(T)]
    if c['prior'] == 'tg':
        for k in range(K):
            vi, la = F(float(c['varinf'][k])), F(float(c['lam'][k]))
            obj2 += (1 + la ** 2) / (2 * vi) * sum(H[t][k] ** 2 for t in range(1, T - 1)) + H[T - 1][k] ** 2 / (2 * vi) + la ** 2 / (2 * vi) * H[0][k] ** 2 \
                - la / vi * sum(H[t][k] * H[t - 1][k] for t in range(1, T))
            d2[0][k] = la ** 2 / vi * H[0][k] - la / vi * H[1][k]
            for t in range(1, T - 1):
                d2[t][k] = (1 + la ** 2) / vi * H[t][k] - la / vi * (H[t + 1][k] + H[t - 1][k])
            d2[T - 1][k] = H[T - 1][k] / vi - la / vi * H[T - 2][k]
    elif c['prior'] == 'ig':
        for k in range(K):
            mu, vi, la = F(float(c['muinf'][k])), F(float(c['varinf'][k])), F(float(c['lam'][k]))
            alp1 = mu ** 2 / vi + 2; bet1 = (alp1 - 1) * mu
            alp = 2 + la ** 2 + mu ** 2 / vi
            a = (alp - 1) * la; b = (alp - 1) * (1 - la) * mu
            ab = [a * H[t][k] + b for t in range(T - 1)]
            obj2 += bet1 / H[0][k] + (alp1 + 1) * logH[0][k] - alp * sum(mp.log(v) for v in ab) + (alp + 1) * sum(logH[t][k] for t in range(1, T)) \
                + sum(ab[t - 1] / H[t][k] for t in range(1, T))
            d2[0][k] = a / H[1][k] - bet1 / H[0][k] ** 2 + (alp1 + 1) / H[0][k] - alp * a / ab[0]
            for t in range(1, T - 1):
                d2[t][k] = a / H[t + 1][k] - ab[t - 1] / H[t][k] ** 2 + (alp + 1) / H[t][k] - alp * a / ab[t]
            d2[T - 1][k] = -ab[T - 2] / H[T - 1][k] ** 2 + (1 + alp) / H[T - 1][k]
    Obj = (obj1 + obj2) / T
    dObj = [(dH[t][k] + d2[t][k]) * H[t][k] / T for k in range(K) for t in range(T)]
    if c['learn']:
        dWW = [[dW[k][d] * W[k][d] for d in range(D)] for k in range(K)]
        rs = [sum(row) for row in dWW]
        dObj += [(dWW[k][d] - rs[k] * W[k][d]) / T for d in range(D) for k in range(K)]
    return Obj, dObj


if __name__ == '__main__':
    path = os.path.join(ROOT, 'tests', 'golden', 'nmf_temp_multiprecision.npz')
    names = sys.argv[1:] or sorted(ref.CASES)
    out = dict(np.load(path)) if sys.argv[1:] and os.path.exists(path) else {}
    for name in names:
        c = ref.case(name)
        Obj, dObj = objective(c)
        out[name + '_sums'] = np.array([c['x'].sum(), c['A'].sum()])
        out[name + '_Obj'] = np.array(float(Obj)); out[name + '_dObj'] = np.array([float(v) for v in dObj])
        for rev in (False, True):
            O, d = ref.objective(c, reverse=rev)
            print(name, 'reverse %d: the restatement against 60 digits: Obj %.2e dObj %.2e'
                  % (rev, ref.dist(O, out[name + '_Obj']), ref.dist(d, out[name + '_dObj'])), flush=True)
        print(name, 'Obj', mp.nstr(Obj, 20), flush=True)
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')
