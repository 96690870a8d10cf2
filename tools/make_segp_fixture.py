"""Writes tests/golden/segp_multiprecision.npz: the objective and gradient of the modulator prior fit (getObjSEGP.m on getGPSESpec.m,
the formulae of include/nagp.h, nagp_segp_obj) in 60-digit arithmetic (mpmath), on the cases of tests/segp_ref.py.  The float64
inputs of a case are what the 60-digit run starts from; pi, exp(param) and everything after them are formed at 60 digits.  Stored per
case: <case>_Obj, <case>_dObj, and <case>_param, <case>_sumSpec so that a change of the case builder is noticed.

Printed per case: the distance of the float64 restatement from the 60-digit Obj with pairwise sums (tests/segp_ref.py) and with a
single running accumulator (np.cumsum), in both orders; asserted: the pairwise one is within 1e-14 on every case.

Asserted while generating, for every case with T <= 513: dObj equals a central difference of Obj taken at 60 digits (step 1e-20,
agreement 1e-30 of the largest entry).

    python tools/make_segp_fixture.py [case ...]
"""
import os
import sys

import mpmath as mp
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import segp_ref as ref  # noqa: E402

mp.mp.dps = 60
F = mp.mpf


def objective(param, c, grad=True):
    """param: mpf entries (log len [, log varx [, log vary]])"""
    T, n_param = c['T'], c['n_param']
    ell = mp.exp(param[0])
    varx = mp.exp(param[1]) if n_param >= 2 else F(float(c['varx']))
    vary = mp.exp(param[2]) if n_param >= 3 else F(float(c['vary']))
    amp = mp.sqrt(2 * mp.pi * ell ** 2)
    s_log = F(0); s_div = F(0); s0 = F(0); s1 = F(0); s2 = F(0)
    half = -(-T // 2)
    for j in range(T):
        f = j if j <= half else j - T
        w = 2 * mp.pi * f / T
        cj = amp * mp.exp(-w ** 2 * ell ** 2 / 2)
        S = varx * cj + vary
        sy = F(float(c['specy'][j]))
        s_log += mp.log(S); s_div += sy / S
        if grad:
            g = 1 / (2 * S) - sy / (2 * T * S ** 2)
            s0 += g * cj * (1 / ell - w ** 2 * ell); s1 += g * cj; s2 += g
    Obj = (s_log / 2 + s_div / (2 * T)) / T
    if not grad:
        return Obj
    return Obj, [v / T for v in (ell * varx * s0, varx * s1, vary * s2)][:n_param]


def central_difference(param, c):
    h = F(10) ** -20
    out = []
    for k in range(len(param)):
        tp = list(param); tm = list(param); tp[k] += h; tm[k] -= h
        out.append((objective(tp, c, grad=False) - objective(tm, c, grad=False)) / (2 * h))
    return out


if __name__ == '__main__':
    path = os.path.join(ROOT, 'tests', 'golden', 'segp_multiprecision.npz')
    names = sys.argv[1:] or sorted(ref.CASES)
    out = dict(np.load(path)) if sys.argv[1:] and os.path.exists(path) else {}
    for name in names:
        c = ref.case(name); param = [F(float(v)) for v in c['param']]
        Obj, dObj = objective(param, c)
        if c['T'] <= 513:
            cd = central_difference(param, c)
            e = max(abs(a - b) for a, b in zip(cd, dObj)) / max(abs(b) for b in dObj)
            print(name, 'dObj against the central difference: %s' % mp.nstr(e, 3), flush=True)
            assert e < F(10) ** -30, (name, e)
        out[name + '_param'] = c['param']; out[name + '_sumSpec'] = np.array(c['specy'].sum())
        out[name + '_Obj'] = np.array(float(Obj)); out[name + '_dObj'] = np.array([float(v) for v in dObj])
        Of = float(Obj); S = np.exp(c['param'][1]) if c['n_param'] >= 2 else c['varx']
        S = S * ref.se_spec(np.exp(c['param'][0]), c['T'])[1] + (np.exp(c['param'][2]) if c['n_param'] >= 3 else c['vary'])
        for rev in (False, True):
            a, b = np.log(S), c['specy'] / S
            if rev:
                a, b = a[::-1], b[::-1]
            run = (0.5 * np.cumsum(a)[-1] + 1 / (2 * c['T']) * np.cumsum(b)[-1]) / c['T']
            pw = ref.objective(c, reverse=rev, grad=False)
            print(name, 'reverse %d: Obj of the restatement against 60 digits: pairwise %.2e, running accumulator %.2e'
                  % (rev, abs(pw - Of) / abs(Of), abs(run - Of) / abs(Of)), flush=True)
            assert abs(pw - Of) <= 1e-14 * abs(Of), (name, rev)
        print(name, 'Obj', mp.nstr(Obj, 20), 'dObj', [mp.nstr(v, 12) for v in dObj], flush=True)
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')
