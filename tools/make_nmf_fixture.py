"""Writes tests/golden/nmf_multiprecision.npz: the statement sequence of experiments/nmf/nmf_fp.m:65-87 (update_w = 1) and
nmf_inf_fp.m:42-55 (update_w = 0), with the objective of getObj_nmf_temp.m:45-54, :134 (its renormalisation of W included), in
60-digit arithmetic (mpmath) on the six cases of tests/nmf_ref.py:case.  The float64 inputs of a case are what the 60-digit run
starts from; the fixture stores W0 and the sums of A and H0 so that a change of the case builder is noticed.
Stored per case and per update_w (suffix _w1 / _w0): W, H, Obj.

    python tools/make_nmf_fixture.py
"""
import os
import sys

import mpmath as mp
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'nonstationary-audio-gp_amd')); sys.path.insert(0, os.path.join(ROOT, 'tests'))
import nmf_ref as ref  # noqa: E402

mp.mp.dps = 60

to_mp = np.frompyfunc(lambda x: mp.mpf(float(x)), 1, 1)
mlog = np.frompyfunc(mp.log, 1, 1)
to_f = lambda M: np.array(M, dtype=object).astype(float)


def rownorm(W):
    return W / W.sum(axis=1)[:, None]


def obj(H, W, A, vary):
    Ahat = H.dot(rownorm(W)) + vary
    return (A / Ahat + mlog(Ahat)).sum() / A.shape[0]


def run(c, update_w):
    A = to_mp(c['A']); W = to_mp(c['W0']); H = to_mp(c['H0'])
    vary = A * 0 if c['vary'] is None else to_mp(c['vary'])
    Obj = []
    for _ in range(c['its']):
        R = 1 / (H.dot(W) + vary)
        H = (A * R * R).dot(W.T) / R.dot(W.T) * H
        Obj.append(obj(H, W, A, vary))
        if update_w:
            R = 1 / H.dot(W)
            W = rownorm(H.T.dot(A * R * R) / H.T.dot(R) * W)
            Obj.append(obj(H, W, A, vary))
    return dict(W=to_f(W), H=to_f(H), Obj=to_f(Obj))


if __name__ == '__main__':
    out = {}
    for name in sorted(ref.CASES):
        c = ref.case(name)
        out['%s_W0' % name] = c['W0']; out['%s_sumA' % name] = np.array(c['A'].sum()); out['%s_sumH0' % name] = np.array(c['H0'].sum())
        for uw in (1, 0):
            for k, v in run(c, uw).items():
                out['%s_%s_w%d' % (name, k, uw)] = v
            print(name, uw, out['%s_Obj_w%d' % (name, uw)][-1], flush=True)
    path = os.path.join(ROOT, 'tests', 'golden', 'nmf_multiprecision.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')
