"""Writes tests/golden/slowfb_multiprecision.npz: the statement sequence of unifying_prob_tf/kernel_ss_kalmanSlowFB_rewrite.m (forward
filter :55-84, RTS smoother :100-134, plus the library's NaN guard) in 60-digit arithmetic (mpmath) on the two cases of
tests/slowfb_ref.py:case -- `m32` (matern32, D = 2: S = 8, T = 120) and `m52` (matern52, D = 3: S = 18, T = 60), each with a
1e5-variance gap, a NaN gap and a NaN at T-2.  The float64 inputs are stored and are what the 60-digit run starts from.
Stored per case: lik, MS, Pdiag, the full P at a few steps (first, last, gap edges, mid-gap), and the filter-only MF, PFdiag, PF.

    python tools/make_slowfb_fixture.py
"""
import os
import sys

import mpmath as mp
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'nonstationary-audio-gp_amd')); sys.path.insert(0, os.path.join(ROOT, 'tests'))
import slowfb_ref as ref  # noqa: E402

mp.mp.dps = 60


def to_np(M):
    return np.array([[float(M[i, j]) for j in range(M.cols)] for i in range(M.rows)])


def run(c):
    A = mp.matrix(c['A'].tolist()); Q = mp.matrix(c['Q'].tolist()); H = mp.matrix([c['H'].tolist()]); P = mp.matrix(c['P0'].tolist())
    y, vary = c['y'], c['vary']; T = y.size; S = A.rows
    m = mp.zeros(S, 1); lik = mp.mpf(0)
    MF, PF = [], []
    for k in range(T):
        if k > 0:
            m = A * m; P = A * P * A.T + Q
        if not np.isnan(y[k]):
            s = (H * P * H.T)[0, 0] + mp.mpf(float(vary[k]))
            K = P * H.T / s
            v = mp.mpf(float(y[k])) - (H * m)[0, 0]
            m = m + K * v
            P = P - K * H * P
            lik += mp.log(2 * mp.pi) / 2 + mp.log(s) / 2 + v * v / s / 2
        MF.append(m.copy()); PF.append(P.copy())
    MS, PS = list(MF), list(PF)
    for k in range(T - 2, -1, -1):
        PSk = PF[k]
        PSkp = A * PSk * A.T + Q
        G = PSk * A.T * mp.inverse(PSkp)
        m = MF[k] + G * (m - A * MF[k])
        P = PSk + G * (P - PSkp) * G.T
        MS[k] = m; PS[k] = P
    st = [int(k) for k in c['steps']]
    col = lambda Ms: np.stack([to_np(x)[:, 0] for x in Ms], axis=1)
    dg = lambda Ps: np.stack([np.diag(to_np(x)) for x in Ps], axis=1)
    return dict(lik=float(-lik), MS=col(MS), Pdiag=dg(PS), P=np.stack([to_np(PS[k]) for k in st], axis=2),
                MF=col(MF), PFdiag=dg(PF), PF=np.stack([to_np(PF[k]) for k in st], axis=2))


if __name__ == '__main__':
    out = {}
    for name in ('m32', 'm52'):
        c = ref.case(name)
        for k in ('A', 'Q', 'H', 'P0', 'y', 'vary', 'steps'):
            out['%s_%s' % (name, k)] = c[k]
        out['%s_block' % name] = np.array(c['block']); out['%s_tau' % name] = np.array(c['tau'])
        for k, v in run(c).items():
            out['%s_%s' % (name, k)] = v
    path = os.path.join(ROOT, 'tests', 'golden', 'slowfb_multiprecision.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')
