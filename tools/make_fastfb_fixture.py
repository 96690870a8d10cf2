"""Writes tests/golden/fastfb_multiprecision.npz: the set-up and the two loops of unifying_prob_tf/kernel_ss_kalmanFastFB.m (the
stationary filterbank: infinite-horizon Kalman filter, steady-state RTS smoother) in 60-digit arithmetic (mpmath).

Models (get_disc_model with the recipe of tests/fastfb_ref.py:recipe, seed D + 700, vary = 0.01), keys '<model>__<array>':
  m32  matern32 D = 2 (S = 8)     m52    matern52 D = 3  (S = 18)    m52d5  matern52 D = 5 (S = 30)
  exp3 exp D = 3 (S = 6)          m52d10 matern52 D = 10 (S = 60)    wide   matern32 D = 16 (S = 64; recursion inputs only)
  inputs   A, Q = (Q + Q')/2 exactly, H, vary as float64 -- what the 60-digit run starts from (lti_disc leaves Q asymmetric by about
           1e-18, which a 60-digit residual check sees);
  set-up   PP = dare(A', H', Q, vary) by doubling (residual < 1e-40 |PP|), Sinn, Kg, HA, AKHA, PF2 (:52-75), G = PF2 A' / PP,
           QQ = sym(PF2 - G PP G'), Psm = G Psm G' + QQ by doubling (residual < 1e-40) (:129-134); each rounded to nearest float64.
Recursion cases, keys 'run_<case>__<array>': both loops (:81-110, :137-151) in 60 digits from those float64-rounded matrices,
  m32, m52   T = 300, NaN on [40, 75), at 0 and at T-1
  span       model m32, T = 2305 (18 spans of 129 steps): NaN at 0, at T-1, on L-2 .. L+2 and on all of span 3
  span_wide  model wide, T = 2100 (16 spans of 132 steps): NaN on L-1 .. L and at T-2
  stored: y, steps, MF and MS at `steps` (all steps for m32 / m52; the span edges, the gap edges and a stride for the long ones),
  sum_v2 and lik (from the float64 Sinn).

    python tools/make_fastfb_fixture.py [--jobs 8]      (about ten minutes on 8 cores; the bytes depend on the contents only)
"""
import argparse
import os
import sys

import numpy as np
from mpmath import mp
from mpmath.libmp import round_nearest, to_float

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'nonstationary-audio-gp_amd')); sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import fastfb_ref as ref                                             # noqa: E402
from make_dare_fixture import DPS, dare, stein, write_npz, _mat      # noqa: E402
from nagp import get_disc_model                                      # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden', 'fastfb_multiprecision.npz')
MODELS = {'m32': ('matern32', 2), 'm52': ('matern52', 3), 'm52d5': ('matern52', 5), 'm52d10': ('matern52', 10), 'exp3': ('exp', 3),
          'wide': ('matern32', 16)}
RECURSION_ONLY = ('wide',)                # no PP / PF2 / Psm stored
RUNS = {'m32': 300, 'm52': 300, 'span': 2305, 'span_wide': 2100}


def rnd(x):
    return to_float(mp.mpf(x)._mpf_, rnd=round_nearest)


def to_np(M):
    return np.array([[rnd(M[i, j]) for j in range(M.cols)] for i in range(M.rows)])


def model_inputs(name):
    kernel, D = MODELS[name]
    lam, var, om = ref.recipe(kernel, D, D + 700)
    A, Q, H, Pinf, K, tau1 = get_disc_model(lam, var, om, D, kernel, 6)
    A = np.array(A, float); Q = np.array(Q, float); Q = (Q + Q.T) / 2
    assert np.array_equal(Q, Q.T)
    return dict(A=A, Q=Q, H=np.array(H, float).reshape(1, -1), vary=np.array(ref.VARY), Pinf=np.array(Pinf, float),
                lamx=lam, varx=var, omega=om)


def solve_setup(name):
    mp.dps = DPS
    c = model_inputs(name)
    A = _mat(c['A']); Q = _mat(c['Q']); H = _mat(c['H']); R = mp.mpf(float(c['vary']))
    PP, n1 = dare(A, Q, H, R)                                        # :49, residual checked inside
    Sinn = (H * PP * H.T)[0, 0] + R
    Kg = PP * H.T / Sinn                                             # :59
    HA = H * A
    AKHA = A - Kg * HA                                               # :62
    PF2 = PP - Kg * (H * PP)                                         # :74
    G = PF2 * A.T * mp.inverse(PP)                                   # :129
    out = dict(c, Sinn=np.array(rnd(Sinn)), Kg=to_np(Kg)[:, 0], HA=to_np(HA)[0], AKHA=to_np(AKHA), G=to_np(G))
    n2 = 0
    if name not in RECURSION_ONLY:
        QQ = PF2 - G * PP * G.T; QQ = (QQ + QQ.T) / 2                # :132-133
        Psm, n2 = stein(G, QQ)                                       # :134, residual checked inside
        out.update(PP=to_np(PP), PF2=to_np(PF2), Psm=to_np(Psm))
    print('set-up %-7s S = %2d  doubling steps DARE %d / Stein %d' % (name, A.rows, n1, n2), flush=True)
    return name, out


def run_inputs(name, m):
    """y and the stored steps of a recursion case on its model's inputs"""
    T = RUNS[name]
    y = ref.simulate_y(m['A'], m['Q'], m['H'], m['Pinf'], T, T + m['A'].shape[0])
    if name in ('m32', 'm52'):
        y[40:75] = np.nan; y[0] = np.nan; y[T - 1] = np.nan
        return y, np.arange(T)
    ns, L, nss = ref.spans(T, m['A'].shape[0])
    edges = np.arange(1, ns) * L
    if name == 'span':
        assert (ns, L, nss) == (18, 129, 18)
        y[0] = np.nan; y[T - 1] = np.nan; y[L - 2:L + 3] = np.nan; y[3 * L:4 * L] = np.nan
        st = np.concatenate([np.arange(6), np.arange(T - 6, T), np.arange(0, T, 16)] + [e + np.arange(-3, 3) for e in edges])
    else:
        assert (ns, L, nss) == (16, 132, 16)
        y[L - 1:L + 1] = np.nan; y[T - 2] = np.nan
        st = np.concatenate([[0, 1, T - 3, T - 2, T - 1], edges - 1, edges])
    return y, np.unique(st[(st >= 0) & (st < T)])


def solve_run(job):
    """both loops in DPS digits from the float64 set-up"""
    name, m, y, steps = job
    mp.dps = DPS
    S = m['A'].shape[0]; T = y.size
    row = lambda M: [[mp.mpf(float(v)) for v in r] for r in np.asarray(M, float)]
    A = row(m['A']); B = row(m['AKHA']); G = row(m['G']); ha = row([m['HA']])[0]; kg = row([m['Kg']])[0]
    Sinn = mp.mpf(float(m['Sinn']))
    x = [mp.mpf(0)] * S; sv2 = mp.mpf(0); MF = []
    for k in range(T):                                               # :81-110
        if not np.isnan(y[k]):
            yk = mp.mpf(float(y[k]))
            v = yk - mp.fdot(ha, x)
            x = [mp.fdot(B[i], x) + kg[i] * yk for i in range(S)]
            sv2 += v * v
        else:
            x = [mp.fdot(A[i], x) for i in range(S)]
        MF.append(x)
    MS = list(MF)
    for k in range(T - 2, -1, -1):                                   # :137-151
        d = [x[i] - mp.fdot(A[i], MF[k]) for i in range(S)]
        x = [MF[k][i] + mp.fdot(G[i], d) for i in range(S)]
        MS[k] = x
    lik = -(mp.log(2 * mp.pi) / 2 * T + mp.log(Sinn) / 2 * T + sv2 / Sinn / 2)
    col = lambda Ms: np.array([[rnd(Ms[k][i]) for k in steps] for i in range(S)])
    print('run %-9s S = %2d T = %d' % (name, S, T), flush=True)
    return name, dict(y=y, steps=steps, MF=col(MF), MS=col(MS), sum_v2=np.array(rnd(sv2)), lik=np.array(rnd(lik)))


def build(jobs):
    from multiprocessing import Pool
    names = sorted(MODELS, key=lambda n: -MODELS[n][1] * {'exp': 2, 'matern32': 4, 'matern52': 6}[MODELS[n][0]])     # largest first
    with Pool(jobs) as pool:
        models = dict(pool.map(solve_setup, names, chunksize=1))
        runs = []
        for name in sorted(RUNS, key=lambda n: -RUNS[n] * models[ref.MODEL_OF[n]]['A'].shape[0] ** 2):
            m = models[ref.MODEL_OF[name]]
            runs.append((name, m) + run_inputs(name, m))
        runs = dict(pool.map(solve_run, runs, chunksize=1))
    arrays = {'dps': np.array(DPS)}
    for name, m in models.items():
        arrays[name + '__kernel'] = np.array(MODELS[name][0]); arrays[name + '__D'] = np.array(MODELS[name][1])
        for k, v in m.items():
            if k != 'Pinf' or name in ref.MODEL_OF.values():
                arrays['%s__%s' % (name, k)] = v
    for name, r in runs.items():
        for k, v in r.items():
            arrays['run_%s__%s' % (name, k)] = v
    return arrays


if __name__ == '__main__':
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--jobs', type=int, default=8)
    ap.add_argument('--out', default=OUT)
    a = ap.parse_args()
    write_npz(a.out, build(a.jobs))
    print('wrote %s (%d bytes)' % (os.path.relpath(a.out, ROOT), os.path.getsize(a.out)))
