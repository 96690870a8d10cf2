#!/usr/bin/env python3
"""How fast the fixed-site Kalman filter of sweep 2 forgets its start (CPU only; the table behind nagp_plan_set_windows' overlap).

    python tools/window_contraction.py [--models cfg2,cfg2audio,cfg5seg,cfg5,sixstate] [--T steps] [--out profiles/r07_window_contraction.txt]

Per model: sweep 1 (ADF filter, smoother, site refresh) by the sequential CPU algorithm (the compiled oracle; the NumPy oracle where no
compiled one is built) gives the sites the filter of sweep 2 runs on.  That filter (dense NumPy: gf_ep_modulator_nmf.m:126-198 with the
sites fixed) then runs once from the true start and, restarted from the prior (m = 0, P = Pinf) at several k0, for L more steps.
Printed against L, the two figures the library's boundary check uses (include/nagp.h):
    mismatch_m = max|dm| / max(max|m|, sqrt(max|P|)),   mismatch_P = max|dP| / max|P|      at step k0 + L - 1.
models (bench.py / tools/full_length_parity.py recipes, a prefix of T steps of the same prior sample):
  cfg2      gf_ep_modulator_nmf, 16 ch / 3 comps, seed 1000, damping 0.5 (S = 73)
  cfg2audio the same model on the first steps of the decoded speech file (tests/golden/audio_speech_74.npz), damping 0.1
  cfg5seg   gf_ep_modulator_nmf_constraints model, 32 ch / 6 comps, seed 1000 (S = 146, balanced)
  cfg5      the same model family, seed 5000 (the first of bench.py's eight cfg5 segments)
  sixstate  8 ch / 3 comps, Matern-5/2 sub-bands (blocks of six states), seed 11, damping 0.1 (S = 57), 30 000 steps
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'nonstationary-audio-gp_amd'))

import numpy as np  # noqa: E402

MODELS = {
    'cfg2': dict(D=16, N=3, p=9, recipe='demo_nmf', balance=False, seed=1000, k1='matern32', damping=0.5),
    'cfg2audio': dict(D=16, N=3, p=9, recipe='demo_nmf', balance=False, seed=1000, k1='matern32', damping=0.1, audio='speech_74'),
    'cfg5seg': dict(D=32, N=6, p=7, recipe='constraints', balance=True, seed=1000, k1='matern32', damping=0.5),
    'cfg5': dict(D=32, N=6, p=7, recipe='constraints', balance=True, seed=5000, k1='matern32', damping=0.5),
    'sixstate': dict(D=8, N=3, p=7, recipe='demo_nmf', balance=False, seed=11, k1='matern52', damping=0.1, T=30000),
}
LS = (250, 500, 1000, 1500, 2000, 2500, 3000, 3500, 4000, 5000, 6000, 8000, 10000, 12000)


def sweep2_sites(c, T):
    from nagp import harness
    from oracle import gf_ep as ogf, lik as olik, ss as oss
    pr = harness.nmf_problem(c['D'], c['N'], T, c['seed'], c['recipe'], kernel1=c['k1'])
    if c.get('audio'):
        x = np.load(os.path.join(ROOT, 'tests', 'golden', 'audio_%s.npz' % c['audio']))['samples'].astype(np.float64) / 32768.0
        pr['y'] = (x / np.std(x))[:T]
    lik_param, p1, p2, W = oss.unpack_log(pr['w'], 1, c['D'], c['N'])
    model = ogf.assemble(lik_param, p1, p2, W, c['k1'], 'matern52', c['balance'])
    omom = olik.Mom(olik.LIK_POWER_NMF, p=c['p'])
    d = c['damping'] * np.ones(2)
    r = None
    if c['k1'] == 'matern32':
        try:
            from oracle import cpu as ocpu
            ocpu.build()
            r = ocpu.gf_predict(model, pr['y'], omom, 0.5, d, 2, c['D'], c['N'], structured=True)
        except Exception as e:          # no compiler: the NumPy oracle below
            print('# compiled oracle unavailable (%s): NumPy oracle' % e, flush=True)
    if r is None:
        r = ogf.run_predict(model, pr['y'], omom, 0.5, d, 2)
    # with two sweeps the sites of the steps k < T-1 are those the filter of sweep 2 ran on (the last sweep refreshes none of them)
    return model, pr['y'], np.asarray(r['ttau'], float), np.asarray(r['tnu'], float)


def fixed_site_filter(model, y, ttau, tnu, k_from, k_to, m=None, P=None, keep=()):
    """steps [k_from, k_to) of the fixed-site filter from (m, P) after step k_from - 1 (None: the prior); returns {k: (m, P)} for k in keep"""
    from oracle import gf_ep as ogf
    A, Q, H, Pinf = model['A'], model['Q'], model['H'], model['Pinf']
    if m is None:
        m = np.zeros(A.shape[0]); P = Pinf.copy()
    out = {}
    for k in range(k_from, k_to):
        if k > 0:
            m = A @ m; P = A @ P @ A.T + Q
        if not np.isnan(y[k]):
            fmu = H @ m; W = P @ H.T; HPH = np.diag(H @ P @ H.T).copy()
            m, P = ogf.kalman_update_split(m, P, H, W, HPH, fmu, ttau[:, k], tnu[:, k])
        if k in keep:
            out[k] = (m.copy(), P.copy())
    return out


def mismatch(a, ref):
    (m, P), (mr, Pr) = a, ref
    return (float(np.max(np.abs(m - mr)) / max(np.max(np.abs(mr)), np.sqrt(np.max(np.abs(Pr))))), float(np.max(np.abs(P - Pr)) / np.max(np.abs(Pr))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--models', default='cfg2,cfg2audio,cfg5seg,cfg5,sixstate')
    ap.add_argument('--T', type=int, default=0, help='steps per model (default: 12 000; 30 000 for sixstate)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r07_window_contraction.txt'))
    a = ap.parse_args()
    lines = ['# tools/window_contraction.py: fixed-site filter of sweep 2 restarted from the prior at k0, mismatch against the filter run from the true',
             '# start after L steps (at step k0 + L - 1): mismatch_m = max|dm| / max(max|m|, sqrt(max|P|)), mismatch_P = max|dP| / max|P|.',
             '# CPU, float64, dense NumPy recursion on the sites of the sequential CPU algorithm.', '']
    for name in [n for n in a.models.split(',') if n]:
        c = MODELS[name]
        T = a.T or c.get('T', 12000)
        t0 = time.time()
        model, y, ttau, tnu = sweep2_sites(c, T)
        k0s = [k for k in (T // 6, T // 3, T // 2) if k > 0]
        ends = sorted({k0 + L - 1 for k0 in k0s for L in LS if k0 + L - 1 < T - 1})
        ref = fixed_site_filter(model, y, ttau, tnu, 0, T - 1, keep=set(ends))
        lines.append('%s  (T = %d, D = %d, N = %d, S = %d, %s sub-bands, damping %.1f; %d clamped sites of %d)' % (
            name, T, c['D'], c['N'], model['A'].shape[0], c['k1'], c['damping'], int(np.sum(ttau[:, :T - 1] == 0)), ttau[:, :T - 1].size))
        lines.append('    %6s' % 'L' + ''.join('   k0 = %-6d m        P ' % k0 for k0 in k0s) + '   worst m    worst P')
        rows = {}
        for k0 in k0s:
            Ls = [L for L in LS if k0 + L - 1 < T - 1]
            got = fixed_site_filter(model, y, ttau, tnu, k0, k0 + max(Ls), keep={k0 + L - 1 for L in Ls})
            for L in Ls:
                rows.setdefault(L, {})[k0] = mismatch(got[k0 + L - 1], ref[k0 + L - 1])
        for L in sorted(rows):
            r = rows[L]
            lines.append('    %6d' % L + ''.join(('   %9.2e %9.2e  ' % r[k0]) if k0 in r else ' ' * 24 for k0 in k0s) +
                         '   %9.2e  %9.2e' % (max(v[0] for v in r.values()), max(v[1] for v in r.values())))
        lines.append('    (%.0f s)' % (time.time() - t0))
        lines.append('')
        print('\n'.join(lines[-(len(rows) + 4):]), flush=True)
    txt = '\n'.join(lines) + '\n'
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as fh:
        fh.write(txt)
    return 0


if __name__ == '__main__':
    sys.exit(main())
