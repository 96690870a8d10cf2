#!/usr/bin/env python3
"""Time-parallel fixed-site filter (nagp_plan_set_windows) against the sequential schedule, same process, same card (GPU).

    python tools/bench_windows.py [--cases cfg2,cfg5x1,cfg5x8] [--repeats 5] [--windows 8] [--overlap 8000] [--off-only] [--out FILE]

cases (bench.py's workloads):  cfg2  = gf_ep_modulator_nmf on the decoded speech file (T = 84 010, S = 73, damping 0.1)
                               cfg5x1 / cfg5x8 = one / eight segments of the constraints model (T = 100 000, S = 146)
Per case one plan; `repeats` rounds of: execute with the windows off, execute with them on (interleaved).  Reported per variant: the
median and the range of the execute time, the per-kernel times of nagp_plan_timings (median), the window statistics, and the largest
difference between the windowed and the sequential outputs (an observation, not a tolerance).
--off-only: the sequential schedule alone; with --pkg DIR (a directory holding another checkout's nagp/ package and its libnagp.so) that
checkout's -- the parent commit's, for the A/B on the same card.
"""
import argparse
import os
os.environ.setdefault('NAGP_DEVELOPER', '1')      # developer tool (NAGP_LIB is honoured regardless; the switches only with this set)
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
PKG = os.path.join(ROOT, 'nonstationary-audio-gp_amd')
for _i, _v in enumerate(sys.argv):
    if _v == '--pkg' and _i + 1 < len(sys.argv):
        PKG = os.path.abspath(sys.argv[_i + 1])
sys.path.insert(0, PKG)

import numpy as np  # noqa: E402


def problems(case):
    import full_length_parity as flp
    from nagp import harness, ss as pss
    if case == 'cfg2':
        pr = flp.problem('cfg2audio')
        blk = pss.ss_blocks_nmf(pr['param1'], pr['param2'], 'matern32', 'matern52')
        return [(blk, pr['W'], np.log(pr['w_lik']))], [pr['y']], dict(p=9, damping=0.1)
    n = {'cfg5x1': 1, 'cfg5x8': 8}[case]
    T, Tp = 100000, 12500
    probs, ys = [], []
    for q in range(n):      # bench.py's cfg5 segments (seeds 5000 ..): a prior sample of 12 500 steps, tiled (timing does not depend on the numbers)
        pr = harness.nmf_problem(32, 6, Tp, 5000 + q, 'constraints')
        blk = pss.balance_blocks(pss.ss_blocks_nmf(pr['param1'], pr['param2'], 'matern32', 'matern52'))
        probs.append((blk, pr['W'], np.log(pr['w_lik']))); ys.append(np.tile(pr['y'], T // Tp))
    return probs, ys, dict(p=7, damping=0.5)


def rel(a, b):
    return float(np.nanmax(np.abs(a - b)) / max(np.nanmax(np.abs(b)), 1e-300))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cases', default='cfg2,cfg5x1,cfg5x8')
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--windows', type=int, default=8)
    ap.add_argument('--overlap', type=int, default=8000)
    ap.add_argument('--tol', type=float, default=1e-10)
    ap.add_argument('--off-only', action='store_true')
    ap.add_argument('--pkg', default='')
    ap.add_argument('--out', default='')
    a = ap.parse_args()
    from nagp import Mom, Plan, _lib as L
    lines = ['# tools/bench_windows.py  library %s  windows %d, overlap %d, tol %g, %d interleaved repeats' % (
        os.path.relpath(L.LIB_PATH, ROOT), a.windows, a.overlap, a.tol, a.repeats)]
    for case in [c for c in a.cases.split(',') if c]:
        probs, ys, kw = problems(case)
        T = ys[0].size
        plan = Plan(L.KIND_GF_EP, probs, T, mom=Mom('likModulatorNMFPower', p_cubature=kw['p']), ep_fraction=0.5, ep_damping=kw['damping'] * np.ones(3), ep_itts=3)
        plan.upload(ys)
        plan.execute()      # warm-up (code objects, clocks)
        res = {'off': [], 'on': []}; outs = {}; stats = None
        for r in range(a.repeats):
            for variant in (('off',) if a.off_only else ('off', 'on')):
                if not a.off_only:
                    plan.set_windows(a.windows if variant == 'on' else 1, a.overlap, a.tol)
                t0 = time.perf_counter(); plan.execute(); wall = (time.perf_counter() - t0) * 1e3
                res[variant].append((wall, plan.timings()))
                if variant == 'on':
                    stats = plan.window_stats()
                if r == 0 and not a.off_only:
                    outs[variant] = plan.download(want_MS=False)
        lines.append('%s  (B = %d, T = %d, S = %d)' % (case, len(probs), T, probs[0][0].S))
        for variant in ('off', 'on'):
            if not res[variant]:
                continue
            w = np.array([x[0] for x in res[variant]])
            km = {k: float(np.median([x[1]['ms'][k] for x in res[variant]])) for k in L.KERNEL_NAMES}
            lines.append('  windows %-3s execute ms: median %.1f  min %.1f  max %.1f  (all: %s)' % (variant, np.median(w), w.min(), w.max(), ' '.join('%.1f' % v for v in w)))
            lines.append('              kernels (ms, median; the streams overlap, so they do not add up): ' + '  '.join('%s %.1f' % (k, v) for k, v in km.items() if v > 0))
        if stats is not None:
            lines.append('              last execute: %s' % stats)
            d = {f: max(rel(getattr(outs['on'][q], f), getattr(outs['off'][q], f)) for q in range(len(probs))) for f in ('Eft', 'Varft', 'ttau', 'tnu', 'nlZ')}
            lines.append('              windowed vs sequential outputs, max |diff| / max |value| (observation): ' + '  '.join('%s %.2e' % kv for kv in d.items()))
        plan.close()
        print('\n'.join(lines[-6:]), flush=True)
    txt = '\n'.join(lines) + '\n'
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'a') as fh:
            fh.write(txt)
    return 0


if __name__ == '__main__':
    sys.exit(main())
