"""Timing of the GPPAD envelope objective (nagp_gppad_obj) on a GPU machine: python tools/bench_gppad.py [out.txt]
  - one batched evaluation (objective and gradient) of 16 problems at (T = 84 010, Tx = 131072), the finest level of speech_74, and at
    (T = 657, Tx = 1024), its coarsest level, per-sample vary = 0 as the drivers pass it, the spectrum formed from len;
  - one GPPAD on 16 channels of T = 84 010, len = 1600 (NumIts as given by GPPAD_BENCH_NUMITS, default 80: ten line searches on each of
    the eight levels; the drivers' 2000 take 25 x as long): total time and the share inside the evaluations.
`kernels` is the device time between two HIP events inside the call (nagp_gppad_timings); `resident` is the host clock around
nagp_gppad_eval on a handle made before (x in, kernels, Obj and dObj out); `one-shot` is the host clock around nagp_gppad_obj (create --
allocation, upload of y, vary, the parameters, the spectrum kernel -- eval, destroy).  WARM warm-up calls, then REPS calls; median
(min .. max).  Beside each: the wall time of the NumPy restatement (tests/gppad_ref.py, spectrum precomputed) of the same problems on the
same box, median of 5 -- the yardstick, since no earlier code of this project computes the objective."""
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'nonstationary-audio-gp_amd')); sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np
import nagp
from nagp import _lib as L
from nagp import gppad as gp
import gppad_ref as ref

out_path = sys.argv[1] if len(sys.argv) > 1 else None
WARM, REPS = 3, 15
NUMITS = int(os.environ.get('GPPAD_BENCH_NUMITS', '80'))
lines = []


def say(s):
    print(s, flush=True); lines.append(s)


def stats(a):
    a = np.asarray(a)
    return '%.3f (%.3f .. %.3f)' % (float(np.median(a)), float(a.min()), float(a.max()))


def device_ms():
    ms = C.c_double(0.0)
    L.check(L.lib().nagp_gppad_timings(C.byref(ms)))
    return ms.value


nagp.build()
assert L.lib().nagp_device_count() >= 1, 'no GPU visible'
P = 16
say('nagp_gppad_obj, %d problems with the gradient, per-sample vary, spectrum from len: ms per call, median (min .. max) of %d calls after %d warm-up calls; NumPy restatement of the same problems: median of 5'
    % (P, REPS, WARM))
for T, Tx, ell in ((84010, 131072, 1600.0), (657, 1024, 12.5)):
    rng = np.random.default_rng(T)
    x = np.stack([0.3 * ref.se_draw(rng, ell, Tx) for _ in range(P)])
    y = np.log(1 + np.exp(x[:, :T])) * rng.standard_normal((P, T))
    vary = np.zeros((P, T))
    dev, res, one = [], [], []
    with gp.GppadHandle(y, Tx, vary, 1.0, 0.0, 1.0, len=ell) as h:
        for r in range(WARM + REPS):
            t = time.perf_counter()
            h.eval(x)
            dt = time.perf_counter() - t
            if r >= WARM:
                dev.append(device_ms()); res.append(1e3 * dt)
    for r in range(WARM + REPS):
        t = time.perf_counter()
        nagp.gppad_obj(x, y, vary, 1.0, 0.0, 1.0, len=ell)
        dt = time.perf_counter() - t
        if r >= WARM:
            one.append(1e3 * dt)
    c = ref.fft_cov(ell, Tx)
    host = []
    for r in range(5):
        t = time.perf_counter()
        for q in range(P):
            ref.obj(x[q], y[q], c, 1.0, 0.0, 1.0, vary[q])
        host.append(1e3 * (time.perf_counter() - t))
    moved = 8.0 * P * (2 * Tx + 1) / 1e6
    say('  T %6d Tx %6d: kernels %s ms, resident call %s ms (%.1f MB of x, Obj and dObj cross the bus), one-shot call %s ms, NumPy %s ms'
        % (T, Tx, stats(dev), stats(res), moved, stats(one), stats(host)))

T, D, ell = 84010, 16, 1600.0
rng = np.random.default_rng(9)
Y = np.stack([ref.envelope_signal(T, ell, 40 + d)[0] for d in range(D)], axis=1)
Params = dict(len=ell, varx=1.0, varc=1.0, mux=0.0)           # the marginal parameters are host work and not part of this figure
acc = dict(n=0, call=0.0, dev=0.0)
orig = gp.GppadHandle.eval


def timed(self, *a, **k):
    t = time.perf_counter()
    out = orig(self, *a, **k)
    acc['call'] += time.perf_counter() - t; acc['dev'] += 1e-3 * device_ms(); acc['n'] += 1
    return out


gp.GppadHandle.eval = timed
t = time.perf_counter()
A, Cc, Pout, Info, X = nagp.GPPAD(Y, Params, 0, dict(NumIts=NUMITS))
total = time.perf_counter() - t
gp.GppadHandle.eval = orig
say('GPPAD, %d channels of T = %d, len = %g, NumIts = %d (%d levels), Params given: total %.2f s, %d batched evaluations, inside nagp_gppad_eval %.2f s (%.0f %%; kernels %.3f s)'
    % (D, T, ell, NUMITS, Info[0][1]['DSs'].size, total, acc['n'], acc['call'], 100 * acc['call'] / total, acc['dev']))
t = time.perf_counter()
nagp.GPPAD(Y[:, :1], Params, 0, dict(NumIts=NUMITS), evaluator=ref.evaluator())
say('  one channel of the same on the NumPy restatement: %.2f s (x %d channels, one after the other, in the reference)' % (time.perf_counter() - t, D))
if out_path:
    with open(out_path, 'w') as fh:
        fh.write('\n'.join(lines) + '\n')
