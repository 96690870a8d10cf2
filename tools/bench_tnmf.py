"""Timing of the objectives of the squared-exponential basis-function NMF (nagp_tnmf_obj) on a GPU machine:
python tools/bench_tnmf.py [out.txt]
  - one evaluation (objective and gradient) at T = 84 010, D = 16, K = 3, lenx = [200, 800, 1500], tol = 11 (tau = 1556, 6223, 11668: 38 897
    taps per sample and convolution), in the learning and in the inference form, for 1 problem and for 20;
  - per kernel group the achieved FP64 FMA rate of the two convolutions (T (2 tau + 1) FMAs per column, the zero padding counted as the
    direct sum counts it) beside the chip's FP64 VALU peak, 78.6 TFLOP/s = 39.3 T FMA/s (half the FP32 vector rate).
`kernels` is the device time between HIP events inside the call (nagp_tnmf_timings: forward convolution, rows, adjoint convolution);
`resident` is the host clock around nagp_tnmf_eval on a handle made before (x in, kernels, Obj and dObj out); `one-shot` is the host
clock around nagp_tnmf_obj (create -- the taps, allocation, upload of A, vary -- eval, destroy).  WARM warm-up calls, then REPS calls;
median (min .. max).  Beside each: the wall time of the forward NumPy restatement (tests/tnmf_ref.py, np.convolve: a direct sum as
MATLAB's conv) of ONE of the problems on the same box, once; the restatement is a loop over the problems, so 20 problems are 20 x that.
The one gate: the resident evaluation is not slower than the restatement of the same problems (the tool exits with status 1 otherwise)."""
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'nonstationary-audio-gp_amd')); sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np
import nagp
from nagp import _lib as L
from nagp import tnmf as tn
import tnmf_ref as ref

out_path = sys.argv[1] if len(sys.argv) > 1 else None
WARM, REPS = 2, 7
PEAK_TFMA = 39.3
lines = []


def say(s):
    print(s, flush=True); lines.append(s)


def stats(a):
    a = np.asarray(a)
    return '%.3f (%.3f .. %.3f)' % (float(np.median(a)), float(a.min()), float(a.max()))


def device_ms():
    ms = (C.c_double * 3)()
    L.check(L.lib().nagp_tnmf_timings(ms))
    return list(ms)


nagp.build()
assert L.lib().nagp_device_count() >= 1, 'no GPU visible'
T, D, K, tol = 84010, 16, 3, 11
lenx = np.array([200.0, 800.0, 1500.0]); varx = np.array([.5, 1.0, .75]); mux = np.array([0.0, -.5, .5])
rng = np.random.default_rng(8)
X0 = rng.standard_normal((T, K))
H = np.exp(nagp.basis2SEGP(X0, lenx, varx, tol) + mux[None, :])
W = 0.05 + rng.random((K, D)) ** 2
W = W / W.sum(axis=1)[:, None]
vary = np.full((T, D), 0.01)
A = (H @ W + vary) * rng.gamma(4.0, 0.25, (T, D))
taus = tn.tau_of(lenx, tol)
fma = float(T) * float(np.sum(2 * taus + 1))                  # per problem and convolution
say('nagp_tnmf_obj, T = %d, D = %d, K = %d, lenx = %s, tol = %d (tau = %s), with the gradient: ms per call, median (min .. max) of %d calls after %d warm-up calls;'
    ' NumPy restatement: one problem, once' % (T, D, K, [float(v) for v in lenx], tol, [int(v) for v in taus], REPS, WARM))
ok = True
for learn in (True, False):
    host = None
    for P in (1, 20):
        r2 = np.random.default_rng(P)
        x = np.stack([np.concatenate([(X0 + 0.1 * r2.standard_normal((T, K))).reshape(-1, order='F')] + ([np.log(W).reshape(-1, order='F')] if learn else []))
                      for _ in range(P)])
        Wg = None if learn else W
        h = tn.TnmfHandle(A, vary, Wg, lenx, mux, varx, tol, n_problems=P)
        dev, res = [], []
        for r in range(WARM + REPS):
            t = time.perf_counter()
            O, d = h.eval(x)
            dt = time.perf_counter() - t
            if r >= WARM:
                dev.append(device_ms()); res.append(1e3 * dt)
        h.close()
        one = []
        for r in range(1 + 3):
            t = time.perf_counter()
            nagp.tnmf_obj(x, A, vary, Wg, lenx, mux, varx, tol)
            if r >= 1:
                one.append(1e3 * (time.perf_counter() - t))
        if host is None:
            t = time.perf_counter()
            Oh, dh = ref.obj(x[0], A, vary, Wg, lenx, mux, varx, tol)
            host = 1e3 * (time.perf_counter() - t)
            say('  %s form: the device agrees with the restatement within %.1e in Obj and %.1e in dObj' % ('learning' if learn else 'inference', ref.dist(O[0], Oh), ref.dist(d[0], dh)))
        dev = np.array(dev)
        med = np.median(dev, axis=0)
        rate = [P * fma / (med[s] * 1e-3) / 1e12 for s in (0, 2)]
        say('  %s form, %2d problem%s: kernels forward conv %s ms = %.2f T FMA/s (%.0f %% of %.1f), rows %s ms, adjoint conv and sum X^2 %s ms = %.2f T FMA/s (%.0f %%)'
            % ('learning' if learn else 'inference', P, 's' if P > 1 else ' ', stats(dev[:, 0]), rate[0], 100 * rate[0] / PEAK_TFMA, PEAK_TFMA, stats(dev[:, 1]), stats(dev[:, 2]),
               rate[1], 100 * rate[1] / PEAK_TFMA))
        gate = float(np.median(res)) <= P * host
        ok = ok and gate
        say('      resident call %s ms (%.1f MB of x, Obj and dObj cross the bus); one-shot call %s ms; NumPy %.0f ms per problem, %.0f ms for these: %.0f x the resident call -- gate %s'
            % (stats(res), 8.0 * P * (2 * x.shape[1] + 1) / 1e6, stats(one), host, P * host, P * host / float(np.median(res)), 'met' if gate else 'MISSED'))
if out_path:
    with open(out_path, 'w') as fh:
        fh.write('\n'.join(lines) + '\n')
sys.exit(0 if ok else 1)
