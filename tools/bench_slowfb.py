"""Timing of the exact filterbank smoother (nagp_slowfb_run) on a GPU machine: python tools/bench_slowfb.py [T] [out.txt]
matern32 sub-bands, D = 16 (S = 64) and D = 32 (S = 128), T = 20 000, n_series = 1 and 8, cov = 'diag' (Pdiag) and cov = 'sub' with the
covS indices (first state of every sub-band).  The three kernels are timed separately with HIP events inside the call
(nagp_slowfb_timings): one warm-up call, then REPS calls; median and min..max spread.  Reported per configuration: microseconds per
step of the two sequential kernels (forward, backward) and the achieved FP64-MFMA rate of the time-parallel one (2 S^2 x panel columns
flops per series and step over its device time) -- the figures a later tuning change is held to.  Beside them, for the same model and
T: nagp_fastfb_run (the steady-state pair, wall time of the call) and the NumPy restatement tests/slowfb_ref.py on the CPU at a T it
can finish, scaled linearly."""
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'nonstationary-audio-gp_amd')); sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np
import nagp
from nagp import _lib as L
from nagp import fastfb
import slowfb_ref as ref

T = int(sys.argv[1]) if len(sys.argv) > 1 else 20000
out_path = sys.argv[2] if len(sys.argv) > 2 else None
REPS, T_CPU = 3, 200
lines = []


def say(s):
    print(s, flush=True); lines.append(s)


def stats(a):
    a = np.asarray(a)
    return float(np.median(a)), float(a.min()), float(a.max())


say('nagp_slowfb_run: matern32, T = %d, warm-up 1 + %d calls, median (min .. max)' % (T, REPS))
lib = L.lib()
for D in (16, 32):
    A, Q, H, P0, tau = ref.model('matern32', D); S = A.shape[0]
    y1 = ref.sample_y(A, Q, H, P0, T, 3); vary1 = np.full(T, 1e-4)
    vary1[T // 4:T // 4 + 500] = 1e5; y1[T // 4:T // 4 + 500] = 0.0; y1[T // 2:T // 2 + 100] = np.nan
    covS = np.arange(0, S, 2 * tau)
    # the two references
    t0 = time.perf_counter(); ref.slowfb(A, Q, H, P0, y1[:T_CPU], vary1[:T_CPU]); t_cpu = (time.perf_counter() - t0) * T / T_CPU
    Af, Hf, R, Sinn, Kg, HA, AKHA, PF2, G, Psm = fastfb._steady_state(A, Q, H, 1e-4)
    MSf = np.zeros((S, T), order='F'); sv2 = C.c_double(0.0); yc = L.f64(np.nan_to_num(y1), 'C'); tf = []
    for i in range(REPS + 1):
        t0 = time.perf_counter()
        L.check(lib.nagp_fastfb_run(S, L.dptr(Af), L.dptr(AKHA), L.dptr(L.f64(HA, 'C')), L.dptr(L.f64(Kg, 'C')), L.dptr(G), L.dptr(yc), T, L.dptr(MSf), C.byref(sv2), 0))
        tf.append(time.perf_counter() - t0)
    say('S = %3d  references: nagp_fastfb_run %.1f ms (%.1f .. %.1f, whole call); NumPy restatement on the CPU %.1f s (T = %d scaled to %d)'
        % ((S,) + tuple(1e3 * x for x in stats(tf[1:])) + (t_cpu, T_CPU, T)))
    for n in (1, 8):
        ys = np.tile(y1, (n, 1)); vs = np.tile(vary1, (n, 1))
        for cov in ('diag', 'sub'):
            ms = []; wall = []
            for i in range(REPS + 1):
                t0 = time.perf_counter()
                lik, MS, Pd, Ps = nagp.slowfb_run(A, Q, H, P0, ys, vs, want_diag=(cov == 'diag'), sub_idx=(covS if cov == 'sub' else None), block=2 * tau)
                wall.append(time.perf_counter() - t0)
                m3 = (C.c_double * 3)(); lib.nagp_slowfb_timings(m3); ms.append(list(m3))
            ms = np.array(ms[1:]); f, b, c = (stats(ms[:, j]) for j in range(3))
            cols = 16 * ((S + 15) // 16) if cov == 'diag' else 16 * ((covS.size + 15) // 16)
            flops = 2.0 * S * S * cols * T * n
            say('S = %3d n_series = %d cov = %-4s  forward %8.1f ms (%.1f .. %.1f) = %.2f us/step   backward %8.1f ms (%.1f .. %.1f) = %.2f us/step   '
                'time-parallel %8.1f ms (%.1f .. %.1f) = %.2f TFLOP/s FP64 MFMA   call %.2f s   finite %s'
                % (S, n, cov, f[0], f[1], f[2], 1e3 * f[0] / T, b[0], b[1], b[2], 1e3 * b[0] / T, c[0], c[1], c[2], flops / (c[0] * 1e-3) / 1e12,
                   float(np.median(wall[1:])), bool(np.all(np.isfinite(MS)) and np.all(np.isfinite(lik)))))
if out_path:
    with open(out_path, 'w') as fh:
        fh.write('\n'.join(lines) + '\n')
