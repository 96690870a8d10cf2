"""Timing of the fixed-point NMF (nagp_nmf_fp) on a GPU machine: python tools/bench_nmf.py [out.txt]
The workload of experiments/train_GTFNMF.m:76-83 at the size of speech_74.wav: T = 84 010, D = 16, K = 3, 20 restarts x 10 inference
iterations (one batched call, update_w = 0) plus 500 full iterations (update_w = 1), vary = zeros (passed as NULL), on synthetic
amplitudes of that size (A = (Ht Wt) .* Exp(1) noise, as the test cases).  Device time is that of the enqueued kernel sequence between
two HIP events inside the call (nagp_nmf_timings): one warm-up, then REPS calls; median and min..max.  Beside it:
  - the same statements in NumPy on the CPU (BLAS products and np.sum, not the sequential-order restatement of tests/nmf_ref.py) for one
    tenth of the iterations, scaled by ten;
  - the bytes a pass reads and writes and the fraction of the HBM bandwidth (8 TB/s) the measured time per iteration implies;
  - the time per iteration of the same two kernels on one workgroup of rows (T = 256), which is their launch and dependency cost: a
    workload within a factor two of it is latency-bound at this size."""
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'nonstationary-audio-gp_amd')); sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np
import nagp
from nagp import _lib as L

out_path = sys.argv[1] if len(sys.argv) > 1 else None
T, D, K, R, ITS_R, ITS = 84010, 16, 3, 20, 10, 500
REPS, HBM = 3, 8e12
lines = []


def say(s):
    print(s, flush=True); lines.append(s)


def stats(a):
    a = np.asarray(a)
    return float(np.median(a)), float(a.min()), float(a.max())


def problem(T, seed=1):
    rng = np.random.default_rng(seed)
    Ht = np.exp(rng.standard_normal((T, K))); Wt = rng.random((K, D)) + 0.05
    A = (Ht @ (Wt / Wt.sum(axis=1, keepdims=True))) * rng.exponential(1.0, (T, D))
    W0 = np.stack([A[rng.integers(0, T, K)] + 1e-6 for _ in range(R)]); W0 /= W0.sum(axis=2, keepdims=True)
    H0 = np.exp(rng.standard_normal((R, T, K)))
    return A, W0, H0


def device(A, W0, H0, its, update_w):
    """device ms and wall s of REPS calls after one warm-up"""
    ms, wall = [], []
    for i in range(REPS + 1):
        t0 = time.perf_counter()
        out = nagp.nmf_run(A, None, W0, H0, its, update_w=update_w)
        wall.append(time.perf_counter() - t0)
        m = (C.c_double * 1)(); L.lib().nagp_nmf_timings(m); ms.append(m[0])
    assert all(np.all(np.isfinite(o)) for o in out)
    return stats(ms[1:]), float(np.median(wall[1:])), out


def numpy_iterations(A, W, H, its, update_w):
    obj = lambda H, W: np.sum(A / (H @ W) + np.log(H @ W)) / A.shape[0]
    for _ in range(its):
        R1 = 1.0 / (H @ W)
        H = ((A * R1 * R1) @ W.T) / (R1 @ W.T) * H
        o = obj(H, W)
        if update_w:
            R1 = 1.0 / (H @ W)
            W = (H.T @ (A * R1 * R1)) / (H.T @ R1) * W
            W = (1.0 / W.sum(axis=1))[:, None] * W
            o = obj(H, W)
    return W, H, o


A, W0, H0 = problem(T)
nwg = (T + 255) // 256
say('nagp_nmf_fp: T = %d, D = %d, K = %d, vary = NULL; warm-up 1 + %d calls, median (min .. max)' % (T, D, K, REPS))
(r_ms, r_wall, _) = device(A, W0, H0, ITS_R, False)
say('restarts: %d problems x %d iterations, one call    device %8.2f ms (%.2f .. %.2f) = %.1f us per iteration of the batch = %.2f us per problem-iteration   call %.3f s'
    % (R, ITS_R, r_ms[0], r_ms[1], r_ms[2], 1e3 * r_ms[0] / ITS_R, 1e3 * r_ms[0] / ITS_R / R, r_wall))
(m_ms, m_wall, out) = device(A, W0[0], H0[0], ITS, True)
per_it = 1e-3 * m_ms[0] / ITS
say('main loop: 1 problem x %d iterations                device %8.2f ms (%.2f .. %.2f) = %.1f us per iteration   call %.3f s   last Obj %.6f'
    % (ITS, m_ms[0], m_ms[1], m_ms[2], 1e6 * per_it, m_wall, out[2][-1]))
# bytes of one full iteration (pass + finish): A is read by both loops of the pass (the second read of a workgroup's 32 KiB can hit in
# cache), H is read and written once, the partial sums are written by the pass and read by the finish kernel
issued = 8 * (2 * T * D + 2 * T * K + 2 * nwg * (2 * K * D + 2))
unique = 8 * (T * D + 2 * T * K + 2 * nwg * (2 * K * D + 2))
say('bytes per iteration: %.2f MB issued (A twice), %.2f MB if the second read of A hits in cache: %.1f%% .. %.1f%% of %.0f TB/s at %.1f us per iteration'
    % (issued / 1e6, unique / 1e6, 100 * unique / per_it / HBM, 100 * issued / per_it / HBM, HBM / 1e12, 1e6 * per_it))
rb = 8 * R * (T * D + 2 * T * K + nwg * 2)
say('restart batch: %.2f MB per iteration of the batch (A read per problem): %.1f%% of %.0f TB/s' % (rb / 1e6, 100 * rb / (1e-3 * r_ms[0] / ITS_R) / HBM, HBM / 1e12))
# the same two kernels on one workgroup of rows: launch + dependency cost of an iteration
As, Ws, Hs = problem(256, 2)
(s_ms, _, _) = device(As, Ws[0], Hs[0], ITS, True)
floor = 1e-3 * s_ms[0] / ITS
say('one workgroup of rows (T = 256), %d iterations:       device %8.2f ms = %.1f us per iteration (launch and dependency cost of the two kernels)' % (ITS, s_ms[0], 1e6 * floor))
say('main loop / that cost = %.2f%s' % (per_it / floor, ': within a factor two -- the main loop is latency-bound at this size; the batch of restarts is where the chip is used'
                                        if per_it < 2 * floor else ''))
# NumPy on the CPU: one tenth of the iterations, scaled
t0 = time.perf_counter()
for r in range(R):
    numpy_iterations(A, W0[r], H0[r], ITS_R // 10, False)
t_r = (time.perf_counter() - t0) * 10
t0 = time.perf_counter(); numpy_iterations(A, W0[0], H0[0], ITS // 10, True); t_m = (time.perf_counter() - t0) * 10
say("NumPy on the CPU, one tenth of the iterations scaled by ten: restarts %.2f s, main loop %.2f s" % (t_r, t_m))
say('device / CPU: restarts %.2f ms vs %.0f ms, main loop %.2f ms vs %.0f ms' % (r_ms[0], 1e3 * t_r, m_ms[0], 1e3 * t_m))
if out_path:
    with open(out_path, 'w') as fh:
        fh.write('\n'.join(lines) + '\n')
