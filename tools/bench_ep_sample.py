"""Joint posterior draws of a full-covariance EP run, timing on a GPU machine: python tools/bench_ep_sample.py [T] [T_numpy]
The speech shape of BASELINE configs[2]: D/N = 16/3 (S = 73, M = 19), T = 84 010, a gap of 4 000 steps.  First the inference the draws
belong to -- nagp.gf_ep_modulator_nmf, two sweeps -- then nagp_ep_sample on its sites for 16 and for 256 draws (Sdraw and the mean
chain; for 16 draws also with Fdraw crossing PCIe).  Every figure after one warm-up call, median and range of REPS calls; the three
kernel times are those of nagp_ep_sample_timings (HIP events) of the median call.  The NumPy restatement of the tests runs the same
law at T_numpy steps, once.  Prints one JSON line."""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'nonstationary-audio-gp_amd')); sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np
import nagp
from nagp import harness, Mom, SSHandle, ss as pss
from nagp.api import _Problem

T = int(sys.argv[1]) if len(sys.argv) > 1 else 84010
T_NUMPY = int(sys.argv[2]) if len(sys.argv) > 2 else 1000
D, N, REPS = 16, 3, 3
pr = harness.nmf_problem(D, N, T, 42)
y = pr['y'].copy(); y[T // 2:T // 2 + min(4000, T // 4)] = np.nan
t = np.arange(1, T + 1.0)
mom = Mom('likModulatorNMFPower', p_cubature=5)


def timed(f, reps=REPS):
    f()                                                     # warm-up
    ts, extra = [], []
    for _ in range(reps):
        t0 = time.perf_counter(); r = f(); ts.append(time.perf_counter() - t0); extra.append(r)
    i = int(np.argsort(ts)[len(ts) // 2])
    return dict(median_s=ts[i], min_s=min(ts), max_s=max(ts)), extra[i]


res = {}
run = lambda: nagp.gf_ep_modulator_nmf(pr['w'], t, y, SSHandle(), mom, t, 'matern32', 'matern52', 1, D, N, 0.5, 0.5 * np.ones(2), 2, nargout=6)[5]
res['two_sweep_run'], out = timed(run)
prob = _Problem(pss.ss_blocks_nmf(pr['param1'], pr['param2'], 'matern32', 'matern52'), pr['W'], np.log(pr['w_lik']))
finite = True
for n, fdraw in ((16, False), (16, True), (256, False)):
    def call():
        F, X, Sd, MS, cnt = nagp.ep_sample(prob, out['ttau'], out['tnu'], y, n, 1, 0, False, mom, fdraw=fdraw, return_counters=True)
        return dict(nagp.ep_sample_timings(), counters=[int(c) for c in cnt], finite=bool(np.all(np.isfinite(Sd)) and np.all(np.isfinite(MS))),
                    ms_vs_run=float(np.max(np.abs(MS - out['MS'])) / np.max(np.abs(out['MS']))))
    tm, ex = timed(call)
    finite = finite and ex.pop('finite')
    res['%d_draws%s' % (n, '_with_Fdraw' if fdraw else '')] = dict(call=tm, kernels_ms=ex)
# the NumPy restatement at a length it can finish
import epsample_ref as ref
Tn = min(T_NUMPY, T)
md = dict(A=prob.A, Q=prob.Q, Pinf=prob.Pinf, offsets=prob.blk.offsets, h_val=prob.blk.h_val)
t0 = time.perf_counter()
ref.sample(md, out['ttau'][:, :Tn], out['tnu'][:, :Tn], y[:Tn], False, 16, 1, sig=(pr['W'], 0, 0, 0.0))
res['numpy_restatement'] = dict(T=Tn, n_draws=16, seconds=time.perf_counter() - t0)
print(json.dumps({'workload': 'nagp_ep_sample, matern32/matern52, D/N=%d/%d (S=%d), T=%d, outputs Sdraw + MS' % (D, N, prob.blk.S, T), 'finite': finite, **res}))
