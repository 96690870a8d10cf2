"""Timing of the modulator prior fit objective (nagp_segp_obj) on a GPU machine: python tools/bench_segp.py [out.txt]
  - objective and gradient of one parameter (what trainSEGP_RS evaluates) at T = 84 010 and 200 000, for 1, 3 and 24 problems with
    per-problem spectra;
  - one modulator_prior_init on three components of T = 84 010: total time and the share inside nagp_segp_obj.
Device time is that of the two kernels between two HIP events inside the call (nagp_segp_timings); `call` is the host clock around the
whole entry point (allocation, upload, kernels, download, free).  WARM warm-up calls, then REPS calls; median (min .. max), per call
and per problem.  Beside each: the wall time of the vectorised NumPy restatement (tests/segp_ref.py) of the same problems on the same
box, median of 5 -- the yardstick, since no earlier code of this project computes the objective."""
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'nonstationary-audio-gp_amd')); sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np
import nagp
from nagp import _lib as L
import segp_ref as ref

out_path = sys.argv[1] if len(sys.argv) > 1 else None
WARM, REPS = 3, 25
lines = []


def say(s):
    print(s, flush=True); lines.append(s)


def stats(a):
    a = np.asarray(a)
    return '%.1f (%.1f .. %.1f)' % (float(np.median(a)), float(a.min()), float(a.max()))


def problems(T, P, seed=1):
    rng = np.random.default_rng(seed)
    ell = 40.0 * np.exp(0.3 * rng.standard_normal(P))
    _, c = ref.se_spec(55.0, T)
    spec = T * (c + 0.1)[None, :] * rng.exponential(1.0, (P, T))
    return np.log(ell)[:, None], spec, np.full(P, 0.1), 0.8 + 0.4 * rng.random(P)


def device_ms():
    ms = C.c_double(0.0)
    L.check(L.lib().nagp_segp_timings(C.byref(ms)))
    return ms.value


nagp.build()
assert L.lib().nagp_device_count() >= 1, 'no GPU visible'
say('nagp_segp_obj, n_param = 1 with the gradient, per-problem specy: us per call, median (min .. max) of %d calls after %d warm-up calls; NumPy restatement of the same problems: median of 5' % (REPS, WARM))
for T in (84010, 200000):
    for P in (1, 3, 24):
        param, spec, vary, varx = problems(T, P)
        dev, call = [], []
        for r in range(WARM + REPS):
            t = time.perf_counter()
            nagp.segp_obj(param, spec, vary=vary, varx=varx)
            dt = time.perf_counter() - t
            if r >= WARM:
                dev.append(1e3 * device_ms()); call.append(1e6 * dt)
        host = []
        for r in range(5):
            t = time.perf_counter()
            for q in range(P):
                ref.obj(param[q], spec[q], vary[q], varx[q])
            host.append(1e6 * (time.perf_counter() - t))
        say('  T %6d  %2d problems: kernels %s us, whole call %s us (%.1f us per problem), NumPy %s us (%.1f us per problem)'
            % (T, P, stats(dev), stats(call), float(np.median(call)) / P, stats(host), float(np.median(host)) / P))

T = 84010
rng = np.random.default_rng(7)
HEst = np.stack([np.log1p(np.exp(1.5 * ref.se_signal(T, ell, 20 + k, noise_var=0.05))) for k, ell in enumerate((30.0, 60.0, 90.0))], axis=1)
nagp.segp_obj(np.zeros(1), np.ones(T), vary=0.1, varx=1.0)                  # warm-up evaluation
acc = dict(n=0, call=0.0, dev=0.0)
orig = nagp.segp.segp_obj


def timed(*a, **k):
    t = time.perf_counter()
    out = orig(*a, **k)
    acc['call'] += time.perf_counter() - t; acc['dev'] += 1e-3 * device_ms(); acc['n'] += 1
    return out


nagp.segp.segp_obj = timed
t = time.perf_counter()
lenx_nmf, varx_nmf, mux, infos = nagp.modulator_prior_init(HEst)
total = time.perf_counter() - t
nagp.segp.segp_obj = orig
say('modulator_prior_init, three components of T = %d (one run after a warm-up evaluation): total %.3f s, %d batched calls, inside nagp_segp_obj %.3f s (%.0f %%; kernels %.4f s); lenx_nmf %s'
    % (T, total, acc['n'], acc['call'], 100 * acc['call'] / total, acc['dev'], np.array2string(lenx_nmf, precision=3)))
t = time.perf_counter()
h = ref.modulator_prior_init(HEst)
say('  the same block on the NumPy restatement, one component after the other: total %.3f s; lenx_nmf %s' % (time.perf_counter() - t, np.array2string(h[0], precision=3)))
if out_path:
    with open(out_path, 'w') as fh:
        fh.write('\n'.join(lines) + '\n')
