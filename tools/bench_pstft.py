"""Timing of the spectrum-fit objective (nagp_pstft_obj) on a GPU machine: python tools/bench_pstft.py [out.txt]
  - objective and gradient at a level's size, N = 1998, D = 12 and 32, every kernel and form;
  - objective only at N = 168 018, the full-length spectrum of speech_74.wav (likeUnReg, fit_probSTFT_SD.m:313), same D;
  - the whole fit with the options of experiments/train_GTFNMF.m:47-56 (minT 100, maxT 1000, numIts 10, numLevels 30, bet 750) on the
    samples of tests/golden/audio_speech_74.npz with D = 16, for exp and matern72: total time and the share inside nagp_pstft_obj.
Device time is that of the two kernels between two HIP events inside the call (nagp_pstft_timings); `call` is the host clock around
the whole entry point (allocation, upload, kernels, download, free).  WARM warm-up calls, then REPS calls; median (min .. max).
Beside each: the wall time of the vectorised NumPy restatement (tests/pstft_ref.py) on the same box, median of 5 -- the yardstick,
since no earlier code of this project computes the objective.  At N = 1998, D = 12 the generic file's own per-frequency solves in
NumPy (pstft_ref.generic_literal) are timed once as well."""
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'nonstationary-audio-gp_amd')); sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np
import nagp
from nagp import _lib as L
import pstft_ref as ref

out_path = sys.argv[1] if len(sys.argv) > 1 else None
WARM, REPS = 3, 25
lines = []


def say(s):
    print(s, flush=True); lines.append(s)


def stats(a):
    a = np.asarray(a)
    return '%.1f (%.1f .. %.1f)' % (float(np.median(a)), float(a.min()), float(a.max()))


def problem(N, D, seed=1):
    rng = np.random.default_rng(seed)
    theta = np.concatenate([rng.normal(-1.0, 1.0, D), rng.normal(0.0, 1.5, D), rng.normal(-1.0, 1.0, D)])
    minVar = 1e-3 * np.ones(D); limOm = np.tile([0.0, np.pi], (D, 1)); limLam = np.tile([0.0, 0.4], (D, 1))
    specTar = rng.exponential(1.0, N) / (1.0 + np.abs(ref.omegas(N)) * 3)
    return theta, float(specTar.max() * 1e-4), specTar, minVar, limOm, limLam, 3.0


def device_ms():
    ms = C.c_double(0.0)
    L.check(L.lib().nagp_pstft_timings(C.byref(ms)))
    return ms.value


def measure(kernel, form, N, D, grad):
    a = problem(N, D)
    dev, call = [], []
    for r in range(WARM + REPS):
        t = time.perf_counter()
        nagp.pstft_obj(*a, kernel, form=form, grad=grad)
        dt = time.perf_counter() - t
        if r >= WARM:
            dev.append(1e3 * device_ms()); call.append(1e6 * dt)
    f = ref.closed if form == 0 else ref.generic
    host = []
    for r in range(5):
        t = time.perf_counter(); f(kernel, *a, grad=grad); host.append(1e6 * (time.perf_counter() - t))
    return dev, call, host, a


nagp.build()
assert L.lib().nagp_device_count() >= 1, 'no GPU visible'
FORMS = [('exp', 0), ('exp', 1), ('matern32', 0), ('matern32', 1), ('matern52', 0), ('matern52', 1), ('matern72', 1)]
say('nagp_pstft_obj: us per evaluation, median (min .. max) of %d calls after %d warm-up calls; NumPy restatement: median of 5' % (REPS, WARM))
for grad, N in ((True, 1998), (False, 168018)):
    say('%s, N = %d' % ('objective and gradient' if grad else 'objective only', N))
    for D in (12, 32):
        for kernel, form in FORMS:
            dev, call, host, a = measure(kernel, form, N, D, grad)
            say('  D %2d %-8s form %d: kernels %s us, whole call %s us, NumPy %s us' % (D, kernel, form, stats(dev), stats(call), stats(host)))
a = problem(1998, 12)
t = time.perf_counter(); ref.generic_literal('matern72', *a); dt = time.perf_counter() - t
say('the generic file\'s own solves in NumPy (12 x 1998 systems of 8 x 8, three right-hand sides), N = 1998, D = 12, matern72, once: %.2f s' % dt)
d1, c1, _, _ = measure('exp', 0, 256, 12, True)
say('launch and call cost: N = 256 (one workgroup), D = 12, exp, with gradient: kernels %s us, whole call %s us' % (stats(d1), stats(c1)))
say('  (the whole call adds to the kernels a hipMalloc / hipFree pair, five or six small uploads, a synchronise and one or two downloads; an')
say('   on-device session object that keeps specTar and the limits resident is out of scope here)')

z = np.load(os.path.join(ROOT, 'tests', 'golden', 'audio_speech_74.npz'))
y = z['samples'].astype(float); y = y / np.std(y)
opts = dict(verbose=0, minT=100, maxT=1000, numIts=10, numLevels=30, bet=750, reassign=0)
say('fit_probSTFT_SD, %d samples of speech_74, D = 16, options of train_GTFNMF.m:47-56 (one run each after a warm-up evaluation)' % y.size)
for kernel in ('exp', 'matern72'):
    acc = dict(n=0, call=0.0, dev=0.0)

    def ev(theta, vary, specTar, minVar, limOm, limLam, bet, grad, kernel=kernel, acc=acc):
        t = time.perf_counter()
        out = nagp.pstft_obj(theta, vary, specTar, minVar, limOm, limLam, bet, kernel, grad=grad)
        acc['call'] += time.perf_counter() - t; acc['dev'] += 1e-3 * device_ms(); acc['n'] += 1
        return out
    t = time.perf_counter()
    varx, lamx, om, Info = nagp.fit_probSTFT_SD(y, 16, kernel, opts, evaluator=ev)
    total = time.perf_counter() - t
    say('  %-8s total %.2f s, %d evaluations, inside nagp_pstft_obj %.2f s (%.0f %%; kernels %.3f s), last likeUnReg %.6f'
        % (kernel, total, acc['n'], acc['call'], 100 * acc['call'] / total, acc['dev'], Info['likeUnReg'][-1]))
    acc2 = dict(t=0.0)
    rev = ref.evaluator(kernel)

    def evh(*a, acc2=acc2, rev=rev):
        t = time.perf_counter(); out = rev(*a); acc2['t'] += time.perf_counter() - t
        return out
    t = time.perf_counter()
    nagp.fit_probSTFT_SD(y, 16, kernel, opts, evaluator=evh)
    say('  %-8s the same fit on the NumPy restatement: total %.2f s, inside the objective %.2f s' % (kernel, time.perf_counter() - t, acc2['t']))
if out_path:
    with open(out_path, 'w') as fh:
        fh.write('\n'.join(lines) + '\n')
