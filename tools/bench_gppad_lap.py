"""Timing of the Laplace step of GPPAD (nagp_gppad_lap_*) on a GPU machine: python tools/bench_gppad_lap.py [out.txt]
The workload is the committed speech_74 fixture (T = 84 010) at len = 800 with the reference's default options (nev = 100, jmax = 200,
TruncPoint = 8, tol = 8, Overlap = 5): InferAmplitudeErrorBarsGPMAP.m cuts it into 4 overlapping chunks of TxCh = 32 768.
  - the error bars of 16 channels: 64 problems through one handle (the fixture holds one channel: its 4 chunks stand for every channel,
    each of the 64 problems with a start vector of its own, so that the runs differ).  The MAP points come from the device with
    NumIts = 60 (the MAP step is not what is timed).  `device span` is the time between two HIP events around each device batch of
    nagp_gppad_lap_eig (the kernels and the host's control between them: the tridiagonal eigen-solves and the recurrences), `call` the
    host clock around hess + eig + varx + obj; REPS rounds after WARM warm-up rounds, median (min .. max).
  - the NumPy restatement (tests/gppad_lap_ref.py) of the same solve for one of the problems, on the same box.
  - one GetLenGradAscent iteration of one channel end to end (the MAP step of the two time-scales with NumIts = 60 included).
Bytes are counted from the shapes: a reorthogonalisation at step j reads the j - 1 basis vectors twice (h1, then the subtraction; twice
again on a second pass), the Ritz stage reads the basis once per tile of 4 Ritz vectors and writes nconv vectors.  The stages are not
timed one by one here, so no share of the HBM bandwidth is claimed for them."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'nonstationary-audio-gp_amd')); sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np
import nagp
from nagp import _lib as L
from nagp import gppad_lap as gl
import gppad_lap_ref as ref

out_path = sys.argv[1] if len(sys.argv) > 1 else None
WARM, REPS, CHANNELS, NUMITS = 1, 3, 16, 60
lines = []


def say(s):
    print(s, flush=True); lines.append(s)


def stats(a):
    a = np.asarray(a)
    return '%.1f (%.1f .. %.1f)' % (float(np.median(a)), float(a.min()), float(a.max()))


nagp.build()
assert L.lib().nagp_device_count() >= 1, 'no GPU visible'
z = np.load(os.path.join(ROOT, 'tests', 'golden', 'audio_speech_74.npz'))
y = z['samples'].astype(float); y = y / np.sqrt(np.var(y, ddof=1)); T = y.size
Params = dict(len=800.0, varx=1.0, mux=0.0, varc=1.0, vary=1e-6)
Opts = nagp.LoadErrorBarsLapOpts()
plan = gl.chunk_plan(T, Params['len'], Opts)
nev, jmax, Tx = Opts['nev'], 2 * Opts['nev'], plan['TxCh']
say('speech_74, T = %d, len = %g, nev = %d, jmax = %d: %d chunks of TCh = %d, TxCh = %d, Overlap = %d' % (T, Params['len'], nev, jmax, plan['NumChunks'], plan['TCh'], Tx, plan['Overlap']))
ys = [y[a:b] for a, b in plan['bounds']]
t = time.perf_counter()
maps = nagp.InferAmplitudeGPMAP_many(ys, [dict(Params) for _ in ys], dict(Tx=Tx, Long=1, NumIts=NUMITS, MinLength=Opts['MinLength']))
say('MAP step of the %d chunks on the device, NumIts = %d: %.2f s' % (len(ys), NUMITS, time.perf_counter() - t))
rng = np.random.default_rng(19)
groups = {}
for ch, (a, b) in enumerate(plan['bounds']):
    groups.setdefault(b - a, []).append(ch)
for Tc, chs in groups.items():
    P = CHANNELS * len(chs)
    Y = np.stack([ys[ch] for ch in chs] * CHANNELS); X = np.stack([maps[ch][1] for ch in chs] * CHANNELS)
    V0 = rng.standard_normal((P, Tx))
    span, call = [], []
    with gl.GppadLapHandle(Y, Tx, Params['vary'], Params['varx'], Params['mux'], Params['varc'], Params['len'], jmax) as h:
        for r in range(WARM + REPS):
            t = time.perf_counter()
            h.hess(X, d=False); res = h.eig(nev, V0); V, neg = h.varx(); O = h.obj()
            dt = time.perf_counter() - t
            if r >= WARM:
                span.append(h.timings()); call.append(1e3 * dt)
    st, re_, nc = res['steps'], res['reorths'], res['nconv']
    say('error bars, %d problems of T = %d, Tx = %d in one handle (%d channels x %d chunks), ms, median (min .. max) of %d rounds after %d warm-up:' % (P, Tc, Tx, CHANNELS, len(chs), REPS, WARM))
    say('  device span of nagp_gppad_lap_eig %s ms; hess + eig + varx + obj call %s ms' % (stats(span), stats(call)))
    say('  per problem: steps %d .. %d (median %d), reorthogonalisations %d .. %d (median %d), nconv %d .. %d, status all zero: %s, negative Varx entries: %d'
        % (st.min(), st.max(), np.median(st), re_.min(), re_.max(), np.median(re_), nc.min(), nc.max(), bool(np.all(res['status'] == 0)), int(neg.sum())))
    fft_flops = 5.0 * Tx * np.log2(Tx)
    say('  from the shapes, per problem at the median: operator %.2f GFLOP (4 transforms a step), reorthogonalisation about %.2f GB read (the basis twice a pass, mean length steps / 2), '
        'Ritz stage %.2f GB read, %.3f GB written' % (4 * fft_flops * np.median(st) / 1e9, 2 * np.median(re_) * (np.median(st) / 2) * Tx * 8 / 1e9,
                                                     np.ceil(np.median(nc) / 4) * np.median(st) * Tx * 8 / 1e9, np.median(nc) * Tx * 8 / 1e9))
    if Tc == plan['TCh']:
        c = dict(x=X[0], y=Y[0], vary=Params['vary'], len=Params['len'], varx=Params['varx'], mux=Params['mux'], varc=Params['varc'], Tx=Tx, nev=nev, jmax=jmax, vstart=V0[0])
        t = time.perf_counter(); run = ref.solve(c); dt = time.perf_counter() - t
        say('  NumPy restatement of problem 0 alone: %.1f s (steps %d, reorthogonalisations %d, nconv %d; the device: %d, %d, %d); lmb distance %.2e, Varx distance %.2e'
            % (dt, run['steps'], run['reorths'], run['nconv'], st[0], re_[0], nc[0],
               ref.dist(res['lmb'][0, :nc[0]], run['lmb']) if nc[0] == run['nconv'] else float('nan'), ref.dist(V[0], run['Varx'])))
        say('  so %d problems cost the restatement about %.0f s against %.2f s on the device' % (P, dt * P, np.median(call) / 1e3))

OptsLL = nagp.LoadLearnLenGradAscentGPPADOpts(dict(NumItsLL=1, NumIts=NUMITS))
t = time.perf_counter()
ell, Info = nagp.GetLenGradAscent(Params['len'], y, Params, OptsLL, rng=np.random.default_rng(20))
say('one GetLenGradAscent iteration of one channel (stretch %d .. %d, two time-scales, MAP with NumIts = %d included): %.2f s; len %g -> %g'
    % (Info['Ts'][0, 0], Info['Ts'][0, 1], NUMITS, time.perf_counter() - t, Params['len'], ell))
if out_path:
    with open(out_path, 'w') as fh:
        fh.write('\n'.join(lines) + '\n')
