"""Timing of the objective of the conjugate-gradient NMF with temporal priors (nagp_nmf_temp_obj) on a GPU machine:
python tools/bench_nmf_temp.py [out.txt]
  - one evaluation (objective and gradient) at the drivers' shape T = 84 010, D = 16, K = 3, inverse-gamma chain, learning form, for 1
    problem and for 20 (the drivers' restart count), with the H' dA partial products on the matrix cores and, interleaved call by call,
    on the VALU (the developer switch NAGP_NMFT_VALU): the measured choice between the two;
  - the traffic of one evaluation (A, vary, x in, dObj out, once each) against the kernel time, beside the chip's measured stream rate;
  - nmf_inf_many with 20 candidates as one lock-step batch against the same 20 one after another (NMFT_BENCH_NUMITS line searches,
    default 20, in chunks of 10).
`kernels` is the device time between two HIP events inside the call (nagp_nmf_temp_timings); `resident` is the host clock around
nagp_nmf_temp_eval on a handle made before (x in, kernels, Obj and dObj out); `one-shot` is the host clock around nagp_nmf_temp_obj
(create -- allocation, upload of A, vary, the parameters -- eval, destroy).  WARM warm-up calls, then REPS calls; median (min .. max).
Beside each: the wall time of the NumPy restatement (tests/nmf_temp_ref.py) of the same problems on the same box, median of 3 -- the
yardstick, since no earlier code of this project computes the objective."""
import ctypes as C
import os
import sys
import time

os.environ['NAGP_DEVELOPER'] = '1'                           # the VALU form is a developer switch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'nonstationary-audio-gp_amd')); sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np
import nagp
from nagp import _lib as L
from nagp import nmf_temp as nt
import nmf_temp_ref as ref

out_path = sys.argv[1] if len(sys.argv) > 1 else None
WARM, REPS = 3, 15
NUMITS = int(os.environ.get('NMFT_BENCH_NUMITS', '20'))
STREAM_TBS = 6.29                                            # float4 copy measured on this chip (8.0 TB/s spec)
lines = []


def say(s):
    print(s, flush=True); lines.append(s)


def stats(a):
    a = np.asarray(a)
    return '%.3f (%.3f .. %.3f)' % (float(np.median(a)), float(a.min()), float(a.max()))


def device_ms():
    ms = C.c_double(0.0)
    L.check(L.lib().nagp_nmf_temp_timings(C.byref(ms)))
    return ms.value


nagp.build()
assert L.lib().nagp_device_count() >= 1, 'no GPU visible'
T, D, K = 84010, 16, 3
A, W, H, vary, par = ref.planted(T, D, K, seed=8)
IG = ('ig', par['muinf'], par['varinf'], par['lam'])
say('nagp_nmf_temp_obj, T = %d, D = %d, K = %d, inverse-gamma chain, learning form, with the gradient: ms per call, median (min .. max) of %d calls after %d warm-up calls,'
    ' the two forms of H\' dA interleaved call by call; NumPy restatement of the same problems: median of 3' % (T, D, K, REPS, WARM))
keep = {}
for P in (1, 20):
    rng = np.random.default_rng(P)
    x = np.stack([np.concatenate([np.log(H).reshape(-1, order='F') + 0.1 * rng.standard_normal(T * K), np.log(W).reshape(-1, order='F')]) for _ in range(P)])
    os.environ.pop('NAGP_NMFT_VALU', None)
    hm = nt.NmfTempHandle(A, vary, None, *IG, K=K, n_problems=P)
    os.environ['NAGP_NMFT_VALU'] = '1'
    hv = nt.NmfTempHandle(A, vary, None, *IG, K=K, n_problems=P)
    os.environ.pop('NAGP_NMFT_VALU', None)
    tm = {('mfma', 'dev'): [], ('mfma', 'res'): [], ('valu', 'dev'): [], ('valu', 'res'): []}
    for r in range(WARM + REPS):
        for name, h in (('mfma', hm), ('valu', hv)):
            t = time.perf_counter()
            h.eval(x)
            dt = time.perf_counter() - t
            if r >= WARM:
                tm[(name, 'dev')].append(device_ms()); tm[(name, 'res')].append(1e3 * dt)
    Om, dm = hm.eval(x); Ov, dv = hv.eval(x)
    hm.close(); hv.close()
    one = []
    for r in range(WARM + REPS):
        t = time.perf_counter()
        nagp.nmf_temp_obj(x, A, vary, None, *IG)
        dt = time.perf_counter() - t
        if r >= WARM:
            one.append(1e3 * dt)
    host = []
    for r in range(3):
        t = time.perf_counter()
        for q in range(P):
            ref.obj(x[q], A, vary, None, *IG)
        host.append(1e3 * (time.perf_counter() - t))
    traffic = 8.0 * (2 * T * D + P * 2 * (T * K + K * D))                     # A and vary once (the problems of a batch share them through the caches at best), x in, dObj out
    km = float(np.median(tm[('mfma', 'dev')])); kv = float(np.median(tm[('valu', 'dev')]))
    keep[P] = (km, kv, float(np.median(tm[('mfma', 'res')])), float(np.median(host)))
    say('  %2d problem%s: kernels matrix cores %s ms, VALU %s ms; resident call %s ms (VALU %s ms; %.1f MB of x, Obj and dObj cross the bus); one-shot call %s ms; NumPy %s ms'
        % (P, 's' if P > 1 else ' ', stats(tm[('mfma', 'dev')]), stats(tm[('valu', 'dev')]), stats(tm[('mfma', 'res')]), stats(tm[('valu', 'res')]),
           8.0 * P * (2 * (T * K + K * D) + 1) / 1e6, stats(one), stats(host)))
    say('              the two forms agree within %.1e in dObj; %.1f MB streamed once is %.1f us at %.2f TB/s: the kernels take %.1f x that (%.2f TB/s)'
        % (ref.dist(dv, dm), traffic / 1e6, traffic / STREAM_TBS / 1e6, STREAM_TBS, km * 1e-3 / (traffic / (STREAM_TBS * 1e12)), traffic / (km * 1e-3) / 1e12))
say('  the faster form of H\' dA at 20 problems: %s (%.3f against %.3f ms in kernels); resident batched evaluation against NumPy: %.0f x'
    % ('matrix cores' if keep[20][0] <= keep[20][1] else 'VALU', min(keep[20][:2]), max(keep[20][:2]), keep[20][3] / keep[20][2]))

R = 20
rng = np.random.default_rng(4)
Hs = [np.exp(rng.standard_normal((T, K))) for _ in range(R)]
t = time.perf_counter()
many = nt.nmf_inf_many(A, [W] * R, Hs, par['muinf'], par['varinf'], par['lam'], vary, NUMITS, 10)
t_many = time.perf_counter() - t
t = time.perf_counter()
single = [nt.nmf_inf_many(A, [W], [Hs[r]], par['muinf'], par['varinf'], par['lam'], vary, NUMITS, 10)[0] for r in range(R)]
t_single = time.perf_counter() - t
same = all(np.array_equal(many[r][0], single[r][0]) and np.array_equal(many[r][1]['Obj'], single[r][1]['Obj']) for r in range(R))
say('nmf_inf_many, %d candidates of T = %d, inverse-gamma chain, %d line searches each: one lock-step batch %.2f s, one after another %.2f s (results %s)'
    % (R, T, NUMITS, t_many, t_single, 'bit-equal' if same else 'DIFFER'))
if out_path:
    with open(out_path, 'w') as fh:
        fh.write('\n'.join(lines) + '\n')
