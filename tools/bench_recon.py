"""Posterior reconstruction timing (nagp_reconstruct / nagp_reconstruct_sources): python tools/bench_recon.py [repeats] [scale]
Two shapes: D=32, N=6, T=200000, s=250 (one long file) and D=48, N=9, J=3, T=96000, s=100 (source_sep_piano.m).  Per shape, alternating
within every round: (a) nagp_reconstruct, (b) the new entry in linear one-source mode, (c) sqrt amplitude with sources and envelopes
(sampling form), (c_pop) the same in the population form with ut5, then once (d) the NumPy restatement (tests/recon_sources_ref.py) on a
shortened series, scaled to T.  The GPU figures are whole calls on host arrays: copies in, the kernel, the synchronise, copies out.
`scale` < 1 shortens T (rehearsal)."""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'nonstationary-audio-gp_amd')); sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np
import nagp
import recon_sources_ref as ref

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
scale = float(sys.argv[2]) if len(sys.argv) > 2 else 1.0
softplus = lambda g: np.log(1.0 + np.exp(g))
assert nagp.lib().nagp_device_count() >= 1, 'no GPU visible'


def timed(f):
    t0 = time.perf_counter(); r = f(); return time.perf_counter() - t0, r


for D, N, J, T, s in ((32, 6, 2, 200000, 250), (48, 9, 3, 96000, 100)):
    T = max(8, int(T * scale))
    rng = np.random.default_rng(D)
    Eft = rng.normal(0, 1, (D + N, T)); Varft = np.concatenate([rng.uniform(0.05, 0.6, (D, T)), rng.uniform(0.05, 1.0, (N, T))])
    W, off = nagp.recon.stack_sources([rng.uniform(0.05, 0.3, (D // J, N // J)) for _ in range(J)])
    legs = dict(a=lambda: nagp.reconstruct_signal(Eft, Varft, W, n_samples=s, seed=1),
                b=lambda: nagp.reconstruct_sources(Eft, Varft, W, amplitude='linear', n_samples=s, seed=1),
                c=lambda: nagp.reconstruct_sources(Eft, Varft, W, amplitude='sqrt', sources=off, n_samples=s, seed=1),
                c_pop=lambda: nagp.reconstruct_sources(Eft, Varft, W, amplitude='sqrt', sources=off, p_cubature=5))
    res = {k: f() for k, f in legs.items()}                  # warm-up: library load, context, code objects
    dab = max(float(np.max(np.abs(res['a'][k] - res['b'][k])) / np.max(np.abs(res['a'][k]))) for k in ('Esig', 'Vsig', 'Eft_mod', 'Varft_mod'))
    times = {k: [] for k in legs}
    for _ in range(reps):
        for k, f in legs.items():
            times[k].append(timed(f)[0])
    nc = max(8, min(T, 1000))
    t_np = timed(lambda: ref.sampling(Eft[:, :nc], Varft[:, :nc], W, off, softplus, 'sqrt', s, 1))[0] * T / nc
    out = {'workload': 'reconstruction D=%d N=%d J=%d T=%d s=%d' % (D, N, J, T, s), 'repeats': reps,
           'numpy_restatement_s_scaled_from_%d_steps' % nc: t_np, 'max_rel_diff_a_vs_b': dab}
    for k, v in times.items():
        out[k + '_s_min'] = min(v); out[k + '_s_median'] = float(np.median(v)); out[k + '_s_all'] = [round(x, 4) for x in v]
    print(json.dumps(out), flush=True)
