"""Joint posterior draws of the stationary filterbank, timing on a GPU machine: python tools/bench_fastfb_sample.py [n_draws] [T]
16 Matern-3/2 sub-bands (S = 64), T = 84 010, gaps 40:75 and T-3.  One nagp_fastfb_sample call for n_draws = 64 draws (Ydraw and the
smoother mean, what nagp.kernel_ss_sampleFastFB returns without states) against 64 consecutive nagp_fastfb_run calls on the same y --
the simplest way a caller could imitate the batch; both through the C ABI with the set-up (DARE, gains, factors) done once outside the
timed region, after a warm-up call of each, median of 5.  A second figure has the states returned as well (n_draws x S x T doubles
cross PCIe, as the S x T means of every nagp_fastfb_run call do).  Prints one JSON line."""
import ctypes as C
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'nonstationary-audio-gp_amd'))
import numpy as np
import nagp
from nagp import _lib as L
from nagp import fastfb

n_draws = int(sys.argv[1]) if len(sys.argv) > 1 else 64
T = int(sys.argv[2]) if len(sys.argv) > 2 else 84010
D, R, REPS = 16, 0.01, 5
rng = np.random.default_rng(0)
lam = 1.0 / rng.uniform(20, 400, D); var = rng.uniform(0.1, 1.0, D); om = np.linspace(np.pi / 3, np.pi / 50, D)
A, Q, H, Pinf, K, tau1 = nagp.get_disc_model(lam, var, om, D, 'matern32', 6)
A, H, R, Sinn, Kg, HA, AKHA, PF2, G, Psm = fastfb._steady_state(A, Q, H, R)
S = A.shape[0]
Lq = L.f64(fastfb._lower_factor(Q)); Lp = L.f64(fastfb._lower_factor(Pinf))
y = rng.normal(size=T); y[40:75] = np.nan; y[T - 3] = np.nan
HAc, Kc, Hc = L.f64(HA, 'C'), L.f64(Kg, 'C'), L.f64(H.ravel(), 'C')
lib = L.lib()
MS = np.zeros((S, T), order='F'); Yd = np.zeros((n_draws, T)); sv2 = C.c_double(0.0)


def run64():
    for _ in range(n_draws):
        L.check(lib.nagp_fastfb_run(S, L.dptr(A), L.dptr(AKHA), L.dptr(HAc), L.dptr(Kc), L.dptr(G), L.dptr(y), T, L.dptr(MS), C.byref(sv2), 0))


def sample(Xd=None):
    L.check(lib.nagp_fastfb_sample(S, L.dptr(A), L.dptr(AKHA), L.dptr(HAc), L.dptr(Kc), L.dptr(G), L.dptr(Hc), R, L.dptr(Lp), L.dptr(Lq),
                                   L.dptr(y), T, n_draws, 1, L.dptr(Yd), L.dptr(Xd), L.dptr(MS), 0))


def median_of(f, *a):
    f(*a)                                                  # warm-up
    ts = []
    for _ in range(REPS):
        t0 = time.perf_counter(); f(*a); ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), ts


t_runs, all_runs = median_of(run64)
t_samp, all_samp = median_of(sample)
Xd = np.zeros((n_draws, T, S))
t_samp_x, all_samp_x = median_of(sample, Xd)
print(json.dumps({'workload': 'nagp_fastfb_sample, matern32, D=%d (S=%d), T=%d, %d draws in one call vs %d consecutive nagp_fastfb_run calls' % (D, S, T, n_draws, n_draws),
                  'consecutive_runs_s_median': t_runs, 'sample_call_s_median': t_samp, 'ratio_runs_over_sample': t_runs / t_samp,
                  'sample_call_with_states_s_median': t_samp_x, 'ratio_runs_over_sample_with_states': t_runs / t_samp_x,
                  'consecutive_runs_s': all_runs, 'sample_call_s': all_samp, 'sample_call_with_states_s': all_samp_x,
                  'sample_is_faster': bool(t_samp < t_runs), 'finite': bool(np.all(np.isfinite(Yd)) and np.all(np.isfinite(Xd)))}))
