"""nagp_fastfb_sample (joint posterior draws of the stationary filterbank) without a GPU: the export and its binding, the argument
checks of the entry point (all of them run before any device call), and the NumPy restatement the GPU tests compare with
(tests/fbsample_ref.py) pinned to the oracle's smoother and to the two moments a posterior draw must have."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nagp
from nagp import _lib as L
from oracle import fastfb as offb
import fbsample_ref as ref

EINVAL, EUNSUPPORTED, ENOMEM = -1, -2, -4


def test_entry_point_is_exported_and_bound():
    path = nagp.build()
    out = subprocess.run(['nm', '-D', '--defined-only', path], capture_output=True, text=True).stdout
    assert 'nagp_fastfb_sample' in set(re.findall(r' T (nagp_[a-z0-9_]+)', out))
    assert 'nagp_fastfb_sample' in L.EXPORTS
    fn = L.lib().nagp_fastfb_sample
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 18
    assert callable(nagp.kernel_ss_sampleFastFB)


def _call(S=4, T=6, n=3, R=0.01, null=(), outs=('Y', 'X', 'M'), Salloc=None):
    """one call with well-formed arguments except for what the caller breaks; arrays are sized for Salloc, T"""
    Sa = Salloc or max(S, 1); Ta = max(T, 1); na = max(n, 1)
    mats = {k: np.eye(Sa, order='F') * 0.5 for k in ('A', 'AKHA', 'G', 'Lp', 'Lq')}
    vecs = {k: np.ones(Sa) for k in ('HA', 'K', 'H')}
    y = np.zeros(min(Ta, 64))
    p = {k: L.dptr(None if k in null else v) for k, v in {**mats, **vecs, 'y': y}.items()}
    Y = np.zeros((na, min(Ta, 64))); X = np.zeros((na, min(Ta, 64), Sa)); M = np.zeros((Sa, min(Ta, 64)), order='F')
    return L.lib().nagp_fastfb_sample(S, p['A'], p['AKHA'], p['HA'], p['K'], p['G'], p['H'], R, p['Lp'], p['Lq'], p['y'], T, n, 7,
                                      L.dptr(Y if 'Y' in outs else None), L.dptr(X if 'X' in outs else None),
                                      L.dptr(M if 'M' in outs else None), 0)


@pytest.mark.parametrize('name', ['A', 'AKHA', 'HA', 'K', 'G', 'H', 'Lp', 'Lq', 'y'])
def test_null_inputs_are_refused_on_the_host(name):
    assert _call(null=(name,)) == EINVAL
    assert b'null' in L.lib().nagp_last_error()


@pytest.mark.parametrize('kw', [dict(S=0), dict(S=-3), dict(T=0), dict(T=-1), dict(n=0), dict(n=-2),
                                dict(R=0.0), dict(R=-1.0), dict(R=float('nan')), dict(R=float('inf')), dict(outs=())])
def test_bad_sizes_variance_and_missing_outputs_are_refused_on_the_host(kw):
    assert _call(**kw) == EINVAL


def test_too_many_states_and_a_draw_beyond_the_budget_are_refused_on_the_host():
    assert _call(S=257, Salloc=257) == EUNSUPPORTED
    # one draw of S = 64, T = 2^24 takes 2 T S doubles = 16 GiB: beyond the 8 GiB budget of a call (nothing is read before the check)
    assert _call(S=64, Salloc=64, T=1 << 24, n=1, outs=('Y',)) == ENOMEM
    assert b'budget' in L.lib().nagp_last_error()


def test_python_wrapper_checks_its_factors_and_fails_loudly_without_a_gpu(nagp_lib):
    A, Q, H, Pinf = ref.matern32_model(2, 3)
    with pytest.raises(ValueError):
        nagp.kernel_ss_sampleFastFB(A, Q, H, Pinf, 2, 0.01, np.zeros(5), 2, Lq=np.eye(3))
    F = nagp.fastfb._lower_factor(np.diag([1.0, -1e-12, 0.25]))                      # not positive definite: clipped eigen-factor
    assert np.allclose(F @ F.T, np.diag([1.0, 0.0, 0.25]), atol=1e-15)
    assert np.array_equal(nagp.fastfb._lower_factor(Pinf), np.linalg.cholesky((Pinf + Pinf.T) / 2))
    if nagp_lib.nagp_device_count() < 1:               # the library's own view: torch may miss a device that libnagp opened first in this process
        with pytest.raises(nagp.NagpError):
            nagp.kernel_ss_sampleFastFB(A, Q, H, Pinf, 2, 0.01, np.zeros(5), 2)


def test_set_up_helper_solves_the_equations_of_the_m_file():
    """The helper no longer makes the oracle's SciPy calls (tests/test_fastfb_host.py holds it to a 60-digit solution, where the
    QZ route is 1e-12 .. 1e-8 away), so it is held to the equations of kernel_ss_kalmanFastFB.m themselves, each residual within
    1e-13 of the matrix it defines (S = 12: a few hundred roundings of 1.1e-16), and to the oracle within the oracle's own error on
    Matern-3/2 models of this size (G 3e-12 .. 3e-10, the rest below 1e-11: the set-up table of tests/test_fastfb_host.py)."""
    A, Q, H, Pinf = ref.matern32_model(3, 5)
    st = offb.steady_state(A, Q, H, 0.02)
    _, _, R, Sinn, Kg, HA, AKHA, PF2, G, Psm = nagp.fastfb._steady_state(A, Q, H, 0.02)
    amax = lambda X: np.max(np.abs(X))
    PP = A @ PF2 @ A.T + Q                                                         # the predictive covariance the DARE solves for
    Sx = float((H @ PP @ H.T)[0, 0]) + R
    res = dict(Sinn=abs(Sinn - Sx) / Sx, Kg=amax(Kg - (PP @ H.T).ravel() / Sx) / amax(Kg), HA=amax(HA - (H @ A).ravel()),
               AKHA=amax(AKHA - (A - np.outer(Kg, HA))) / amax(AKHA), PF2=amax(PF2 - (PP - np.outer(Kg, (H @ PP).ravel()))) / amax(PF2),
               G=amax(G @ PP - PF2 @ A.T) / amax(PF2 @ A.T), Psm=amax(Psm - (G @ Psm @ G.T + PF2 - G @ PP @ G.T)) / amax(Psm))
    print('set-up residuals: ' + '  '.join('%s %.1e' % kv for kv in res.items()))
    assert max(res.values()) < 1e-13, res
    rel = lambda a, b: amax(np.asarray(a) - np.asarray(b)) / amax(b)
    assert rel(G, st['G']) < 1e-9
    for a, b in ((Kg, st['K']), (HA, st['HA']), (AKHA, st['AKHA']), (PF2, st['PF2']), (Psm, st['P'])):
        assert rel(a, b) < 3e-11
    assert R == 0.02 and abs(Sinn - st['S']) < 1e-13


# ---- the restatement: D = 2 Matern-3/2 sub-bands (S = 8), length-scales 5 .. 20 samples, T = 400, no gaps, 2 048 draws
N_DRAWS, SEED, T_PIN, R_PIN = 2048, 1, 400, 0.01


@pytest.fixture(scope='module')
def pinned():
    A, Q, H, Pinf = ref.matern32_model(2, 7, (5.0, 20.0))
    Lq, Lp = ref.factors(Q, Pinf)
    y = ref.simulate_y(A, Lq, Lp, H, R_PIN, T_PIN, 11)
    Y, X, MS = ref.sample(A, Q, H, Pinf, R_PIN, y, N_DRAWS, SEED, Lq, Lp)
    return dict(A=A, Q=Q, H=H, Pinf=Pinf, y=y, Y=Y, X=X, MS=MS)


def test_restatement_smoother_is_the_oracles(pinned):
    p = pinned
    _, MSo, _, _ = offb.kernel_ss_kalmanFastFB(p['A'], p['Q'], p['H'], p['Pinf'], 2, R_PIN, p['y'])
    assert np.array_equal(p['MS'], MSo)
    yg = p['y'].copy(); yg[50:90] = np.nan; yg[397] = np.nan
    st = offb.steady_state(p['A'], p['Q'], p['H'], R_PIN)
    _, MSg, _, _ = offb.kernel_ss_kalmanFastFB(p['A'], p['Q'], p['H'], p['Pinf'], 2, R_PIN, yg)
    assert np.array_equal(ref.smooth(st, p['A'], yg), MSg)
    both = ref.smooth(st, p['A'], np.stack([yg, 2.0 * yg], axis=1))                  # side by side = one by one
    assert np.allclose(both[0], MSg, rtol=0, atol=1e-14 * np.max(np.abs(MSg))) and np.allclose(both[1], 2.0 * MSg, rtol=0, atol=1e-13 * np.max(np.abs(MSg)))
    assert np.array_equal(np.einsum('s,nst->nt', p['H'][0], p['X']), p['Y'])


def test_restatement_mean_over_draws_is_the_smoother_mean(pinned):
    """for every step 100 .. 300 the mean over draws of Ydraw is within 5 sd / sqrt(n) of H S_y(y)"""
    p = pinned; n = N_DRAWS; sl = slice(100, 301)
    mean = p['Y'].mean(axis=0)[sl]; sd = p['Y'].std(axis=0, ddof=1)[sl]
    z = np.abs(mean - (p['H'] @ p['MS'])[0][sl]) / (sd / np.sqrt(n))
    print('largest |mean - H S_y(y)| in units of sd/sqrt(n): %.2f' % z.max())
    assert np.all(z < 5.0)


def test_restatement_variance_over_draws_is_the_smoother_variance(pinned):
    """for every step 100 .. 300 the sample variance of Ydraw is within a factor 1 +- 5 sqrt(2/(n-1)) of H Psm H'"""
    p = pinned; n = N_DRAWS; sl = slice(100, 301)
    Psm = nagp.fastfb._steady_state(p['A'], p['Q'], p['H'], R_PIN)[9]
    hph = float((p['H'] @ Psm @ p['H'].T)[0, 0])
    ratio = p['Y'].var(axis=0, ddof=1)[sl] / hph
    b = 5.0 * np.sqrt(2.0 / (n - 1))
    print('sample variance / H Psm H\': %.4f .. %.4f (bounds %.4f .. %.4f)' % (ratio.min(), ratio.max(), 1 - b, 1 + b))
    assert np.all(ratio > 1 - b) and np.all(ratio < 1 + b)
