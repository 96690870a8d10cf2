"""GPU (-m gpu): nagp_slowfb_run / nagp.kernel_ss_kalmanSlowFB -- the exact filterbank filter and smoother with an observation variance
per step -- against the multi-precision fixture tests/golden/slowfb_multiprecision.npz and the NumPy restatement tests/slowfb_ref.py
(pinned to the fixture without a GPU in tests/test_slowfb_host.py).  Distances are the project's norm max|d| / max|ref| per array.

Against the fixture an output must (1) be within TOL_MEAN = 1e-7, the filterbank tolerance of the project, and (2) be no more than
32 x as far from the fixture as the restatement is (floored at 1e-15: the fixture is stored in float64) -- five bits for another
summation order (MFMA tiles, fma).  Measured figures: profiles/r08_slowfb_parity.txt."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nagp
from nagp import _lib as L
import slowfb_ref as ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL_MEAN = 1e-7
FACTOR, FLOOR = 32.0, 1e-15


@functools.lru_cache(maxsize=None)
def fixture():
    return dict(np.load(os.path.join(ROOT, 'tests', 'golden', 'slowfb_multiprecision.npz')))


def fx(name):
    f = fixture()
    return {k[len(name) + 1:]: v for k, v in f.items() if k.startswith(name + '_')}


@functools.lru_cache(maxsize=None)
def restated(name, KF):
    c = fx(name)
    return ref.slowfb(c['A'], c['Q'], c['H'], c['P0'], c['y'], c['vary'], KF)


def ldist(a, r):
    return abs(a - r) / abs(r)


def check(tag, got, want, restatement):
    """both conditions of the module docstring, figures printed first"""
    e_gpu, e_ref = ref.dist(got, want), ref.dist(restatement, want)
    print('slowfb-parity %-28s gpu %.3e  restatement %.3e  bound %.3e' % (tag, e_gpu, e_ref, FACTOR * max(e_ref, FLOOR)))
    assert e_gpu < TOL_MEAN, (tag, e_gpu)
    assert e_gpu <= FACTOR * max(e_ref, FLOOR), (tag, e_gpu, e_ref)


@pytest.mark.parametrize('name', ['m32', 'm52'])
def test_smoother_against_the_multiprecision_fixture(nagp_lib, name):
    c = fx(name); S = c['A'].shape[0]; st = c['steps']; tau = int(c['tau'])
    rl, rMS, rPS = restated(name, 0)
    rd = np.einsum('iik->ik', rPS)
    lik, MS, Pd, Ps = nagp.slowfb_run(c['A'], c['Q'], c['H'], c['P0'], c['y'], c['vary'], want_diag=True, sub_idx=np.arange(S))
    check(name + ' lik', np.array([lik[0]]), np.array([c['lik']]), np.array([rl]))
    check(name + ' MS', MS[0], c['MS'], rMS)
    check(name + ' Pdiag', Pd[0], c['Pdiag'], rd)
    check(name + ' Psub(all)', Ps[0][:, :, st], c['P'], rPS[:, :, st])
    check(name + ' diag(Psub)', np.einsum('iik->ik', Ps[0]), c['Pdiag'], rd)
    assert np.array_equal(Ps[0], Ps[0].transpose(1, 0, 2))                                  # symmetric to the bit
    cov = np.arange(0, S, 2 * tau)                                                          # the covS selection: [0, 2 tau, ...]
    lik2, MS2, _, Pc = nagp.slowfb_run(c['A'], c['Q'], c['H'], c['P0'], c['y'], c['vary'], sub_idx=cov)
    assert Pc.shape == (1, cov.size, cov.size, c['y'].size)
    check(name + ' Psub(covS)', Pc[0][:, :, st], c['P'][np.ix_(cov, cov)], rPS[np.ix_(cov, cov, st)])
    assert np.array_equal(Pc[0], Pc[0].transpose(1, 0, 2))
    assert np.array_equal(MS2, MS) and lik2[0] == lik[0]


@pytest.mark.parametrize('name', ['m32', 'm52'])
def test_filter_only_against_the_multiprecision_fixture(nagp_lib, name):
    c = fx(name); S = c['A'].shape[0]; st = c['steps']
    rl, rMF, rPF = restated(name, 1)
    lik, MF, Pd, Ps = nagp.slowfb_run(c['A'], c['Q'], c['H'], c['P0'], c['y'], c['vary'], filter_only=True, want_diag=True, sub_idx=np.arange(S))
    check(name + ' KF lik', np.array([lik[0]]), np.array([c['lik']]), np.array([rl]))
    check(name + ' KF MF', MF[0], c['MF'], rMF)
    check(name + ' KF PFdiag', Pd[0], c['PFdiag'], np.einsum('iik->ik', rPF))
    check(name + ' KF PF', Ps[0][:, :, st], c['PF'], rPF[:, :, st])
    assert np.array_equal(Ps[0], Ps[0].transpose(1, 0, 2))


def against_restatement(tag, A, Q, H, P0, y, vary, sub=None):
    S = A.shape[0]; sub = np.arange(S) if sub is None else sub
    rl, rMS, rPS = ref.slowfb(A, Q, H, P0, y, vary)
    lik, MS, Pd, Ps = nagp.slowfb_run(A, Q, H, P0, y, vary, want_diag=True, sub_idx=sub)
    fig = (ldist(lik[0], rl), ref.dist(MS[0], rMS), ref.dist(Pd[0], np.einsum('iik->ik', rPS)), ref.dist(Ps[0], rPS[np.ix_(sub, sub)]))
    print('slowfb-parity %-28s lik %.3e MS %.3e Pdiag %.3e Psub %.3e' % ((tag,) + fig))
    assert np.all(np.isfinite(MS)) and np.all(np.isfinite(Ps)) and np.isfinite(lik[0])
    assert max(fig) < TOL_MEAN, (tag, fig)
    assert np.array_equal(Ps[0], Ps[0].transpose(1, 0, 2))
    return lik, MS, Pd, Ps


@pytest.mark.parametrize('T', [1, 2, 3])
def test_edge_lengths(nagp_lib, T):
    """no backward step, one, two"""
    A, Q, H, P0, _ = ref.model('exp', 1)
    against_restatement('exp D=1 T=%d' % T, A, Q, H, P0, ref.sample_y(A, Q, H, P0, T, 5), np.full(T, 1e-2))


@pytest.mark.parametrize('kernel,D', [('matern32', 32), ('matern52', 5)])
def test_limit_shapes(nagp_lib, kernel, D):
    """S = 128: the largest P the LDS holds, every MFMA tile full; S = 30: partial tiles in both dimensions"""
    A, Q, H, P0, _ = ref.model(kernel, D); T = 48
    y = ref.sample_y(A, Q, H, P0, T, 6); vary = np.full(T, 1e-4)
    y[17] = np.nan; vary[30] = 1e5
    assert A.shape[0] == (128 if D == 32 else 30)
    against_restatement('%s D=%d T=48' % (kernel, D), A, Q, H, P0, y, vary)


def test_batch_of_three_patterns(nagp_lib):
    """each series of a batch is bit-equal to its own single-series call"""
    c = fx('m32'); T = c['y'].size
    y0 = ref.sample_y(c['A'], c['Q'], c['H'], c['P0'], T, 11)
    ys = np.stack([c['y'], y0, y0.copy()]); vs = np.stack([c['vary'], np.full(T, 1e-2), np.full(T, 1e-4)])
    ys[2, 60:90] = np.nan; vs[2, 5:9] = 1e5
    cov = np.array([0, 4])
    bl, bMS, bPd, bPs = nagp.slowfb_run(c['A'], c['Q'], c['H'], c['P0'], ys, vs, want_diag=True, sub_idx=cov)
    for i in range(3):
        l1, MS1, Pd1, Ps1 = nagp.slowfb_run(c['A'], c['Q'], c['H'], c['P0'], ys[i], vs[i], want_diag=True, sub_idx=cov)
        assert l1[0] == bl[i] and np.array_equal(MS1[0], bMS[i]) and np.array_equal(Pd1[0], bPd[i]) and np.array_equal(Ps1[0], bPs[i]), i


def test_batch_of_seventy_copies(nagp_lib):
    """more series than one wave of workgroups per XCD: all bit-equal to the first"""
    c = fx('m32'); n = 70
    ys = np.tile(c['y'], (n, 1)); vs = np.tile(c['vary'], (n, 1))
    bl, bMS, bPd, bPs = nagp.slowfb_run(c['A'], c['Q'], c['H'], c['P0'], ys, vs, want_diag=True, sub_idx=np.array([0, 4]))
    assert np.all(bl == bl[0]) and np.isfinite(bl[0])
    for a in (bMS, bPd, bPs):
        assert np.all(a == a[0:1])


def test_python_mirror(nagp_lib):
    """nagp.kernel_ss_kalmanSlowFB: shapes of the .m, scalar vary, the cov options, a batch"""
    c = fx('m32'); S = 8; T = c['y'].size
    lik, Xfin, Pfin = nagp.kernel_ss_kalmanSlowFB(c['A'], c['Q'], c['H'], c['P0'], 4, c['vary'], c['y'])
    assert Xfin.shape == (1, S, T) and Pfin.shape == (S, S, T)
    assert ldist(lik, c['lik']) < TOL_MEAN and ref.dist(Xfin[0], c['MS']) < TOL_MEAN and ref.dist(Pfin[:, :, c['steps']], c['P']) < TOL_MEAN
    lik_d, X_d, P_d = nagp.kernel_ss_kalmanSlowFB(c['A'], c['Q'], c['H'], c['P0'], 4, c['vary'], c['y'], cov='diag')
    assert P_d.shape == (S, T) and ref.dist(P_d, c['Pdiag']) < TOL_MEAN and np.array_equal(X_d, Xfin)
    lik_n, X_n, P_n = nagp.kernel_ss_kalmanSlowFB(c['A'], c['Q'], c['H'], c['P0'], 4, c['vary'], c['y'], cov=None)
    assert P_n is None and lik_n == lik
    _, _, P_s = nagp.kernel_ss_kalmanSlowFB(c['A'], c['Q'], c['H'], c['P0'], 4, c['vary'], c['y'], cov='sub', sub_idx=[0, 4])
    assert P_s.shape == (2, 2, T)
    y1 = np.nan_to_num(c['y'])
    rl, rMS, _ = ref.slowfb(c['A'], c['Q'], c['H'], c['P0'], y1, 0.01, KF=1)
    lik_k, X_k, P_k = nagp.kernel_ss_kalmanSlowFB(c['A'], c['Q'], c['H'], c['P0'], 4, 0.01, np.stack([y1, y1]), 0, 1, cov='diag')
    assert lik_k.shape == (2,) and X_k.shape == (2, 1, S, T) and P_k.shape == (2, S, T)
    assert ldist(lik_k[1], rl) < TOL_MEAN and ref.dist(X_k[1, 0], rMS) < TOL_MEAN


def test_zero_observation_variance(nagp_lib):
    """vary = 0 on every step is served (s = H P H' > 0)"""
    A, Q, H, P0, _ = ref.model('exp', 1); T = 40
    against_restatement('exp D=1 vary=0', A, Q, H, P0, ref.sample_y(A, Q, H, P0, T, 8), np.zeros(T))


def test_notpd_series_is_reported_and_leaves_its_batch_mates_alone(nagp_lib):
    """s = 0 (P0 = 0, T = 1, vary = 0): NAGP_ENOTPD after the run, lik = NaN for that series only"""
    A, Q, H, P0, _ = ref.model('exp', 1); S = 2
    A = L.f64(A); Q = L.f64(Q); Z = L.f64(np.zeros((S, S))); Hc = L.f64(H, 'C')
    y = L.f64(np.array([[0.7], [0.7]]), 'C'); vary = L.f64(np.array([[0.0], [1e-2]]), 'C')
    lik = np.zeros(2); MS = np.zeros((2, 1, S))
    st = nagp_lib.nagp_slowfb_run(S, 2, L.dptr(A), L.dptr(Q), L.dptr(Hc), L.dptr(Z), 2, L.dptr(y), L.dptr(vary), 1, 0, 0, L.c_ip(),
                                  L.dptr(lik), L.dptr(MS), L.dptr(None), L.dptr(None), 0)
    assert st == -6 and b'innovation variance' in nagp_lib.nagp_last_error()
    assert np.isnan(lik[0]) and np.isfinite(lik[1])
    l1, MS1, _, _ = nagp.slowfb_run(A, Q, H, Z, y[1], vary[1])
    assert l1[0] == lik[1] and np.array_equal(MS1[0].ravel(), MS[1].ravel())
