"""GPU (-m gpu): nagp_fastfb_sample / nagp.kernel_ss_sampleFastFB -- joint posterior draws of the stationary filterbank -- against
the NumPy restatement of tests/fbsample_ref.py (pinned without a GPU in tests/test_fbsample_host.py), at the tolerance
tests/test_gpu_parity.py uses for the filterbank's Xfin (TOL_MEAN = 1e-7, relative to the largest magnitude of the array).
The generator is counter-based and restated on the host, so every comparison is deterministic."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nagp
import fbsample_ref as ref

pytestmark = pytest.mark.gpu
TOL_MEAN = 1e-7
R = 0.01


def rel(a, b):
    a = np.asarray(a, float); b = np.asarray(b, float)
    assert a.shape == b.shape, (a.shape, b.shape)
    assert not np.any(np.isnan(a)) and not np.any(np.isnan(b))
    return float(np.max(np.abs(a - b)) / (np.max(np.abs(b)) + 1e-300)) if a.size else 0.0


@pytest.fixture(scope='module', autouse=True)
def _lib(nagp_lib):
    assert nagp_lib.nagp_device_count() >= 1
    return nagp_lib


def problem(kernel, D, T, gaps):
    A, Q, H, Pinf = ref.matern32_model(D, D + T, kernel=kernel)
    Lq, Lp = ref.factors(Q, Pinf)
    y = ref.simulate_y(A, Lq, Lp, H, R, T, D + T + 1)
    for a, b in gaps:
        y[a:b] = np.nan
    return dict(A=A, Q=Q, H=H, Pinf=Pinf, Lq=Lq, Lp=Lp, y=y, D=D, T=T)


def gpu(p, n, seed, states=True, y=None):
    return nagp.kernel_ss_sampleFastFB(p['A'], p['Q'], p['H'], p['Pinf'], p['D'], R, p['y'] if y is None else y, n, seed, states, p['Lq'], p['Lp'])


def cpu(p, n, seed, which=None, y=None):
    return ref.sample(p['A'], p['Q'], p['H'], p['Pinf'], R, p['y'] if y is None else y, n, seed, p['Lq'], p['Lp'], which)


@pytest.fixture(scope='module')
def case1():
    T = 300
    return problem('matern32', 2, T, [(40, 75), (T - 3, T - 2)])


@pytest.fixture(scope='module')
def case3():
    T = 2500                     # spans of 132 steps, the last one 124: the second gap crosses a span boundary
    return problem('matern32', 4, T, [(40, 75), (125, 140), (T - 3, T - 2)])


def test_1_short_series_with_gaps_states_returned(case1):
    p = case1
    Y, X, MS = gpu(p, 5, 31)
    Yo, Xo, MSo = cpu(p, 5, 31)
    assert Y.shape == (5, 300) and X.shape == (5, 8, 300) and MS.shape == (8, 300)
    e = (rel(Y, Yo), rel(X, Xo), rel(MS, MSo))
    print('rel diff Ydraw %.2e Xdraw %.2e MS %.2e' % e)
    assert max(e) < TOL_MEAN
    assert rel(Y, np.einsum('s,nst->nt', p['H'][0], X)) < 1e-13                       # Ydraw_i = H Xdraw_i (one fma chain against einsum)
    _, Xfin, _ = nagp.kernel_ss_kalmanFastFB(p['A'], p['Q'], p['H'], p['Pinf'], 2, R, p['y'])
    assert np.array_equal(MS, Xfin[0])                                               # MS = the smoother's means, bit for bit
    Y2, X2, _ = gpu(p, 5, 31, states=False)
    assert X2 is None and np.array_equal(Y2, Y)                                      # without states: the same draws


@pytest.mark.parametrize('T', [1, 2])
def test_2_no_smoothing_step_and_one_smoothing_step(T):
    p = problem('exp', 3, T, [])
    Y, X, MS = gpu(p, 5, 3)
    Yo, Xo, MSo = cpu(p, 5, 3)
    assert X.shape == (5, 6, T)
    assert rel(Y, Yo) < TOL_MEAN and rel(X, Xo) < TOL_MEAN and rel(MS, MSo) < TOL_MEAN


def test_3_parallel_in_time_form_with_a_shorter_last_span(case3, monkeypatch):
    p = case3
    Y, X, MS = gpu(p, 3, 17)
    Yo, Xo, MSo = cpu(p, 3, 17)
    e = (rel(Y, Yo), rel(X, Xo), rel(MS, MSo))
    print('rel diff Ydraw %.2e Xdraw %.2e MS %.2e' % e)
    assert max(e) < TOL_MEAN
    monkeypatch.setenv('NAGP_FB_SEQUENTIAL', '1')                                     # developer switch: one span per draw
    Ys, Xs, _ = gpu(p, 3, 17)
    assert rel(Ys, Yo) < TOL_MEAN and rel(Xs, Xo) < TOL_MEAN and rel(Xs, X) < 1e-10


def test_3_large_batch_runs_one_span_per_draw(case3):
    p = case3; which = [0, 4, 299]
    Y, X, MS = gpu(p, 300, 17)
    Yo, Xo, MSo = cpu(p, 300, 17, which)
    assert Y.shape == (300, 2500) and not np.any(np.isnan(Y)) and not np.any(np.isnan(X))
    e = (rel(Y[which], Yo), rel(X[which], Xo), rel(MS, MSo))
    print('rel diff Ydraw %.2e Xdraw %.2e MS %.2e' % e)
    assert max(e) < TOL_MEAN


def test_4_matrices_in_global_memory():
    p = problem('matern32', 25, 200, [(40, 75), (197, 198)])                          # S = 100 > 96
    Y, X, MS = gpu(p, 2, 5)
    Yo, Xo, MSo = cpu(p, 2, 5)
    assert X.shape == (2, 100, 200)
    assert rel(Y, Yo) < TOL_MEAN and rel(X, Xo) < TOL_MEAN and rel(MS, MSo) < TOL_MEAN


@pytest.mark.parametrize('which_case', ['case1', 'case3'])
def test_5_all_missing_data_returns_the_prior_draw(which_case, request):
    p = request.getfixturevalue(which_case)
    y = np.full(p['T'], np.nan)
    Y, X, MS = gpu(p, 5, 9, y=y)
    xs = ref.prior_draws(p['A'], p['Lq'], p['Lp'], p['T'], 5, 9)
    assert np.array_equal(MS, np.zeros_like(MS))
    e = rel(X, xs)
    print('rel diff of the prior draw %.2e' % e)
    assert e < 1e-12


def test_6_prefix_reproducibility_and_batching(case1, monkeypatch):
    p = case1
    Y2, X2, _ = gpu(p, 2, 31)
    Y5, X5, _ = gpu(p, 5, 31)                                                         # crosses the 4-wide sample block
    assert np.array_equal(Y2, Y5[:2]) and np.array_equal(X2, X5[:2])
    Y5b, X5b, _ = gpu(p, 5, 31)
    assert np.array_equal(Y5, Y5b) and np.array_equal(X5, X5b)
    Y5c, _, _ = gpu(p, 5, 32)
    assert np.min(np.abs(Y5c - Y5).max(axis=1)) > 1e-3
    Y64, X64, _ = gpu(p, 64, 31)
    monkeypatch.setenv('NAGP_FBS_BUDGET_MB', '1')                                     # developer switch: 1 MiB -> several device batches
    Y64b, X64b, _ = gpu(p, 64, 31)
    assert np.array_equal(Y64, Y64b) and np.array_equal(X64, X64b) and np.array_equal(Y64[:5], Y5)


def test_7_mean_over_draws_is_the_smoother_mean(case1):
    """512 draws, one gap: at every step the mean over draws is within 5 sd / sqrt(n) of MS (seed 31: the restatement satisfies the
    bound with largest deviations of 2.4 (signal) and 3.3 (states) sd / sqrt(n))."""
    p = case1; n = 512
    y = p['y'].copy(); y[297] = 0.5 * (y[296] + y[298])                               # one gap: 40:75
    assert np.isnan(y).sum() == 35
    Y, X, MS = gpu(p, n, 31, y=y)
    z = np.abs(Y.mean(axis=0) - (p['H'] @ MS)[0]) / (Y.std(axis=0, ddof=1) / np.sqrt(n))
    zx = np.abs(X.mean(axis=0) - MS) / (X.std(axis=0, ddof=1) / np.sqrt(n))
    print('largest deviation of the mean in units of sd/sqrt(n): signal %.2f, states %.2f' % (z.max(), zx.max()))
    assert np.all(z < 5.0) and np.all(zx < 5.0)
    sd = Y.std(axis=0, ddof=1)
    assert sd[45:70].min() > 3.0 * np.median(sd[100:250])                             # the uncertainty opens up inside the gap


def test_8_sampling_leaves_the_smoother_alone(case3):
    p = case3
    a = nagp.kernel_ss_kalmanFastFB(p['A'], p['Q'], p['H'], p['Pinf'], 4, R, p['y'])
    gpu(p, 6, 1)
    b = nagp.kernel_ss_kalmanFastFB(p['A'], p['Q'], p['H'], p['Pinf'], 4, R, p['y'])
    assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
