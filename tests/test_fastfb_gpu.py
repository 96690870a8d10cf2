"""GPU (-m gpu): nagp_fastfb_run (kernel_ss_kalmanFastFB: the stationary filterbank's filter and steady-state smoother) against the
60-digit fixture tests/golden/fastfb_multiprecision.npz and the float64 restatements of tests/fastfb_ref.py (pinned to the fixture
without a GPU in tests/test_fastfb_host.py).  Distances are the project's norm max|d| / max|ref| per array.

Fixture cases: the kernel gets the fixture's float64 set-up through the C ABI, so the fixture pins the kernel alone.  An output must
(1) be within 1e-10 of the fixture and (2) be no more than 32 x as far from it as the matching restatement is (floored at 1e-15: the
fixture is stored in float64) -- five bits for another summation order, the factor of tests/test_slowfb_gpu.py.  The matching
restatement is span_form where spans run (T >= 2048 and the compose work set fits the LDS: S <= 69) and sequential otherwise.
Every other case: the matching restatement in float64 is the reference, distance < 1e-12 (the restatements are 5e-16 .. 5e-15 from
the fixture, tests/test_fastfb_host.py).  Measured figures: profiles/r14_fastfb_parity.txt."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nagp
from nagp import _lib as L
from nagp import fastfb as pfb
import fastfb_ref as ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL_FIXTURE, TOL_RESTATED = 1e-10, 1e-12
FACTOR, FLOOR = 32.0, 1e-15


@pytest.fixture(scope='module', autouse=True)
def _lib(nagp_lib):
    assert nagp_lib.nagp_device_count() >= 1
    return nagp_lib


@functools.lru_cache(maxsize=None)
def fixture():
    return dict(np.load(os.path.join(ROOT, 'tests', 'golden', 'fastfb_multiprecision.npz')))


@functools.lru_cache(maxsize=None)
def case(name):
    return ref.fixture_case(fixture(), name)


@functools.lru_cache(maxsize=None)
def restated(name, KF, form):
    c = case(name)
    return (ref.span_form if form == 'span' else ref.sequential)(c, c['y'], KF)


def run(setup, y, KF=0):
    """nagp_fastfb_run through ctypes with the caller's matrices: MS (S x T) and sum_v2"""
    A = L.f64(setup['A']); B = L.f64(setup['AKHA']); G = None if KF == 1 else L.f64(setup['G'])
    ha = L.f64(np.ravel(setup['HA']), 'C'); kg = L.f64(np.ravel(setup['Kg']), 'C')
    S = A.shape[0]; y = L.f64(np.ravel(y), 'C'); T = y.size
    assert A.shape == B.shape == (S, S) and ha.size == kg.size == S and (G is None or G.shape == (S, S))
    MS = np.full((S, T), np.nan, order='F'); sv2 = C.c_double(np.nan)
    L.check(L.lib().nagp_fastfb_run(S, L.dptr(A), L.dptr(B), L.dptr(ha), L.dptr(kg), L.dptr(G), L.dptr(y), T, L.dptr(MS), C.byref(sv2), 0))
    return MS, sv2.value


def sdist(a, r):
    return abs(a - r) / abs(r)


def check_fixture(tag, got, want, restatement):
    """both conditions of the module docstring, figures printed first"""
    e_gpu, e_ref = ref.dist(got, want), ref.dist(restatement, want)
    print('fastfb-parity %-34s gpu %.3e  restatement %.3e  bound %.3e' % (tag, e_gpu, e_ref, FACTOR * max(e_ref, FLOOR)))
    assert e_gpu < TOL_FIXTURE, (tag, e_gpu)
    assert e_gpu <= FACTOR * max(e_ref, FLOOR), (tag, e_gpu, e_ref)


def fixture_checks(tag, name, KF, form):
    c = case(name); st = c['steps']; T = c['y'].size
    rMS, rsv = restated(name, KF, form)
    MS, sv = run(c, c['y'], KF)
    assert np.all(np.isfinite(MS)) and np.isfinite(sv)
    one = lambda v: np.array([v], float)
    check_fixture(tag + (' MF' if KF else ' MS'), MS[:, st], c['MF' if KF else 'MS'], rMS[:, st])
    check_fixture(tag + ' sum_v2', one(sv), one(c['sum_v2']), one(rsv))
    check_fixture(tag + ' lik', one(ref.lik(float(c['Sinn']), T, sv)), one(c['lik']), one(ref.lik(float(c['Sinn']), T, rsv)))
    return MS, sv


def against_restatement(tag, setup, y, KF, form):
    rMS, rsv = (ref.span_form if form == 'span' else ref.sequential)(setup, y, KF)
    MS, sv = run(setup, y, KF)
    fig = (ref.dist(MS, rMS), sdist(sv, rsv))
    print('fastfb-parity %-34s vs %-10s MS %.3e  sum_v2 %.3e' % (tag, form + ':', fig[0], fig[1]))
    assert np.all(np.isfinite(MS)) and np.isfinite(sv)
    assert max(fig) < TOL_RESTATED, (tag, fig)
    return MS, sv


def form_of(T, S):
    return 'span' if ref.spans(T, S)[0] > 1 else 'sequential'


@pytest.mark.parametrize('KF', [0, 1])
@pytest.mark.parametrize('name', ['m32', 'm52', 'span', 'span_wide'])
def test_fixture_cases(name, KF):
    """smoother and filter-only; filter-only on span / span_wide is the G == NULL path with more than one span"""
    c = case(name); S = c['A'].shape[0]; T = c['y'].size
    ns = ref.spans(T, S)[0]
    assert ns == {'m32': 1, 'm52': 1, 'span': 18, 'span_wide': 16}[name]
    fixture_checks('%s KF=%d' % (name, KF), name, KF, form_of(T, S))


@pytest.mark.parametrize('name', ['span', 'span_wide'])
def test_fixture_span_cases_in_one_span(name, monkeypatch):
    """the developer switch NAGP_FB_SEQUENTIAL: the same series as one span, against the sequential restatement"""
    monkeypatch.setenv('NAGP_FB_SEQUENTIAL', '1')
    MS1, sv1 = fixture_checks('%s one span' % name, name, 0, 'sequential')
    monkeypatch.delenv('NAGP_FB_SEQUENTIAL')
    c = case(name)
    MS, sv = run(c, c['y'], 0)
    assert ref.dist(MS, MS1) < TOL_RESTATED and sdist(sv, sv1) < TOL_RESTATED


def test_two_identical_calls_are_bit_equal():
    c = case('span')
    for KF in (0, 1):
        a, sa = run(c, c['y'], KF); b, sb = run(c, c['y'], KF)
        assert np.array_equal(a, b) and sa == sb


def raw_problem(S, T, seed):
    """Not a filterbank: a random stable A (0.95 x orthogonal), AKHA = A - K HA with |K||HA| = 0.03, a contractive G (0.95 x orthogonal)
    and a random series with NaN at both ends, across the first span boundary and at T-2."""
    rng = np.random.default_rng(seed)
    orth = lambda: np.linalg.qr(rng.normal(size=(S, S)))[0]
    A = 0.95 * orth(); G = 0.95 * orth()
    kg = rng.normal(size=S); kg *= 0.3 / np.linalg.norm(kg)
    ha = rng.normal(size=S); ha *= 0.1 / np.linalg.norm(ha)
    y = rng.normal(size=T)
    Lspan = ref.spans(T, S)[1]
    y[0] = np.nan; y[T - 1] = np.nan; y[T - 2] = np.nan; y[min(Lspan, T) - 2:min(Lspan, T - 3) + 1] = np.nan
    return dict(A=A, AKHA=A - np.outer(kg, ha), HA=ha, Kg=kg, G=G), y


@pytest.mark.parametrize('S', [1, 3, 5, 62, 69, 70])
def test_raw_abi_shapes_around_the_span_limits(S, monkeypatch):
    """S = 1, 3, 5: the j < S tails, padded tile rows, the column tile of c_j alone or shared; S = 62: 16 x 16 tiles, one for every
    thread of the compose kernel's block (the tile loop takes a second trip from S = 64 on: 16 x 17 -- the fixture's span_wide);
    S = 69: 18 x 18 tiles, the second trip partly filled, and the largest compose work set the LDS holds; S = 70: one span."""
    T = 2305
    assert (ref.compose_lds_doubles(69) * 8 <= ref.LDS_BYTES) and (ref.compose_lds_doubles(70) * 8 > ref.LDS_BYTES)
    assert ref.spans(T, S) == ((18, 129, 18) if S <= 69 else (1, T, 1))
    tiles = lambda s: ((s + 3) // 4) * ((s + 4) // 4)                # RT * CT of fastfb_compose_kernel
    assert tiles(62) == tiles(63) == 256 < tiles(64) == 272 and tiles(69) == 324
    setup, y = raw_problem(S, T, 40 + S)
    MS, sv = against_restatement('raw S=%d T=%d' % (S, T), setup, y, 0, form_of(T, S))
    MF, svf = against_restatement('raw S=%d T=%d KF=1' % (S, T), setup, y, 1, form_of(T, S))
    assert svf == sv
    monkeypatch.setenv('NAGP_FB_SEQUENTIAL', '1')
    MS1, sv1 = against_restatement('raw S=%d T=%d one span' % (S, T), setup, y, 0, 'sequential')
    if S == 70:
        assert np.array_equal(MS1, MS) and sv1 == sv                 # already one span: the switch changes nothing
    elif S >= 62:
        assert not np.array_equal(MS1, MS)                           # spans ran: boundary values come from composed matrices


def exp_problem(D, T):
    lam, var, om = ref.recipe('exp', D, D + T)
    A, Q, H, Pinf, K, tau1 = nagp.get_disc_model(lam, var, om, D, 'exp', 6)
    y = ref.simulate_y(A, Q, H, Pinf, T, D + T + 1)
    return A, Q, H, Pinf, K, y


@pytest.mark.parametrize('D,T', [(1, 2047), (1, 2048), (1, 16513), (3, 16513), (1, 65536), (1, 66000)])
def test_series_lengths_around_the_span_rules(D, T):
    """T = 2047 / 2048: the threshold; 16513: 129 spans, the last of one step and missing, 128 smoother spans; 65536 / 66000: the cap
    of 512 spans with and without a shorter last span.  NaN in the last span and at T-2."""
    A, Q, H, Pinf, K, y = exp_problem(D, T); S = 2 * D
    ns, Lspan, nss = ref.spans(T, S)
    assert (ns, Lspan, nss) == {2047: (1, 2047, 1), 2048: (16, 128, 16), 16513: (129, 129, 128), 65536: (512, 128, 512),
                                66000: (512, 129, 512)}[T]
    y[T - 2] = np.nan
    y[T - 1 if T == 16513 else (ns - 1) * Lspan + 1] = np.nan
    As, Hs, R, Sinn, Kg, HA, AKHA, PF2, G, Psm = pfb._steady_state(A, Q, H, ref.VARY, 0)
    setup = dict(A=As, AKHA=AKHA, HA=HA, Kg=Kg, G=G)
    against_restatement('exp S=%d T=%d' % (S, T), setup, y, 0, form_of(T, S))
    against_restatement('exp S=%d T=%d KF=1' % (S, T), setup, y, 1, form_of(T, S))


def test_a_thread_per_state_through_the_python_mirror():
    """S = 256 (exp, D = 128): every thread of the block holds a state; matrices read from global memory"""
    D, T = 128, 40
    A, Q, H, Pinf, K, y = exp_problem(D, T)
    y[10:14] = np.nan; y[T - 2] = np.nan
    assert A.shape[0] == 256
    As, Hs, R, Sinn, Kg, HA, AKHA, PF2, G, Psm = pfb._steady_state(A, Q, H, ref.VARY, 0)
    setup = dict(A=As, AKHA=AKHA, HA=HA, Kg=Kg, G=G)
    for KF in (0, 1):
        rMS, rsv = ref.sequential(setup, y, KF)
        lik, Xfin, (Ps, Pf) = nagp.kernel_ss_kalmanFastFB(A, Q, H, Pinf, K, ref.VARY, y, 0, KF, steady=True)
        fig = (ref.dist(Xfin[0], rMS), sdist(lik, ref.lik(Sinn, T, rsv)))
        print('fastfb-parity %-34s vs sequential: MS %.3e  lik %.3e' % ('exp S=256 T=40 KF=%d' % KF, fig[0], fig[1]))
        assert Xfin.shape == (1, 256, T) and max(fig) < TOL_RESTATED
        assert np.array_equal(Pf, PF2) and ((Ps is None) if KF else np.array_equal(Ps, Psm))
