"""The stationary filterbank (kernel_ss_kalmanFastFB) without a GPU, against the 60-digit fixture
tests/golden/fastfb_multiprecision.npz (tools/make_fastfb_fixture.py):

  the yardsticks  both float64 restatements of tests/fastfb_ref.py (sequential, span_form) and its mirror of the span arithmetic;
  the set-up      nagp.fastfb._steady_state (DARE, gains, steady-state covariances) per quantity.  PF2 and Psm must be within 1e-10,
                  the figure tests/test_gpu_parity.py states for Pfin; and the smoothed means the product's set-up gives must be no
                  more than 32 x as far from the fixture as those the fixture's own set-up gives (floor 1e-12: G enters the means
                  through cond(PP)).  The oracle's SciPy set-up (the statement of the reference's `dare`) is printed beside it.

Distances are the project's norm max|d| / max|ref| per array."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nagp
from nagp import fastfb as pfb
from oracle import fastfb as offb
import fastfb_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUNS = ('m32', 'm52', 'span', 'span_wide')
SETUPS = ('m32', 'm52', 'm52d5', 'm52d10', 'exp3')
# A contractive recursion forgets rounding errors at its own rate: each step adds about S eps |m| and the sum over the 1/(1 - rho)
# steps of its memory (rho about 0.99 for these filters, S <= 64) stays below 1e-12; measured 5e-16 .. 3e-15 (lik of m32 4e-14).
TOL_RESTATED = 1e-12
TOL_PFIN = 1e-10
FACTOR, FLOOR_MEANS = 32.0, 1e-12


@pytest.fixture(scope='module')
def fx():
    return dict(np.load(os.path.join(ROOT, 'tests', 'golden', 'fastfb_multiprecision.npz')))


def sdist(a, r):
    return abs(a - r) / abs(r)


def test_fixture_inputs_and_patterns(fx):
    assert int(fx['dps']) == 60
    for name in SETUPS + ('wide',):
        m = ref.fixture_model(fx, name); S = m['A'].shape[0]
        assert S == {'m32': 8, 'm52': 18, 'm52d5': 30, 'm52d10': 60, 'exp3': 6, 'wide': 64}[name]
        assert np.array_equal(m['Q'], m['Q'].T) and float(m['vary']) == ref.VARY and m['H'].shape == (1, S)
        A, Q, H, Pinf, K, tau1 = nagp.get_disc_model(m['lamx'], m['varx'], m['omega'], int(m['D']), str(m['kernel']), 6)
        assert ref.dist(A, m['A']) < 1e-13 and ref.dist((Q + Q.T) / 2, m['Q']) < 1e-12 and np.array_equal(H, m['H'])
        assert np.array_equal(m['HA'], (m['H'] @ m['A']).ravel())                 # one non-zero per column of A's rows: exact in float64
        for k in ('AKHA', 'G') + (() if name == 'wide' else ('PP', 'PF2', 'Psm')):
            assert m[k].shape == (S, S)
    for name, T, n_nan in (('m32', 300, 37), ('m52', 300, 37), ('span', 2305, 2 + 5 + 129), ('span_wide', 2100, 3)):
        c = ref.fixture_case(fx, name); y = c['y']
        assert y.size == T and np.isnan(y).sum() == n_nan and c['MS'].shape == c['MF'].shape == (c['A'].shape[0], c['steps'].size)
        assert np.array_equal(c['MS'][:, -1], c['MF'][:, -1]) and c['steps'][-1] == T - 1 and c['steps'][0] == 0
    y = ref.fixture_case(fx, 'span')['y']; L = 129
    assert np.isnan(y[[0, 2304]]).all() and np.isnan(y[L - 2:L + 3]).all() and np.isnan(y[3 * L:4 * L]).all() and not np.isnan(y[4 * L])


@pytest.mark.parametrize('name', RUNS)
def test_restatements_match_the_multiprecision_fixture(fx, name):
    """e_ref per output: what the GPU tests measure the kernels against"""
    c = ref.fixture_case(fx, name); st = c['steps']; T = c['y'].size; Sinn = float(c['Sinn'])
    for form in (ref.sequential, ref.span_form):
        MS, sv = form(c, c['y'], 0)
        MF, svf = form(c, c['y'], 1)
        e = dict(MS=ref.dist(MS[:, st], c['MS']), MF=ref.dist(MF[:, st], c['MF']), sum_v2=sdist(sv, float(c['sum_v2'])),
                 lik=sdist(ref.lik(Sinn, T, sv), float(c['lik'])))
        print('e_ref %-9s %-10s ' % (name, form.__name__) + '  '.join('%s %.2e' % kv for kv in e.items()))
        assert svf == sv and max(e.values()) < TOL_RESTATED, (form.__name__, e)
    if ref.spans(T, c['A'].shape[0])[0] == 1:
        assert np.array_equal(ref.span_form(c, c['y'], 0)[0], ref.sequential(c, c['y'], 0)[0])


def test_span_arithmetic():
    """the mirror of nagp_fastfb_run's span rules at every length the GPU tests use"""
    expect = {300: (1, 300, 1), 40: (1, 40, 1), 2047: (1, 2047, 1), 2048: (16, 128, 16), 2100: (16, 132, 16), 2305: (18, 129, 18),
              16513: (129, 129, 128), 65536: (512, 128, 512), 66000: (512, 129, 512)}
    for T, want in expect.items():
        ns, L, nss = ref.spans(T, 2)
        assert (ns, L, nss) == want, T
        assert (ns - 1) * L < T <= ns * L and ns <= ref.SPAN_CAP and (nss - 1) * L < T - 1 <= nss * L and nss <= ns
    ns, L, nss = ref.spans(16513, 6)
    assert 16513 - (ns - 1) * L == 1 and nss == ns - 1                              # a last filter span of one step, one smoother span fewer
    assert ref.spans(65536, 2)[0] == ref.spans(66000, 2)[0] == ref.SPAN_CAP and 66000 // ref.SPAN_STEPS > ref.SPAN_CAP
    assert ref.spans(1, 2) == (1, 1, 0)
    # the compose work set decides whether spans run: 2 S^2 + 2 (S+4)^2 + 3 S + 8 doubles in 160 KiB
    assert ref.compose_lds_doubles(69) * 8 == 163160 <= ref.LDS_BYTES < ref.compose_lds_doubles(70) * 8 == 167760
    for S in (1, 3, 5, 62, 64, 69):
        assert ref.spans(2305, S) == (18, 129, 18), S
    for S in (70, 96, 256):
        assert ref.spans(2305, S) == (1, 2305, 1), S
    assert ref.spans(2305, 8, sequential=True) == (1, 2305, 1)


def product_setup(m, KF=0):
    A, H, R, Sinn, Kg, HA, AKHA, PF2, G, Psm = pfb._steady_state(m['A'], m['Q'], m['H'], float(m['vary']), KF)
    return dict(A=A, Sinn=Sinn, Kg=Kg, HA=HA, AKHA=AKHA, PF2=PF2, G=G, Psm=Psm)


def oracle_setup(m):
    st = offb.steady_state(m['A'], m['Q'], m['H'], float(m['vary']))
    return dict(PP=st['PP'], Sinn=st['S'], Kg=st['K'], HA=st['HA'], AKHA=st['AKHA'], PF2=st['PF2'], G=st['G'], Psm=st['P'])


@pytest.mark.parametrize('name', SETUPS)
def test_set_up_against_the_multiprecision_fixture(fx, name):
    m = ref.fixture_model(fx, name)
    p, o = product_setup(m), oracle_setup(m)
    keys = ('Sinn', 'Kg', 'HA', 'AKHA', 'PF2', 'G', 'Psm')
    for who, s in (('product', p), ('oracle', o)):
        print('set-up %-7s S = %2d  %-8s ' % (name, m['A'].shape[0], who) + '  '.join('%s %.1e' % (k, ref.dist(s[k], m[k])) for k in keys if k in s)
              + ('  PP %.1e' % ref.dist(s['PP'], m['PP']) if 'PP' in s else ''))
    assert ref.dist(p['PF2'], m['PF2']) <= TOL_PFIN and ref.dist(p['Psm'], m['Psm']) <= TOL_PFIN
    assert np.array_equal(p['PF2'], p['PF2'].T) and np.array_equal(p['Psm'], p['Psm'].T)
    f1 = product_setup(m, KF=1)
    assert f1['G'] is None and f1['Psm'] is None and np.array_equal(f1['PF2'], p['PF2']) and np.array_equal(f1['AKHA'], p['AKHA'])


@pytest.mark.parametrize('name', RUNS)
def test_smoothed_means_on_the_products_set_up(fx, name):
    c = ref.fixture_case(fx, name); st = c['steps']
    own = ref.dist(ref.sequential(c, c['y'], 0)[0][:, st], c['MS'])
    p = product_setup(c); o = oracle_setup(c)
    e_p = ref.dist(ref.sequential(p, c['y'], 0)[0][:, st], c['MS'])
    e_o = ref.dist(ref.sequential(dict(o, A=c['A']), c['y'], 0)[0][:, st], c['MS'])
    bound = max(FACTOR * own, FLOOR_MEANS)
    print('set-up -> MS %-9s fixture\'s set-up %.2e  product\'s %.2e  oracle\'s %.2e  bound %.2e' % (name, own, e_p, e_o, bound))
    assert e_p <= bound, (name, e_p, own)


def test_zero_observation_variance_set_up_solves_the_equations(fx):
    """vary = 0 is what kernel_ss_probFB passes; the doubling iteration has no starting value there (H'H / vary) and the DARE goes to
    SciPy's QZ solver.  No fixture: the set-up is held to the equations of the .m, each residual within 1e-12 of its matrix
    (S = 6, conditioning 1e3: SciPy's DARE is 1e-14 from the 60-digit solution on this model at vary = 0.01)."""
    m = ref.fixture_model(fx, 'exp3'); A, Q, H = m['A'], m['Q'], m['H']
    _, _, R, Sinn, Kg, HA, AKHA, PF2, G, Psm = pfb._steady_state(A, Q, H, 0.0)
    amax = lambda X: np.max(np.abs(X))
    PP = A @ PF2 @ A.T + Q
    res = dict(Sinn=abs(Sinn - (H @ PP @ H.T)[0, 0]) / Sinn, Kg=amax(Kg - (PP @ H.T).ravel() / Sinn) / amax(Kg),
               PF2=amax(PF2 - (PP - np.outer(Kg, (H @ PP).ravel()))) / amax(PF2), HPF2=amax(H @ PF2) / amax(PF2),
               AKHA=amax(AKHA - (A - np.outer(Kg, HA))) / amax(AKHA), G=amax(G @ PP - PF2 @ A.T) / amax(PF2 @ A.T),
               Psm=amax(Psm - (G @ Psm @ G.T + PF2 - G @ PP @ G.T)) / amax(Psm))
    print('set-up residuals at vary = 0: ' + '  '.join('%s %.1e' % kv for kv in res.items()))
    assert R == 0.0 and np.all(np.isfinite(Psm)) and max(res.values()) < 1e-12, res


def test_unstable_dare_is_reported():
    """no stabilising solution: an unobserved unstable mode (the doubling iteration diverges)"""
    A = np.diag([1.5, 0.5]); Q = np.eye(2); H = np.array([[0.0, 1.0]])
    with pytest.raises(nagp.NagpError, match='Unstable DARE solution!'):
        pfb._steady_state(A, Q, H, 0.01)
