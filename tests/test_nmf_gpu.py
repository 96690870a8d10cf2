"""GPU (-m gpu): nagp_nmf_fp / nagp.nmf_run -- the fixed-point NMF of experiments/nmf/nmf_fp.m and nmf_inf_fp.m -- and the host mirrors
on the device path, against the multi-precision fixture tests/golden/nmf_multiprecision.npz and the NumPy restatement tests/nmf_ref.py
(pinned to the fixture without a GPU in tests/test_nmf_host.py).  Distances are the project's norm max|d| / max|ref| per array.

Against the fixture an output must (1) be within TOL = 1e-7 and (2) be no more than 32 x as far from the fixture as the float64
restatement is (floored at 1e-15: the fixture is stored in float64), the rule of tests/test_slowfb_gpu.py.  Where the restatement
with every sum over t formed in the opposite order is itself further than 32 x the forward one's distance, the order of the T-term sums
is what the distance measures, and the bound of that array is 32 x the larger of the two restatement distances -- never a figure
taken from the device.  Every measured triple (device, forward, reverse) is printed, and a run of the whole module writes them to
profiles/r09_nmf_parity.txt."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nagp
from nagp import _lib as L
import nmf_ref as ref
import slowfb_ref as sref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-7
FACTOR, FLOOR = 32.0, 1e-15
CASES = sorted(ref.CASES)
LINES = []
N_LINES = 6 * (3 + 2) + 3      # every case with update_w = 1 (W, H, Obj) and 0 (H, Obj), and the nmf_fp composite


@functools.lru_cache(maxsize=None)
def fixture():
    return dict(np.load(os.path.join(ROOT, 'tests', 'golden', 'nmf_multiprecision.npz')))


@functools.lru_cache(maxsize=None)
def restated(name, update_w, reverse):
    c = ref.case(name)
    return ref.iterate(c['A'], c['vary'], c['W0'], c['H0'], c['its'], update_w=bool(update_w), reverse=reverse)


def check(tag, got, want, fwd, rev):
    """both conditions of the module docstring, figures printed first"""
    e_gpu, e_f, e_r = ref.dist(got, want), ref.dist(fwd, want), ref.dist(rev, want)
    bound = FACTOR * max(e_f, FLOOR)
    if e_r > bound:                                  # the reverse-order restatement is itself outside: the order of the sums decides
        bound = FACTOR * max(e_f, e_r)
    line = 'nmf-parity %-22s device %.3e  forward %.3e  reverse %.3e  bound %.3e' % (tag, e_gpu, e_f, e_r, bound)
    print(line); LINES.append(line)
    assert e_gpu < TOL, (tag, e_gpu)
    assert e_gpu <= bound, (tag, e_gpu, e_f, e_r)


@pytest.fixture(scope='module', autouse=True)
def parity_file():
    yield
    if len(LINES) != N_LINES:                        # a partial run (-k) leaves the file alone
        return
    try:
        with open(os.path.join(ROOT, 'profiles', 'r09_nmf_parity.txt'), 'w') as fh:
            fh.write('# tests/test_nmf_gpu.py: distance to tests/golden/nmf_multiprecision.npz, max|d| / max|ref| per array:\n'
                     '# the device, the float64 restatement, the restatement with the sums over t reversed, and the bound that held\n')
            fh.write('\n'.join(LINES) + '\n')
    except OSError:                                  # a read-only checkout: the figures are in the test output
        pass


@pytest.mark.parametrize('update_w', [1, 0])
@pytest.mark.parametrize('name', CASES)
def test_against_the_multiprecision_fixture(nagp_lib, name, update_w):
    f = fixture(); c = ref.case(name); sfx = '_w%d' % update_w
    W, H, Obj = nagp.nmf_run(c['A'], c['vary'], c['W0'], c['H0'], c['its'], update_w=bool(update_w))
    fw, rv = restated(name, update_w, False), restated(name, update_w, True)
    tag = '%s update_w=%d ' % (name, update_w)
    check(tag + 'H', H, f[name + '_H' + sfx], fw[1], rv[1])
    check(tag + 'Obj', Obj, f[name + '_Obj' + sfx], fw[2], rv[2])
    if update_w:
        check(tag + 'W', W, f[name + '_W' + sfx], fw[0], rv[0])
        s = W.sum(axis=1)
        assert np.all(np.abs(s - 1.0) <= 4 * np.finfo(float).eps), s          # rows of W sum to 1 within 4 ulp
    else:
        assert np.array_equal(W, c['W0'])
    W2, H2, Obj2 = nagp.nmf_run(c['A'], c['vary'], c['W0'], c['H0'], c['its'], update_w=bool(update_w))
    assert np.array_equal(W, W2) and np.array_equal(H, H2) and np.array_equal(Obj, Obj2)      # the same call twice: equal bits


def five_problems(c):
    rng = np.random.default_rng(77)
    T, K = c['H0'].shape
    W0 = np.stack([c['W0']] + [ref.normalise(c['A'][rng.integers(0, T, K)] + 1e-6) for _ in range(4)])
    H0 = np.stack([c['H0']] + [np.exp(rng.standard_normal((T, K))) for _ in range(4)])
    return W0, H0


@pytest.mark.parametrize('update_w', [True, False])
@pytest.mark.parametrize('name', ['a', 'c'])
def test_a_problem_does_not_depend_on_its_batch_mates(nagp_lib, name, update_w):
    """problem p of a 5-problem call equals the same problem run alone, bit for bit"""
    c = ref.case(name)
    W0, H0 = five_problems(c)
    Wb, Hb, Ob = nagp.nmf_run(c['A'], c['vary'], W0, H0, c['its'], update_w=update_w)
    assert Wb.shape == W0.shape and Hb.shape == H0.shape and Ob.shape == (5, (2 if update_w else 1) * c['its'])
    for p in range(5):
        W1, H1, O1 = nagp.nmf_run(c['A'], c['vary'], W0[p], H0[p], c['its'], update_w=update_w)
        assert np.array_equal(W1, Wb[p]) and np.array_equal(H1, Hb[p]) and np.array_equal(O1, Ob[p]), p


def test_device_batches_are_bit_equal_to_one_batch(nagp_lib, monkeypatch):
    """NAGP_NMF_BUDGET_MB=1: case c with 3 iterations takes 8 (T K + K D + 4 (2 K D + 2) + 6) = 37 008 B per problem and
    2 x 136 000 + 4096 B per call, so 1 048 576 - 276 096 = 772 480 B hold 20 problems: 40 problems run as two device batches."""
    c = ref.case('c')
    W0, H0 = five_problems(c)
    W0 = np.tile(W0, (8, 1, 1)); H0 = np.tile(H0, (8, 1, 1))
    full = nagp.nmf_run(c['A'], c['vary'], W0, H0, 3)
    monkeypatch.setenv('NAGP_NMF_BUDGET_MB', '1')
    cut = nagp.nmf_run(c['A'], c['vary'], W0, H0, 3)
    for a, b in zip(full, cut):
        assert np.array_equal(a, b)
    for p in range(5, 40):
        assert np.array_equal(full[1][p], full[1][p % 5])


def test_no_iterations_returns_the_inputs(nagp_lib):
    c = ref.case('a')
    W, H, Obj = nagp.nmf_run(c['A'], c['vary'], c['W0'], c['H0'], 0)
    assert np.array_equal(W, c['W0']) and np.array_equal(H, c['H0']) and Obj.size == 0


def test_nmf_fp_with_given_restart_candidates(nagp_lib):
    """restarts = 4 with `inits`: the device picks the candidate the restatement picks, and the final W, H follow the rule above"""
    c = ref.case('a'); T, K = c['H0'].shape
    rng = np.random.default_rng(31)
    inits = [(c['A'][rng.integers(0, T, K)] + 1e-6, np.exp(rng.standard_normal((T, K)))) for _ in range(3)]
    cands = [(c['W0'], c['H0'])] + inits
    best, _, _, last = ref.select_restart(c['A'], c['vary'], cands)
    margin = np.sort(last)[1] - np.sort(last)[0]
    assert margin > 1e-9 * abs(last[best]), 'the candidates of this test must not tie'
    W, H, info = nagp.nmf_fp(c['A'], c['W0'], c['H0'], c['vary'], {'restarts': 4, 'numIts': 5}, inits=inits)
    assert info['restart'] == best and info['Obj'].size == 10
    assert ref.dist(info['restartObj'], last) < TOL
    rW, rH, rObj = ref.nmf_fp(c['A'], c['W0'], c['H0'], c['vary'], 5, cands=cands)
    rvW, rvH, rvObj = ref.nmf_fp(c['A'], c['W0'], c['H0'], c['vary'], 5, cands=cands, reverse=True)
    # no fixture of this composite: the restatement in long double stands for it (its distance to float64 is the e_ref of the rule)
    lW, lH, lObj = ref.nmf_fp(c['A'], c['W0'], c['H0'], c['vary'], 5, cands=cands, dtype=np.longdouble)
    check('nmf_fp restarts=4 W', W, lW, rW, rvW)
    check('nmf_fp restarts=4 H', H, lH, rH, rvH)
    check('nmf_fp restarts=4 Obj', info['Obj'], lObj, rObj, rvObj)


def test_nmf_inf_fp_is_the_batched_call(nagp_lib):
    c = ref.case('c')
    H, info = nagp.nmf_inf_fp(c['A'], c['W0'], c['H0'], c['vary'], {'numIts': 4})
    from nagp import nmf as nm
    W1, H1, O1 = nagp.nmf_run(c['A'], c['vary'], nm.inf_normalise(c['W0']), c['H0'], 4, update_w=False)
    assert np.array_equal(H, H1) and np.array_equal(info['Obj'], O1)
    assert nagp.nmf_inf_fp(c['A'], c['W0'], c['H0'], c['vary'], {'numIts': 0})[1]['Obj'].size == 0


@pytest.mark.parametrize('slow', [0, 1])
def test_kernel_ss_probFB_on_m32(nagp_lib, slow):
    """Z pairs the rows of the existing smoother's Xfin bit for bit, covS is the selected rows and columns of Pfin, and nmf_init on
    those sub-bands returns its components ordered by fastness"""
    c = sref.case('m32'); tau = int(c['tau']); S = 8
    y = np.nan_to_num(c['y']) if slow == 0 else c['y']
    vary = 1e-2 if slow == 0 else c['vary']
    args = (c['A'], c['Q'], c['H'], c['P0'], 2, vary)
    if slow:
        _, Xfin, Pfin = nagp.kernel_ss_kalmanSlowFB(*args, y)
    else:
        _, Xfin, Pfin = nagp.kernel_ss_kalmanFastFB(*args, y)
    re, im = np.arange(0, S, 2 * tau), np.arange(1, S, 2 * tau)
    Z, = nagp.kernel_ss_probFB(y, *args, tau, 0, 0, slow)
    assert Z.shape == (2, 120) and np.array_equal(Z, Xfin[0][re] + 1j * Xfin[0][im])
    Z2, covS = nagp.kernel_ss_probFB(y, *args, tau, 0, 0, slow, nout=2)
    sel = np.concatenate([re, im])
    assert np.array_equal(Z2, Z) and covS.shape == (4, 4, 120) and np.array_equal(covS, Pfin[np.ix_(sel, sel)])
    Z4, covS4, Zfull, covfull = nagp.kernel_ss_probFB(y, *args, tau, 0, 0, slow, nout=4)
    fsel = np.concatenate([np.arange(0, S, 2), np.arange(1, S, 2)])
    assert np.array_equal(covS4, covS) and np.array_equal(covfull, Pfin[np.ix_(fsel, fsel)])
    assert np.array_equal(Zfull, Xfin[0][0::2] + 1j * Xfin[0][1::2]) and np.array_equal(Z4, Z)
    WEst, HEst, info = nagp.nmf_init(Z, 2, restarts=3, numIts=5)
    assert WEst.shape == (2, 2) and HEst.shape == (120, 2) and info['Obj'].size == 10
    fast = np.mean(np.diff(HEst, axis=0) ** 2, axis=0) / np.var(HEst, axis=0, ddof=1)
    assert fast[0] >= fast[1] and np.all(np.isfinite(WEst)) and np.all(np.isfinite(HEst))
    assert np.all(np.abs(WEst.sum(axis=1) - 1.0) <= 4 * np.finfo(float).eps)
