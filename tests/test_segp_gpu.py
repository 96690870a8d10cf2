"""GPU (-m gpu): nagp_segp_obj / nagp.segp_obj -- the objective and gradient of experiments/toolsGP/getObjSEGP.m -- and the drivers
trainSEGP_RS, trainSEGP_RS_many and modulator_prior_init on the device path, against the multi-precision fixture
tests/golden/segp_multiprecision.npz and the NumPy restatement tests/segp_ref.py (pinned to the fixture without a GPU in
tests/test_segp_host.py).  Distances are the project's norm max|d| / max|ref| per array.

The rule is that of tests/test_pstft_gpu.py.  A device array must (1) be within TOL = 1e-7 and (2) be no more than 32 x as far from the
fixture as the forward float64 restatement is, with a floor of 1e-15 (the fixture is stored in float64).  Where the restatement with
every sum over the frequencies formed in the opposite order is itself outside that bound, the order of the sums is what the distance
measures, and the bound widens to 32 x the larger of the two restatement distances -- never a figure taken from the device.  Every
measured triple (device, forward, reverse) is printed, and a run of the whole module writes them to profiles/r11_segp_parity.txt.

End to end: the minimum in log(lenx) is flat, so the last digits of lenx follow the noise of the gradient; on the CPU the forward and
the reverse restatement runs of the three signals differ in lenx by 4.9e-11, 1.3e-10 and 2.6e-9 and in the last info.Obj by at most
1.4e-16 (signals drawn by segp_ref.se_signal; with these draws it is the first pair that takes a different number of line searches,
6 against 5).  The tests compute those distances themselves: the device's lenx must be within 32 x the largest of them, and in any case
within 1e-6, of the forward run, its last info.Obj within 1e-12; evaluation counts and info.it are not compared."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nagp
from nagp import _lib as L
import segp_ref as ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-7
FACTOR, FLOOR = 32.0, 1e-15
LEN_TOL, OBJ_TOL = 1e-6, 1e-12
CASES = sorted(ref.CASES)
SIGNALS = [(2000, 20.0, 3), (2001, 8.0, 4), (1500, 60.0, 5)]
LINES = []
N_LINES = 2 * len(CASES) + 2 * len(SIGNALS) + 2      # Obj and dObj of every case, lenx and the last Obj of the three fits and of the chain


@functools.lru_cache(maxsize=None)
def fixture():
    return dict(np.load(os.path.join(ROOT, 'tests', 'golden', 'segp_multiprecision.npz')))


@functools.lru_cache(maxsize=None)
def restated(name, reverse):
    return ref.objective(ref.case(name), reverse=reverse)


def check(tag, got, want, fwd, rev):
    """both conditions of the module docstring, figures printed first"""
    e_gpu, e_f, e_r = ref.dist(got, want), ref.dist(fwd, want), ref.dist(rev, want)
    bound = FACTOR * max(e_f, FLOOR)
    if e_r > bound:                                  # the reverse-order restatement is itself outside: the order of the sums decides
        bound = FACTOR * max(e_f, e_r)
    line = 'segp-parity %-26s device %.3e  forward %.3e  reverse %.3e  bound %.3e' % (tag, e_gpu, e_f, e_r, bound)
    print(line); LINES.append(line)
    assert e_gpu < TOL, (tag, e_gpu)
    assert e_gpu <= bound, (tag, e_gpu, e_f, e_r)


@pytest.fixture(scope='module', autouse=True)
def parity_file():
    yield
    if len(LINES) != N_LINES:                        # a partial run (-k) leaves the file alone
        return
    try:
        with open(os.path.join(ROOT, 'profiles', 'r11_segp_parity.txt'), 'w') as fh:
            fh.write('# tests/test_segp_gpu.py: distance to tests/golden/segp_multiprecision.npz (the fits: to the forward restatement run),\n'
                     '# max|d| / max|ref| per array: the device, the float64 restatement, the restatement with the sums over the frequencies\n'
                     '# reversed, and the bound that held\n')
            fh.write('\n'.join(LINES) + '\n')
    except OSError:                                  # a read-only checkout: the figures are in the test output
        pass


def device(c, **kw):
    return nagp.segp_obj(c['param'], c['specy'], vary=c['vary'], varx=c['varx'], **kw)


@pytest.mark.parametrize('name', CASES)
def test_against_the_multiprecision_fixture(nagp_lib, name):
    f = fixture(); c = ref.case(name)
    Obj, dObj = device(c)
    fw, rv = restated(name, False), restated(name, True)
    check(name + ' Obj', Obj, f[name + '_Obj'], fw[0], rv[0])
    check(name + ' dObj', dObj, f[name + '_dObj'], fw[1], rv[1])
    assert dObj.shape == (c['n_param'],)
    Obj2, dObj2 = device(c)
    assert Obj == Obj2 and np.array_equal(dObj, dObj2)                      # the same call twice: equal bits
    assert device(c, grad=False) == Obj                                     # dObj = NULL: the same Obj bits


def three_problems(c):
    """the case in the middle of two neighbours with their own param, specy, vary and varx"""
    rng = np.random.default_rng(5)
    param = np.stack([c['param'] + 0.2 * rng.standard_normal(c['n_param']), c['param'], c['param'] - 0.1])
    spec = np.stack([c['specy'][::-1].copy(), c['specy'], c['specy'] * rng.exponential(1.0, c['T'])])
    vary = None if c['vary'] is None else np.array([2 * c['vary'], c['vary'], 0.5 * c['vary']])
    varx = None if c['varx'] is None else np.array([0.5 * c['varx'], c['varx'], 3 * c['varx']])
    return param, spec, vary, varx


@pytest.mark.parametrize('name', ['t5', 't257', 't1998', 't1999'])
def test_a_problem_does_not_depend_on_its_batch_mates(nagp_lib, name):
    """n_problems = 3 with shared and with per-problem specy: problem 1 equals the same problem run alone, bit for bit, and the
    objective-only call gives the same Obj bits"""
    c = ref.case(name)
    param, spec, vary, varx = three_problems(c)
    O1, d1 = device(c)
    Ob, db = nagp.segp_obj(param, spec, vary=vary, varx=varx)                                        # per-problem specy
    assert Ob.shape == (3,) and db.shape == (3, c['n_param'])
    assert Ob[1] == O1 and np.array_equal(db[1], d1)
    Os, ds = nagp.segp_obj(param, c['specy'], vary=vary, varx=varx)                                  # shared specy
    assert Os[1] == O1 and np.array_equal(ds[1], d1)
    for p in (0, 2):
        Oa, da = nagp.segp_obj(param[p], spec[p], vary=None if vary is None else vary[p], varx=None if varx is None else varx[p])
        assert Oa == Ob[p] and np.array_equal(da, db[p]), p
    assert np.array_equal(nagp.segp_obj(param, spec, vary=vary, varx=varx, grad=False), Ob)


def test_device_batches_are_bit_equal_to_one_batch(nagp_lib, monkeypatch):
    """NAGP_SEGP_BUDGET_MB=1 (read behind NAGP_DEVELOPER, which tests/conftest.py sets): the three-problem batch of case t1998
    (n_param = 3, 8 workgroups) with per-problem specy takes 8 (1998 + 8 * 5 + 6 + 3) = 16 376 B per problem and 4096 B per call, so
    1 MiB holds 63 problems: the batch repeated 64 times, 192 problems, runs as four device batches"""
    c = ref.case('t1998')
    param, spec, _, _ = three_problems(c)
    O3, d3 = nagp.segp_obj(param, spec)
    param = np.tile(param, (64, 1)); spec = np.tile(spec, (64, 1))
    full = nagp.segp_obj(param, spec)
    monkeypatch.setenv('NAGP_SEGP_BUDGET_MB', '1')
    cut = nagp.segp_obj(param, spec)
    assert np.array_equal(full[0], cut[0]) and np.array_equal(full[1], cut[1])
    assert np.array_equal(cut[0], np.tile(O3, 64)) and np.array_equal(cut[1], np.tile(d3, (64, 1)))
    assert np.array_equal(nagp.segp_obj(param, spec, grad=False), cut[0])


def test_a_problem_beyond_the_memory_budget_is_unsupported(nagp_lib, monkeypatch):
    """one problem of T = 200 000 shared frequencies takes 1.6 MB: beyond a budget lowered to 1 MiB it is NAGP_EUNSUPPORTED (-2), and
    it runs under the budget of the header"""
    T = 200000
    assert np.isfinite(nagp.segp_obj(np.log([50.0]), np.ones(T), vary=0.1, varx=1.0, grad=False))
    monkeypatch.setenv('NAGP_SEGP_BUDGET_MB', '1')
    with pytest.raises(L.NagpError, match=r'\(-2\).*budget'):
        nagp.segp_obj(np.log([50.0]), np.ones(T), vary=0.1, varx=1.0)


def test_getObjSEGP_is_the_batched_call_and_non_finite_results_come_back(nagp_lib):
    c = ref.case('t255')                                     # three parameters
    O, d = device(c)
    O3, d3 = nagp.getObjSEGP(c['param'][:, None], c['specy'][:, None])
    assert O3 == O and np.array_equal(d3, d) and nagp.getObjSEGP(c['param'], c['specy'], nout=1) == O
    vary, varx = np.exp(c['param'][2]), np.exp(c['param'][1])
    O2, d2 = nagp.getObjSEGP(c['param'][:2], c['specy'], vary)                   # the reference's order: vary, then varx
    O1, d1 = nagp.getObjSEGP(c['param'], c['specy'], vary, varx)                 # param(1) alone is used
    assert d2.shape == (2,) and d1.shape == (1,)
    for a, b in ((O2, O), (O1, O), (d2, d[:2]), (d1, d[:1])):
        assert ref.dist(a, b) < 1e-14                        # exp(log(v)) against v: an ulp of the inputs
    with np.errstate(all='ignore'):                          # exp(param) underflows: S = 0, log S = -inf; returned as it is
        Ou = nagp.segp_obj(np.array([0.0, -800.0, -800.0]), c['specy'], grad=False)
    assert not np.isfinite(Ou)


@functools.lru_cache(maxsize=None)
def signal(k):
    return ref.se_signal(*SIGNALS[k])


@functools.lru_cache(maxsize=None)
def host_fit(k, reverse):
    return ref.train(signal(k), reverse=reverse)


@functools.lru_cache(maxsize=None)
def device_fit(k):
    return nagp.trainSEGP_RS(signal(k))


def fit_bounds(pairs):
    """(lenx bound, figures) from the forward / reverse restatement runs themselves"""
    e_len = max(abs(r[0] - f[0]) / abs(f[0]) for f, r in pairs)
    return min(max(FACTOR * e_len, FACTOR * FLOOR), LEN_TOL), e_len


def check_fit(tag, dv, fw, rv, len_bound):
    e_len, e_len_r = abs(dv[0] - fw[0]) / abs(fw[0]), abs(rv[0] - fw[0]) / abs(fw[0])
    e_obj, e_obj_r = ref.dist(dv[2]['Obj'][-1], fw[2]['Obj'][-1]), ref.dist(rv[2]['Obj'][-1], fw[2]['Obj'][-1])
    for what, e, er, b in (('lenx', e_len, e_len_r, len_bound), ('last Obj', e_obj, e_obj_r, OBJ_TOL)):
        line = 'segp-parity %-26s device %.3e  forward %.3e  reverse %.3e  bound %.3e' % ('%s %s' % (tag, what), e, 0.0, er, b)
        print(line); LINES.append(line)
    assert e_len <= len_bound and e_len <= LEN_TOL, (tag, e_len, len_bound)
    assert e_obj <= OBJ_TOL, (tag, e_obj)
    assert dv[1] == fw[1]                                    # varx = var(x) is not optimised


@pytest.mark.parametrize('k', range(len(SIGNALS)))
def test_fit_on_the_device_against_the_restatement(nagp_lib, k):
    len_bound, e_len = fit_bounds([(host_fit(j, False), host_fit(j, True)) for j in range(len(SIGNALS))])
    print('forward / reverse restatement runs: largest lenx distance %.3e -> bound %.3e' % (e_len, len_bound))
    dv = device_fit(k)
    check_fit('fit T=%d len=%g' % SIGNALS[k][:2], dv, host_fit(k, False), host_fit(k, True), len_bound)
    assert np.isfinite(dv[0]) and dv[0] > 0 and np.all(np.diff(dv[2]['Obj']) <= 0)


def test_fit_many_is_bit_equal_to_the_single_fits(nagp_lib):
    many = nagp.trainSEGP_RS_many([signal(k) for k in range(len(SIGNALS))])
    for k, m in enumerate(many):
        s = device_fit(k)
        assert m[0] == s[0] and m[1] == s[1]
        assert np.array_equal(m[2]['Obj'], s[2]['Obj']) and np.array_equal(m[2]['it'], s[2]['it'])
    two = nagp.trainSEGP_RS_many([signal(0), signal(0)[::-1].copy()], dict(numIts=6, progress_chunk=3), [5.0, 9.0], 1.1, 0.1)      # equal T: one call per round
    for x, l0, m in zip((signal(0), signal(0)[::-1].copy()), (5.0, 9.0), two):
        s = nagp.trainSEGP_RS(x, dict(numIts=6, progress_chunk=3), l0, 1.1, 0.1)
        assert m[0] == s[0] and np.array_equal(m[2]['Obj'], s[2]['Obj']) and np.array_equal(m[2]['it'], s[2]['it']) and m[2]['it'].shape == (2,)


def test_chain_from_a_waveform_to_the_modulator_prior(nagp_lib):
    """the first 4000 samples of the committed speech_74 fixture: fit_probSTFT_SD (exp, D = 4, 3 levels) -> sort -> get_disc_model ->
    kernel_ss_probFB -> nmf_init(Z, 2, restarts=2, numIts=20) -> modulator_prior_init(HEst): finite positive lenx_nmf, varx_nmf, equal to
    the restatement's on the same HEst under the two bounds of the module docstring"""
    from nagp.fastfb import get_disc_model
    z = np.load(os.path.join(ROOT, 'tests', 'golden', 'audio_speech_74.npz'))
    y = z['samples'][:4000].astype(float); y = y / np.std(y)
    D = 4
    varx, lamx, om, Info = nagp.fit_probSTFT_SD(y, D, 'exp', dict(numLevels=3, numIts=5, minT=100, maxT=400, bet=750, reassign=0))
    order = np.argsort(om)                                   # train_GTFNMF.m:57-59
    A, Q, H, Pinf, K, tau = get_disc_model(lamx[order], varx[order], om[order], D, 'exp')
    Z, = nagp.kernel_ss_probFB(y, A, Q, H, Pinf, K, 0, tau)
    W, HEst, info = nagp.nmf_init(Z, 2, restarts=2, numIts=20)
    assert HEst.shape == (4000, 2) and np.all(np.isfinite(HEst))
    lenx_nmf, varx_nmf, mux, infos = nagp.modulator_prior_init(HEst)
    assert lenx_nmf.shape == (2,) and varx_nmf.shape == (2,) and mux.shape == (2,) and len(infos) == 2
    assert np.all(np.isfinite(lenx_nmf)) and np.all(lenx_nmf > 0) and np.all(np.isfinite(varx_nmf)) and np.all(varx_nmf > 0)
    fw, rv = ref.modulator_prior_init(HEst), ref.modulator_prior_init(HEst, reverse=True)
    assert ref.dist(mux, fw[2]) < 1e-14 and ref.dist(varx_nmf, fw[1]) < 1e-12
    e_len_r = float(np.max(np.abs(rv[0] - fw[0]) / np.abs(fw[0])))
    len_bound = min(max(FACTOR * e_len_r, FACTOR * FLOOR), LEN_TOL)
    e_len = float(np.max(np.abs(lenx_nmf - fw[0]) / np.abs(fw[0])))
    e_obj = max(ref.dist(infos[n]['Obj'][-1], fw[3][n]['Obj'][-1]) for n in range(2))
    e_obj_r = max(ref.dist(rv[3][n]['Obj'][-1], fw[3][n]['Obj'][-1]) for n in range(2))
    for what, e, er, b in (('lenx_nmf', e_len, e_len_r, len_bound), ('last Obj', e_obj, e_obj_r, OBJ_TOL)):
        line = 'segp-parity %-26s device %.3e  forward %.3e  reverse %.3e  bound %.3e' % ('chain ' + what, e, 0.0, er, b)
        print(line); LINES.append(line)
    print('chain: lenx_nmf %s varx_nmf %s mux %s' % (lenx_nmf, varx_nmf, mux))
    assert e_len <= len_bound and e_obj <= OBJ_TOL, (e_len, len_bound, e_obj)
