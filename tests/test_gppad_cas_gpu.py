"""GPU (-m gpu): nagp_gppad_cas_obj / nagp.gppad_cas_obj -- the objective and gradient of experiments/gppad/Cascade/GetObjCasGPFAST.m -- its
resident form and the drivers MAPGPCasFast, CasGPMAP and FBCasGPMAP on the device path, against the multi-precision fixture
tests/golden/gppad_cas_multiprecision.npz and the NumPy restatement tests/gppad_cas_ref.py (pinned to the fixture without a GPU in
tests/test_gppad_cas_host.py).  Distances are the project's norm max|d| / max|ref| per array.

The rule is that of tests/test_gppad_gpu.py.  A device array must (1) be within TOL = 1e-7 and (2) be no more than 32 x as far from the
reference as the forward float64 restatement is, with a floor of 1e-15.  Where the restatement with every sum formed in the opposite
order is itself outside that bound, the bound widens to 32 x the larger of the two restatement distances -- never a figure taken from
the device.  Every measured triple (device, forward, reverse) is printed, and a run of the whole module writes them to
profiles/r18_gppad_cas_parity.txt.

Where no 60-digit value is stored (the sweep over every size, over M, the replay) the reference is the same objective in extended
precision (gppad_cas_ref.obj_ext), held to the fixture within 1e-12 in the host tests; the rule is applied to it unchanged.

End to end the trajectories are not compared, for the reason tests/test_gppad_gpu.py gives; the replay test checks every evaluation the
device was asked for at the point it was asked for."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nagp
from nagp import _lib as L
from nagp import gppad as gp
from nagp import gppad_cas as gc
import gppad_cas_ref as ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-7
FACTOR, FLOOR = 32.0, 1e-15
CASES = sorted(ref.CASES)
SIZES = list(range(1, 18))
MS = list(range(1, 9))
REPLAY = dict(T=1500, lens=[8.0, 64.0], NumIts=40, NumItsCas=30, seed=21)
LINES = []
N_LINES = 2 * len(CASES) + 2 * len(SIZES) + 2 * len(MS) + 2


@functools.lru_cache(maxsize=None)
def fixture():
    return dict(np.load(os.path.join(ROOT, 'tests', 'golden', 'gppad_cas_multiprecision.npz')))


@functools.lru_cache(maxsize=None)
def restated(name, reverse):
    return ref.objective(ref.case(name), reverse=reverse)


def bound_of(e_f, e_r):
    bound = FACTOR * max(e_f, FLOOR)
    if e_r > bound:                                      # the reverse-order restatement is itself outside: the order of the sums decides
        bound = FACTOR * max(e_f, e_r)
    return bound


def check(tag, got, want, fwd, rev, log=True):
    """both conditions of the module docstring, figures printed first"""
    e_gpu, e_f, e_r = ref.dist(got, want), ref.dist(fwd, want), ref.dist(rev, want)
    bound = bound_of(e_f, e_r)
    line = 'gppad-cas-parity %-28s device %.3e  forward %.3e  reverse %.3e  bound %.3e' % (tag, e_gpu, e_f, e_r, bound)
    if log:
        print(line); LINES.append(line)
    assert e_gpu < TOL, (tag, e_gpu)
    assert e_gpu <= bound, (tag, e_gpu, e_f, e_r)
    return e_gpu, e_f, e_r, bound


@pytest.fixture(scope='module', autouse=True)
def parity_file():
    yield
    if len(LINES) != N_LINES:                            # a partial run (-k) leaves the file alone
        return
    try:
        with open(os.path.join(ROOT, 'profiles', 'r18_gppad_cas_parity.txt'), 'w') as fh:
            fh.write('# tests/test_gppad_cas_gpu.py: distance to tests/golden/gppad_cas_multiprecision.npz (the sizes 2^k, M = 1 .. 8 and the replay: to the\n'
                     '# extended-precision evaluation), max|d| / max|ref| per array: the device, the float64 restatement, the restatement with every\n'
                     '# sum reversed, and the bound that held\n')
            fh.write('\n'.join(LINES) + '\n')
    except OSError:                                      # a read-only checkout: the figures are in the test output
        pass


def spectra(c):
    return dict(fftCovs=c['fftCovs']) if c['given'] else dict(len=c['len'])


def device(c, **kw):
    return nagp.gppad_cas_obj(c['x'], c['y'], c['varx'], c['mux'], c['varc'], **spectra(c), **kw)


@pytest.mark.parametrize('name', CASES)
def test_against_the_multiprecision_fixture(nagp_lib, name):
    f = fixture(); c = ref.case(name)
    Obj, dObj = device(c)
    fw, rv = restated(name, False), restated(name, True)
    check(name + ' Obj', Obj, f[name + '_Obj'], fw[0], rv[0])
    check(name + ' dObj', dObj, f[name + '_dObj'], fw[1], rv[1])
    assert dObj.shape == (c['M'], c['Tx'])
    Obj2, dObj2 = device(c)
    assert Obj == Obj2 and np.array_equal(dObj, dObj2)                      # the same call twice: equal bits
    assert device(c, grad=False) == Obj                                     # dObj = NULL: the same Obj bits
    with gc.GppadCasHandle(c['y'], c['M'], c['Tx'], c['varx'], c['mux'], c['varc'], **spectra(c)) as h:
        for _ in range(2):                                                  # the resident form: equal bits on its first and on its second evaluation
            Or, dr = h.eval(c['x'])
            assert Or[0] == Obj and np.array_equal(dr[0], dObj.reshape(-1))
        assert h.eval(c['x'], grad=False)[0] == Obj


def drawn(M, T, Tx, seed):
    """a white x around mux per column, a length-scale ladder from max(0.7, Tx / 64) down the columns, y of unit scale"""
    rng = np.random.default_rng(seed)
    mux = 0.3 - 0.1 * np.arange(M); varx = 1.3 - 0.1 * np.arange(M)
    x = mux[:, None] + rng.standard_normal((M, Tx)); y = rng.standard_normal(T)
    lens = np.array([max(0.7, Tx / 64.0) * 1.5 ** m for m in range(M)])
    return x, y, lens, varx, mux, 0.9


def against_ext(tag, x, y, lens, varx, mux, varc):
    c = np.stack([ref.fft_cov(ell, x.shape[1]) for ell in lens])
    fw = ref.obj(x, y, c, varx, mux, varc); rv = ref.obj(x, y, c, varx, mux, varc, reverse=True)
    Obj, dObj = nagp.gppad_cas_obj(x, y, varx, mux, varc, len=lens)
    want = ref.obj_ext(x, y, lens, varx, mux, varc)
    check(tag + ' Obj', Obj, want[0], fw[0], rv[0])
    check(tag + ' dObj', dObj, want[1], fw[1], rv[1])
    assert nagp.gppad_cas_obj(x, y, varx, mux, varc, len=lens, grad=False) == Obj


@pytest.mark.parametrize('k', SIZES)
def test_every_size(nagp_lib, k):
    """Tx = 2^k, M = 2, T = max(1, floor(0.64 Tx)): the device, the forward and the reverse restatement against the extended-precision
    evaluation, under the rule"""
    Tx = 2 ** k; T = max(1, int(0.64 * Tx))
    against_ext('2^%d' % k, *drawn(2, T, Tx, 7100 + k))


@pytest.mark.parametrize('M', MS)
def test_every_M(nagp_lib, M):
    """M = 1 .. 8 at Tx = 256, T = 163"""
    against_ext('M=%d' % M, *drawn(M, 163, 256, 7200 + M))


def three_cascades(c):
    """the case in the middle of two neighbours with their own x, y, parameters and length-scales"""
    rng = np.random.default_rng(5)
    x = np.stack([c['x'][:, ::-1].copy(), c['x'], c['x'] + 0.1 * rng.standard_normal(c['x'].shape)])
    y = np.stack([c['y'][::-1].copy(), c['y'], 2.0 * c['y']])
    return (x, y, np.stack([c['varx'] + 0.5, c['varx'], 0.7 * c['varx']]), np.stack([c['mux'] + 0.3, c['mux'], c['mux'] - 1.0]),
            np.array([1.5, c['varc'], 0.4]), np.stack([0.5 * c['len'], c['len'], 1.5 * c['len']]))


@pytest.mark.parametrize('name', ['k3_40_64', 'k2_3000_4096', 'k3_5000_8192'])
def test_a_cascade_does_not_depend_on_its_batch_mates(nagp_lib, name):
    """n_problems = 3 with spectra formed from len, with their own and with shared fftCovs, on both sides of the LDS / four-step switch:
    cascade 1 equals the same cascade run alone, bit for bit, and the objective-only call gives the same Obj bits"""
    c = ref.case(name); M, Tx = c['M'], c['Tx']
    x, y, varx, mux, varc, lens = three_cascades(c)
    alone_len = nagp.gppad_cas_obj(c['x'], c['y'], c['varx'], c['mux'], c['varc'], len=c['len'])
    alone_cov = nagp.gppad_cas_obj(c['x'], c['y'], c['varx'], c['mux'], c['varc'], fftCovs=c['fftCovs'])
    Ob, db = nagp.gppad_cas_obj(x, y, varx, mux, varc, len=lens)
    assert Ob.shape == (3,) and db.shape == (3, M, Tx)
    assert Ob[1] == alone_len[0] and np.array_equal(db[1], alone_len[1])
    covs = np.stack([[ref.fft_cov(ell, Tx) for ell in row] for row in lens])
    Oc, dc = nagp.gppad_cas_obj(x, y, varx, mux, varc, fftCovs=covs)                                  # their own spectra
    assert Oc[1] == alone_cov[0] and np.array_equal(dc[1], alone_cov[1])
    Os, ds = nagp.gppad_cas_obj(x, y, varx, mux, varc, fftCovs=c['fftCovs'])                          # shared spectra
    assert Os[1] == alone_cov[0] and np.array_equal(ds[1], alone_cov[1])
    for p in (0, 2):
        Oa, da = nagp.gppad_cas_obj(x[p], y[p], varx[p], mux[p], varc[p], fftCovs=covs[p])
        assert Oa == Oc[p] and np.array_equal(da, dc[p]), p
    assert np.array_equal(nagp.gppad_cas_obj(x, y, varx, mux, varc, fftCovs=covs, grad=False), Oc)


def test_device_batches_are_bit_equal_to_one_batch(nagp_lib, monkeypatch):
    """NAGP_GPPAD_BUDGET_MB=1 (read behind NAGP_DEVELOPER, which tests/conftest.py sets): a cascade of M = 3, T = 5000, Tx = 8192 takes
    8 (3 (4 x 8192 + 4) + 5000 + 2 x 20 + 1) = 826 856 B of the per-evaluation buffers, so 1 MiB holds 1: the three cascades run as three
    device batches; and one cascade of M = 8 at Tx = 8192 is beyond that budget (NAGP_EUNSUPPORTED, -2)"""
    c = ref.case('k3_5000_8192')
    x, y, varx, mux, varc, lens = three_cascades(c)
    full = nagp.gppad_cas_obj(x, y, varx, mux, varc, len=lens)
    monkeypatch.setenv('NAGP_GPPAD_BUDGET_MB', '1')
    cut = nagp.gppad_cas_obj(x, y, varx, mux, varc, len=lens)
    assert np.array_equal(full[0], cut[0]) and np.array_equal(full[1], cut[1])
    covs = np.stack([[ref.fft_cov(ell, c['Tx']) for ell in row] for row in lens])
    monkeypatch.delenv('NAGP_GPPAD_BUDGET_MB')
    full = nagp.gppad_cas_obj(x, y, varx, mux, varc, fftCovs=covs)
    monkeypatch.setenv('NAGP_GPPAD_BUDGET_MB', '1')
    cut = nagp.gppad_cas_obj(x, y, varx, mux, varc, fftCovs=covs)
    assert np.array_equal(full[0], cut[0]) and np.array_equal(full[1], cut[1])
    with pytest.raises(L.NagpError, match=r'\(-2\).*budget'):
        nagp.gppad_cas_obj(np.zeros((8, 8192)), np.ones(10), np.ones(8), np.zeros(8), 1.0, len=np.full(8, 5.0))


def test_GetObjCasGPFAST_is_the_batched_call(nagp_lib):
    c = ref.case('k3_200_256')
    O, d = device(c)
    P = dict(varx=c['varx'], mux=c['mux'], varc=c['varc'], len=c['len'])
    D = nagp.PackDimsCas(c['T'], c['Tx'], c['M'])
    O2, d2 = nagp.GetObjCasGPFAST(c['x'].reshape(-1), c['y'][:, None], c['fftCovs'].T, P, D)          # x = X(:), fftCovs Tx x M
    assert O2 == O and d2.shape == (c['M'] * c['Tx'],) and np.array_equal(d2, d.reshape(-1))
    assert nagp.GetObjCasGPFAST(c['x'].T, c['y'], c['fftCovs'].T, P, D, nout=1) == O                  # X itself, Tx x M
    ms = np.zeros(1)
    assert L.lib().nagp_gppad_cas_timings(L.dptr(ms)) == 0 and ms[0] > 0


def recording_evaluator(record):
    """the device behind a recorder for the joint objective; the levels (Dims without M) on the device as they are"""
    level = gp._device_evaluator(0); joint = gc._device_evaluator(0)

    def open_(y, Params, Dims):
        if 'M' not in Dims:
            return level(y, Params, Dims)
        f = joint(y, Params, Dims)

        def g(x):
            out = f(x)
            record.append((y, dict(Params), dict(Dims), np.array(x), out[0], np.array(out[1])))
            return out
        g.close = f.close
        return g
    return open_


def test_replay_of_every_evaluation(nagp_lib):
    """CasGPMAP on T = 1500, lens [8, 64], NumIts = 40, NumItsCas = 30 (Tx = 2048) with the device behind a recorder: every (Obj, dObj)
    MAPGPCasFast's line searches asked for, and the forward and reverse restatements at the same point, against the extended-precision
    evaluation there, under the rule; the evaluation that stands closest to its bound is the one logged"""
    y, _ = ref.g1.envelope_signal(REPLAY['T'], 32.0, REPLAY['seed'])
    rec = []
    A, X, c, Params, Info = nagp.CasGPMAP(y, REPLAY['lens'], dict(NumIts=REPLAY['NumIts'], NumItsCas=REPLAY['NumItsCas']), evaluator=recording_evaluator(rec))
    assert Info['Tx'] == 2048 and A.shape == (REPLAY['T'], 2) and len(rec) >= 2 and rec[0][4] == Info['ObjFT'][0]
    worst = {0: (0.0, 0.0, 0.0, 0.0), 1: (0.0, 0.0, 0.0, 0.0)}
    for n, (yy, P, Dims, xx, O, d) in enumerate(rec):
        Xm = xx.reshape(Dims['M'], Dims['Tx'])
        cov = np.stack([ref.fft_cov(ell, Dims['Tx']) for ell in P['len']])
        fw = ref.obj(Xm, yy, cov, P['varx'], P['mux'], P['varc']); rv = ref.obj(Xm, yy, cov, P['varx'], P['mux'], P['varc'], reverse=True)
        want = ref.obj_ext(Xm, yy, P['len'], P['varx'], P['mux'], P['varc'])
        for j, (got, f_, r_) in enumerate(((O, fw[0], rv[0]), (d.reshape(Xm.shape), fw[1], rv[1]))):
            e = check('replay %d %s' % (n, 'dObj' if j else 'Obj'), got, want[j], f_, r_, log=False)
            if e[0] / e[3] >= worst[j][0] / max(worst[j][3], 1e-300):
                worst[j] = e
    for j, what in enumerate(('Obj', 'dObj')):
        line = 'gppad-cas-parity %-28s device %.3e  forward %.3e  reverse %.3e  bound %.3e' % (('replay (%d evals) %s' % (len(rec), what),) + worst[j])
        print(line); LINES.append(line)


def test_FBCasGPMAP_in_lock_step_is_bit_equal_to_one_channel_at_a_time(nagp_lib):
    """three channels, the third with its own time-scales and so its own Tx (2048 against 1024): the lock-step run shares the level
    handles and one cascade handle among the first two; every output equals CasGPMAP on the channel alone, bit for bit"""
    y, _ = ref.g1.envelope_signal(600, 40.0, 33)
    Y = np.stack([y, 0.5 * y[::-1].copy(), y * np.linspace(0.5, 2.0, y.size)], axis=1)
    Len = np.array([[8.0, 8.0, 8.0], [48.0, 48.0, 120.0]])
    opts = dict(NumIts=40, NumItsCas=6)
    for ft in (False, True):
        A, X, Cc, Params, Info = nagp.FBCasGPMAP(Y, Len, opts, fine_tuned=ft)
        assert A.shape == X.shape == (600, 3, 2) and Cc.shape == (600, 3) and [I['Tx'] for I in Info] == [1024, 1024, 2048]
        for d in range(3):
            A1, X1, c1, P1, I1 = nagp.CasGPMAP(Y[:, d], Len[:, d], opts, fine_tuned=ft)
            assert np.array_equal(A[:, d, :], A1) and np.array_equal(X[:, d, :], X1) and np.array_equal(Cc[:, d], c1), (ft, d)
            assert Params['varc'][d] == P1['varc'] and np.array_equal(Params['varx'][:, d], P1['varx']) and np.array_equal(Params['mux'][:, d], P1['mux'])
            assert np.array_equal(Info[d]['ObjFT'], I1['ObjFT']), (ft, d)
