"""GPU (-m gpu): nagp_gppad_obj / nagp.gppad_obj -- the objective and gradient of experiments/gppad/GPModelFast/GetGPObjFast.m -- its
resident form and the drivers InferAmplitudeGPMAP, InferAmplitudeGPMAP_many and GPPAD on the device path, against the multi-precision
fixture tests/golden/gppad_multiprecision.npz and the NumPy restatement tests/gppad_ref.py (pinned to the fixture without a GPU in
tests/test_gppad_host.py).  Distances are the project's norm max|d| / max|ref| per array.

The rule is that of tests/test_segp_gpu.py.  A device array must (1) be within TOL = 1e-7 and (2) be no more than 32 x as far from the
reference as the forward float64 restatement is, with a floor of 1e-15 (the fixture is stored in float64).  Where the restatement with
every sum formed in the opposite order is itself outside that bound, the order of the sums is what the distance measures, and the
bound widens to 32 x the larger of the two restatement distances -- never a figure taken from the device.  Every measured triple
(device, forward, reverse) is printed, and a run of the whole module writes them to profiles/r12_gppad_parity.txt.

The transform is held in LDS for Tx <= 4096 and split four-step, (Tx / 4096) x 4096, from Tx = 8192: the fixture cases (3000, 4096) and
(4095, 4096) lie on one side of the switch, (5000, 8192) and (20000, 32768) on the other, and the sweep over every size crosses it.

Where no 60-digit value is stored (the sweep over every size, the replay) the reference is the same objective in extended precision
(gppad_ref.obj_ext: np.longdouble, eps 1.1e-19, through scipy.fft), 2^11 times finer than the float64 restatements it judges; the rule
is applied to it unchanged.  (The restatement cannot be its own reference: its distance to itself is 0 and the rule would then hold
the device to the floor alone, wherever the forward and the reverse restatement differ by more than that.)

End to end the trajectories are not compared: c spans 1e-6 .. sqrt(2 pi) len, so a line search amplifies any rounding difference (on the
CPU the forward and the reverse restatement runs of the replay case end 2.7e-5 apart in the envelope at NumIts = 60 and 2 - 4 % apart at
NumIts = 3000).  The replay test checks every evaluation the device was asked for at the point it was asked for; the quality test
holds the device's envelope to the correlation the forward NumPy run reaches, minus 0.05."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nagp
from nagp import _lib as L
from nagp import gppad as gp
import gppad_ref as ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-7
FACTOR, FLOOR = 32.0, 1e-15
CASES = sorted(ref.CASES)
SIZES = list(range(1, 21))
REPLAY = dict(T=1500, len=32.0, NumIts=60, seed=21)
LINES = []
N_LINES = 2 * len(CASES) + 2 * len(SIZES) + 2            # Obj and dObj of every case and of every size, the worst Obj and dObj of the replay


@functools.lru_cache(maxsize=None)
def fixture():
    return dict(np.load(os.path.join(ROOT, 'tests', 'golden', 'gppad_multiprecision.npz')))


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
    line = 'gppad-parity %-28s device %.3e  forward %.3e  reverse %.3e  bound %.3e' % (tag, e_gpu, e_f, e_r, bound)
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
        with open(os.path.join(ROOT, 'profiles', 'r12_gppad_parity.txt'), 'w') as fh:
            fh.write('# tests/test_gppad_gpu.py: distance to tests/golden/gppad_multiprecision.npz (the sizes 2^k and the replay: to the extended-precision evaluation),\n'
                     '# max|d| / max|ref| per array: the device, the float64 restatement, the restatement with every sum reversed, and the bound\n'
                     '# that held\n')
            fh.write('\n'.join(LINES) + '\n')
    except OSError:                                      # a read-only checkout: the figures are in the test output
        pass


def device(c, **kw):
    if c['given']:
        return nagp.gppad_obj(c['x'], c['y'], c['vary'], c['varx'], c['mux'], c['varc'], fftCov=c['fftCov'], **kw)
    return nagp.gppad_obj(c['x'], c['y'], c['vary'], c['varx'], c['mux'], c['varc'], len=c['len'], **kw)


@pytest.mark.parametrize('name', CASES)
def test_against_the_multiprecision_fixture(nagp_lib, name):
    f = fixture(); c = ref.case(name)
    Obj, dObj = device(c)
    fw, rv = restated(name, False), restated(name, True)
    check(name + ' Obj', Obj, f[name + '_Obj'], fw[0], rv[0])
    check(name + ' dObj', dObj, f[name + '_dObj'], fw[1], rv[1])
    assert dObj.shape == (c['Tx'],)
    Obj2, dObj2 = device(c)
    assert Obj == Obj2 and np.array_equal(dObj, dObj2)                      # the same call twice: equal bits
    assert device(c, grad=False) == Obj                                     # dObj = NULL: the same Obj bits
    with gp.GppadHandle(c['y'], c['Tx'], c['vary'] if np.ndim(c['vary']) == 0 else c['vary'][None, :], c['varx'], c['mux'], c['varc'],
                        **(dict(fftCov=c['fftCov']) if c['given'] else dict(len=c['len']))) as h:
        Or, dr = h.eval(c['x'])
        assert Or[0] == Obj and np.array_equal(dr[0], dObj)                 # the resident form: equal bits, also on its second evaluation
        assert h.eval(c['x'], grad=False)[0] == Obj


@pytest.mark.parametrize('k', SIZES)
def test_every_size(nagp_lib, k):
    """Tx = 2^k, T = max(1, floor(0.64 Tx)), one problem: a white x around mux, len = max(0.7, Tx / 64), scalar vary; the device, the forward
    and the reverse restatement against the extended-precision evaluation, under the rule"""
    Tx = 2 ** k; T = max(1, int(0.64 * Tx))
    rng = np.random.default_rng(7000 + k)
    x = -0.3 + rng.standard_normal(Tx); y = rng.standard_normal(T); ell = max(0.7, Tx / 64.0)
    c = ref.fft_cov(ell, Tx)
    fw = ref.obj(x, y, c, 1.3, -0.3, 0.9, 0.01); rv = ref.obj(x, y, c, 1.3, -0.3, 0.9, 0.01, reverse=True)
    Obj, dObj = nagp.gppad_obj(x, y, 0.01, 1.3, -0.3, 0.9, len=ell)
    want = ref.obj_ext(x, y, ell, 1.3, -0.3, 0.9, 0.01)
    check('2^%d Obj' % k, Obj, want[0], fw[0], rv[0])
    check('2^%d dObj' % k, dObj, want[1], fw[1], rv[1])
    assert nagp.gppad_obj(x, y, 0.01, 1.3, -0.3, 0.9, len=ell, grad=False) == Obj


def three_problems(c):
    """the case in the middle of two neighbours with their own x, y, parameters and length-scale"""
    rng = np.random.default_rng(5)
    x = np.stack([c['x'][::-1].copy(), c['x'], c['x'] + 0.1 * rng.standard_normal(c['Tx'])])
    y = np.stack([c['y'][::-1].copy(), c['y'], 2.0 * c['y']])
    return x, y, np.array([2.0, c['varx'], 0.7]), np.array([0.3, c['mux'], -1.0]), np.array([1.5, c['varc'], 0.4]), np.array([0.5 * c['len'], c['len'], 3.0])


@pytest.mark.parametrize('name', ['c50_64', 'c3000_4096', 'c5000_8192'])
def test_a_problem_does_not_depend_on_its_batch_mates(nagp_lib, name):
    """n_problems = 3 with their own and with a shared fftCov, with scalar and with per-sample vary, on both sides of the LDS / four-step
    switch: problem 1 equals the same problem run alone, bit for bit, and the objective-only call gives the same Obj bits"""
    c = ref.case(name); T, Tx = c['T'], c['Tx']
    x, y, varx, mux, varc, lens = three_problems(c)
    for vary1 in (0.02, np.linspace(0.0, 1.0, T)):
        per = np.ndim(vary1) > 0
        vary3 = np.stack([vary1[::-1], vary1, 2 * vary1]) if per else np.array([0.5, vary1, 0.0])
        alone_len = nagp.gppad_obj(c['x'], c['y'], vary1, c['varx'], c['mux'], c['varc'], len=c['len'])
        alone_cov = nagp.gppad_obj(c['x'], c['y'], vary1, c['varx'], c['mux'], c['varc'], fftCov=c['fftCov'])
        Ob, db = nagp.gppad_obj(x, y, vary3, varx, mux, varc, len=lens)                               # spectra formed on the device
        assert Ob.shape == (3,) and db.shape == (3, Tx)
        assert Ob[1] == alone_len[0] and np.array_equal(db[1], alone_len[1])
        covs = np.stack([ref.fft_cov(l, Tx) for l in lens])
        Oc, dc = nagp.gppad_obj(x, y, vary3, varx, mux, varc, fftCov=covs)                            # their own fftCov
        assert Oc[1] == alone_cov[0] and np.array_equal(dc[1], alone_cov[1])
        Os, ds = nagp.gppad_obj(x, y, vary3, varx, mux, varc, fftCov=c['fftCov'])                     # a shared fftCov
        assert Os[1] == alone_cov[0] and np.array_equal(ds[1], alone_cov[1])
        for p in (0, 2):
            Oa, da = nagp.gppad_obj(x[p], y[p], vary3[p], varx[p], mux[p], varc[p], fftCov=covs[p])
            assert Oa == Oc[p] and np.array_equal(da, dc[p]), p
        assert np.array_equal(nagp.gppad_obj(x, y, vary3, varx, mux, varc, fftCov=covs, grad=False), Oc)


def test_device_batches_are_bit_equal_to_one_batch(nagp_lib, monkeypatch):
    """NAGP_GPPAD_BUDGET_MB=1 (read behind NAGP_DEVELOPER, which tests/conftest.py sets): a problem of Tx = 8192 takes 8 (4 x 8192 + 2 x 2 + 1)
    = 262 184 B of the per-evaluation buffers, so 1 MiB holds 3: the three-problem batch of case c5000_8192 repeated 3 times, 9 problems,
    runs as three device batches; and one problem of Tx = 65536 is beyond that budget (NAGP_EUNSUPPORTED, -2)"""
    c = ref.case('c5000_8192')
    x, y, varx, mux, varc, lens = three_problems(c)
    O3, d3 = nagp.gppad_obj(x, y, 0.0, varx, mux, varc, len=lens)
    rep = lambda a: np.tile(a, (3,) + (1,) * (a.ndim - 1))
    full = nagp.gppad_obj(rep(x), rep(y), 0.0, rep(varx), rep(mux), rep(varc), len=rep(lens))
    monkeypatch.setenv('NAGP_GPPAD_BUDGET_MB', '1')
    cut = nagp.gppad_obj(rep(x), rep(y), 0.0, rep(varx), rep(mux), rep(varc), len=rep(lens))
    assert np.array_equal(full[0], cut[0]) and np.array_equal(full[1], cut[1])
    assert np.array_equal(cut[0], np.tile(O3, 3)) and np.array_equal(cut[1], np.tile(d3, (3, 1)))
    with pytest.raises(L.NagpError, match=r'\(-2\).*budget'):
        nagp.gppad_obj(np.zeros(65536), np.ones(10), 0.0, 1.0, 0.0, 1.0, len=5.0)


def test_GetGPObjFast_is_the_batched_call(nagp_lib):
    c = ref.case('c657_1024')
    O, d = device(c)
    P = gp.PackParamsGP(c['varx'], c['len'], c['mux'], c['varc'], c['vary'])
    O2, d2 = nagp.GetGPObjFast(c['x'][:, None], c['y'][:, None], c['fftCov'], P, dict(T=c['T'], Tx=c['Tx']))
    assert O2 == O and np.array_equal(d2, d) and nagp.GetGPObjFast(c['x'], c['y'], c['fftCov'], P, dict(T=c['T'], Tx=c['Tx']), nout=1) == O
    ms = np.zeros(1)
    assert L.lib().nagp_gppad_timings(L.dptr(ms)) == 0 and ms[0] > 0


@functools.lru_cache(maxsize=None)
def replay_signal():
    return ref.envelope_signal(REPLAY['T'], REPLAY['len'], REPLAY['seed'])


def recording_device_evaluator(record):
    inner = gp._device_evaluator(0)

    def open_level(y, Params, Dims):
        f = inner(y, Params, Dims)

        def g(x):
            out = f(x)
            record.append((y, dict(Params), dict(Dims), np.array(x), out[0], np.array(out[1])))
            return out
        g.close = f.close
        return g
    return open_level


@functools.lru_cache(maxsize=None)
def device_run():
    y, a = replay_signal()
    rec = []
    P = gp.PackParamsGP(1.0, REPLAY['len'], 0.0, 1.0, np.zeros(y.size))
    out = nagp.InferAmplitudeGPMAP(y, P, dict(NumIts=REPLAY['NumIts']), evaluator=recording_device_evaluator(rec))
    return out, rec


def test_replay_of_every_evaluation(nagp_lib):
    """InferAmplitudeGPMAP on T = 1500, len = 32, NumIts = 60 (Tx = 2048, DSs = 4, 2, 1) with the device evaluator behind a recorder: every
    recorded (Obj, dObj), and the forward and reverse restatements at the same point, against the extended-precision evaluation there, under
    the rule; the evaluation that stands closest to its bound is the one logged"""
    (a, x, Info), rec = device_run()
    assert Info['Tx'] == 2048 and np.array_equal(Info['DSs'], [4, 2, 1]) and {r[2]['Tx'] for r in rec} == {512, 1024, 2048}
    assert len(rec) >= REPLAY['NumIts']
    worst = {0: (0.0, 0.0, 0.0, 0.0), 1: (0.0, 0.0, 0.0, 0.0)}
    for n, (y, P, Dims, xx, O, d) in enumerate(rec):
        c = ref.fft_cov(P['len'], Dims['Tx'])
        fw = ref.obj(xx, y, c, P['varx'], P['mux'], P['varc'], P['vary']); rv = ref.obj(xx, y, c, P['varx'], P['mux'], P['varc'], P['vary'], reverse=True)
        want = ref.obj_ext(xx, y, P['len'], P['varx'], P['mux'], P['varc'], P['vary'])
        for j, (got, f_, r_) in enumerate(((O, fw[0], rv[0]), (d, fw[1], rv[1]))):
            e = check('replay %d %s' % (n, 'dObj' if j else 'Obj'), got, want[j], f_, r_, log=False)
            if e[0] / e[3] >= worst[j][0] / max(worst[j][3], 1e-300):
                worst[j] = e
    for j, what in enumerate(('Obj', 'dObj')):
        line = 'gppad-parity %-28s device %.3e  forward %.3e  reverse %.3e  bound %.3e' % (('replay (%d evals) %s' % (len(rec), what),) + worst[j])
        print(line); LINES.append(line)


def test_many_is_bit_equal_to_the_single_runs(nagp_lib):
    y, _ = replay_signal()
    ys = [y, 0.5 * y[::-1].copy(), y * np.linspace(0.5, 2.0, y.size)]
    Ps = [gp.PackParamsGP(1.0, 32.0, 0.0, 1.0, 0.0), gp.PackParamsGP(0.8, 32.0, 0.2, 0.5, np.zeros(y.size)), gp.PackParamsGP(1.5, 20.0, -0.1, 1.2, 0.01)]
    opts = dict(NumIts=12)
    many = nagp.InferAmplitudeGPMAP_many(ys, Ps, opts)
    for k in range(3):
        a, x, Info = nagp.InferAmplitudeGPMAP(ys[k], Ps[k], opts)
        assert np.array_equal(many[k][0], a) and np.array_equal(many[k][1], x) and np.array_equal(many[k][2]['Obj'], Info['Obj']), k


def test_quality_of_the_envelope(nagp_lib):
    """a drawn envelope times white noise at the replay's shape through GPPAD: the correlation of the device's envelope with the drawn one is
    no lower than that of the forward NumPy run (computed here) minus 0.05; each level's objective history does not increase"""
    y, a = replay_signal()
    opts = dict(NumIts=REPLAY['NumIts'])
    Ad, Cd, Pd, Infod, Xd = nagp.GPPAD(y[:, None], REPLAY['len'], 0, opts)
    Ah, Ch, Ph, Infoh, Xh = nagp.GPPAD(y[:, None], REPLAY['len'], 0, opts, evaluator=ref.evaluator())
    cd, ch = np.corrcoef(Ad[:, 0], a)[0, 1], np.corrcoef(Ah[:, 0], a)[0, 1]
    print('gppad-quality: correlation with the drawn envelope: device %.4f, NumPy %.4f' % (cd, ch))
    assert cd >= ch - 0.05
    assert np.all(Ad > 0) and np.allclose(Ad * Cd, y[:, None], rtol=1e-12, atol=0) and Pd['varc'] == Ph['varc']          # the marginal parameters are host work
    assert all(np.all(np.diff(o) <= 0) for o in Infod[0][1]['ObjLevels'])


def test_chain_from_a_waveform_to_W(nagp_lib):
    """the first 2000 samples of the committed speech_74 fixture: fit_probSTFT_SD (exp, D = 4) -> sort -> get_disc_model -> kernel_ss_probFB
    -> GPPAD(real(Z).T, 20) -> nmf_init(Z, 2, mods=A) -> modulator_prior_init(HEst): finite, positive where they must be, right shapes"""
    from nagp.fastfb import get_disc_model
    z = np.load(os.path.join(ROOT, 'tests', 'golden', 'audio_speech_74.npz'))
    y = z['samples'][:2000].astype(float); y = y / np.std(y)
    D = 4
    varx, lamx, om, Info = nagp.fit_probSTFT_SD(y, D, 'exp', dict(numLevels=3, numIts=5, minT=100, maxT=400, bet=750, reassign=0))
    order = np.argsort(om)
    A_, Q, H, Pinf, K, tau = get_disc_model(lamx[order], varx[order], om[order], D, 'exp')
    Z, = nagp.kernel_ss_probFB(y, A_, Q, H, Pinf, K, 0, tau)
    A, Cc, Params, Info, X = nagp.GPPAD(np.real(Z).T, 20.0, 0, dict(NumIts=30))
    assert A.shape == Cc.shape == X.shape == (2000, D) and np.all(np.isfinite(A)) and np.all(A > 0) and np.all(np.isfinite(Cc))
    assert all(np.all(np.isfinite(Params[k])) and np.all(Params[k] > 0) for k in ('varx', 'varc')) and np.all(np.isfinite(Params['mux']))
    assert np.allclose(A * Cc, np.real(Z).T, rtol=1e-10, atol=0)
    W, HEst, info = nagp.nmf_init(Z, 2, restarts=2, numIts=20, mods=A)
    assert W.shape == (2, D) and HEst.shape == (2000, 2) and np.all(np.isfinite(HEst)) and np.all(W >= 0) and np.all(HEst >= 0)
    lenx_nmf, varx_nmf, mux, infos = nagp.modulator_prior_init(HEst)
    assert lenx_nmf.shape == (2,) and np.all(np.isfinite(lenx_nmf)) and np.all(lenx_nmf > 0) and np.all(np.isfinite(varx_nmf)) and np.all(varx_nmf > 0)
    assert np.all(np.isfinite(mux))
