"""GPU (-m gpu): the Laplace step of GPPAD on the device (nagp_gppad_lap_*, nagp.gppad_lap) against the multi-precision fixture
tests/golden/gppad_lap_multiprecision.npz and the NumPy restatement tests/gppad_lap_ref.py (pinned to the fixture without a GPU in
tests/test_gppad_lap_host.py).  Distances are the project's norm max|d| / max|ref| per array.

The parts without decisions (d, A v, Varx from given pairs, Obj1, Obj2) follow the rule of tests/test_gppad_gpu.py unchanged: a device
array must (1) be within TOL = 1e-7 and (2) be no more than 32 x as far from the reference as the forward float64 restatement is, with
a floor of 1e-15; where the restatement with every sum formed in the opposite order is itself outside that bound, the bound widens to
32 x the larger of the two restatement distances -- never a figure taken from the device.  Where no 60-digit value is stored (the sizes
beyond 256) the reference is the same formula in extended precision (ext=True), held to the fixture within 1e-15 in the host tests.

The Lanczos run has decisions in it, so on the stable cases of the fixture the device must give the restatement's (steps,
reorthogonalisations, nconv), lmb and Varx within 32 x the case's stored self-deviation (floor 1e-15) and never beyond TOL, and every
returned pair must satisfy |A xv - lmb xv| <= 2 tolconv anorm with A and anorm from the restatement.

Every measured figure is printed, and a run of the whole module writes them to profiles/r19_gppad_lap_parity.txt.  End to end the
trajectories are not compared, for the reason tests/test_gppad_gpu.py gives; the replay test checks every Laplace solve the device was
asked for at the point it was asked for."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nagp
from nagp import _lib as L
from nagp import gppad_lap as gl
import gppad_lap_ref as ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-7
FACTOR, FLOOR = 32.0, 1e-15
FIXED = sorted(ref.FIXED)
STABLE = sorted(ref.STABLE)
SIZES = ['s20_32', 's333_512', 's3000_4096', 's4096_4096', 's5000_8192', 's11111_16384']
REPLAY = dict(T=1500, len=16.0, opts=dict(nev=16, tol=3, Overlap=1, NumIts=20))
LINES = []
N_LINES = 4 * len(FIXED) + 4 * len(SIZES) + len(STABLE) + 2


@functools.lru_cache(maxsize=None)
def fixture():
    return dict(np.load(os.path.join(ROOT, 'tests', 'golden', 'gppad_lap_multiprecision.npz')))


@functools.lru_cache(maxsize=None)
def clean(name):
    return ref.solve(ref.stable_case(name))


def bound_of(e_f, e_r):
    bound = FACTOR * max(e_f, FLOOR)
    if e_r > bound:                                      # the reverse-order restatement is itself outside: the order of the sums decides
        bound = FACTOR * max(e_f, e_r)
    return bound


def check(tag, got, want, fwd, rev):
    """both conditions of the module docstring, figures printed first"""
    e_gpu, e_f, e_r = ref.dist(got, want), ref.dist(fwd, want), ref.dist(rev, want)
    bound = bound_of(e_f, e_r)
    line = 'gppad-lap-parity %-28s device %.3e  forward %.3e  reverse %.3e  bound %.3e' % (tag, e_gpu, e_f, e_r, bound)
    print(line); LINES.append(line)
    assert e_gpu < TOL, (tag, e_gpu)
    assert e_gpu <= bound, (tag, e_gpu, e_f, e_r)


@pytest.fixture(scope='module', autouse=True)
def parity_file():
    yield
    if len(LINES) != N_LINES:                            # a partial run (-k) leaves the file alone
        return
    try:
        with open(os.path.join(ROOT, 'profiles', 'r19_gppad_lap_parity.txt'), 'w') as fh:
            fh.write('# tests/test_gppad_lap_gpu.py: distance to tests/golden/gppad_lap_multiprecision.npz (the sizes beyond 256: to the extended-precision\n'
                     '# evaluation), max|d| / max|ref| per array: the device, the float64 restatement, the restatement with every sum reversed, and\n'
                     '# the bound that held; for the Lanczos runs: the counts, the distance of lmb and Varx to the restatement and 32 x the self-deviation\n')
            fh.write('\n'.join(LINES) + '\n')
    except OSError:                                      # a read-only checkout: the figures are in the test output
        pass


def handle(c, jmax=1):
    return gl.GppadLapHandle(c['y'], c['Tx'], c['vary'], c['varx'], c['mux'], c['varc'], c['len'], jmax)


def fixed_parts(tag, c, want):
    """d, A v, Varx from the given pairs, Obj1 and Obj2 of one case under the rule; want: a dict with d, Av, Varx, Obj"""
    K = len(c['lmb'])
    with handle(c, jmax=K) as h:
        d = h.hess(c['x'])[0]; Av = h.apply(c['v'])[0]; O = h.obj()[0]
        V, neg = h.varx(c['xv'], c['lmb'])
        V2, _ = h.varx(c['xv'], c['lmb'])
        assert np.array_equal(V, V2) and np.isnan(O[0]) and neg[0] == int(np.sum(V[0] < 0))
        assert np.array_equal(h.hess(c['x'])[0], d) and np.array_equal(h.apply(c['v'])[0], Av)          # the same call twice: equal bits
    r = {}
    for reverse in (False, True):
        dd = ref.hessian(c['x'], c['y'], c['varc'], c['vary']); hs = ref.hhalf(c['len'], c['Tx'], c['varx'])
        r[reverse] = dict(d=dd, Av=ref.apply(c['v'], dd, hs, reverse), Varx=ref.varx_from(c['xv'], c['lmb'], hs, c['varx'], reverse),
                          Obj=ref.obj_terms(c['x'], c['y'], c['len'], c['varx'], c['mux'], c['varc'], c['vary'], c['lmb'], reverse))
    check(tag + ' d', d, want['d'], r[False]['d'], r[True]['d'])
    check(tag + ' Av', Av, want['Av'], r[False]['Av'], r[True]['Av'])
    check(tag + ' Varx', V[0], want['Varx'], r[False]['Varx'], r[True]['Varx'])
    check(tag + ' Obj1,Obj2', O[1:], want['Obj'][1:], r[False]['Obj'][1:], r[True]['Obj'][1:])


@pytest.mark.parametrize('name', FIXED)
def test_against_the_multiprecision_fixture(nagp_lib, name):
    f = fixture()
    fixed_parts(name, ref.fixed_case(name), {k: f['%s_%s' % (name, k)] for k in ('d', 'Av', 'Varx', 'Obj')})


@pytest.mark.parametrize('name', SIZES)
def test_every_code_path_of_the_transforms(nagp_lib, name):
    """Tx = 32 (idle threads), 512 (a leading radix-2 pass), 4096 (the largest single-workgroup transform; T = 3000 and T = Tx), 8192
    (N1 = 2) and 16384 (N1 = 4) on the inputs of the stable cases, with a drawn v and three drawn pairs, against the extended-precision
    evaluation under the rule"""
    c = dict(ref.stable_case(name)); rng = np.random.default_rng(900 + c['Tx'])
    c.update(v=rng.standard_normal(c['Tx']), xv=rng.standard_normal((3, c['Tx'])) / np.sqrt(c['Tx']), lmb=np.array([3.0, 0.0, -0.2]))
    d = ref.hessian(c['x'], c['y'], c['varc'], c['vary'], ext=True); hs = ref.hhalf(c['len'], c['Tx'], c['varx'], ext=True)
    want = dict(d=d.astype(float), Av=ref.apply(c['v'], d, hs, ext=True).astype(float), Varx=ref.varx_from(c['xv'], c['lmb'], hs, c['varx'], ext=True).astype(float),
                Obj=ref.obj_terms(c['x'], c['y'], c['len'], c['varx'], c['mux'], c['varc'], c['vary'], c['lmb'], ext=True).astype(float))
    fixed_parts(name, c, want)


def eig_checks(tag, c, got, run, selfdev, Varx, log=True):
    """the rule of the Lanczos run: got = the device's dict for one problem (lmb (nconv,), xv (nconv, Tx) or None, steps, reorths, nconv)"""
    counts = (got['steps'], got['reorths'], got['nconv'])
    e_l = ref.dist(got['lmb'], run['lmb']) if run['nconv'] and counts == ref.counts(run) else 0.0
    e_v = ref.dist(Varx, run['Varx'])
    line = 'gppad-lap-parity %-28s counts %s (restatement %s)  lmb %.3e (bound %.3e)  Varx %.3e (bound %.3e)' % (
        tag, counts, ref.counts(run), e_l, FACTOR * max(selfdev[0], FLOOR), e_v, FACTOR * max(selfdev[1], FLOOR))
    print(line)
    if log:
        LINES.append(line)
    assert counts == ref.counts(run), (tag, counts, ref.counts(run))
    assert e_l <= FACTOR * max(selfdev[0], FLOOR) and e_l < TOL, (tag, e_l)
    assert e_v <= FACTOR * max(selfdev[1], FLOOR) and e_v < TOL, (tag, e_v)
    if got.get('xv') is not None and run['nconv']:
        res = ref.residuals(got, run['d'], run['hs'])
        print('gppad-lap-parity %-28s largest residual %.3e of the bound 2 tolconv anorm = %.3e' % (tag, np.max(res), 2 * ref.TOLCONV * run['anorm']))
        assert np.max(res) <= 2 * ref.TOLCONV * run['anorm'], (tag, res)


def one(r, p):
    n = int(r['nconv'][p])
    return dict(lmb=r['lmb'][p, :n].copy(), xv=r['xv'][p, :n].copy() if 'xv' in r else None, steps=int(r['steps'][p]), reorths=int(r['reorths'][p]), nconv=n)


@pytest.mark.parametrize('name', STABLE)
def test_the_eigen_solve_on_the_stable_cases(nagp_lib, name):
    """nagp_gppad_lap_eig and the Varx it leaves, on every stable case (jmax = 2 among them: nconv = 0, Varx = varx, Obj0 = 0; and the
    short length-scale that ends at jmax); Obj0 from the device's own lmb; the same call twice gives equal bits"""
    f = fixture(); c = ref.stable_case(name); run = clean(name)
    with handle(c, jmax=c['jmax']) as h:
        h.hess(c['x'], d=False)
        r = h.eig(c['nev'], c['vstart'], xv=True)
        V, neg = h.varx(); O = h.obj()[0]
        r2 = h.eig(c['nev'], c['vstart'], xv=True)
        assert all(np.array_equal(r[k], r2[k], equal_nan=True) for k in r) and np.array_equal(h.varx()[0], V)
        assert h.timings() > 0
    got = one(r, 0)
    assert r['status'][0] == 0 and np.all(np.isnan(r['lmb'][0, got['nconv']:])) and abs(r['anorm'][0] - run['anorm']) <= 1e-12 * run['anorm']
    eig_checks(name, c, got, run, f[name + '_selfdev'], V[0])
    assert neg[0] == 0
    want0 = -0.5 * float(np.sum(np.log(np.abs(1 + np.maximum(got['lmb'], 0))))) if got['nconv'] else 0.0
    assert abs(O[0] - want0) <= 1e-14 * max(abs(want0), 1.0)
    if got['nconv'] == 0:
        assert np.all(V[0] == c['varx']) and O[0] == 0.0


def three_problems():
    """the case s200_256 in the middle of the short length-scale (which runs to jmax) and a neighbour of its own"""
    a, b = ref.stable_case('s200_256_short'), ref.stable_case('s200_256')
    rng = np.random.default_rng(8)
    c = dict(b); c.update(x=b['x'][::-1].copy(), y=b['y'][::-1].copy() * 1.5, vstart=rng.standard_normal(256), varx=0.9, mux=0.1, varc=1.1, len=b['len'] * 1.2)
    return [a, b, c]


def batch_of(cs, jmax):
    st = lambda k: np.stack([np.asarray(c[k], float) for c in cs])
    return gl.GppadLapHandle(st('y'), cs[0]['Tx'], st('vary'), st('varx'), st('mux'), st('varc'), st('len'), jmax)


def solve_batch(cs, nev, jmax):
    with batch_of(cs, jmax) as h:
        d = h.hess(np.stack([c['x'] for c in cs]))
        Av = h.apply(np.stack([c['vstart'] for c in cs]))
        r = h.eig(nev, np.stack([c['vstart'] for c in cs]), xv=True)
        V, _ = h.varx(); O = h.obj()
    return d, Av, r, V, O


def test_a_problem_does_not_depend_on_its_batch_mates(nagp_lib):
    """three problems that stop at different steps in one lock-step batch: every one equals the same problem run alone, bit for bit"""
    cs = three_problems()
    d, Av, r, V, O = solve_batch(cs, 8, 16)
    assert len(set(r['steps'].tolist())) > 1, r['steps']
    for p, c in enumerate(cs):
        d1, Av1, r1, V1, O1 = solve_batch([c], 8, 16)
        assert np.array_equal(d[p], d1[0]) and np.array_equal(Av[p], Av1[0]) and np.array_equal(V[p], V1[0]) and np.array_equal(O[p], O1[0]), p
        for k in r:
            assert np.array_equal(r[k][p], r1[k][0], equal_nan=True), (p, k)
    eig_checks('batch of three, problem 1', cs[1], one(r, 1), clean('s200_256'), fixture()['s200_256_selfdev'], V[1], log=False)


def test_device_batches_are_bit_equal_to_one_batch(nagp_lib, monkeypatch):
    """NAGP_GPPAD_BUDGET_MB=1 (read behind NAGP_DEVELOPER, which tests/conftest.py sets): a problem at Tx = 2048, jmax = 16 takes
    8 ((2 x 16 + 2) x 2048 + 16^2 + 3 x 16 + 2 x 8 + 8) = 559 680 B of the per-solve buffers, so 1 MiB holds 1: the three problems run as three
    device batches; and one problem at Tx = 4096, jmax = 16 is beyond that budget (NAGP_EUNSUPPORTED, -2)"""
    rng = np.random.default_rng(12)
    cs = []
    for k in range(3):
        x = 0.2 * k + ref.se_draw(rng, 40.0, 2048); y = ref.GetAmp(x[:1500]) * rng.standard_normal(1500)
        cs.append(dict(T=1500, Tx=2048, x=x, y=y, vary=0.01 * (k + 1), varx=1.0 + 0.1 * k, mux=0.1 * k, varc=0.8, len=40.0 + 5 * k, vstart=rng.standard_normal(2048)))
    full = solve_batch(cs, 8, 16)
    monkeypatch.setenv('NAGP_GPPAD_BUDGET_MB', '1')
    cut = solve_batch(cs, 8, 16)
    for a, b in zip(full, cut):
        if isinstance(a, dict):
            assert all(np.array_equal(a[k], b[k], equal_nan=True) for k in a)
        else:
            assert np.array_equal(a, b)
    with pytest.raises(L.NagpError, match=r'\(-2\).*budget'):
        gl.GppadLapHandle(np.ones((1, 10)), 4096, 0.0, 1.0, 0.0, 1.0, 5.0, 16)


def test_a_resident_handle_against_fresh_ones(nagp_lib):
    """one handle that is given another point and another start in between returns, for the first point again, the bits of a fresh handle"""
    a, b = ref.stable_case('s200_256'), ref.stable_case('s200_256_short')
    fresh = solve_batch([a], 8, 16)
    with batch_of([a], 16) as h:
        for x, v in ((a['x'], a['vstart']), (b['x'], b['vstart'][::-1]), (a['x'], a['vstart'])):
            d = h.hess(x); r = h.eig(8, v, xv=True); V, _ = h.varx(); O = h.obj()
        with pytest.raises(L.NagpError, match='hess'):
            batch_of([a], 16).apply(a['vstart'])
    assert np.array_equal(d, fresh[0]) and np.array_equal(V, fresh[3]) and np.array_equal(O, fresh[4])
    assert all(np.array_equal(r[k], fresh[2][k], equal_nan=True) for k in r)


def selfdev_of(c, run):
    """the self-deviation of a solve that is not in the fixture, formed as tools/make_gppad_lap_fixture.py forms it; None: not a stable case"""
    dl = dv = 0.0
    for k in range(4):
        p = ref.solve(c, perturb=np.random.default_rng(7700 + k))
        if ref.counts(p) != ref.counts(run):
            return None
        if run['nconv']:
            dl = max(dl, ref.dist(p['lmb'], run['lmb'])); dv = max(dv, ref.dist(p['Varx'], run['Varx']))
    return dl, dv


def test_replay_of_every_laplace_solve(nagp_lib):
    """InferAmplitudeErrorBarsGPMAP (T = 1500, len = 16, nev = 16, tol = 3, Overlap = 1, NumIts = 20: 24 chunks of Tx = 128, the last one
    shorter), GetLaplaceObjGPPAD on the head of the same signal and two iterations of GetLenGradAscent (stretches of 208 and then fewer samples, two
    time-scales each), on the device with a recorder: every (x, vstart) the device was given goes through the restatement.  Where the restatement's own perturbed runs keep their counts (a stable solve, as in the fixture tool) the
    device is held to the rule of the stable cases with the self-deviation formed here; the terms Obj1 and Obj2 of every solve are held to
    the rule of the parts without decisions against the extended-precision evaluation.  Most solves must be stable ones."""
    y, _ = ref.g1.envelope_signal(REPLAY['T'], 32.0, 23)
    Params = dict(len=REPLAY['len'], varx=1.0, mux=0.0, varc=1.0, vary=0.0)
    rec = []
    a, x, Varx, Info = nagp.InferAmplitudeErrorBarsGPMAP(y, Params, REPLAY['opts'], rng=np.random.default_rng(5), record=rec)
    assert Info['TxCh'] == 128 and Info['NumChunks'] == 24 == len(rec) and np.all(np.isfinite(Varx)) and a.shape == x.shape == Varx.shape == (1500,)
    Obj = nagp.GetLaplaceObjGPPAD(y[:400], Params, dict(REPLAY['opts'], TCh=80, TxCh=128), rng=np.random.default_rng(6), record=rec)
    ell, InfoLL = nagp.GetLenGradAscent(REPLAY['len'], y, Params, nagp.LoadLearnLenGradAscentGPPADOpts(dict(REPLAY['opts'], NumItsLL=2)), rng=np.random.default_rng(7), record=rec)
    assert len(rec) == 33 and np.isfinite(Obj) and np.all(np.isfinite(InfoLL['ObjHist'])) and ell != REPLAY['len'] and InfoLL['Ts'][0, 1] - InfoLL['Ts'][0, 0] == 207
    stable = 0; worst = (0.0, 0.0)
    for n, (ch, r) in enumerate(rec):
        P = ch['Params']
        c = dict(x=ch['x'], y=ch['y'], vary=P['vary'], len=float(P['len']), varx=P['varx'], mux=P['mux'], varc=P['varc'], Tx=ch['Dims']['Tx'], nev=16, jmax=32, vstart=r['vstart'])
        run = ref.solve(c)
        ext = ref.obj_terms(c['x'], c['y'], c['len'], c['varx'], c['mux'], c['varc'], c['vary'], [], ext=True).astype(float)[1:]
        fw, rv = (ref.obj_terms(c['x'], c['y'], c['len'], c['varx'], c['mux'], c['varc'], c['vary'], [], reverse=q)[1:] for q in (False, True))
        e = ref.dist(r['Obj'][1:], ext); bound = bound_of(ref.dist(fw, ext), ref.dist(rv, ext))
        assert e < TOL and e <= bound, (n, e, bound)
        worst = max(worst, (e / bound, e))
        sd = selfdev_of(c, run)
        if sd is None:
            continue
        stable += 1
        eig_checks('replay %d' % n, c, dict(lmb=r['lmb'], steps=r['steps'], reorths=r['reorths'], nconv=r['nconv']), run, sd, r['Varx'], log=False)
    line = 'gppad-lap-parity %-28s %d of %d solves stable and within the rule; Obj1,Obj2 closest to its bound: %.3e (%.2f of the bound)' % (
        'replay', stable, len(rec), worst[1], worst[0])
    print(line); LINES.append(line); LINES.append('gppad-lap-parity replay GetLaplaceObjGPPAD(y[:400]) = %.17g' % Obj)
    assert stable >= len(rec) // 2


def test_FBGPMAPLearnLen_in_lock_step_is_bit_equal_to_one_channel_at_a_time(nagp_lib):
    """three channels with given parameters, the third with a time-scale (and so chunks) of its own, two iterations of the gradient
    ascent and the error bars (nout = 8) on the device in lock-step: every column equals FBGPMAPLearnLen on that channel alone with its
    child stream, bit for bit"""
    y, _ = ref.g1.envelope_signal(600, 24.0, 41)
    Y = np.stack([y, 0.5 * y[::-1], y * np.linspace(0.5, 2.0, y.size)], axis=1)
    P = dict(len=np.array([16.0, 16.0, 12.0]), varx=1.0, varc=np.array([1.0, 0.25, 1.5]), mux=0.0, vary=0.0)
    opts = dict(REPLAY['opts'], LearnLengths=1, NumItsLL=2)
    out = nagp.FBGPMAPLearnLen(Y, P, opts, nout=8, rng=np.random.default_rng(13))
    kids = np.random.default_rng(13).spawn(3)
    for d in range(3):
        one_ = nagp.FBGPMAPLearnLen(Y[:, d], dict(P, len=P['len'][d], varc=P['varc'][d]), opts, nout=8, rng=[kids[d]])
        for k in (0, 1, 2, 5, 6, 7):
            assert np.array_equal(out[k][:, d], one_[k][:, 0]), (d, k)
        assert out[3]['len'][d] == one_[3]['len'][0] != P['len'][d] and np.array_equal(out[4][d][1]['LenHist'], one_[4][0][1]['LenHist'])
        assert np.all(out[5][:, d] > 0) and np.all(out[5][:, d] <= 1.0) and np.all(out[7][:, d] <= out[0][:, d]) and np.all(out[0][:, d] <= out[6][:, d])
