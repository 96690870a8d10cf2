"""GPU (-m gpu): nagp_nmf_temp_obj / nagp.nmf_temp_obj -- the objectives and gradients of experiments/nmf/getObj_nmf_temp.m and
getObj_nmf_temp_inf.m -- its resident form and the drivers nmf_inf and nmf on the device path, against the multi-precision fixture
tests/golden/nmf_temp_multiprecision.npz and the NumPy restatement tests/nmf_temp_ref.py (pinned to the fixture without a GPU in
tests/test_nmf_temp_host.py).  Distances are the project's norm max|d| / max|ref| per array.

The rule is that of tests/test_segp_gpu.py.  A device array must (1) be within TOL = 1e-7 and (2) be no more than 32 x as far from the
fixture as the forward float64 restatement is, with a floor of 1e-15 (the fixture is stored in float64).  Where the restatement with
every sum over t formed in the opposite order is itself outside that bound, the order of the sums is what the distance measures, and the
bound widens to 32 x the larger of the two restatement distances -- never a figure taken from the device.  Every measured triple
(device, forward, reverse) is printed, and a run of the whole module writes them to profiles/r13_nmf_temp_parity.txt.

End to end (planted data, T = 400, D = 6, K = 2): nmf_inf with the inverse-gamma chain and 3 restarts as one batch (numIts = 100) and nmf
with the truncated-Gaussian chain (numIts = 60), each on the device and on the forward restatement.  The yardstick is the distance
between the forward and the reverse restatement runs in the last info.Obj, computed here (floor 1e-15); the device's last Obj must be
within 32 x of it from the forward run and in any case within 1e-6 relative.  Iteration counts are not compared."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nagp
from nagp import _lib as L
from nagp import nmf_temp as nt
import nmf_temp_ref as ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-7
FACTOR, FLOOR = 32.0, 1e-15
CASES = sorted(ref.CASES)
LINES = []
N_LINES = 2 * len(CASES) + 2                             # Obj and dObj of every case, the last Obj of the two end-to-end runs


@functools.lru_cache(maxsize=None)
def fixture():
    return dict(np.load(os.path.join(ROOT, 'tests', 'golden', 'nmf_temp_multiprecision.npz')))


@functools.lru_cache(maxsize=None)
def restated(name, reverse):
    return ref.objective(ref.case(name), reverse=reverse)


def bound_of(e_f, e_r):
    bound = FACTOR * max(e_f, FLOOR)
    if e_r > bound:                                      # the reverse-order restatement is itself outside: the order of the sums decides
        bound = FACTOR * max(e_f, e_r)
    return bound


def check(tag, got, want, fwd, rev):
    """both conditions of the module docstring, figures printed first"""
    e_gpu, e_f, e_r = ref.dist(got, want), ref.dist(fwd, want), ref.dist(rev, want)
    bound = bound_of(e_f, e_r)
    line = 'nmf-temp-parity %-24s device %.3e  forward %.3e  reverse %.3e  bound %.3e' % (tag, e_gpu, e_f, e_r, bound)
    print(line); LINES.append(line)
    assert e_gpu < TOL, (tag, e_gpu)
    assert e_gpu <= bound, (tag, e_gpu, e_f, e_r)


@pytest.fixture(scope='module', autouse=True)
def parity_file():
    yield
    if len(LINES) != N_LINES:                            # a partial run (-k) leaves the file alone
        return
    try:
        with open(os.path.join(ROOT, 'profiles', 'r13_nmf_temp_parity.txt'), 'w') as fh:
            fh.write('# tests/test_nmf_temp_gpu.py: distance to tests/golden/nmf_temp_multiprecision.npz (the end-to-end lines: of the last Obj to the forward\n'
                     '# restatement run; "forward" is then 0 and "reverse" the yardstick), max|d| / max|ref| per array: the device, the float64 restatement,\n'
                     '# the restatement with every sum over t reversed, and the bound that held\n')
            fh.write('\n'.join(LINES) + '\n')
    except OSError:                                      # a read-only checkout: the figures are in the test output
        pass


def device(c, **kw):
    return nagp.nmf_temp_obj(c['x'], c['A'], c['vary'], c['W'], c['prior'], c['muinf'], c['varinf'], c['lam'], **kw)


@pytest.mark.parametrize('name', CASES)
def test_against_the_multiprecision_fixture(nagp_lib, name):
    f = fixture(); c = ref.case(name)
    Obj, dObj = device(c)
    fw, rv = restated(name, False), restated(name, True)
    check(name + ' Obj', Obj, f[name + '_Obj'], fw[0], rv[0])
    check(name + ' dObj', dObj, f[name + '_dObj'], fw[1], rv[1])
    assert dObj.shape == c['x'].shape
    Obj2, dObj2 = device(c)
    assert Obj == Obj2 and np.array_equal(dObj, dObj2)                      # the same call twice: equal bits
    assert device(c, grad=False) == Obj                                     # dObj = NULL: the same Obj bits
    with nagp.NmfTempHandle(c['A'], c['vary'], c['W'], c['prior'], c['muinf'], c['varinf'], c['lam'], K=c['K']) as h:
        Or, dr = h.eval(c['x'])
        assert Or[0] == Obj and np.array_equal(dr[0], dObj)                 # the resident form: equal bits, also on its second evaluation
        assert h.eval(c['x'], grad=False)[0] == Obj
        Or, dr = h.eval(c['x'])
        assert Or[0] == Obj and np.array_equal(dr[0], dObj)


def three_problems(c):
    """the case in the middle of two neighbours with their own x (and their own W in the inference form)"""
    rng = np.random.default_rng(5)
    x = np.stack([c['x'][::-1].copy(), c['x'], c['x'] + 0.1 * rng.standard_normal(c['x'].size)])
    W = None if c['learn'] else np.stack([c['W'][::-1] + 0.5, c['W'], 2.0 * c['W']])
    return x, W


@pytest.mark.parametrize('name', ['r20_none_l', 't2_tg_i', 'w257_ig_l', 'm513_tg_l', 'b1999_tg_i', 'b1999_ig_i'])
def test_a_problem_does_not_depend_on_its_batch_mates(nagp_lib, name):
    """n_problems = 3: problem 1 equals the same problem run alone, bit for bit, so do its neighbours, and the objective-only call gives
    the same Obj bits"""
    c = ref.case(name)
    x, W = three_problems(c)
    par = (c['prior'], c['muinf'], c['varinf'], c['lam'])
    Ob, db = nagp.nmf_temp_obj(x, c['A'], c['vary'], W, *par)
    assert Ob.shape == (3,) and db.shape == x.shape
    alone = device(c)
    assert Ob[1] == alone[0] and np.array_equal(db[1], alone[1])
    for p in (0, 2):
        Oa, da = nagp.nmf_temp_obj(x[p], c['A'], c['vary'], None if W is None else W[p], *par)
        assert Oa == Ob[p] and np.array_equal(da, db[p]), p
    assert np.array_equal(nagp.nmf_temp_obj(x, c['A'], c['vary'], W, *par, grad=False), Ob)


@pytest.mark.parametrize('name', ['b1999_ig_l', 'b1999_tg_i'])
def test_device_batches_are_bit_equal_to_one_batch(nagp_lib, monkeypatch, name):
    """NAGP_NMFT_BUDGET_MB=1 (read behind NAGP_DEVELOPER, which tests/conftest.py sets).  T = 1999, D = 16, K = 3 is 8 workgroups.  In the
    learning form with the IG chain a problem takes 8 (2 x 6045 + 8 x (48 + 16) + 1) = 100 824 B of the per-evaluation buffers, so 1 MiB
    holds 10; in the inference form with the TG chain 8 (2 x 5997 + 8 x 13 + 1) = 96 792 B, 10 as well: the three-problem batch repeated
    4 times, 12 problems, runs as two device batches (10 + 2, the second starting inside a repetition).  One problem of T = 70000,
    D = K = 1 takes 1 124 408 B and is beyond that budget (NAGP_EUNSUPPORTED, -2)."""
    c = ref.case(name)
    x, W = three_problems(c)
    par = (c['prior'], c['muinf'], c['varinf'], c['lam'])
    O3, d3 = nagp.nmf_temp_obj(x, c['A'], c['vary'], W, *par)
    rep = lambda a: None if a is None else np.tile(a, (4,) + (1,) * (a.ndim - 1))
    full = nagp.nmf_temp_obj(rep(x), c['A'], c['vary'], rep(W), *par)
    monkeypatch.setenv('NAGP_NMFT_BUDGET_MB', '1')
    cut = nagp.nmf_temp_obj(rep(x), c['A'], c['vary'], rep(W), *par)
    assert np.array_equal(full[0], cut[0]) and np.array_equal(full[1], cut[1])
    assert np.array_equal(cut[0], np.tile(O3, 4)) and np.array_equal(cut[1], np.tile(d3, (4, 1)))
    assert np.array_equal(nagp.nmf_temp_obj(rep(x), c['A'], c['vary'], rep(W), *par, grad=False), cut[0])
    with pytest.raises(L.NagpError, match=r'\(-2\).*budget'):
        nagp.nmf_temp_obj(np.zeros(70001), np.ones((70000, 1)), None)


def test_the_m_signatures_are_the_batched_call(nagp_lib):
    c = ref.case('r20_ig_l'); ci = ref.case('r20_tg_i')
    O, d = device(c)
    O2, d2 = nagp.getObj_nmf_temp(c['x'][:, None], c['A'], c['vary'], c['muinf'], c['varinf'], c['lam'])
    assert O2 == O and np.array_equal(d2, d) and nagp.getObj_nmf_temp(c['x'], c['A'], c['vary'], c['muinf'], c['varinf'], c['lam'], nout=1) == O
    O, d = device(ci)
    O2, d2 = nagp.getObj_nmf_temp_inf(ci['x'], ci['A'], ci['W'], ci['vary'], ci['varinf'], ci['lam'])
    assert O2 == O and np.array_equal(d2, d)
    ms = np.zeros(1)
    assert L.lib().nagp_nmf_temp_timings(L.dptr(ms)) == 0 and ms[0] > 0


# ---------------------------------------------------------------------------------------------------------------- end to end
def run_inf(evaluator=None):
    """nmf_inf, IG chain, the true W, 3 restarts as one batch (the caller's flat H and two seeded draws), numIts = 100"""
    A, W, H, vary, par = ref.planted()
    rng = np.random.default_rng(11)
    inits = [np.exp(rng.standard_normal(H.shape)) for _ in range(2)]
    return nagp.nmf_inf(A, W, np.full_like(H, np.mean(A)), par['muinf'], par['varinf'], par['lam'], vary, dict(numIts=100, restarts=3), inits=inits,
                        evaluator=evaluator)


def run_nmf(evaluator=None):
    """nmf, TG chain, from a flat H and a seeded W, numIts = 60 in chunks of 20 (with the default progress_chunk = 1000 the .m's
    ceil(numIts / progress_chunk) chunks of progress_chunk would run 1000 line searches).  Measured on the CPU for seeds 12 .. 17: the
    forward and the reverse restatement runs end 1.0e-11 .. 1.2e-8 apart in the last Obj, 6.9e-10 for this seed"""
    A, W, H, vary, par = ref.planted()
    rng = np.random.default_rng(12)
    W0 = 0.5 + rng.random(W.shape)
    return nt.nmf(A, W0, np.full_like(H, np.mean(A)), [], par['varinf'], par['lam'], vary, dict(numIts=60, progress_chunk=20), evaluator=evaluator)


@pytest.mark.parametrize('run', [run_inf, run_nmf], ids=['nmf_inf', 'nmf'])
def test_end_to_end_against_the_restatement_runs(nagp_lib, run):
    dev = run(None); fwd = run(ref.evaluator(False)); rev = run(ref.evaluator(True))
    last = lambda r: r[-1]['Obj'][-1]
    yard = max(abs(last(fwd) - last(rev)) / abs(last(fwd)), FLOOR)
    e = abs(last(dev) - last(fwd)) / abs(last(fwd))
    line = 'nmf-temp-parity %-24s device %.3e  forward %.3e  reverse %.3e  bound %.3e' % (run.__name__ + ' last Obj', e, 0.0, yard, min(FACTOR * yard, 1e-6))
    print(line); LINES.append(line)
    assert np.all(np.isfinite(dev[-1]['Obj'])) and np.all(np.diff(dev[-1]['Obj']) <= 0)
    assert e <= FACTOR * yard and e <= 1e-6, (e, yard)
    if 'restart_Obj' in fwd[-1]:
        ro = np.sort(fwd[-1]['restart_Obj'])
        if (ro[1] - ro[0]) / abs(ro[0]) > yard:                             # the restarts' last Obj differ by more than the yardstick
            assert dev[-1]['restart'] == fwd[-1]['restart']
