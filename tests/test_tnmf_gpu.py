"""GPU (-m gpu): nagp_sebf_conv, nagp_sebf_fit_* and nagp_tnmf_* / nagp.tnmf -- the convolution of basis2SEGP.m and the objectives and
gradients of getObj_fitSE_basis_func.m, getObj_nmf_log_norm.m and getObj_nmf_log_norm_inf.m --, their resident forms and the drivers
fitSEGP_BF_many, tnmf_inf and tnmf on the device path, against the multi-precision fixture tests/golden/tnmf_multiprecision.npz and the
NumPy restatement tests/tnmf_ref.py (pinned to the fixture without a GPU in tests/test_tnmf_host.py).  Distances are the project's norm
max|d| / max|ref| per array.

The rule is that of tests/test_nmf_temp_gpu.py.  A device array must (1) be within TOL = 1e-7 and (2) be no more than 32 x as far from the
fixture as the forward float64 restatement is, with a floor of 1e-15 (the fixture is stored in float64).  Where the restatement with
every sum over t and over the taps formed in the opposite order is itself outside that bound, the order of the sums is what the distance
measures, and the bound widens to 32 x the larger of the two restatement distances -- never a figure taken from the device.  Every
measured line (device, forward, reverse, bound) is printed, and a run of the whole module writes them to profiles/r17_tnmf_parity.txt.

End to end (planted data of tests/tnmf_ref.py, T = 400, D = 6, K = 2, lenx = [10, 25], varx = [.5, 1], mux = [0, -.5], vary = 0.01):
fitSEGP_BF_many (50 line searches at tol = 9), tnmf_inf (the conversion, then 2 x 25 at tol = 11) and tnmf (the conversion, then 2 x 10),
each on the device and on the forward restatement.  The yardstick is the distance between the forward and the reverse restatement runs
in the last info.Obj, computed here (floor 1e-15); the device's last Obj must be within 32 x of it from the forward run and in any case
within 1e-6 relative.  Iteration counts are not compared."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nagp
from nagp import _lib as L
from nagp import tnmf as tn
import tnmf_ref as ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-7
FACTOR, FLOOR = 32.0, 1e-15
CASES = sorted(ref.CASES)
LINES = []
N_LINES = 7 * len(CASES) + 3                             # Y, and Obj, dObj of the three objectives, of every case; the last Obj of the three end-to-end runs


@functools.lru_cache(maxsize=None)
def fixture():
    return dict(np.load(os.path.join(ROOT, 'tests', 'golden', 'tnmf_multiprecision.npz')))


@functools.lru_cache(maxsize=None)
def restated(name, reverse):
    c = ref.case(name)
    fo = ref.fit_objective(c, reverse)
    l = ref.objective(c, True, reverse); i = ref.objective(c, False, reverse)
    return dict(Y=ref.basis2SEGP(c['X'], c['lenx'], c['varx'], c['tol'], reverse), fit_Obj=fo[0], fit_dObj=fo[1], l_Obj=l[0], l_dObj=l[1], i_Obj=i[0], i_dObj=i[1])


def bound_of(e_f, e_r):
    bound = FACTOR * max(e_f, FLOOR)
    if e_r > bound:                                      # the reverse-order restatement is itself outside: the order of the sums decides
        bound = FACTOR * max(e_f, e_r)
    return bound


def check(tag, got, want, fwd, rev):
    """both conditions of the module docstring, figures printed first"""
    e_gpu, e_f, e_r = ref.dist(got, want), ref.dist(fwd, want), ref.dist(rev, want)
    bound = bound_of(e_f, e_r)
    line = 'tnmf-parity %-24s device %.3e  forward %.3e  reverse %.3e  bound %.3e' % (tag, e_gpu, e_f, e_r, bound)
    print(line); LINES.append(line)
    assert e_gpu < TOL, (tag, e_gpu)
    assert e_gpu <= bound, (tag, e_gpu, e_f, e_r)


@pytest.fixture(scope='module', autouse=True)
def parity_file():
    yield
    if len(LINES) != N_LINES:                            # a partial run (-k) leaves the file alone
        return
    try:
        with open(os.path.join(ROOT, 'profiles', 'r17_tnmf_parity.txt'), 'w') as fh:
            fh.write('# tests/test_tnmf_gpu.py: distance to tests/golden/tnmf_multiprecision.npz (the end-to-end lines: of the last Obj to the forward\n'
                     '# restatement run; "forward" is then 0 and "reverse" the yardstick), max|d| / max|ref| per array: the device, the float64 restatement,\n'
                     '# the restatement with every sum over t and over the taps reversed, and the bound that held\n')
            fh.write('\n'.join(LINES) + '\n')
    except OSError:                                      # a read-only checkout: the figures are in the test output
        pass


def par(c):
    return c['lenx'], c['mux'], c['varx'], c['tol']


def device(c, learn, **kw):
    x = c['x'] if learn else c['x'][:c['T'] * c['K']]
    return nagp.tnmf_obj(x, c['A'], c['vary'], None if learn else c['W'], *par(c), **kw)


def device_fit(c, **kw):
    return nagp.sebf_fit_obj(c['X'].T, c['y'].T, c['lenx'], c['varx'], c['tol'], **kw)


@pytest.mark.parametrize('name', CASES)
def test_against_the_multiprecision_fixture(nagp_lib, name):
    f = fixture(); c = ref.case(name)
    fw, rv = restated(name, False), restated(name, True)
    want = lambda key: f['%s_%s' % (name, key)]
    Y = nagp.basis2SEGP(c['X'], c['lenx'], c['varx'], c['tol'])
    check(name + ' Y', Y, want('Y'), fw['Y'], rv['Y'])
    assert np.array_equal(nagp.basis2SEGP(c['X'], c['lenx'], c['varx'], c['tol']), Y)
    for k in range(c['K']):                                                  # a column alone: equal bits
        assert np.array_equal(nagp.basis2SEGP(c['X'][:, k], c['lenx'][k], c['varx'][k], c['tol']), Y[:, k])
    fO, fd = device_fit(c)
    check(name + ' fit Obj', fO, want('fit_Obj'), fw['fit_Obj'], rv['fit_Obj'])
    check(name + ' fit dObj', fd, want('fit_dObj'), fw['fit_dObj'], rv['fit_dObj'])
    assert np.array_equal(device_fit(c, grad=False), fO)
    with nagp.SebfFitHandle(c['y'].T, c['lenx'], c['varx'], c['tol']) as h:
        for _ in range(2):                                                   # the resident form: equal bits, also on its second evaluation
            Or, dr = h.eval(c['X'].T)
            assert np.array_equal(Or, fO) and np.array_equal(dr, fd)
    for learn, tag in ((True, 'l'), (False, 'i')):
        Obj, dObj = device(c, learn)
        check('%s %s Obj' % (name, tag), Obj, want(tag + '_Obj'), fw[tag + '_Obj'], rv[tag + '_Obj'])
        check('%s %s dObj' % (name, tag), dObj, want(tag + '_dObj'), fw[tag + '_dObj'], rv[tag + '_dObj'])
        Obj2, dObj2 = device(c, learn)
        assert Obj == Obj2 and np.array_equal(dObj, dObj2)                   # the same call twice: equal bits
        assert device(c, learn, grad=False) == Obj                           # dObj = NULL: the same Obj bits
        with nagp.TnmfHandle(c['A'], c['vary'], None if learn else c['W'], *par(c)) as h:
            x = c['x'] if learn else c['x'][:c['T'] * c['K']]
            Or, dr = h.eval(x)
            assert Or[0] == Obj and np.array_equal(dr[0], dObj)
            assert h.eval(x, grad=False)[0] == Obj
            Or, dr = h.eval(x)
            assert Or[0] == Obj and np.array_equal(dr[0], dObj)


def three_problems(c, learn):
    """the case in the middle of two neighbours with their own x (and their own W in the inference form)"""
    rng = np.random.default_rng(5)
    x0 = c['x'] if learn else c['x'][:c['T'] * c['K']]
    x = np.stack([x0[::-1].copy(), x0, x0 + 0.1 * rng.standard_normal(x0.size)])
    W = None if learn else np.stack([c['W'][::-1] + 0.5, c['W'], 2.0 * c['W']])
    return x, W


@pytest.mark.parametrize('learn', [True, False], ids=['learn', 'inf'])
@pytest.mark.parametrize('name', ['r20', 'w257', 'b1999', 'e2049'])
def test_a_problem_does_not_depend_on_its_batch_mates(nagp_lib, name, learn):
    c = ref.case(name)
    x, W = three_problems(c, learn)
    Ob, db = nagp.tnmf_obj(x, c['A'], c['vary'], W, *par(c))
    assert Ob.shape == (3,) and db.shape == x.shape
    alone = device(c, learn)
    assert Ob[1] == alone[0] and np.array_equal(db[1], alone[1])
    for p in (0, 2):
        Oa, da = nagp.tnmf_obj(x[p], c['A'], c['vary'], None if W is None else W[p], *par(c))
        assert Oa == Ob[p] and np.array_equal(da, db[p]), p
    assert np.array_equal(nagp.tnmf_obj(x, c['A'], c['vary'], W, *par(c), grad=False), Ob)


@pytest.mark.parametrize('learn', [True, False], ids=['learn', 'inf'])
def test_device_batches_are_bit_equal_to_one_batch(nagp_lib, monkeypatch, learn):
    """NAGP_SEBF_BUDGET_MB=1 (read behind NAGP_DEVELOPER, which tests/conftest.py sets).  b1999 is T = 1999, D = 7, K = 3, 8 workgroups of the
    row kernel.  In the learning form a problem takes 8 (4 x 6018 + 8 x (21 + 1) + 1) = 193 992 B of the per-evaluation buffers, in the
    inference form 8 (4 x 5997 + 8 + 1) = 191 976 B: 1 MiB holds 5 of either, so the three-problem batch repeated 4 times, 12 problems,
    runs as three device batches (5 + 5 + 2, each starting inside a repetition).  The fit and the primitive are cut the same way: a
    column of T = 1999 takes 8 (3 x 1999 + 1) = 47 984 B (21 per MiB) and 16 x 1999 = 31 984 B (32 per MiB), 36 columns here.  One problem
    of T = 70000, D = K = 1 takes 2 244 424 B and is beyond that budget (NAGP_EUNSUPPORTED, -2)."""
    c = ref.case('b1999')
    x, W = three_problems(c, learn)
    O3, d3 = nagp.tnmf_obj(x, c['A'], c['vary'], W, *par(c))
    rep = lambda a: None if a is None else np.tile(a, (4,) + (1,) * (a.ndim - 1))
    full = nagp.tnmf_obj(rep(x), c['A'], c['vary'], rep(W), *par(c))
    Z = np.tile(c['X'], (1, 12)); Yt = np.tile(c['y'], (1, 12)); lx = np.tile(c['lenx'], 12); vx = np.tile(c['varx'], 12)
    full_fit = nagp.sebf_fit_obj(Z.T, Yt.T, lx, vx, c['tol']); full_Y = nagp.basis2SEGP(Z, lx, vx, c['tol'])
    monkeypatch.setenv('NAGP_SEBF_BUDGET_MB', '1')
    cut = nagp.tnmf_obj(rep(x), c['A'], c['vary'], rep(W), *par(c))
    assert np.array_equal(full[0], cut[0]) and np.array_equal(full[1], cut[1])
    assert np.array_equal(cut[0], np.tile(O3, 4)) and np.array_equal(cut[1], np.tile(d3, (4, 1)))
    assert np.array_equal(nagp.tnmf_obj(rep(x), c['A'], c['vary'], rep(W), *par(c), grad=False), cut[0])
    cut_fit = nagp.sebf_fit_obj(Z.T, Yt.T, lx, vx, c['tol'])
    assert np.array_equal(cut_fit[0], full_fit[0]) and np.array_equal(cut_fit[1], full_fit[1])
    assert np.array_equal(nagp.basis2SEGP(Z, lx, vx, c['tol']), full_Y)
    with pytest.raises(L.NagpError, match=r'\(-2\).*budget'):
        nagp.tnmf_obj(np.zeros(70001), np.ones((70000, 1)), None, None, [1.0], [0.0], [1.0], 1.0)


@pytest.mark.parametrize('name', ['w257', 'r20'])
def test_the_convolution_is_self_adjoint(nagp_lib, name):
    """<conv(u), v> = <u, conv(v)> (the taps are symmetric) to 1e-12 relative, at tau < T (w257: 7, 80, 256) and tau > T (r20: 20, 287)"""
    c = ref.case(name)
    rng = np.random.default_rng(21)
    u = rng.standard_normal((c['T'], c['K'])); v = rng.standard_normal((c['T'], c['K']))
    cu = nagp.basis2SEGP(u, c['lenx'], c['varx'], c['tol']); cv = nagp.basis2SEGP(v, c['lenx'], c['varx'], c['tol'])
    for k in range(c['K']):
        a, b = float(cu[:, k] @ v[:, k]), float(u[:, k] @ cv[:, k])
        print('self-adjoint %s column %d: %.17g %.17g' % (name, k, a, b))
        assert abs(a - b) <= 1e-12 * abs(a)


def test_the_m_signatures_are_the_batched_call(nagp_lib):
    c = ref.case('r20')
    O, d = device(c, True)
    O2, d2 = nagp.getObj_nmf_log_norm(c['x'][:, None], c['A'], c['vary'], *par(c))
    assert O2 == O and np.array_equal(d2, d) and nagp.getObj_nmf_log_norm(c['x'], c['A'], c['vary'], *par(c), nout=1) == O
    O, d = device(c, False)
    O2, d2 = nagp.getObj_nmf_log_norm_inf(c['x'][:40], c['A'], c['W'], c['vary'], *par(c))
    assert O2 == O and np.array_equal(d2, d)
    fO, fd = device_fit(c)
    for k in range(c['K']):
        O2, d2 = nagp.getObj_fitSE_basis_func(c['X'][:, k:k + 1], c['y'][:, k], c['lenx'][k], c['varx'][k], c['tol'])
        assert O2 == fO[k] and np.array_equal(d2, fd[k])
        assert nagp.getObj_fitSE_basis_func(c['X'][:, k], c['y'][:, k], c['lenx'][k], c['varx'][k], c['tol'], nout=1) == fO[k]
    ms = np.zeros(3)
    device(c, True)
    assert L.lib().nagp_tnmf_timings(L.dptr(ms)) == 0 and np.all(ms > 0)
    A, H = nagp.randtnmf(c['W'], c['lenx'], c['mux'], c['varx'], 50, seed=4)
    X = np.random.default_rng(4).standard_normal((50, 2))
    assert A.shape == (50, 3) and np.array_equal(H, np.exp(nagp.basis2SEGP(X, c['lenx'], c['varx'], 20) + c['mux'][None, :])) and np.array_equal(A, H @ c['W'])


# ---------------------------------------------------------------------------------------------------------------- end to end
SEED = 4


def run_fit(evaluator=None):
    """the K conversions of the planted activations as one batch: 50 line searches at tol = 9 (the defaults but for numIts)"""
    A, W, H, vary, p = ref.planted(seed=SEED)
    ys = [np.log(H[:, k]) - p['mux'][k] for k in range(H.shape[1])]
    res = nagp.fitSEGP_BF_many(ys, p['lenx'], p['varx'], dict(numIts=50), seed=7, evaluator=evaluator)
    return [{'Obj': np.array([sum(i['Obj'][-1] for _, i in res)])}]


def run_inf(evaluator=None):
    """tnmf_inf with the true W from a flat H: the conversion (50 line searches at tol = 9), then 2 x 25 line searches at tol = 11"""
    A, W, H, vary, p = ref.planted(seed=SEED)
    return tn.tnmf_inf(A, W, np.full_like(H, np.mean(A)), p['lenx'], p['mux'], p['varx'], vary, dict(numIts=50, progress_chunk=25), seed=7, evaluator=evaluator, convert_opts=dict(numIts=50))


def run_tnmf(evaluator=None):
    """tnmf from a flat H and a seeded W: the conversion (50 line searches at tol = 9), then 2 x 10 line searches at tol = 11"""
    A, W, H, vary, p = ref.planted(seed=SEED)
    W0 = 0.5 + np.random.default_rng(12).random(W.shape)
    return tn.tnmf(A, W0, np.full_like(H, np.mean(A)), p['lenx'], p['mux'], p['varx'], vary, dict(numIts=20, progress_chunk=10), seed=7, evaluator=evaluator, convert_opts=dict(numIts=50))


@pytest.mark.parametrize('run', [run_fit, run_inf, run_tnmf], ids=['fitSEGP_BF_many', 'tnmf_inf', 'tnmf'])
def test_end_to_end_against_the_restatement_runs(nagp_lib, run):
    dev = run(None); fwd = run(ref.evaluator(False)); rev = run(ref.evaluator(True))
    last = lambda r: r[-1]['Obj'][-1]
    yard = max(abs(last(fwd) - last(rev)) / abs(last(fwd)), FLOOR)
    e = abs(last(dev) - last(fwd)) / abs(last(fwd))
    line = 'tnmf-parity %-24s device %.3e  forward %.3e  reverse %.3e  bound %.3e' % (run.__name__ + ' last Obj', e, 0.0, yard, min(FACTOR * yard, 1e-6))
    print(line); LINES.append(line)
    assert np.all(np.isfinite(dev[-1]['Obj']))
    assert e <= FACTOR * yard and e <= 1e-6, (e, yard)
