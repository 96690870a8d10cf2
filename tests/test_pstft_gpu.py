"""GPU (-m gpu): nagp_pstft_obj / nagp.pstft_obj -- the objective and gradient of unifying_prob_tf/get_Obj_pSTFT_{exp,matern32,
matern52,all}.m -- and the driver fit_probSTFT_SD on the device path, against the multi-precision fixture
tests/golden/pstft_multiprecision.npz and the NumPy restatement tests/pstft_ref.py (pinned to the fixture without a GPU in
tests/test_pstft_host.py).  Distances are the project's norm max|d| / max|ref| per array.

The rule is that of tests/test_slowfb_gpu.py and tests/test_nmf_gpu.py.  A device array must (1) be within TOL = 1e-7 and (2) be no
more than 32 x as far from the fixture as the forward float64 restatement is, with a floor of 1e-15 (the fixture is stored in
float64).  Where the restatement with every sum over the frequencies formed in the opposite order is itself outside that bound, the
order of the sums is what the distance measures, and the bound widens to 32 x the larger of the two restatement distances -- never a
figure taken from the device.  Every measured triple (device, forward, reverse) is printed, and a run of the whole module writes them
to profiles/r10_pstft_parity.txt.

End to end (test_fit_on_the_device_against_the_restatement): seed 11, T = 4000, D = 3, numLevels = 4, numIts = 5, minT = 100,
maxT = 400 as asked; on the CPU the forward-order and reverse-order restatement runs of that seed differ by at most 1.9e-12 (exp) and
6.6e-13 (matern72) in varx, lamx, om, Info.Objs and Info.likeUnReg, well inside 1e-7 / 32, with the same line-search branches
(Info.ins equal), so nothing had to be shrunk."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nagp
from nagp import _lib as L
import pstft_ref as ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-7
FACTOR, FLOOR = 32.0, 1e-15
CASES = sorted(ref.CASES)
CASE_FORMS = [(n, f) for n in CASES for f in ref.forms(n)]
LINES = []
N_LINES = 2 * len(CASE_FORMS) + 2 * 5          # Obj and dObj of every case and form, five arrays of the two end-to-end fits


@functools.lru_cache(maxsize=None)
def fixture():
    return dict(np.load(os.path.join(ROOT, 'tests', 'golden', 'pstft_multiprecision.npz')))


@functools.lru_cache(maxsize=None)
def restated(name, form, reverse):
    return ref.objective(ref.case(name), form, reverse=reverse)


def check(tag, got, want, fwd, rev):
    """both conditions of the module docstring, figures printed first"""
    e_gpu, e_f, e_r = ref.dist(got, want), ref.dist(fwd, want), ref.dist(rev, want)
    bound = FACTOR * max(e_f, FLOOR)
    if e_r > bound:                                  # the reverse-order restatement is itself outside: the order of the sums decides
        bound = FACTOR * max(e_f, e_r)
    line = 'pstft-parity %-26s device %.3e  forward %.3e  reverse %.3e  bound %.3e' % (tag, e_gpu, e_f, e_r, bound)
    print(line); LINES.append(line)
    assert e_gpu < TOL, (tag, e_gpu)
    assert e_gpu <= bound, (tag, e_gpu, e_f, e_r)


@pytest.fixture(scope='module', autouse=True)
def parity_file():
    yield
    if len(LINES) != N_LINES:                        # a partial run (-k) leaves the file alone
        return
    try:
        with open(os.path.join(ROOT, 'profiles', 'r10_pstft_parity.txt'), 'w') as fh:
            fh.write('# tests/test_pstft_gpu.py: distance to tests/golden/pstft_multiprecision.npz (the fits: to the forward restatement run),\n'
                     '# max|d| / max|ref| per array: the device, the float64 restatement, the restatement with the sums over the frequencies\n'
                     '# reversed, and the bound that held\n')
            fh.write('\n'.join(LINES) + '\n')
    except OSError:                                  # a read-only checkout: the figures are in the test output
        pass


def device(c, form, **kw):
    return nagp.pstft_obj(c['theta'], c['vary'], c['specTar'], c['minVar'], c['limOm'], c['limLam'], c['bet'], c['kernel'], form=form, **kw)


@pytest.mark.parametrize('name,form', CASE_FORMS)
def test_against_the_multiprecision_fixture(nagp_lib, name, form):
    f = fixture(); c = ref.case(name)
    Obj, dObj = device(c, form)
    fw, rv = restated(name, form, False), restated(name, form, True)
    tag = '%s form %d ' % (name, form)
    check(tag + 'Obj', Obj, f['%s_Obj_f%d' % (name, form)], fw[0], rv[0])
    check(tag + 'dObj', dObj, f['%s_dObj_f%d' % (name, form)], fw[1], rv[1])
    Obj2, dObj2 = device(c, form)
    assert Obj == Obj2 and np.array_equal(dObj, dObj2)                      # the same call twice: equal bits
    assert device(c, form, grad=False) == Obj                               # dObj = NULL: the same Obj bits
    if len(ref.forms(name)) == 2 and form == 1:                             # a kernel with a file of its own: f0 and f1 of the fixture are one
        O0, d0 = device(c, 0)                                               # number (tests/test_pstft_host.py), and the device has one code path
        assert O0 == Obj and np.array_equal(d0, dObj)


def three_problems(c):
    rng = np.random.default_rng(5)
    theta = np.stack([c['theta'] + 0.2 * rng.standard_normal(c['theta'].size), c['theta'], c['theta'] - 0.1])
    spec = np.stack([c['specTar'][::-1].copy(), c['specTar'], c['specTar'] * rng.exponential(1.0, c['N'])])
    return theta, spec, np.array([2 * c['vary'], c['vary'], 0.5 * c['vary']]), np.array([0.0, c['bet'], 750.0])


@pytest.mark.parametrize('name', ['n257', 'n1998', 'g65'])
def test_a_problem_does_not_depend_on_its_batch_mates(nagp_lib, name):
    """n_problems = 3 with shared and with per-problem specTar: problem 1 equals the same problem run alone, bit for bit, and the
    objective-only call gives the same Obj bits"""
    c = ref.case(name); form = ref.forms(name)[-1]
    theta, spec, vary, bet = three_problems(c)
    if c['vary'] == 0.0:
        vary = np.zeros(3)
    args = (c['minVar'], c['limOm'], c['limLam'])
    O1, d1 = device(c, form)
    Ob, db = nagp.pstft_obj(theta, vary, spec, *args, bet, c['kernel'], form=form)                    # per-problem specTar
    assert Ob.shape == (3,) and db.shape == (3, 3 * c['D'])
    assert Ob[1] == O1 and np.array_equal(db[1], d1)
    Os, ds = nagp.pstft_obj(theta, vary, c['specTar'], *args, bet, c['kernel'], form=form)            # shared specTar
    assert Os[1] == O1 and np.array_equal(ds[1], d1)
    for p in (0, 2):
        Oa, da = nagp.pstft_obj(theta[p], vary[p], spec[p], *args, bet[p], c['kernel'], form=form)
        assert Oa == Ob[p] and np.array_equal(da, db[p]), p
    assert np.array_equal(nagp.pstft_obj(theta, vary, spec, *args, bet, c['kernel'], form=form, grad=False), Ob)


def test_device_batches_are_bit_equal_to_one_batch(nagp_lib, monkeypatch):
    """NAGP_PSTFT_BUDGET_MB=1 (read behind NAGP_DEVELOPER, which tests/conftest.py sets): case n1998 (D = 12, 8 workgroups) with per-problem specTar takes
    8 (1998 + 8 * 38 + 72 + 3) = 19 016 B per problem and 8 * 60 + 4096 B per call, so 1 MiB holds 54 problems: 120 run as three
    device batches"""
    c = ref.case('n1998')
    theta, spec, vary, bet = three_problems(c)
    theta = np.tile(theta, (40, 1)); spec = np.tile(spec, (40, 1)); vary = np.tile(vary, 40); bet = np.tile(bet, 40)
    args = (c['minVar'], c['limOm'], c['limLam'])
    full = nagp.pstft_obj(theta, vary, spec, *args, bet, 'matern52')
    monkeypatch.setenv('NAGP_PSTFT_BUDGET_MB', '1')
    cut = nagp.pstft_obj(theta, vary, spec, *args, bet, 'matern52')
    assert np.array_equal(full[0], cut[0]) and np.array_equal(full[1], cut[1])
    assert np.array_equal(full[1][3:], np.tile(full[1][:3], (39, 1)))


def test_a_problem_beyond_the_memory_budget_is_unsupported(nagp_lib, monkeypatch):
    """one problem of N = 200 000 shared frequencies takes 1.6 MB: beyond a budget lowered to 1 MiB it is NAGP_EUNSUPPORTED (-2), and
    it runs under the budget of the header"""
    N = 200000
    theta = np.array([-1.0, 0.2, -1.0]); args = (1e-4, np.ones(N), [1e-3], [[0.0, np.pi]], [[0.0, 0.4]], 3.0, 'exp')
    assert np.isfinite(nagp.pstft_obj(theta, *args, grad=False))
    monkeypatch.setenv('NAGP_PSTFT_BUDGET_MB', '1')
    with pytest.raises(L.NagpError, match=r'\(-2\).*budget'):
        nagp.pstft_obj(theta, *args)


def test_get_Obj_wrappers_are_the_batched_call(nagp_lib):
    c = ref.case('n64'); a = (c['theta'][:, None], c['vary'], c['specTar'][:, None], c['minVar'], c['limOm'], c['limLam'], c['bet'])
    O, d = device(c, 0)
    O1, d1 = nagp.get_Obj_pSTFT_exp(*a)
    assert O1 == O and np.array_equal(d1, d) and nagp.get_Obj_pSTFT_exp(*a, None, nout=1) == O
    O2, d2 = nagp.get_Obj_pSTFT_all(*a, 'exp')
    assert (O2, list(d2)) == (device(c, 1)[0], list(device(c, 1)[1]))
    c = ref.case('n257'); a = (c['theta'], c['vary'], c['specTar'], c['minVar'], c['limOm'], c['limLam'], c['bet'])
    assert nagp.get_Obj_pSTFT_matern32(*a)[0] == device(c, 0)[0]
    c = dict(c, kernel='matern52')
    assert nagp.get_Obj_pSTFT_matern52(*a)[0] == device(c, 0)[0]
    with pytest.raises(L.NagpError, match=r'\(-2\)'):
        nagp.pstft_obj(c['theta'], c['vary'], c['specTar'], c['minVar'], c['limOm'], c['limLam'], c['bet'], 'matern72', form=0)


FIT_OPTS = dict(numLevels=4, numIts=5, minT=100, maxT=400)


@functools.lru_cache(maxsize=None)
def fit_signal():
    return ref.ar_signal(11, 4000)


@pytest.mark.parametrize('kernel', ['exp', 'matern72'])
def test_fit_on_the_device_against_the_restatement(nagp_lib, kernel):
    """fit_probSTFT_SD through the same driver with the device objective and with the restatement objective (module docstring)"""
    y = fit_signal()
    fw = nagp.fit_probSTFT_SD(y, 3, kernel, FIT_OPTS, evaluator=ref.evaluator(kernel))
    rv = nagp.fit_probSTFT_SD(y, 3, kernel, FIT_OPTS, evaluator=ref.evaluator(kernel, reverse=True))
    dv = nagp.fit_probSTFT_SD(y, 3, kernel, FIT_OPTS)
    assert np.array_equal(fw[3]['ins'], rv[3]['ins']) and np.array_equal(fw[3]['ins'], dv[3]['ins']) and len(dv[3]['ins']) == 4
    for tag, g, a, b in [('varx', dv[0], fw[0], rv[0]), ('lamx', dv[1], fw[1], rv[1]), ('om', dv[2], fw[2], rv[2]),
                         ('Objs', dv[3]['Objs'], fw[3]['Objs'], rv[3]['Objs']), ('likeUnReg', dv[3]['likeUnReg'], fw[3]['likeUnReg'], rv[3]['likeUnReg'])]:
        e_gpu, e_r = ref.dist(g, a), ref.dist(b, a)
        assert e_r < TOL / FACTOR, (tag, e_r)                               # the two float64 runs themselves
        bound = FACTOR * max(e_r, FLOOR)
        line = 'pstft-parity %-26s device %.3e  forward %.3e  reverse %.3e  bound %.3e' % ('fit %s %s' % (kernel, tag), e_gpu, 0.0, e_r, bound)
        print(line); LINES.append(line)
        assert e_gpu < TOL and e_gpu <= bound, (tag, e_gpu, e_r)
    assert abs(np.sum(dv[0] / (1 - dv[1] ** 2)) / np.var(y, ddof=1) - 1) < 1e-12


def test_fit_many_is_bit_equal_to_the_single_fits(nagp_lib):
    ys = [fit_signal()[:2000], ref.ar_signal(12, 2000)]
    opts = dict(numLevels=3, numIts=4, minT=100, maxT=300)
    many = nagp.fit_probSTFT_SD_many(ys, 3, 'matern72', opts)
    for y, m in zip(ys, many):
        s = nagp.fit_probSTFT_SD(y, 3, 'matern72', opts)
        for a, b in zip(s[:3], m[:3]):
            assert np.array_equal(a, b)
        for k in ('Objs', 'ins', 'likeUnReg'):
            assert np.array_equal(s[3][k], m[3][k]), k


def test_chain_from_a_waveform_to_W(nagp_lib):
    """the first 4000 samples of the committed speech_74 fixture: fit_probSTFT_SD (exp, D = 4, 3 levels) -> sort -> get_disc_model ->
    kernel_ss_probFB -> nmf_init(Z, 2, restarts=2, numIts=20): everything finite, W is 2 x 4"""
    from nagp.fastfb import get_disc_model
    z = np.load(os.path.join(ROOT, 'tests', 'golden', 'audio_speech_74.npz'))
    y = z['samples'][:4000].astype(float); y = y / np.std(y)
    D = 4
    varx, lamx, om, Info = nagp.fit_probSTFT_SD(y, D, 'exp', dict(numLevels=3, numIts=5, minT=100, maxT=400, bet=750, reassign=0))
    assert all(np.all(np.isfinite(v)) for v in (varx, lamx, om, Info['Objs'], Info['likeUnReg']))
    order = np.argsort(om)                                   # train_GTFNMF.m:57-59
    A, Q, H, Pinf, K, tau = get_disc_model(lamx[order], varx[order], om[order], D, 'exp')
    Z, = nagp.kernel_ss_probFB(y, A, Q, H, Pinf, K, 0, tau)
    assert Z.shape == (D, 4000) and np.all(np.isfinite(Z))
    W, Hn, info = nagp.nmf_init(Z, 2, restarts=2, numIts=20)
    assert W.shape == (2, D) and Hn.shape == (4000, 2) and np.all(np.isfinite(W)) and np.all(np.isfinite(Hn)) and np.all(np.isfinite(info['Obj']))
