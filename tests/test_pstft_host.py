"""nagp_pstft_obj (the objective of unifying_prob_tf/fit_probSTFT_SD.m: get_Obj_pSTFT_{exp,matern32,matern52,all}.m) and the host
mirrors around it, without a GPU: the yardstick -- tests/pstft_ref.py against the multi-precision fixture
tests/golden/pstft_multiprecision.npz --, welchMethod, freq2probSpec, minimize, the driver fit_probSTFT_SD on the restatement
objective, the export and its binding, and the argument checks of include/nagp.h, which answer on a machine with no device (they run
before any device call).  Distances are the project's norm max|d| / max|ref| per array."""
import ctypes as C
import functools
import glob
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nagp
from nagp import _lib as L
from nagp import pstft as ps
from nagp import ss
import pstft_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EUNSUPPORTED = -1, -2
CASES = sorted(ref.CASES)


@functools.lru_cache(maxsize=None)
def fixture():
    return dict(np.load(os.path.join(ROOT, 'tests', 'golden', 'pstft_multiprecision.npz')))


@pytest.mark.parametrize('name', CASES)
def test_restatement_matches_the_multiprecision_fixture(name):
    """e_ref per array: what the GPU tests measure the kernels against.  Bound 1e-12 on every case and form, both orders of the sums."""
    f = fixture(); c = ref.case(name)
    assert np.array_equal(c['theta'], f[name + '_theta']) and c['specTar'].sum() == f[name + '_sumSpec']
    for form in ref.forms(name):
        for reverse in (False, True):
            Obj, dObj = ref.objective(c, form, reverse=reverse)
            e = ref.dist(Obj, f['%s_Obj_f%d' % (name, form)]), ref.dist(dObj, f['%s_dObj_f%d' % (name, form)])
            print('e_ref %s form %d reverse %d: Obj %.2e dObj %.2e' % (name, form, reverse, e[0], e[1]))
            assert dObj.shape == (3 * c['D'],) and max(e) < 1e-12, e
            assert ref.objective(c, form, reverse=reverse, grad=False) == Obj


def test_fixture_covers_what_it_must():
    f = fixture()
    for k in ref.KERNELS:                                    # form 1 for all four kernels, form 0 for the three with a file
        assert any(ref.CASES[n][0] == k and 1 in ref.forms(n) for n in CASES)
        assert k == 'matern72' or any(ref.CASES[n][0] == k and 0 in ref.forms(n) for n in CASES)
    assert {ref.CASES[n][1] for n in CASES} >= {4, 5, 63, 64, 65, 255, 256, 257, 1998, 1999, 70001}
    assert {ref.CASES[n][2] for n in CASES} >= {1, 3, 12, 64}
    assert {ref.CASES[n][4] for n in CASES} >= {0.0, 750.0} and any(ref.CASES[n][3] == 0.0 for n in CASES)
    for n in CASES:                                          # where both forms are stored they are one number
        if len(ref.forms(n)) == 2:
            assert f[n + '_Obj_f0'] == f[n + '_Obj_f1'] and np.array_equal(f[n + '_dObj_f0'], f[n + '_dObj_f1'])
    c = ref.case('n255'); _, _, om, lam = ref.transforms(c['theta'], c['minVar'], c['limOm'], c['limLam'])
    assert np.pi - om[0] < 1e-12 and om[1] < 1e-12 and lam[2] < 1e-13 and 0.4 - lam[0] < 1e-13          # saturated sigmoids
    c = ref.case('n256'); _, _, om, _ = ref.transforms(c['theta'], c['minVar'], c['limOm'], c['limLam'])
    assert abs(om[0] - 1e-3) < 1e-12 and abs(np.pi - om[1] - 1e-3) < 1e-12


def test_generic_restatement_against_the_literal_solves():
    """the closed form of the generic file's solves against the solves themselves, in float64 (their accuracy bounds the agreement)"""
    for name in ('g64', 'n63'):
        c = ref.case(name)
        a = ref.generic_literal(c['kernel'], c['theta'], c['vary'], c['specTar'], c['minVar'], c['limOm'], c['limLam'], c['bet'])
        b = ref.objective(c, 1)
        assert ref.dist(a[0], b[0]) < 1e-10 and ref.dist(a[1], b[1]) < 1e-10


def test_matern72_state_space_derivatives():
    """cf_matern72_to_ss.m:134-150 written out"""
    s2, ell = 1.7, 0.6
    dF, dQc = ss.kernel_ss_derivs('matern72', s2, ell)
    want = np.array([196 / ell ** 5, 84 * np.sqrt(7) / ell ** 4, 84 / ell ** 3, 4 * np.sqrt(7) / ell ** 2])
    assert np.allclose(dF[3, :, 1], want, rtol=1e-14) and not dF[:3].any() and not dF[:, :, 0].any()
    assert np.allclose(dQc, [10976 * np.sqrt(7) / 5 / ell ** 7, -s2 * 76832 * np.sqrt(7) / 5 / ell ** 8], rtol=1e-14)
    for k in ('exp', 'matern32', 'matern52', 'matern72'):    # against a central difference of kernel_block
        h = 1e-6
        Fp, _, Qp, _ = ss.kernel_block(k, s2, ell + h); Fm, _, Qm, _ = ss.kernel_block(k, s2, ell - h)
        dF, dQc = ss.kernel_ss_derivs(k, s2, ell)
        assert np.allclose(dF[:, :, 1], (Fp - Fm) / (2 * h), rtol=1e-7, atol=1e-7) and np.isclose(dQc[1], (Qp - Qm) / (2 * h), rtol=1e-7)


def direct_welch(y, numFreq, ovLp):
    """O(n^2): the even extension of a chunk has the real transform y_0 + (-1)^k y_(Tc-1) + 2 sum_n y_n cos(2 pi k n / M), M = 2 (Tc - 1)"""
    T = y.size; Tc = numFreq; M = 2 * (Tc - 1)
    K = (T - ovLp) // (Tc - ovLp)
    k = np.arange(numFreq)[:, None]; n = np.arange(1, Tc - 1)[None, :]
    Cm = np.cos(2 * np.pi * k * n / M)
    pg = np.zeros(numFreq)
    for j in range(K):
        yc = y[(Tc - ovLp) * j:(Tc - ovLp) * j + Tc]
        Z = yc[0] + (-1.0) ** k[:, 0] * yc[-1] + 2 * Cm @ yc[1:-1]
        pg += Z ** 2 / M ** 2 / K
    return pg


@pytest.mark.parametrize('T,numFreq,ovLp', [(50, 7, 0), (50, 8, 3), (1000, 100, 10)])
def test_welchMethod_against_the_direct_cosine_sum(T, numFreq, ovLp):
    y = np.random.default_rng(T + numFreq).standard_normal(T)
    pg, varpg = nagp.welchMethod(y, numFreq, ovLp)
    assert pg.shape == (numFreq,) and varpg.shape == (numFreq,) and np.all(varpg >= -1e-18)
    assert ref.dist(pg, direct_welch(y, numFreq, ovLp)) < 1e-12
    if T == 1000:      # "mean(y.^2) = 2*sum(pg)", approximately (the .m's docstring: the chunks are windowed versions of the signal)
        assert abs(2 * pg.sum() / np.mean(y ** 2) - 1) < 0.1
    assert np.isnan(nagp.welchMethod(y, 5, 6)[0])            # :36-41


def test_freq2probSpec_spot_values():
    om, lamx, varx = nagp.freq2probSpec(np.array([0.1, 0.25]), np.array([0.0, 0.25]), np.array([2.0, 3.0]))
    assert np.allclose(om, [0.2 * np.pi, 0.5 * np.pi], rtol=1e-15)
    assert np.allclose(lamx, [1.0, 2 - np.sqrt(3)], rtol=1e-15)             # cos = 1: 2 - 1 - sqrt(0); cos = 0: 2 - sqrt(3)
    assert np.allclose(varx, [0.0, 3 * (1 - (2 - np.sqrt(3)) ** 2)], atol=1e-15)


def test_minimize_invariants():
    rng = np.random.default_rng(3); Q = rng.standard_normal((5, 5)); A = Q @ Q.T + 0.5 * np.eye(5); m = rng.standard_normal(5)
    n_eval = [0]

    def f(x):
        n_eval[0] += 1
        return 0.5 * (x - m) @ A @ (x - m), A @ (x - m)
    X, fX, i = nagp.minimize(np.zeros(5), f, 100)
    import scipy.optimize as so
    r = so.minimize(lambda x: f(x)[0], np.zeros(5), jac=lambda x: f(x)[1], method='CG')
    d_ours, d_scipy = np.linalg.norm(X - m), np.linalg.norm(r.x - m)
    print('distance to the minimiser: minimize %.3e, scipy CG %.3e' % (d_ours, d_scipy))
    assert d_ours <= 10 * d_scipy
    assert np.all(np.diff(fX) <= 0) and fX[0] == f(np.zeros(5))[0] and i <= 100 and len(fX) - 1 <= i
    for length in (1, 3, 7):
        X, fX, i = nagp.minimize(np.zeros(5), f, length)
        assert i <= length and len(fX) - 1 <= length and np.all(np.diff(fX) <= 0)
    for length in (-1, -4, -9):
        n_eval[0] = 0
        X, fX, i = nagp.minimize(np.zeros(5), f, length)
        assert n_eval[0] <= -length and np.all(np.diff(fX) <= 0)
    X0 = np.array([[1.0, 2.0], [3.0, 4.0]])
    X, fX, i = nagp.minimize(X0, lambda x: (1.0, np.zeros((2, 2))), 5)      # a zero gradient returns the start, in the caller's shape
    assert np.array_equal(X, X0) and np.array_equal(fX, [1.0])
    assert (ps.INT, ps.EXT, ps.MAX, ps.RATIO, ps.SIG, ps.RHO) == (0.1, 3.0, 20, 10.0, 0.1, 0.05)


OPTS = dict(numLevels=3, numIts=4, minT=60, maxT=200)


@pytest.mark.parametrize('kernel', ['exp', 'matern72'])
def test_fit_on_the_restatement_objective(kernel):
    y = ref.ar_signal(5, 1500) * 3.0 + 0.7
    varx, lamx, om, Info = nagp.fit_probSTFT_SD(y, 3, kernel, OPTS, evaluator=ref.evaluator(kernel))
    assert abs(np.sum(varx / (1 - lamx ** 2)) / np.var(y, ddof=1) - 1) < 1e-12
    assert len(Info['ins']) == 3 and Info['likeUnReg'].shape == (3,) and np.all(np.isfinite(Info['likeUnReg'])) and 'likeHO' not in Info
    assert np.all(Info['ins'] <= 4) and Info['nObjs'].sum() == Info['Objs'].size and np.all(Info['nObjs'] <= Info['ins'] + 1)
    for seg in np.split(Info['Objs'], np.cumsum(Info['nObjs'])[:-1]):        # non-increasing inside each level
        assert seg.size >= 1 and np.all(np.diff(seg) <= 0)
    assert np.all((om > 0) & (om < np.pi)) and np.all((lamx > 0) & (lamx < 0.4))


def test_fit_mirror_follows_the_signal_length_and_held_out_likelihood():
    """odd T: specTar has 2 numFreq - 1 entries whatever numFreq is; with opts.yHO the held-out objective is there, mirrored by THO"""
    y = ref.ar_signal(6, 1201)                              # odd T: the other mirror
    sizes = []
    ev = ref.evaluator('exp')

    def spy(theta, vary, specTar, *a):
        sizes.append(specTar.size)
        return ev(theta, vary, specTar, *a)
    varx, lamx, om, Info = nagp.fit_probSTFT_SD(y, 2, 'exp', dict(OPTS, yHO=y[:400]), evaluator=spy)
    assert Info['likeHO'].shape == (3,) and np.all(np.isfinite(Info['likeHO'])) and len(Info['ins']) == 3
    assert 2 * 1201 - 1 in sizes and 2 * 400 - 2 in sizes and 2 * 60 - 1 in sizes        # parity of T (and of THO), not of numFreq
    for seg in np.split(Info['Objs'], np.cumsum(Info['nObjs'])[:-1]):
        assert np.all(np.diff(seg) <= 0)


@pytest.mark.parametrize('kernel', ['matern32', 'matern52'])
def test_fit_theta_init_branch(kernel):
    y = ref.ar_signal(7, 1000)
    ti = np.concatenate([[0.05, 0.03], [0.02, 0.04], [0.4, 1.2]])           # cvar, lam, om
    varx, lamx, om, Info = nagp.fit_probSTFT_SD(y, 2, kernel, dict(OPTS, theta_init=ti, bandwidth_lim=3), evaluator=ref.evaluator(kernel))
    c = np.sqrt(3.0) if kernel == 'matern32' else np.sqrt(5.0)
    assert np.all(lamx < ti[2:4] * c * 3) and np.all(lamx > 0) and len(Info['ins']) == 3
    assert abs(np.sum(varx / (1 - lamx ** 2)) / np.var(y, ddof=1) - 1) < 1e-12


def test_fit_refusals():
    y = ref.ar_signal(8, 500)
    ev = ref.evaluator('exp')
    with pytest.raises(NotImplementedError):
        nagp.fit_probSTFT_SD(y, 2, 'exp', dict(OPTS, reassign=1), evaluator=ev)
    with pytest.raises(ValueError, match='outside its limits'):
        nagp.fit_probSTFT_SD(y, 2, 'exp', dict(OPTS, theta_init=np.array([0.05, 0.03, 0.02, 0.04, 0.4, 3.5])), evaluator=ev)       # om > pi
    with pytest.raises(ValueError, match='outside its limits'):
        nagp.fit_probSTFT_SD(y, 2, 'exp', dict(OPTS, theta_init=np.array([0.05, 0.03, 0.02, 0.04, 0.4, 1.0]), bandwidth_lim=0.5), evaluator=ev)
    with pytest.raises(ValueError, match='unsupported kernel'):
        nagp.fit_probSTFT_SD(y, 2, 'se', OPTS, evaluator=ev)
    nagp.fit_probSTFT_SD(y, 2, 'exp', dict(OPTS, reassign=0, verbose=1), evaluator=ev)     # what every driver sets


def test_exported_and_bound():
    nagp.build()
    out = subprocess.run(['nm', '-D', '--defined-only', L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert {'nagp_pstft_obj', 'nagp_pstft_timings'} <= set(re.findall(r' T (nagp_[a-z0-9_]+)', out))
    assert 'nagp_pstft_obj' in L.EXPORTS
    hdr = open(os.path.join(ROOT, 'include', 'nagp.h')).read()
    assert re.search(r'^int nagp_pstft_obj\(int32_t n_problems, int32_t kernel, int32_t form /\* 0 closed, 1 generic \*/, int32_t D, int64_t N,', hdr, re.M)
    fn = L.lib().nagp_pstft_obj
    assert len(fn.argtypes) == 16 and fn.restype is C.c_int
    for name in ('pstft_obj', 'get_Obj_pSTFT_exp', 'get_Obj_pSTFT_matern32', 'get_Obj_pSTFT_matern52', 'get_Obj_pSTFT_all', 'welchMethod',
                 'freq2probSpec', 'minimize', 'fit_probSTFT_SD', 'fit_probSTFT_SD_many'):
        assert getattr(nagp, name) is getattr(ps, name)


def call(c, kernel=0, form=0, D=None, N=None, stride=0, **over):
    a = {k: L.f64(np.asarray(v, float), 'C') for k, v in dict(theta=c['theta'], specTar=c['specTar'], vary=[c['vary']], bet=[c['bet']],
                                                              minVar=c['minVar']).items()}
    a['limOm'] = L.f64(c['limOm']); a['limLam'] = L.f64(c['limLam'])
    for k, v in over.items():
        a[k] = L.f64(np.asarray(v, float), 'F' if k.startswith('lim') else 'C')
    Obj = np.zeros(1); dObj = np.zeros(3 * c['D'])
    return L.lib().nagp_pstft_obj(1, kernel, form, c['D'] if D is None else D, c['N'] if N is None else N, L.dptr(a['theta']), L.dptr(a['specTar']),
                                  stride, L.dptr(a['vary']), L.dptr(a['bet']), L.dptr(a['minVar']), L.dptr(a['limOm']), L.dptr(a['limLam']),
                                  L.dptr(Obj), L.dptr(dObj), 0)


def test_argument_errors_answer_without_a_device():
    nagp.build()
    c = ref.case('n64')
    big = dict(theta=np.zeros(3 * 65), minVar=np.ones(65), limOm=np.tile([0.0, 3.0], (65, 1)), limLam=np.tile([0.0, 0.4], (65, 1)))
    assert call(c, D=65, **big) == EUNSUPPORTED and b'64' in L.lib().nagp_last_error()
    assert call(c, kernel=3, form=0) == EUNSUPPORTED and b'matern72' in L.lib().nagp_last_error()
    assert call(c, kernel=4, form=1) == EUNSUPPORTED and call(c, kernel=-1) == EUNSUPPORTED
    assert call(c, N=3) == EINVAL and call(c, form=2) == EINVAL and call(c, stride=5) == EINVAL
    for bad in (np.nan, np.inf, -1e-9):
        s = c['specTar'].copy(); s[-1] = bad
        assert call(c, specTar=s) == EINVAL
        assert call(c, vary=[bad]) == EINVAL
    t = c['theta'].copy(); t[4] = np.nan
    assert call(c, theta=t) == EINVAL and call(c, bet=[np.inf]) == EINVAL
    lo = c['limOm'].copy(); lo[1, 1] = lo[1, 0]
    assert call(c, limOm=lo) == EINVAL
    ll = c['limLam'].copy(); ll[2, 1] = ll[2, 0] - 0.01
    assert call(c, limLam=ll) == EINVAL
    ll = c['limLam'].copy(); ll[0, 1] = 1.2
    assert call(c, limLam=ll) == EINVAL and b'[0, 1]' in L.lib().nagp_last_error()
    # vary = 0 (case n64) is fine with lam bounded away from 0, and refused once every lam has saturated onto a lower limit of 0
    t = c['theta'].copy(); t[6:] = -800.0
    ll = c['limLam'].copy(); ll[:, 0] = 0.0
    assert call(c, theta=t, limLam=ll) == EINVAL and b'vary = 0' in L.lib().nagp_last_error()
    with pytest.raises(ValueError):
        nagp.pstft_obj(c['theta'][:-1], c['vary'], c['specTar'], c['minVar'], c['limOm'], c['limLam'], c['bet'], 'exp')
    with pytest.raises(ValueError, match='unsupported kernel'):
        nagp.get_Obj_pSTFT_all(c['theta'], c['vary'], c['specTar'], c['minVar'], c['limOm'], c['limLam'], c['bet'], 'se')


def test_argument_checks_under_the_address_sanitizer():
    """tests/c/abi_pstft_errors.c: a stand-alone C program on exactly-sized heap blocks against libnagp_asan.so (the host code of the C
    ABI built with AddressSanitizer), on the CPU only: every invalid call returns its status and ASan reports nothing."""
    import tempfile
    lib = nagp.build(asan=True)
    clang = '/opt/rocm/lib/llvm/bin/clang'
    rt = glob.glob('/opt/rocm/lib/llvm/lib/clang/*/lib/linux') + glob.glob('/opt/rocm/lib/llvm/lib/clang/*/lib/x86_64-unknown-linux-gnu')
    with tempfile.TemporaryDirectory() as td:
        exe = os.path.join(td, 'abi_pstft_errors')
        r = subprocess.run([clang, '-fsanitize=address', '-shared-libsan', '-g', '-O1', '-std=c99', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'include'),
                            '-o', exe, os.path.join(ROOT, 'tests', 'c', 'abi_pstft_errors.c'), lib, '-lm', '-Wl,-rpath,/opt/rocm/lib',
                            '-Wl,-rpath-link,/opt/rocm/lib'] + ['-Wl,-rpath,' + d for d in rt], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        env = dict(os.environ, ASAN_OPTIONS='detect_leaks=0:abort_on_error=0:exitcode=66', LD_LIBRARY_PATH=':'.join(rt + [os.environ.get('LD_LIBRARY_PATH', '')]))
        r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
        assert r.returncode == 0 and 'all error paths returned their status' in r.stdout, r.stdout + r.stderr
        assert 'AddressSanitizer' not in r.stderr, r.stderr
