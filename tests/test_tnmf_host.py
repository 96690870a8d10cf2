"""nagp_sebf_conv, nagp_sebf_fit_*, nagp_tnmf_* (basis2SEGP.m, getObj_fitSE_basis_func.m, getObj_nmf_log_norm.m, getObj_nmf_log_norm_inf.m) and
the host mirrors around them (nagp/tnmf.py), without a GPU: the yardstick -- tests/tnmf_ref.py against the multi-precision fixture
tests/golden/tnmf_multiprecision.npz --, the reference's own gradient check restated, the bookkeeping of fitSEGP_BF, tnmf_inf and tnmf on
the restatement objective, the exports and their binding, and the argument checks of include/nagp.h, which answer on a machine with no
device (they run before any device call).  Distances are the project's norm max|d| / max|ref| per array.

Bound of the restatement against the fixture: 1e-12, forward and reverse.  Measured on the CPU (tools/make_tnmf_fixture.py prints every
figure): every array within 8.0e-16 but the single gradient entry of the fit at T = 1 (2.1e-15: one subtraction)."""
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
from nagp import tnmf as tn
import tnmf_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EUNSUPPORTED = -1, -2
CASES = sorted(ref.CASES)
BOUND = 1e-12
KEYS = ('Y', 'fit_Obj', 'fit_dObj', 'l_Obj', 'l_dObj', 'i_Obj', 'i_dObj')
NAMES = {'nagp_sebf_conv', 'nagp_sebf_fit_obj', 'nagp_sebf_fit_create', 'nagp_sebf_fit_eval', 'nagp_sebf_fit_destroy', 'nagp_tnmf_obj', 'nagp_tnmf_create',
         'nagp_tnmf_eval', 'nagp_tnmf_destroy', 'nagp_tnmf_timings'}


@functools.lru_cache(maxsize=None)
def fixture():
    return dict(np.load(os.path.join(ROOT, 'tests', 'golden', 'tnmf_multiprecision.npz')))


@pytest.mark.parametrize('name', CASES)
def test_restatement_matches_the_multiprecision_fixture(name):
    f = fixture(); c = ref.case(name)
    assert np.array_equal([c['x'].sum(), c['A'].sum()], f[name + '_sums'])
    for reverse in (False, True):
        fo = ref.fit_objective(c, reverse)
        l = ref.objective(c, True, reverse); i = ref.objective(c, False, reverse)
        got = dict(Y=ref.basis2SEGP(c['X'], c['lenx'], c['varx'], c['tol'], reverse), fit_Obj=fo[0], fit_dObj=fo[1], l_Obj=l[0], l_dObj=l[1], i_Obj=i[0], i_dObj=i[1])
        e = {k: ref.dist(got[k], f['%s_%s' % (name, k)]) for k in KEYS}
        print('e_ref %s reverse %d: %s' % (name, reverse, '  '.join('%s %.2e' % kv for kv in e.items())))
        assert max(e.values()) <= BOUND, e
        assert got['l_dObj'].shape == c['x'].shape and got['i_dObj'].shape == (c['T'] * c['K'],) and got['Y'].shape == (c['T'], c['K'])
        assert ref.objective(c, True, reverse, grad=False) == l[0]


def test_fixture_covers_what_it_must():
    tau = lambda n: [ref.tau_of(l, ref.CASES[n][6]) for l in ref.CASES[n][3]]
    assert ref.CASES['r20'] == (20, 3, 2, [3, 45], [1, 2], [.1, .3], 9, True) and tau('r20') == [20, 287]        # test_getObj_nmf_log_norm.m:13-31
    assert ref.CASES['t1'][:3] == (1, 1, 1) and ref.CASES['t2'][0] == 2
    assert ref.CASES['w257'][0] == 257 and tau('w257') == [7, 80, 256]
    assert ref.CASES['m513'][:3] == (513, 5, 2) and tau('m513') == [257, 4] and ref.CASES['m513'][6] == 11
    assert ref.CASES['b1999'][:3] == (1999, 7, 3) and tau('b1999') == [39, 389, 778]
    assert ref.CASES['lim70'][:3] == (70, 64, 16) and tau('tol0') == [0, 0]
    assert sum(ref.case(n)['vary'] is None for n in CASES) == 1
    # T and tau one below, at and one above the tile length; tau, and the tap count 2 tau + 1, around the chunk length
    src = open(os.path.join(ROOT, 'nonstationary-audio-gp_amd', 'csrc', 'nagp_sebf_check.hpp')).read()
    assert re.search(r'SEBF_NT = 256;', src) and re.search(r'SEBF_R = 8;', src) and re.search(r'SEBF_C = 512;', src) and (ref.TILE, ref.CHUNK) == (256 * 8, 512)
    Ts = {ref.CASES[n][0] for n in CASES}; taus = {t for n in CASES for t in tau(n)}
    assert {ref.TILE - 1, ref.TILE, ref.TILE + 1} <= Ts and {ref.TILE - 1, ref.TILE, ref.TILE + 1} <= taus
    assert {ref.CHUNK - 1, ref.CHUNK, ref.CHUNK + 1} <= taus and {ref.CHUNK // 2 - 1, ref.CHUNK // 2} <= taus          # 511 and 513 taps
    f = fixture()
    assert set(f) == {'%s_%s' % (n, k) for n in CASES for k in KEYS + ('sums',)}                 # results (and two checksums) only
    for n in CASES:
        assert all(np.all(np.isfinite(f['%s_%s' % (n, k)])) for k in KEYS)
    w = ref.case('r20')['W']
    assert not np.allclose(w.sum(axis=1), 1.0)                                                   # a given W is not renormalised: the case can tell
    assert os.path.getsize(os.path.join(ROOT, 'tests', 'golden', 'tnmf_multiprecision.npz')) < 1 << 20


def checkgrad(f, x, delta=1e-5):
    """checkgrad.m: central differences on every coordinate, norm(dh - dy) / norm(dh + dy)"""
    _, dy = f(x)
    dh = np.zeros_like(dy)
    for j in range(x.size):
        xp = x.copy(); xp[j] += delta; xm = x.copy(); xm[j] -= delta
        dh[j] = (f(xp)[0] - f(xm)[0]) / (2 * delta)
    return np.linalg.norm(dh - dy) / np.linalg.norm(dh + dy)


@pytest.mark.parametrize('form', ['learn', 'inf', 'fit'])
def test_gradient_as_the_reference_checks_it(form):
    """nmf/tests/test_getObj_nmf_log_norm.m:33-38, test_getObj_nmf_log_norm_inf.m and toolsGP/tests/test_fitSEGP_BF.m restated: checkgrad
    with delta = 1e-5, within 1e-6 absolute, at the reference's shape and parameter values"""
    c = ref.case('r20')
    if form == 'fit':
        d = max(checkgrad(lambda z, k=k: ref.fit_obj(z, c['y'][:, k], c['lenx'][k], c['varx'][k], c['tol']), c['X'][:, k].copy()) for k in range(2))
    else:
        learn = form == 'learn'
        x = c['x'] if learn else c['x'][:40]
        d = checkgrad(lambda v: ref.obj(v, c['A'], c['vary'], None if learn else c['W'], c['lenx'], c['mux'], c['varx'], c['tol']), x.copy())
    print('checkgrad %s: %.2e' % (form, d))
    assert d < 1e-6


def test_fitSEGP_BF_reads_tol_as_the_m_does():
    """fitSEGP_BF.m:41-45: tol comes from opts only when opts has progress_chunk, and is then required; otherwise 9 -- whatever opts.tol says"""
    assert tn.fit_options(None) == (100, 50, 9) and tn.fit_options({}) == (100, 50, 9)
    assert tn.fit_options(dict(numIts=7)) == (7, 50, 9)
    assert tn.fit_options(dict(tol=13)) == (100, 50, 9)                                          # tol alone is ignored
    assert tn.fit_options(dict(progress_chunk=5, tol=13)) == (100, 5, 13)
    with pytest.raises(ValueError, match='opts.tol'):
        tn.fit_options(dict(progress_chunk=5))
    rec = []
    y = np.sin(np.arange(60) / 7.0)
    z, info = nagp.fitSEGP_BF(y, 5.0, 1.0, dict(tol=13, numIts=3), seed=1, evaluator=ref.evaluator(record=rec))
    assert rec[0]['kind'] == 'fit' and rec[0]['tol'] == 9 and rec[0]['n_problems'] == 1 and z.shape == (60,)
    assert info['it'].shape == (1,) and info['it'][0] > 3                                        # numIts = 3 still runs one whole chunk of 50
    z, info = nagp.fitSEGP_BF(y, 5.0, 1.0, dict(tol=13, numIts=7, progress_chunk=3), seed=1, evaluator=ref.evaluator(record=rec))
    assert rec[1]['tol'] == 13 and info['it'].shape == (3,) and np.all(info['it'] <= 3)          # ceil(7 / 3) chunks of 3
    a = nagp.fitSEGP_BF(y, 5.0, 1.0, dict(numIts=1, progress_chunk=2, tol=9), seed=5, evaluator=ref.evaluator())
    b = nagp.fitSEGP_BF(y, 5.0, 1.0, dict(numIts=1, progress_chunk=2, tol=9), seed=5, evaluator=ref.evaluator())
    assert np.array_equal(a[0], b[0])                                                            # the same seed gives the same run
    z0 = np.full(60, 0.01)
    c = nagp.fitSEGP_BF(y, 5.0, 1.0, dict(numIts=1, progress_chunk=1, tol=9), init=z0, evaluator=ref.evaluator())
    assert c[1]['Obj'][0] == ref.fit_obj(z0, y, 5.0, 1.0, 9)[0]                                  # the caller's start is where the search starts
    with pytest.raises(ValueError, match='init'):
        nagp.fitSEGP_BF_many([y, y], [5.0, 5.0], [1.0, 1.0], init=[z0])


PLANT = dict(T=120, D=4, K=2, seed=3)


def test_chunking_and_the_bookkeeping_of_the_drivers():
    A, W, H, vary, p = ref.planted(**PLANT)
    T, K = H.shape
    H0 = np.full_like(H, np.mean(A))
    rec = []
    Hn, info = tn.tnmf_inf(A, 2.0 * W, H0, p['lenx'], p['mux'], p['varx'], vary, dict(numIts=7, progress_chunk=3), seed=2, evaluator=ref.evaluator(record=rec))
    # the K conversions are ONE batch with the defaults of fitSEGP_BF (tol = 9, 2 chunks of 50), whatever the driver's opts say; then tol = 11
    assert [r['kind'] for r in rec] == ['fit', 'tnmf'] and rec[0]['n_problems'] == K and rec[0]['tol'] == 9 and rec[1]['tol'] == 11
    assert np.array_equal(rec[0]['lenx'], p['lenx']) and np.array_equal(rec[0]['varx'], p['varx'])
    assert np.array_equal(rec[1]['W'], (2.0 * W)[None]) and rec[1]['n_problems'] == 1              # W as given, never normalised
    assert Hn.shape == (T, K) and info['it'].shape == (3,) and np.all(info['it'] <= 3)           # ceil(7 / 3) chunks of 3 (tnmf_inf.m:73-74)
    assert info['Obj'].ndim == 1 and np.all(np.diff(info['Obj']) <= 0)
    rec = []
    Wn, Hn, info = tn.tnmf(A, 2.0 * W, H0, p['lenx'], p['mux'], p['varx'], vary, dict(numIts=4, progress_chunk=3, tol=7), seed=2, evaluator=ref.evaluator(record=rec))
    assert [r['kind'] for r in rec] == ['fit', 'tnmf'] and rec[0]['tol'] == 9 and rec[1]['tol'] == 7 and rec[1]['W'] is None
    assert np.array_equal(info['it'], [3, 3])                                                    # numIts = 4 in chunks of 3 is 2 x 3
    assert Wn.shape == W.shape and np.allclose(Wn.sum(axis=1), 1.0, rtol=1e-14) and Hn.shape == (T, K)       # tnmf.m:107-108
    # the defaults: tnmf 1000 in chunks of 100, tnmf_inf 100 in chunks of 25 -- numIts = 1 still runs one whole chunk
    assert tn.tnmf_inf(A, W, H0, p['lenx'], p['mux'], p['varx'], vary, dict(numIts=1), seed=2, evaluator=ref.evaluator(), convert_opts=dict(numIts=1))[1]['it'][0] > 1
    # H comes back as exp(conv(X) + mux) with the driver's tol, and an empty vary stands for zeros
    Hn, info = tn.tnmf_inf(A, W, H0, p['lenx'], p['mux'], p['varx'], [], dict(numIts=1, progress_chunk=1), seed=2, evaluator=ref.evaluator(),
                           convert_opts=dict(numIts=1, progress_chunk=1, tol=9))
    assert Hn.shape == (T, K) and np.all(Hn > 0) and info['it'].shape == (1,)
    with pytest.raises(ValueError):
        tn.tnmf_inf(A, W, H0, p['lenx'][:1], p['mux'], p['varx'], vary, evaluator=ref.evaluator())
    with pytest.raises(ValueError):
        tn.tnmf(A, W, H0[:-1], p['lenx'], p['mux'], p['varx'], vary, evaluator=ref.evaluator())


def test_the_conversion_fits_the_activations():
    """tnmf.m:61-72: the conversion fits y = log H(:, k) - mux(k).  The line searches only lower 1/2 sum dx^2 + 1/2 sum z^2, which at the start
    z = randn / 1000 is 1/2 sum y^2 to within the start's own size: afterwards sum dx^2 + sum z^2 < sum y^2, per column"""
    A, W, H, vary, p = ref.planted(**PLANT)
    X = tn._convert(H, p['lenx'], p['mux'], p['varx'], None, 3, ref.evaluator(), 0)
    assert X.shape == H.shape
    for k in range(H.shape[1]):
        y = np.log(H[:, k]) - p['mux'][k]
        dx = ref.conv1(X[:, k], p['lenx'][k], p['varx'][k], 9) - y
        assert dx @ dx + X[:, k] @ X[:, k] < y @ y


def test_forward_and_reverse_runs_agree_for_the_committed_seeds():
    """the yardstick of the GPU end-to-end test: for its seed and iteration counts the forward and the reverse restatement runs end
    within 1e-6 / 32 of each other in the last Obj (tests/test_tnmf_gpu.py computes the distance itself), and the last Obj of the two NMF
    runs is O(1)"""
    import test_tnmf_gpu as g
    for run in (g.run_fit, g.run_inf, g.run_tnmf):
        f = run(ref.evaluator(False)); r = run(ref.evaluator(True))
        lf = f[-1]['Obj'][-1]
        d = abs(lf - r[-1]['Obj'][-1]) / abs(lf)
        print('%s: last Obj %.4f, forward / reverse distance %.2e' % (run.__name__, lf, d))
        assert d < 1e-6 / 32
        assert run is g.run_fit or 0.5 < abs(lf) < 5


def test_the_refusals_of_nmf_temp_stay_and_the_module_is_not_shadowed():
    import types
    from nagp import nmf_temp as nt
    assert isinstance(nagp.tnmf, types.ModuleType) and callable(nagp.tnmf.tnmf) and callable(nagp.tnmf.tnmf_inf)
    with pytest.raises(NotImplementedError, match=re.escape('tnmf.m')):
        nt.tnmf()
    assert 'nagp.tnmf' in nt.__doc__
    for name in ('basis2SEGP', 'getObj_fitSE_basis_func', 'getObj_nmf_log_norm', 'getObj_nmf_log_norm_inf', 'tnmf_obj', 'TnmfHandle', 'fitSEGP_BF',
                 'fitSEGP_BF_many', 'randtnmf'):
        assert getattr(nagp, name) is getattr(tn, name)


def test_exported_and_bound():
    nagp.build()
    out = subprocess.run(['nm', '-D', '--defined-only', L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r' T (nagp_[a-z0-9_]+)', out))
    hdr = open(os.path.join(ROOT, 'include', 'nagp.h')).read()
    declared = set(re.findall(r'^(?:int|void) (nagp_(?:sebf|tnmf)_[a-z_]+)\(', hdr, re.M))
    assert declared == NAMES and {n for n in exported if re.match(r'nagp_(sebf|tnmf)_', n)} == NAMES and NAMES <= set(L.EXPORTS)
    assert re.search(r'^int nagp_tnmf_obj\(int32_t n_problems, int64_t T, int32_t D, int32_t K,$', hdr, re.M)
    assert re.search(r'^int nagp_tnmf_timings\(double\* ms /\* 3: forward conv, rows, adjoint conv \*/\);', hdr, re.M)
    lib = L.lib()
    arity = dict(nagp_sebf_conv=8, nagp_sebf_fit_obj=10, nagp_sebf_fit_create=8, nagp_sebf_fit_eval=4, nagp_sebf_fit_destroy=1, nagp_tnmf_obj=15,
                 nagp_tnmf_create=13, nagp_tnmf_eval=4, nagp_tnmf_destroy=1, nagp_tnmf_timings=1)
    for name, n in arity.items():
        proto = re.search(r'^(?:int|void) %s\((.*?)\);' % name, hdr, re.M | re.S).group(1)
        proto = re.sub(r'/\*.*?\*/', '', proto, flags=re.S)
        assert len(getattr(lib, name).argtypes) == n == proto.count(',') + 1, name
    ms = (C.c_double * 3)(-1.0, -1.0, -1.0)
    assert lib.nagp_tnmf_timings(ms) == 0 and min(ms) >= 0.0 and lib.nagp_tnmf_timings(None) == EINVAL


def call(P=1, T=5, D=3, K=2, x=True, A=None, vary=None, W=None, lenx=(2.0, 3.0), mux=(.1, .2), varx=(.5, .5), tol=9.0, Obj=True):
    f = lambda v: L.f64(np.asarray(v, float), 'C') if v is not None else None
    n = max(P, 1) * (max(T, 1) * max(K, 1) + max(K, 1) * max(D, 1))
    xx = f(np.zeros(n)) if x else None
    aa = f(np.ones(max(T, 1) * max(D, 1)) if A is None else A) if A is not False else None
    O = np.zeros(max(P, 1)); d = np.zeros(n)
    return L.lib().nagp_tnmf_obj(P, T, D, K, L.dptr(xx), L.dptr(aa), L.dptr(f(vary)), L.dptr(f(W)), L.dptr(f(lenx)), L.dptr(f(mux)), L.dptr(f(varx)), float(tol),
                                 L.dptr(O) if Obj else None, L.dptr(d), 0)


def test_argument_errors_answer_without_a_device(monkeypatch):
    nagp.build()
    err = lambda: L.lib().nagp_last_error()
    assert call(x=False) == EINVAL and call(A=False) == EINVAL and call(Obj=False) == EINVAL
    assert call(lenx=None) == EINVAL and call(mux=None) == EINVAL and call(varx=None) == EINVAL
    assert call(P=0) == EINVAL and call(D=0) == EINVAL and call(K=0) == EINVAL and call(T=0) == EINVAL
    assert call(D=65) == EUNSUPPORTED and b'at most 64' in err() and call(K=17) == EUNSUPPORTED and b'at most 16' in err()
    for bad in (np.nan, np.inf, -np.inf, -1e-9):
        a = np.ones(15); a[-1] = bad
        assert call(A=a) == EINVAL and call(vary=a) == EINVAL
        w = np.ones(6); w[-1] = bad
        assert call(W=w) == EINVAL
        assert call(varx=(.5, bad)) == EINVAL and b'varx[1]' in err() and call(tol=bad) == EINVAL and b'tol' in err()
    for bad in (np.nan, np.inf, -np.inf, 0.0, -1.0):
        assert call(lenx=(2.0, bad)) == EINVAL and b'lenx[1]' in err()
    for bad in (np.nan, np.inf, -np.inf):
        assert call(mux=(bad, .2)) == EINVAL and b'mux[0]' in err()
    w = np.ones(6); w[[1, 3, 5]] = 0.0
    assert call(W=w) == EINVAL and b'row 1 of W' in err()
    assert call(lenx=(2.0, 2.0 ** 30 * np.sqrt(2)), tol=1.0) == EUNSUPPORTED and b'int32' in err()
    h = C.c_void_p(1)
    assert L.lib().nagp_tnmf_create(C.byref(h), 1, 5, 3, 2, None, None, None, None, None, None, 9.0, 0) == EINVAL and not h.value
    assert L.lib().nagp_tnmf_eval(None, None, None, None) == EINVAL and L.lib().nagp_sebf_fit_eval(None, None, None, None) == EINVAL
    one = L.f64(np.ones(5), 'C'); two = L.f64(np.array([2.0]), 'C')
    assert L.lib().nagp_sebf_conv(1, 5, L.dptr(one), L.dptr(two), L.dptr(two), -1.0, L.dptr(one), 0) == EINVAL
    assert L.lib().nagp_sebf_fit_obj(1, 5, L.dptr(one), L.dptr(one), L.dptr(two), L.dptr(two), np.nan, L.dptr(one), None, 0) == EINVAL
    # one problem beyond the budget of the per-evaluation buffers (lowered to 1 MiB behind NAGP_DEVELOPER, which tests/conftest.py sets):
    # T = 70000, D = K = 1, learning form: 8 (4 * 70001 + 274 * (1 + 1) + 1) = 2 244 424 B
    monkeypatch.setenv('NAGP_SEBF_BUDGET_MB', '1')
    assert call(T=70000, D=1, K=1, lenx=(2.0,), mux=(0.0,), varx=(.5,)) == EUNSUPPORTED and b'budget' in err() and b'2244424' in err()


def test_binding_checks_its_arguments():
    c = ref.case('r20')
    p = (c['lenx'], c['mux'], c['varx'], c['tol'])
    for args in ((c['x'][:-1], c['A'], c['vary'], None) + p, (c['x'], c['A'], c['vary'][:-1], None) + p, (c['x'], c['A'][:, 0], c['vary'], None) + p,
                 (c['x'], c['A'], c['vary'], None, c['lenx'][:1], c['mux'], c['varx'], 9), (c['x'][:40], c['A'], c['vary'], np.ones((2, 4))) + p,
                 (c['x'], c['A'], c['vary'], np.ones((2, 3))) + p):
        with pytest.raises(ValueError):
            nagp.tnmf_obj(*args)
    with pytest.raises(ValueError):
        nagp.sebf_fit_obj(np.zeros(5), np.zeros(6), 2.0, 1.0, 9)
    with pytest.raises(ValueError):
        nagp.basis2SEGP(np.zeros((5, 2)), [1.0, 2.0, 3.0], [1.0, 1.0], 9)
    with pytest.raises(ValueError, match='rows'):
        nagp.TnmfHandle(c['A'], c['vary'], np.ones((3, 3)), *p)


def test_argument_checks_in_plain_c():
    """tests/c/abi_tnmf_errors.c: a stand-alone C program on exactly-sized heap blocks against libnagp_asan.so (the host code of the C ABI
    built with AddressSanitizer), on the CPU only: every invalid call returns its status and ASan reports nothing."""
    import tempfile
    lib = nagp.build(asan=True)
    clang = '/opt/rocm/lib/llvm/bin/clang'
    rt = glob.glob('/opt/rocm/lib/llvm/lib/clang/*/lib/linux') + glob.glob('/opt/rocm/lib/llvm/lib/clang/*/lib/x86_64-unknown-linux-gnu')
    with tempfile.TemporaryDirectory() as td:
        exe = os.path.join(td, 'abi_tnmf_errors')
        r = subprocess.run([clang, '-fsanitize=address', '-shared-libsan', '-g', '-O1', '-std=c99', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'include'),
                            '-o', exe, os.path.join(ROOT, 'tests', 'c', 'abi_tnmf_errors.c'), lib, '-lm', '-Wl,-rpath,/opt/rocm/lib',
                            '-Wl,-rpath-link,/opt/rocm/lib'] + ['-Wl,-rpath,' + d for d in rt], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        env = dict(os.environ, ASAN_OPTIONS='detect_leaks=0:abort_on_error=0:exitcode=66', LD_LIBRARY_PATH=':'.join(rt + [os.environ.get('LD_LIBRARY_PATH', '')]))
        r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
        assert r.returncode == 0 and 'all error paths returned their status' in r.stdout, r.stdout + r.stderr
        assert 'AddressSanitizer' not in r.stderr, r.stderr


def test_host_checks_as_a_stand_alone_program_under_the_sanitizers(tmp_path):
    """tools/sebf_host_check.cpp: csrc/nagp_sebf_check.hpp -- every check, the byte rules, tau and the taps -- with its own main under
    -fsanitize=address,undefined, on exactly-sized heap blocks; no device, nothing loaded into Python"""
    exe = str(tmp_path / 'sebf_host_check')
    r = subprocess.run(['c++', '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined', '-I',
                        os.path.join(ROOT, 'nonstationary-audio-gp_amd', 'csrc'), '-o', exe, os.path.join(ROOT, 'tools', 'sebf_host_check.cpp')],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=dict(os.environ, ASAN_OPTIONS='detect_leaks=1:exitcode=66'))
    assert r.returncode == 0 and 'all host checks returned their status' in r.stdout, r.stdout + r.stderr
    assert 'Sanitizer' not in r.stderr and 'runtime error' not in r.stderr, r.stderr
