"""nagp_gppad_cas_obj (the objective of experiments/gppad/Cascade/MAPGPCasFast.m: GetObjCasGPFAST.m) and the host drivers around it, without
a GPU: the yardstick -- tests/gppad_cas_ref.py against the multi-precision fixture tests/golden/gppad_cas_multiprecision.npz --, its
gradient against central differences, the drivers CasGPMAP, FBCasGPMAP and MAPGPCasFast on the restatement objective, the exports and
their binding, the argument checks of include/nagp.h (they run before any device call) from Python and from a plain-C program, and the
kernel bodies run on the host under the sanitizers.  Distances are the project's norm max|d| / max|ref| per array.

Bound of the restatement against the fixture: 1e-7, for the reason tests/test_gppad_host.py gives -- the same division by c down to 1e-6;
measured on the CPU: Obj within 9.2e-15, dObj within 3.9e-12."""
import ctypes as C
import functools
import glob
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nagp
from nagp import _lib as L
from nagp import gppad_cas as gc
import gppad_cas_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EUNSUPPORTED = -1, -2
CASES = sorted(ref.CASES)


@functools.lru_cache(maxsize=None)
def fixture():
    return dict(np.load(os.path.join(ROOT, 'tests', 'golden', 'gppad_cas_multiprecision.npz')))


@pytest.mark.parametrize('name', CASES)
def test_restatement_matches_the_multiprecision_fixture(name):
    f = fixture(); c = ref.case(name)
    for reverse in (False, True):
        Obj, dObj = ref.objective(c, reverse=reverse)
        e = ref.dist(Obj, f[name + '_Obj']), ref.dist(dObj, f[name + '_dObj'])
        print('e_ref %s reverse %d: Obj %.2e dObj %.2e' % (name, reverse, e[0], e[1]))
        assert dObj.shape == (c['M'], c['Tx']) and max(e) < 1e-7, e
        assert ref.objective(c, reverse=reverse, grad=False) == Obj
    if not c['given']:                                         # the extended-precision form, the reference of the GPU tests where no 60-digit value is stored
        Oe, de = ref.obj_ext(c['x'], c['y'], c['len'], c['varx'], c['mux'], c['varc'])
        assert ref.dist(Oe, f[name + '_Obj']) < 1e-12 and ref.dist(de, f[name + '_dObj']) < 1e-12


def test_fixture_covers_what_it_must():
    shapes = {ref.CASES[n][:3] for n in CASES}
    assert shapes == {(1, 1, 2), (2, 64, 64), (3, 40, 64), (8, 100, 128), (2, 3000, 4096), (3, 5000, 8192), (3, 200, 256), (2, 100, 128)}
    f = fixture()
    assert set(f) == {n + s for n in CASES for s in ('_Obj', '_dObj')}                                # results only
    for n in CASES:
        c = ref.case(n)
        assert f[n + '_dObj'].shape == (c['M'], c['Tx']) and np.isfinite(f[n + '_Obj']) and np.all(np.isfinite(f[n + '_dObj']))
        assert c['x'].shape == (c['M'], c['Tx']) and c['y'].shape == (c['T'],) and c['fftCovs'].shape == (c['M'], c['Tx'])
    g = ref.case('k3_200_256')
    assert g['given'] and np.array_equal(g['len'], [2.0, 16.0, 64.0]) and [ref.case(n)['given'] for n in CASES].count(True) == 1
    s = ref.case('k2_100_128')
    xs = set(s['x'][:, :s['T']].ravel())
    assert {-35.0, 0.0, 600.0} <= xs and np.count_nonzero(s['y'] == 0.0) == 1 and s['y'][5] == 0.0 and s['x'][0, 5] == -35.0
    assert os.path.getsize(os.path.join(ROOT, 'tests', 'golden', 'gppad_cas_multiprecision.npz')) < 1000000
    # wherever the plain log(1 + exp(x)) is finite, amp equals it to rounding; beyond, it stays finite
    x = np.array([-35.0, -31.0, -30.0, -1.0, 0.0, 30.0, 499.0, 500.0, 501.0, 600.0, 700.0])
    with np.errstate(over='ignore'):
        plain = np.log(1 + np.exp(x))
    a = ref.GetAmp(x)
    assert np.all(np.isfinite(plain)) and np.allclose(a[2:], plain[2:], rtol=1e-15, atol=0) and np.allclose(a[:2], np.exp(x[:2]), rtol=0, atol=0)
    assert ref.GetAmp(np.array([800.0]))[0] == 800.0


@pytest.mark.parametrize('name', ['k2_64_64', 'k3_40_64', 'k8_100_128'])
def test_gradient_against_central_differences(name):
    """entries of dObj of every column (the 24 first, the boundary at T and the last one) against a central difference of the
    restatement's Obj, step 1e-5 |x| + 1e-6, relative to the largest entry of dObj, bound 1e-5 (the step and bound of
    tests/test_gppad_host.py::test_gradient_against_central_differences)"""
    c = ref.case(name)
    Obj, dObj = ref.objective(c)
    M, T, Tx = c['M'], c['T'], c['Tx']
    idx = sorted((set(range(24)) | {T - 1, T, Tx - 1}) & set(range(Tx)))
    worst = 0.0
    for m in range(M):
        for i in idx:
            h = 1e-5 * abs(c['x'][m, i]) + 1e-6
            cp = dict(c); cm = dict(c)
            cp['x'] = c['x'].copy(); cp['x'][m, i] += h; cm['x'] = c['x'].copy(); cm['x'][m, i] -= h
            fd = (ref.objective(cp, grad=False) - ref.objective(cm, grad=False)) / (cp['x'][m, i] - cm['x'][m, i])
            worst = max(worst, abs(fd - dObj[m, i]) / np.max(np.abs(dObj)))
    print('central differences %s: %.2e' % (name, worst))
    assert worst < 1e-5


# ---------------------------------------------------------------------------------------------------------------- the drivers
DRV = dict(T=600, lens=[8.0, 48.0], NumIts=40)               # (NumIts = 40: the levels end smooth enough for the line searches of the fine tuning to succeed
#                                                              from the raw starting point; at 12 and at 100 the joint objective starts at 1e10 and none does)


@functools.lru_cache(maxsize=None)
def signal():
    return ref.g1.envelope_signal(DRV['T'], 40.0, 33)[0]


@functools.lru_cache(maxsize=None)
def host_run(NumItsCas, fine_tuned, lens=tuple(DRV['lens'])):
    seen = []
    inner = ref.evaluator()

    def spy(y, P, D):
        seen.append((np.size(y), dict(D)))
        return inner(y, P, D)
    out = nagp.CasGPMAP(signal(), np.array(lens), dict(NumIts=DRV['NumIts'], NumItsCas=NumItsCas), fine_tuned=fine_tuned, evaluator=spy)
    return out, seen


def test_CasGPMAP_on_the_restatement_objective():
    y = signal(); T = y.size; sigy = np.sqrt(np.var(y, ddof=1))
    (A, X, c, Params, Info), seen = host_run(10, False)
    assert A.shape == X.shape == (T, 2) and c.shape == (T,) and np.all(A > 0) and np.all(np.isfinite(X))
    assert np.allclose(np.prod(A, axis=1) * c, y / sigy, rtol=1e-12, atol=0)
    assert Info['Tx'] == 1024 == nagp.GetTx(T, 48.0 * 5) and np.array_equal(Params['len'], DRV['lens'])
    assert Params['varx'].shape == Params['mux'].shape == (2,) and len(Info['Levels']) == 2
    # level m learns its own marginal parameters; varc is their product times sigy^2 (CasGPMAP.m:72, :93)
    # (each level's FBGPMAP is repeated here on the signal the driver gave it)
    A1, C1, P1, I1, X1 = nagp.FBGPMAP((y / sigy)[:, None], 8.0, dict(NumIts=DRV['NumIts'], Long=1, Tx=1024), evaluator=ref.evaluator())
    A2, C2, P2, I2, X2 = nagp.FBGPMAP(A1[:1024 - 240], 48.0, dict(NumIts=DRV['NumIts'], Long=1, Tx=1024), evaluator=ref.evaluator())
    assert Params['varc'] == P1['varc'][0] * P2['varc'][0] * sigy ** 2
    assert np.array_equal(Params['varx'], [P1['varx'][0], P2['varx'][0]]) and np.array_equal(Params['mux'], [P1['mux'][0], P2['mux'][0]])
    # the raw starting point X = log(exp(A) - 1) of the level estimates, A(:,1) ./ A(:,2) and A(:,2) (:69, :81)
    Al = np.stack([A1[:, 0] / A2[:, 0], A2[:, 0]], axis=1)
    assert np.array_equal(X, np.log(np.exp(Al) - 1)[:T]) and np.array_equal(A, np.log(1 + np.exp(X)))
    # the joint objective was opened once, on (T, Tx, M); the levels before it on their own T
    assert seen[-1] == (T, dict(T=T, Tx=1024, M=2)) and all('M' not in d for _, d in seen[:-1])
    assert {d['T'] for _, d in seen[:-1] if d['Tx'] == 1024} == {T, 1024 - 240}


def test_the_literal_form_discards_the_fine_tuning():
    """fine_tuned=False (MAPGPCasFast.m returns its input): the outputs are bit-equal for NumItsCas 0 and 10 while Info['ObjFT'] differs"""
    (A0, X0, c0, P0, I0), _ = host_run(0, False)
    (A1, X1, c1, P1, I1), _ = host_run(10, False)
    assert np.array_equal(A0, A1) and np.array_equal(X0, X1) and np.array_equal(c0, c1) and P0['varc'] == P1['varc']
    assert I0['ObjFT'].size == 1 and I1['ObjFT'].size > 1 and I1['ObjFT'][0] == I0['ObjFT'][0] and I1['ObjFT'][-1] < I0['ObjFT'][0]


def test_the_consistent_form_returns_the_fine_tuned_cascade():
    (A0, X0, c0, P0, I0), _ = host_run(10, False)
    (A1, X1, c1, P1, I1), _ = host_run(10, True)
    y = signal()
    assert np.all(np.diff(I1['ObjFT']) <= 0) and np.array_equal(I1['ObjFT'], I0['ObjFT'])
    assert X1.shape == X0.shape and not np.array_equal(X1, X0) and np.array_equal(A1, np.log(1 + np.exp(X1)))
    assert np.allclose(np.prod(A1, axis=1) * c1, y / np.sqrt(np.var(y, ddof=1)), rtol=1e-12, atol=0)


def test_a_non_integer_len_tol_takes_the_floored_length():
    """len(2) tol = 241.5: Tx = 1024 and level 2 demodulates A(1:782, 1), the colon's end floored"""
    (A, X, c, Params, Info), seen = host_run(0, False, lens=(8.0, 48.3))
    assert Info['Tx'] == 1024 and A.shape == (DRV['T'], 2)
    assert {d['T'] for _, d in seen if 'M' not in d and d['Tx'] == 1024} == {DRV['T'], 782}


def test_MAPGPCasFast_returns_its_input_and_the_trace():
    c = ref.case('k3_40_64')
    P = dict(len=c['len'], varx=c['varx'], mux=c['mux'], varc=c['varc']); D = nagp.PackDimsCas(c['T'], c['Tx'], c['M'])
    assert D == dict(T=40, Tx=64, M=3) and nagp.UnpackDimsCas(D) == (40, 64, 3)
    X = c['x'].T.copy()                                        # Tx x M, the .m's layout
    rec = []
    Xo, Obj = nagp.MAPGPCasFast(X, c['y'], P, D, 5, evaluator=ref.evaluator(record=rec))
    assert np.array_equal(Xo, X) and Obj.size >= 2 and np.all(np.diff(Obj) <= 0)
    assert np.array_equal(rec[0][3], X.T.reshape(-1)) and Obj[0] == ref.objective(c)[0]                 # x = X(:): column m contiguous
    Xf, Objf = nagp.MAPGPCasFast(X, c['y'], P, D, 5, evaluator=ref.evaluator(), fine_tuned=True)
    assert np.array_equal(Objf, Obj) and Xf.shape == X.shape and not np.array_equal(Xf, X)
    assert ref.obj(Xf.T, c['y'], c['fftCovs'], c['varx'], c['mux'], c['varc'], grad=False) <= Obj[-1]


def test_FBCasGPMAP_Len_as_a_column_and_per_channel():
    y = signal(); T = y.size
    Y = np.stack([y, 0.5 * y[::-1]], axis=1)
    opts = dict(NumIts=DRV['NumIts'], NumItsCas=3)
    A, X, Cc, Params, Info = nagp.FBCasGPMAP(Y, np.array([[8.0], [48.0]]), opts, evaluator=ref.evaluator())
    assert A.shape == X.shape == (T, 2, 2) and Cc.shape == (T, 2) and len(Info) == 2
    assert Params['len'].shape == (2, 2) and Params['varc'].shape == (2,) and Params['varx'].shape == Params['mux'].shape == (2, 2)
    B = nagp.FBCasGPMAP(Y, np.array([[8.0, 8.0], [48.0, 48.0]]), opts, evaluator=ref.evaluator())
    assert np.array_equal(A, B[0]) and np.array_equal(X, B[1]) and np.array_equal(Cc, B[2]) and np.array_equal(Params['varc'], B[3]['varc'])
    # channel 0 is CasGPMAP on its column; D = 1 squeezes to (T, M)
    (A0, X0, c0, P0, I0) = nagp.CasGPMAP(y, [8.0, 48.0], opts, evaluator=ref.evaluator())
    assert np.array_equal(A[:, 0, :], A0) and np.array_equal(Cc[:, 0], c0) and Params['varc'][0] == P0['varc'] and np.array_equal(Params['varx'][:, 0], P0['varx'])
    A1, X1, C1, P1, I1 = nagp.FBCasGPMAP(y, [8.0, 48.0], opts, evaluator=ref.evaluator())
    assert A1.shape == X1.shape == (T, 2) and C1.shape == (T, 1) and np.array_equal(A1, A0)
    with pytest.raises(ValueError):
        nagp.FBCasGPMAP(Y, np.ones((2, 3)), opts, evaluator=ref.evaluator())
    with pytest.raises(ValueError):
        nagp.CasGPMAP(y, np.ones(9), opts, evaluator=ref.evaluator())
    assert gc.LoadCasGPMAPOpts()['NumItsCas'] == 500 and gc.LoadCasGPMAPOpts()['tol'] == 5 and gc.LoadCasGPMAPOpts()['NumIts'] == 2000
    assert gc.LoadCasGPMAPOpts(dict(NumItsCas=7))['NumItsCas'] == 7 and gc.LoadCasGPMAPOpts()['MinLength'] == 8


# ---------------------------------------------------------------------------------------------------------------- the boundary
def test_exported_and_bound():
    nagp.build()
    out = subprocess.run(['nm', '-D', '--defined-only', L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    names = {'nagp_gppad_cas_obj', 'nagp_gppad_cas_create', 'nagp_gppad_cas_eval', 'nagp_gppad_cas_destroy', 'nagp_gppad_cas_timings'}
    assert names <= set(re.findall(r' T (nagp_[a-z0-9_]+)', out)) and names <= set(L.EXPORTS)
    hdr = open(os.path.join(ROOT, 'include', 'nagp.h')).read()
    assert re.search(r'^int nagp_gppad_cas_obj\(int32_t n_problems, int32_t M, int64_t T, int64_t Tx,', hdr, re.M)
    assert re.search(r'^int nagp_gppad_cas_timings\(double\* ms /\* 1 \*/\);', hdr, re.M) and re.search(r'^void nagp_gppad_cas_destroy\(nagp_gppad_cas\* handle\);', hdr, re.M)
    fn = L.lib().nagp_gppad_cas_obj
    assert len(fn.argtypes) == 15 and fn.restype is C.c_int and len(L.lib().nagp_gppad_cas_create.argtypes) == 13
    ms = C.c_double(-1.0)
    assert L.lib().nagp_gppad_cas_timings(C.byref(ms)) == 0 and ms.value >= 0.0 and L.lib().nagp_gppad_cas_timings(None) == EINVAL
    for name in ('gppad_cas_obj', 'GppadCasHandle', 'GetObjCasGPFAST', 'PackDimsCas', 'UnpackDimsCas', 'MAPGPCasFast', 'CasGPMAP', 'FBCasGPMAP'):
        assert getattr(nagp, name) is getattr(gc, name)
    assert issubclass(gc.GppadCasHandle, nagp._drive.ResidentHandle)


def call(P=1, M=2, T=5, Tx=8, x=True, y=None, ln=(3.0, 9.0), cov=None, cs=0, varx=(1.0, 1.0), mux=(0.0, 0.0), varc=(1.0,), Obj=True):
    f = lambda v: L.f64(np.asarray(v, float), 'C') if v is not None else None
    n = max(P, 1) * max(M, 1) * max(Tx, 1)
    xx = f(np.zeros(n)) if x else None
    yy = f(np.ones(max(P, 1) * max(T, 1)) if y is None else y) if y is not False else None
    O = np.zeros(max(P, 1)); d = np.zeros(n)
    return L.lib().nagp_gppad_cas_obj(P, M, T, Tx, L.dptr(xx), L.dptr(yy), L.dptr(f(ln)), L.dptr(f(cov)), cs, L.dptr(f(varx)), L.dptr(f(mux)),
                                      L.dptr(f(varc)), L.dptr(O) if Obj else None, L.dptr(d), 0)


def test_argument_errors_answer_without_a_device(monkeypatch):
    nagp.build()
    err = lambda: L.lib().nagp_last_error()
    assert call(x=False) == EINVAL and call(y=False) == EINVAL and call(Obj=False) == EINVAL
    assert call(varx=None) == EINVAL and call(mux=None) == EINVAL and call(varc=None) == EINVAL
    assert call(ln=None) == EINVAL and b'one of len and fftCovs' in err() and call(cov=np.ones(16)) == EINVAL and b'one of len and fftCovs' in err()
    assert call(M=0) == EUNSUPPORTED and b'1 to 8' in err() and call(M=9, ln=[3.0] * 9, varx=[1.0] * 9, mux=[0.0] * 9) == EUNSUPPORTED and b'M=9' in err()
    assert call(P=0) == EINVAL and call(T=0) == EINVAL and call(T=9) == EINVAL and b'T=9 > Tx=8' in err()
    assert call(ln=None, cov=np.ones(16), cs=8) == EINVAL and b'cov_stride' in err()
    for Tx in (0, 1, 3, 6, 12, 2 ** 20 + 2, 2 ** 21):
        assert call(Tx=Tx, T=1) == EUNSUPPORTED and b'power of two' in err(), Tx
    for bad in (np.nan, np.inf, -np.inf):
        y = np.ones(5); y[-1] = bad
        assert call(y=y) == EINVAL and b'y[4]' in err()
        assert call(ln=[3.0, bad]) == EINVAL and call(varx=[1.0, bad]) == EINVAL and call(mux=[0.0, bad]) == EINVAL and call(varc=[bad]) == EINVAL
        cv = np.ones(16); cv[-1] = bad
        assert call(ln=None, cov=cv) == EINVAL
    for kw in (dict(varx=[1.0, 0.0]), dict(varx=[-1.0, 1.0]), dict(varc=[0.0]), dict(varc=[-1.0]), dict(ln=[0.0, 3.0]), dict(ln=[3.0, -2.0])):
        assert call(**kw) == EINVAL and b'> 0' in err(), kw
    cv = np.ones(16); cv[11] = 0.0
    assert call(ln=None, cov=cv) == EINVAL and b'fftCovs[11]' in err()
    h = C.c_void_p(1)
    assert L.lib().nagp_gppad_cas_create(C.byref(h), 1, 2, 5, 8, None, None, None, 0, None, None, None, 0) == EINVAL and not h.value
    assert L.lib().nagp_gppad_cas_eval(None, None, None, None) == EINVAL
    # the Python layer refuses what it can see before the library does
    with pytest.raises(ValueError, match='one of len and fftCovs'):
        nagp.gppad_cas_obj(np.zeros((2, 8)), np.ones(5), [1.0, 1.0], [0.0, 0.0], 1.0)
    with pytest.raises(ValueError, match='fftCovs must be'):
        nagp.gppad_cas_obj(np.zeros((2, 8)), np.ones(5), [1.0, 1.0], [0.0, 0.0], 1.0, fftCovs=np.ones((8, 2)))
    with pytest.raises(L.NagpError, match=r'\(-2\).*M=9'):
        nagp.gppad_cas_obj(np.zeros((9, 8)), np.ones(5), np.ones(9), np.zeros(9), 1.0, len=np.ones(9))
    with pytest.raises(L.NagpError, match=r'\(-1\).*T=9 > Tx=8'):
        nagp.gppad_cas_obj(np.zeros((2, 8)), np.ones(9), [1.0, 1.0], [0.0, 0.0], 1.0, len=[3.0, 9.0])
    with pytest.raises(L.NagpError, match=r'\(-1\).*varx\[1\]'):
        nagp.GetObjCasGPFAST(np.zeros(16), np.ones(5), np.ones((8, 2)), dict(varx=[1.0, 0.0], mux=[0.0, 0.0], varc=1.0), dict(T=5, Tx=8, M=2))
    # one cascade beyond the budget of the per-evaluation buffers (lowered to 1 MiB behind NAGP_DEVELOPER, which tests/conftest.py sets)
    monkeypatch.setenv('NAGP_GPPAD_BUDGET_MB', '1')
    assert call(Tx=65536) == EUNSUPPORTED and b'budget' in err()


def test_argument_checks_in_plain_c():
    """tests/c/abi_gppad_cas_errors.c: a stand-alone C program on exactly-sized heap blocks against libnagp_asan.so (the host code of the C
    ABI built with AddressSanitizer), on the CPU only: every invalid call returns its status and ASan reports nothing."""
    lib = nagp.build(asan=True)
    clang = '/opt/rocm/lib/llvm/bin/clang'
    rt = glob.glob('/opt/rocm/lib/llvm/lib/clang/*/lib/linux') + glob.glob('/opt/rocm/lib/llvm/lib/clang/*/lib/x86_64-unknown-linux-gnu')
    with tempfile.TemporaryDirectory() as td:
        exe = os.path.join(td, 'abi_gppad_cas_errors')
        r = subprocess.run([clang, '-fsanitize=address', '-shared-libsan', '-g', '-O1', '-std=c99', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'include'),
                            '-o', exe, os.path.join(ROOT, 'tests', 'c', 'abi_gppad_cas_errors.c'), lib, '-lm', '-Wl,-rpath,/opt/rocm/lib',
                            '-Wl,-rpath-link,/opt/rocm/lib'] + ['-Wl,-rpath,' + d for d in rt], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        env = dict(os.environ, ASAN_OPTIONS='detect_leaks=0:abort_on_error=0:exitcode=66', LD_LIBRARY_PATH=':'.join(rt + [os.environ.get('LD_LIBRARY_PATH', '')]))
        r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
        assert r.returncode == 0 and 'all error paths returned their status' in r.stdout, r.stdout + r.stderr
        assert 'AddressSanitizer' not in r.stderr, r.stderr


def test_kernel_bodies_on_the_host_under_the_sanitizers():
    """tests/c/gppad_cas_host_check.cpp: the cascade's kernel bodies, one "thread" per workgroup, at the fixture shapes against plain
    long double loops, host code only, under AddressSanitizer and UndefinedBehaviorSanitizer (a stand-alone program: nothing of it is
    loaded into Python)"""
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    with tempfile.TemporaryDirectory() as td:
        exe = os.path.join(td, 'gppad_cas_host_check')
        r = subprocess.run([hipcc, '-x', 'hip', '--offload-host-only', '-O1', '-g', '-std=c++17', '-Xarch_host', '-fsanitize=address,undefined',
                            '-Xarch_host', '-fno-sanitize-recover=undefined', '-I', L.CSRC, '-o', exe, os.path.join(ROOT, 'tests', 'c', 'gppad_cas_host_check.cpp')],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS='detect_leaks=0:exitcode=66'))
        assert r.returncode == 0 and r.stdout.rstrip().endswith('ok') and r.stdout.count('err Obj ') == 16 and r.stdout.count('err ObjA ') == 16, r.stdout + r.stderr
        assert 'Sanitizer' not in r.stderr and 'runtime error' not in r.stderr, r.stderr
