"""nagp_nmf_temp_obj (the objectives of experiments/nmf/nmf.m and nmf_inf.m: getObj_nmf_temp.m, getObj_nmf_temp_inf.m) and the host mirrors
around it, without a GPU: the yardstick -- tests/nmf_temp_ref.py against the multi-precision fixture
tests/golden/nmf_temp_multiprecision.npz --, the reference's own gradient checks restated, the drivers nmf_inf and nmf on the restatement
objective, the export and its binding, and the argument checks of include/nagp.h, which answer on a machine with no device (they run
before any device call).  Distances are the project's norm max|d| / max|ref| per array.

Bound of the restatement against the fixture: 32 x 1e-15.  Measured on the CPU (tools/make_nmf_temp_fixture.py prints every figure): Obj
within 2.9e-16, dObj within 4.4e-16 on every case but the two of T = 1, D = K = 1, whose single gradient entry (Ahat - A) / Ahat^2 carries
the cancellation of one subtraction (4.4e-15)."""
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
from nagp import nmf_temp as nt
import nmf_temp_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EUNSUPPORTED = -1, -2
CASES = sorted(ref.CASES)
BOUND = 32 * 1e-15


@functools.lru_cache(maxsize=None)
def fixture():
    return dict(np.load(os.path.join(ROOT, 'tests', 'golden', 'nmf_temp_multiprecision.npz')))


@pytest.mark.parametrize('name', CASES)
def test_restatement_matches_the_multiprecision_fixture(name):
    f = fixture(); c = ref.case(name)
    assert np.array_equal([c['x'].sum(), c['A'].sum()], f[name + '_sums'])
    for reverse in (False, True):
        Obj, dObj = ref.objective(c, reverse=reverse)
        e = ref.dist(Obj, f[name + '_Obj']), ref.dist(dObj, f[name + '_dObj'])
        print('e_ref %s reverse %d: Obj %.2e dObj %.2e' % (name, reverse, e[0], e[1]))
        assert dObj.shape == c['x'].shape and max(e) < BOUND, e
        assert ref.objective(c, reverse=reverse, grad=False) == Obj


def test_fixture_covers_what_it_must():
    shapes = {ref.CASES[n][:5] for n in CASES}
    for p in ('none', 'tg', 'ig'):
        assert {(20, 3, 2, p, 'l'), (20, 3, 2, p, 'i'), (1999, 16, 3, p, 'l'), (1999, 16, 3, p, 'i')} <= shapes
        assert any(s[:4] == (2, 1, 1, p) for s in shapes) and any(s[:4] == (3, 1, 1, p) for s in shapes)
    assert any(s[:4] == (1, 1, 1, 'none') for s in shapes) and (513, 64, 16, 'tg', 'l') in shapes
    for T in (255, 256, 257):
        assert {(T, 16, 3, 'tg', 'l'), (T, 16, 3, 'ig', 'l')} <= shapes
    assert sum(ref.case(n)['vary'] is None for n in CASES) == 1
    lams = [tuple(ref.case(n)['lam']) for n in CASES if ref.CASES[n][3] == 'ig']
    assert (0.0, 0.0, 0.0) in lams and (1.0, 1.0, 1.0) in lams
    assert ref.CASES['r20_tg_l'][6] == dict(varinf=[1 / 16, 1 / 32], lam=[.1, .3])
    assert ref.CASES['r20_ig_l'][6] == dict(muinf=[1 / 4, 1 / 4], varinf=[1 / 16, 1 / 16], lam=[.1, .1])
    f = fixture()
    assert set(f) == {n + s for n in CASES for s in ('_Obj', '_dObj', '_sums')}                  # results (and two checksums) only
    for n in CASES:
        assert f[n + '_dObj'].shape == ref.case(n)['x'].shape and np.isfinite(f[n + '_Obj']) and np.all(np.isfinite(f[n + '_dObj']))
    w = ref.case('r20_none_i')['W']
    assert not np.allclose(w.sum(axis=1), 1.0)                                                   # a given W is not renormalised: the case can tell
    assert os.path.getsize(os.path.join(ROOT, 'tests', 'golden', 'nmf_temp_multiprecision.npz')) < 1000000


@pytest.mark.parametrize('name', ['r20_%s_%s' % (p, f) for p in ('none', 'tg', 'ig') for f in 'li'])
def test_gradient_as_the_reference_checks_it(name):
    """nmf/tests/test_getObj_nmf_temp.m and test_getObj_nmf_temp_inf.m restated: checkgrad's central differences with delta = 1e-5 on every
    coordinate, norm(dh - dy) / norm(dh + dy) < 1e-6, at the reference's shape and parameter values"""
    c = ref.case(name)
    _, dy = ref.objective(c)
    delta = 1e-5
    dh = np.zeros_like(dy)
    for j in range(dy.size):
        cp = dict(c); cm = dict(c)
        cp['x'] = c['x'].copy(); cp['x'][j] += delta; cm['x'] = c['x'].copy(); cm['x'][j] -= delta
        dh[j] = (ref.objective(cp, grad=False) - ref.objective(cm, grad=False)) / (2 * delta)
    d = np.linalg.norm(dh - dy) / np.linalg.norm(dh + dy)
    print('checkgrad %s: %.2e' % (name, d))
    assert d < 1e-6


PLANT = dict(T=400, D=6, K=2, seed=3)


@functools.lru_cache(maxsize=None)
def planted():
    return ref.planted(**PLANT)


def test_chunking_and_the_info_shapes():
    A, W, H, vary, par = planted()
    rec = []
    H0 = np.ones_like(H)
    Hn, info = nagp.nmf_inf(A, W, H0, [], [], [], vary, dict(numIts=7, progress_chunk=3), evaluator=ref.evaluator(record=rec))
    assert Hn.shape == H.shape and info['it'].shape == (3,) and np.all(info['it'] <= 3)                # ceil(7 / 3) chunks of 3 (nmf_inf.m:70-71)
    assert info['Obj'].ndim == 1 and 3 <= info['Obj'].size <= np.sum(info['it']) + 3                   # per chunk: its start value and one per accepted line search
    assert len(rec) == 1 and rec[0]['n_problems'] == 1 and rec[0]['prior'] == 'none' and rec[0]['W'].shape == (1, 2, 6)
    Wn, Hn, info = nt.nmf(A, W, H0, [], [], [], vary, dict(numIts=5, progress_chunk=2), evaluator=ref.evaluator())
    assert Wn.shape == W.shape and Hn.shape == H.shape and info['it'].shape == (3,) and np.allclose(Wn.sum(axis=1), 1.0, rtol=1e-14)
    # kept from the .m: EVERY chunk runs progress_chunk line searches, so numIts = 4 in chunks of 3 is 2 x 3, and numIts below the
    # default chunk (1000 in nmf, 50 in nmf_inf) still runs one whole chunk
    assert np.array_equal(nt.nmf(A, W, H0, [], [], [], vary, dict(numIts=4, progress_chunk=3), evaluator=ref.evaluator())[2]['it'], [3, 3])
    assert nagp.nmf_inf(A, W, H0, [], [], [], vary, dict(numIts=1), evaluator=ref.evaluator())[1]['it'][0] > 1


def test_prior_dispatch_as_the_drivers_write_it():
    """[] / None exactly as nmf.m:119-131: varinf empty -> none (whatever muinf and lam hold), muinf empty -> TG, else IG"""
    A, W, H, vary, par = planted()
    for mu, vi, la, want in (([], [], [], 'none'), (None, None, None, 'none'), (par['muinf'], [], par['lam'], 'none'), ([], par['varinf'], par['lam'], 'tg'),
                             (None, par['varinf'], par['lam'], 'tg'), (par['muinf'], par['varinf'], par['lam'], 'ig')):
        rec = []
        nagp.nmf_inf(A, W, H, mu, vi, la, vary, dict(numIts=1, progress_chunk=1), evaluator=ref.evaluator(record=rec))
        assert rec[0]['prior'] == want and (rec[0]['muinf'] is None) == (want != 'ig') and (rec[0]['varinf'] is None) == (want == 'none')
        rec = []
        nt.nmf(A, W, H, mu, vi, la, vary, dict(numIts=1, progress_chunk=1), evaluator=ref.evaluator(record=rec))
        assert rec[0]['prior'] == want and rec[0]['W'] is None
    with pytest.raises(ValueError, match='lam is empty'):
        nagp.nmf_inf(A, W, H, [], par['varinf'], [], vary, dict(numIts=1), evaluator=ref.evaluator())


def test_one_extra_argument_is_an_error_as_in_the_m():
    c = ref.case('r20_tg_l')
    with pytest.raises(TypeError, match='varargin'):
        nagp.getObj_nmf_temp(c['x'], c['A'], c['vary'], c['varinf'])
    with pytest.raises(TypeError, match='varargin'):
        nagp.getObj_nmf_temp_inf(c['x'][:40], c['A'], np.ones((2, 3)), c['vary'], c['varinf'])
    with pytest.raises(TypeError):
        nagp.getObj_nmf_temp(c['x'], c['A'], c['vary'], 1, 2, 3, 4)


def test_restart_selection_and_the_kept_initial_W():
    """nmf_inf: the restarts are ONE batch of n_problems = restarts, each 500 iterations in chunks of 50, the smallest last Obj wins and
    the main loop starts from it.  nmf: the candidates carry their own W, the winner keeps its INITIAL W (nmf_inf returns only H)."""
    A, W, H, vary, par = planted()
    rng = np.random.default_rng(0)
    bad = np.exp(3 + rng.standard_normal(H.shape))                     # a start far from the data: it cannot catch up in a few searches
    rec = []
    ev = ref.evaluator(record=rec)
    # (the restart loop's own numIts = 500 is fixed by nmf_inf.m:83; the chunks end early where a line search fails twice)
    Hn, info = nagp.nmf_inf(A, W, bad, par['muinf'], par['varinf'], par['lam'], vary, dict(numIts=2, progress_chunk=2, restarts=2), inits=[H], evaluator=ev)
    assert rec[0]['n_problems'] == 2 and rec[0]['prior'] == 'ig' and rec[1]['n_problems'] == 1
    assert info['restart_Obj'].shape == (2,) and info['restart'] == int(np.argmin(info['restart_Obj']))
    assert info['Obj'][0] <= info['restart_Obj'].min() + 1e-12 and info['it'].shape == (1,)
    with pytest.raises(ValueError, match='initialisations'):
        nagp.nmf_inf(A, W, H, [], [], [], vary, dict(numIts=1, progress_chunk=1, restarts=3), inits=[H], evaluator=ev)
    # seeded candidates: the same seed gives the same run
    a = nagp.nmf_inf(A, W, H, [], [], [], vary, dict(numIts=1, progress_chunk=1, restarts=2), seed=5, evaluator=ref.evaluator())
    b = nagp.nmf_inf(A, W, H, [], [], [], vary, dict(numIts=1, progress_chunk=1, restarts=2), seed=5, evaluator=ref.evaluator())
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1]['restart_Obj'], b[1]['restart_Obj'])
    # nmf: the first candidate is hopeless, the second is the planted pair; a recorder sees the start of the joint optimisation
    W_bad = np.full_like(W, 1.0 / W.shape[1])
    rec = []
    seen = []

    def ev2(*a):
        f = ref.evaluator(record=rec)(*a)

        def g(X):
            seen.append(np.array(X))
            return f(X)
        return g
    Wn, Hn, info = nt.nmf(A, W_bad, bad, [], par['varinf'], par['lam'], vary, dict(numIts=1, progress_chunk=1, restarts=2, restart_numIts=3), inits=[(2.0 * W, H)], evaluator=ev2)
    assert rec[0]['n_problems'] == 2 and np.array_equal(rec[0]['W'], np.stack([W_bad, 2.0 * W])) and rec[0]['prior'] == 'tg'
    assert info['restart'] == 1 and rec[1]['W'] is None and rec[1]['n_problems'] == 1
    T, K = H.shape
    first_joint = [X for X in seen if X.shape[1] == T * K + K * A.shape[1]][0][0]
    assert np.array_equal(first_joint[T * K:], np.log(2.0 * W).reshape(-1, order='F'))        # the INITIAL W of the winning candidate, not normalised


def test_nmf_inf_lowers_the_objective_on_planted_data():
    """T = 400, D = 6, K = 2, IG prior, the true W: Obj falls monotonically over the accepted line searches of every chunk, and the
    result explains the data better than the flat start"""
    A, W, H, vary, par = planted()
    H0 = np.full_like(H, np.mean(A))
    Hn, info = nagp.nmf_inf(A, W, H0, par['muinf'], par['varinf'], par['lam'], vary, dict(numIts=40, progress_chunk=20), evaluator=ref.evaluator())
    assert info['it'].shape == (2,) and np.all(np.diff(info['Obj']) <= 0) and info['Obj'][-1] < info['Obj'][0] - 0.1
    assert np.corrcoef(np.log(Hn).ravel(), np.log(H).ravel())[0, 1] > 0.8


def test_forward_and_reverse_runs_agree_for_the_committed_seeds():
    """the yardstick of the GPU end-to-end test: for its seeds and iteration counts the forward and the reverse restatement runs end
    within 1e-6 / 32 of each other in the last Obj (tests/test_nmf_temp_gpu.py computes the distance itself)"""
    import test_nmf_temp_gpu as g
    for run in (g.run_inf, g.run_nmf):
        f = run(ref.evaluator(False)); r = run(ref.evaluator(True))
        d = abs(f[-1]['Obj'][-1] - r[-1]['Obj'][-1]) / abs(f[-1]['Obj'][-1])
        print('%s: forward / reverse distance of the last Obj %.2e' % (run.__name__, d))
        assert d < 1e-6 / 32


def test_refused_forms_name_the_reference_file():
    for fn, text in ((nt.tnmf, 'tnmf.m'), (nt.tnmf_inf, 'getObj_nmf_log_norm'), (nt.randnmf, 'randnmf.m'), (nt.randtnmf, 'randtnmf.m')):
        with pytest.raises(NotImplementedError, match=re.escape(text)):
            fn()


def test_exported_and_bound():
    nagp.build()
    out = subprocess.run(['nm', '-D', '--defined-only', L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    names = {'nagp_nmf_temp_obj', 'nagp_nmf_temp_create', 'nagp_nmf_temp_eval', 'nagp_nmf_temp_destroy', 'nagp_nmf_temp_timings'}
    assert names <= set(re.findall(r' T (nagp_[a-z0-9_]+)', out)) and names <= set(L.EXPORTS)
    hdr = open(os.path.join(ROOT, 'include', 'nagp.h')).read()
    assert re.search(r'^int nagp_nmf_temp_obj\(int32_t n_problems, int64_t T, int32_t D, int32_t K, int32_t prior,', hdr, re.M)
    assert re.search(r'^int nagp_nmf_temp_timings\(double\* ms /\* 1 \*/\);', hdr, re.M) and re.search(r'^void nagp_nmf_temp_destroy\(nagp_nmf_temp\* handle\);', hdr, re.M)
    assert 'enum { NAGP_NMFT_NONE = 0, NAGP_NMFT_TG = 1, NAGP_NMFT_IG = 2 };' in hdr and (L.NMFT_NONE, L.NMFT_TG, L.NMFT_IG) == (0, 1, 2)
    fn = L.lib().nagp_nmf_temp_obj
    assert len(fn.argtypes) == 15 and fn.restype is C.c_int and len(L.lib().nagp_nmf_temp_create.argtypes) == 13
    ms = C.c_double(-1.0)
    assert L.lib().nagp_nmf_temp_timings(C.byref(ms)) == 0 and ms.value >= 0.0 and L.lib().nagp_nmf_temp_timings(None) == EINVAL
    for name in ('nmf_temp_obj', 'NmfTempHandle', 'getObj_nmf_temp', 'getObj_nmf_temp_inf', 'nmf_inf', 'nmf_inf_many'):
        assert getattr(nagp, name) is getattr(nt, name)
    import types
    assert isinstance(nagp.nmf, types.ModuleType) and callable(nagp.nmf_temp.nmf)                # nagp.nmf stays the fixed-point module


def call(P=1, T=5, D=3, K=2, prior=2, x=True, A=None, vary=None, W=None, mu=(.25, .25), vi=(1 / 16, 1 / 16), la=(.1, .1), Obj=True):
    f = lambda v: L.f64(np.asarray(v, float), 'C') if v is not None else None
    n = max(P, 1) * (max(T, 1) * max(K, 1) + max(K, 1) * max(D, 1))
    xx = f(np.zeros(n)) if x else None
    aa = f(np.ones(max(T, 1) * max(D, 1)) if A is None else A) if A is not False else None
    O = np.zeros(max(P, 1)); d = np.zeros(n)
    return L.lib().nagp_nmf_temp_obj(P, T, D, K, prior, L.dptr(xx), L.dptr(aa), L.dptr(f(vary)), L.dptr(f(W)), L.dptr(f(mu)), L.dptr(f(vi)), L.dptr(f(la)),
                                     L.dptr(O) if Obj else None, L.dptr(d), 0)


def test_argument_errors_answer_without_a_device(monkeypatch):
    nagp.build()
    err = lambda: L.lib().nagp_last_error()
    assert call(x=False) == EINVAL and call(A=False) == EINVAL and call(Obj=False) == EINVAL
    assert call(P=0) == EINVAL and call(D=0) == EINVAL and call(K=0) == EINVAL and call(T=0) == EINVAL
    assert call(T=1) == EINVAL and b'T >= 2' in err() and call(T=1, prior=1) == EINVAL
    assert call(prior=3) == EINVAL and b'prior=3' in err() and call(prior=-1) == EINVAL
    assert call(vi=None) == EINVAL and call(la=None) == EINVAL and call(mu=None) == EINVAL and b'muinf' in err()
    assert call(prior=1, vi=None) == EINVAL and call(prior=1, la=None) == EINVAL
    assert call(D=65) == EUNSUPPORTED and b'at most 64' in err() and call(K=17) == EUNSUPPORTED and b'at most 16' in err()
    for bad in (np.nan, np.inf, -np.inf, -1e-9):
        a = np.ones(15); a[-1] = bad
        assert call(A=a) == EINVAL and call(vary=a) == EINVAL
        w = np.ones(6); w[-1] = bad
        assert call(W=w) == EINVAL
    for bad in (np.nan, np.inf, -np.inf, 0.0, -1.0):
        assert call(vi=(1 / 16, bad)) == EINVAL and call(prior=1, vi=(bad, 1.0)) == EINVAL and call(mu=(.25, bad)) == EINVAL
    for bad in (np.nan, np.inf, -1e-9, 1 + 1e-9):
        assert call(la=(.1, bad)) == EINVAL
    assert call(prior=1, la=(.1, np.nan)) == EINVAL
    w = np.ones(6); w[[1, 3, 5]] = 0.0
    assert call(W=w) == EINVAL and b'row 1 of W' in err()
    h = C.c_void_p(1)
    assert L.lib().nagp_nmf_temp_create(C.byref(h), 1, 5, 3, 2, 0, None, None, None, None, None, None, 0) == EINVAL and not h.value
    assert L.lib().nagp_nmf_temp_eval(None, None, None, None) == EINVAL
    # one problem beyond the budget of the per-evaluation buffers (lowered to 1 MiB behind NAGP_DEVELOPER, which tests/conftest.py sets):
    # T = 70000, D = K = 1, no prior, learning form: 8 (2 * 70001 + 274 * (1 + 1) + 1) = 1 124 408 B
    monkeypatch.setenv('NAGP_NMFT_BUDGET_MB', '1')
    assert call(T=70000, D=1, K=1, prior=0) == EUNSUPPORTED and b'budget' in err() and b'1124408' in err()


def test_binding_checks_its_arguments():
    c = ref.case('r20_ig_l')
    kw = dict(prior='ig', muinf=c['muinf'], varinf=c['varinf'], lam=c['lam'])
    for args, k in (((c['x'][:-1], c['A'], c['vary']), kw), ((c['x'], c['A'], c['vary'][:-1]), kw), ((c['x'], c['A'][:, 0], c['vary']), kw),
                    ((c['x'], c['A'], c['vary']), dict(kw, lam=c['lam'][:1])), ((c['x'], c['A'], c['vary']), dict(kw, muinf=None)),
                    ((c['x'], c['A'], c['vary']), dict(kw, prior='gamma')), ((c['x'], c['A'], c['vary'], np.ones((2, 4))), kw),
                    ((c['x'], c['A'], c['vary'], np.ones((2, 3))), kw)):
        with pytest.raises(ValueError):
            nagp.nmf_temp_obj(*args, **k)
    with pytest.raises(ValueError, match='needs K'):
        nagp.NmfTempHandle(c['A'], c['vary'])
    with pytest.raises(ValueError):
        nagp.nmf_inf(c['A'], np.ones((2, 3)), np.ones((19, 2)), [], [], [], c['vary'], evaluator=ref.evaluator())


def test_argument_checks_in_plain_c():
    """tests/c/abi_nmf_temp_errors.c: a stand-alone C program on exactly-sized heap blocks against libnagp_asan.so (the host code of the C
    ABI built with AddressSanitizer), on the CPU only: every invalid call returns its status and ASan reports nothing."""
    import tempfile
    lib = nagp.build(asan=True)
    clang = '/opt/rocm/lib/llvm/bin/clang'
    rt = glob.glob('/opt/rocm/lib/llvm/lib/clang/*/lib/linux') + glob.glob('/opt/rocm/lib/llvm/lib/clang/*/lib/x86_64-unknown-linux-gnu')
    with tempfile.TemporaryDirectory() as td:
        exe = os.path.join(td, 'abi_nmf_temp_errors')
        r = subprocess.run([clang, '-fsanitize=address', '-shared-libsan', '-g', '-O1', '-std=c99', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'include'),
                            '-o', exe, os.path.join(ROOT, 'tests', 'c', 'abi_nmf_temp_errors.c'), lib, '-lm', '-Wl,-rpath,/opt/rocm/lib',
                            '-Wl,-rpath-link,/opt/rocm/lib'] + ['-Wl,-rpath,' + d for d in rt], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        env = dict(os.environ, ASAN_OPTIONS='detect_leaks=0:abort_on_error=0:exitcode=66', LD_LIBRARY_PATH=':'.join(rt + [os.environ.get('LD_LIBRARY_PATH', '')]))
        r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
        assert r.returncode == 0 and 'all error paths returned their status' in r.stdout, r.stdout + r.stderr
        assert 'AddressSanitizer' not in r.stderr, r.stderr


def test_host_checks_as_a_stand_alone_program_under_the_sanitizers(tmp_path):
    """tools/nmf_temp_host_check.cpp: csrc/nagp_nmf_temp_check.hpp -- every check and the byte rule -- with its own main under
    -fsanitize=address,undefined, on exactly-sized heap blocks; no device, nothing loaded into Python"""
    exe = str(tmp_path / 'nmf_temp_host_check')
    r = subprocess.run(['c++', '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined', '-I',
                        os.path.join(ROOT, 'nonstationary-audio-gp_amd', 'csrc'), '-o', exe, os.path.join(ROOT, 'tools', 'nmf_temp_host_check.cpp')],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=dict(os.environ, ASAN_OPTIONS='detect_leaks=1:exitcode=66'))
    assert r.returncode == 0 and 'all host checks returned their status' in r.stdout, r.stdout + r.stderr
    assert 'Sanitizer' not in r.stderr and 'runtime error' not in r.stderr, r.stderr
