"""nagp_nmf_fp (the fixed-point NMF of experiments/nmf/nmf_fp.m / nmf_inf_fp.m) and the host mirrors around it, without a GPU: the
yardstick -- tests/nmf_ref.py against the multi-precision fixture tests/golden/nmf_multiprecision.npz --, the quirks the mirrors keep,
the export and its binding, and the argument checks of include/nagp.h, which answer on a machine with no device (they run before any
device call).  Distances are the project's norm max|d| / max|ref| per array."""
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
from nagp import nmf as nm
import nmf_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EUNSUPPORTED = -1, -2
CASES = sorted(ref.CASES)


@functools.lru_cache(maxsize=None)
def fixture():
    return dict(np.load(os.path.join(ROOT, 'tests', 'golden', 'nmf_multiprecision.npz')))


@pytest.mark.parametrize('update_w', [1, 0])
@pytest.mark.parametrize('name', CASES)
def test_restatement_matches_the_multiprecision_fixture(name, update_w):
    """e_ref per array: what the GPU tests measure the kernels against.  Bound 1e-13: the float64 restatement against an 80-bit run of
    itself measured 4e-16 ... 3e-15 on cases a-d, which leaves a factor 30."""
    f = fixture(); c = ref.case(name)
    assert np.array_equal(c['W0'], f[name + '_W0']) and c['A'].sum() == f[name + '_sumA'] and c['H0'].sum() == f[name + '_sumH0']
    W, H, Obj = ref.iterate(c['A'], c['vary'], c['W0'], c['H0'], c['its'], update_w=bool(update_w))
    sfx = '_w%d' % update_w
    e = dict(W=ref.dist(W, f[name + '_W' + sfx]), H=ref.dist(H, f[name + '_H' + sfx]), Obj=ref.dist(Obj, f[name + '_Obj' + sfx]))
    print('e_ref %s update_w=%d: ' % (name, update_w) + '  '.join('%s %.2e' % kv for kv in e.items()))
    assert Obj.size == (2 if update_w else 1) * c['its'] and H.shape == c['H0'].shape and W.shape == c['W0'].shape
    assert max(e.values()) < 1e-13, e
    if not update_w:
        assert np.array_equal(W, c['W0'])


def test_objective_of_every_fixture_case_is_monotone():
    """Obj of nmf_fp.m is non-increasing to 1e-12 on every case (vary = 1e-3 or absent), despite the missing vary of nmf_fp.m:81.
    A case whose fixture is itself not monotone would be left out of the assertion; at most one may be."""
    f = fixture(); left_out = []
    for name in CASES:
        Obj = f[name + '_Obj_w1']
        if np.all(np.diff(Obj) <= 1e-12 * np.maximum(1.0, np.abs(Obj[:-1]))):
            continue
        left_out.append(name)
    print('not monotone in the fixture:', left_out)
    assert len(left_out) <= 1, left_out
    for name in CASES:
        if name in left_out:
            continue
        c = ref.case(name)
        _, _, Obj = ref.iterate(c['A'], c['vary'], c['W0'], c['H0'], c['its'])
        assert np.all(np.diff(Obj) <= 1e-12 * np.maximum(1.0, np.abs(Obj[:-1]))), name


def test_line_37_normalises_only_when_every_row_sum_differs_from_one():
    W = np.array([[0.25, 0.75], [2.0, 6.0]])                 # first row sums to exactly 1: MATLAB's `if` on the vector is false
    assert np.array_equal(nm.inf_normalise(W), W)
    assert np.array_equal(ref.normalise(W)[1], [0.25, 0.75])
    W2 = np.array([[0.5, 1.5], [2.0, 6.0]])                  # every row differs: normalised
    assert np.array_equal(nm.inf_normalise(W2), [[0.25, 0.75], [0.25, 0.75]])
    H, Obj = ref.nmf_inf_fp(np.ones((3, 2)), W, np.ones((3, 2)), None, 1)      # the restatement keeps the same quirk
    H2, _ = ref.iterate(np.ones((3, 2)), None, W, np.ones((3, 2)), 1, update_w=False)[1:]
    assert np.array_equal(H, H2)


def test_restart_selection_keeps_the_first_of_a_tie():
    assert nm.pick_restart(np.array([3.0, 2.0, 2.0, 5.0])) == 1
    assert nm.pick_restart(np.array([2.0, 2.0])) == 0
    assert nm.pick_restart(np.array([np.nan, 4.0, 1.0])) == 2          # NaN < x is false
    c = ref.case('a')
    cands = [(c['W0'], c['H0']), (c['W0'] * 2.0, c['H0']), (c['A'][[5, 9, 200]], c['H0'][::-1])]      # candidate 2 normalises to candidate 1
    best, W, H, last = ref.select_restart(c['A'], c['vary'], cands)
    assert last[0] == last[1] and best == int(np.argmin(last)) and (best != 1)
    assert nm.pick_restart(last) == best


def test_restart_candidates_follow_the_reference_order():
    A = np.arange(40.0).reshape(10, 4) + 1
    c = nm.restart_candidates(A, 3, 3, seed=5)
    rng = np.random.default_rng(5)
    for Wc, Hc in c:
        ks = np.ceil(10 * rng.random(3)).astype(int)
        assert np.array_equal(Wc, A[ks - 1]) and np.array_equal(Hc, np.exp(rng.standard_normal((10, 3))))
    assert len(c) == 2


@pytest.mark.parametrize('tau', [1, 2, 3])
def test_getFBLDSOutput_tau_index_sets(tau):
    """hand-written expectations: the state is [Re, Im] pairs, tau pairs per sub-band; S takes the first pair of every sub-band"""
    D, T = 2, 3; n2 = 2 * D * tau
    X = (np.arange(n2)[None, :, None] + 100.0 * np.arange(T)[None, None, :])
    P = np.arange(n2)[:, None, None] * 10.0 + np.arange(n2)[None, :, None] + 1000.0 * np.arange(T)[None, None, :]
    re = {1: [0, 2], 2: [0, 4], 3: [0, 6]}[tau]; im = {1: [1, 3], 2: [1, 5], 3: [1, 7]}[tau]
    fre = {1: [0, 2], 2: [0, 2, 4, 6], 3: [0, 2, 4, 6, 8, 10]}[tau]; fim = [i + 1 for i in fre]
    S, = nagp.getFBLDSOutput_tau(X, None, tau, 1)
    assert S.shape == (D, T) and np.array_equal(S, X[0][re] + 1j * X[0][im])
    S2, covS = nagp.getFBLDSOutput_tau(X, P, tau, 2)
    sel = re + im
    assert np.array_equal(S2, S) and covS.shape == (2 * D, 2 * D, T) and np.array_equal(covS, P[np.ix_(sel, sel)])
    S3, covS3, Sfull = nagp.getFBLDSOutput_tau(X, P, tau, 3)
    assert np.array_equal(covS3, covS) and np.array_equal(Sfull, X[0][fre] + 1j * X[0][fim]) and np.array_equal(S3, S)
    S4, covS4, Sfull4, covSfull = nagp.getFBLDSOutput_tau(X, P, tau, 4)
    fsel = fre + fim
    assert np.array_equal(covSfull, P[np.ix_(fsel, fsel)]) and np.array_equal(Sfull4, Sfull) and np.array_equal(S4, S)
    assert np.array_equal(nm.covS_rows(n2, tau), sorted(sel))


def test_exported_and_bound():
    nagp.build()
    out = subprocess.run(['nm', '-D', '--defined-only', L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert {'nagp_nmf_fp', 'nagp_nmf_timings'} <= set(re.findall(r' T (nagp_[a-z0-9_]+)', out))
    assert 'nagp_nmf_fp' in L.EXPORTS
    hdr = open(os.path.join(ROOT, 'include', 'nagp.h')).read()
    assert re.search(r'^int nagp_nmf_fp\(int32_t n_problems, int64_t T, int32_t D, int32_t K,', hdr, re.M)
    fn = L.lib().nagp_nmf_fp
    assert len(fn.argtypes) == 14 and fn.restype is C.c_int
    for name in ('nmf_run', 'nmf_fp', 'nmf_inf_fp', 'nmf_init', 'kernel_ss_probFB', 'getFBLDSOutput_tau'):
        assert getattr(nagp, name) is getattr(nm, name)


def call(A, vary, W0, H0, n_its=2, update_w=1, D=None, K=None):
    A = L.f64(A); T, D_ = A.shape; W0 = np.asarray(W0, float); K_ = W0.shape[0]
    w0 = L.f64(W0); h0 = L.f64(H0); v = None if vary is None else L.f64(vary)
    W = np.zeros_like(w0); H = np.zeros_like(h0); Obj = np.zeros(2 * max(n_its, 1))
    return L.lib().nagp_nmf_fp(1, T, D_ if D is None else D, K_ if K is None else K, L.dptr(A), L.dptr(v), L.dptr(w0), L.dptr(h0),
                               n_its, update_w, L.dptr(W), L.dptr(H), L.dptr(Obj), 0), W, H


def test_argument_errors_answer_without_a_device():
    nagp.build()
    c = ref.case('a'); A, v, W0, H0 = c['A'], c['vary'], c['W0'], c['H0']
    assert call(A, v, W0, H0, D=65)[0] == EUNSUPPORTED
    assert call(A, v, W0, H0, K=17)[0] == EUNSUPPORTED and b'16' in L.lib().nagp_last_error()
    for D, K, its in ((0, None, 2), (None, 0, 2), (None, None, -1)):
        assert call(A, v, W0, H0, n_its=its, D=D, K=K)[0] == EINVAL
    Ab = A.copy(); Ab[100, 2] = -1e-12
    assert call(Ab, v, W0, H0)[0] == EINVAL and b'A[' in L.lib().nagp_last_error()
    vb = v.copy(); vb[3, 1] = -1.0
    assert call(A, vb, W0, H0)[0] == EINVAL
    Wz = W0.copy(); Wz[1, :] = 0.0
    assert call(A, v, Wz, H0)[0] == EINVAL and b'row 1' in L.lib().nagp_last_error()
    Wc = W0.copy(); Wc[:, 4] = 0.0
    assert call(A, v, Wc, H0)[0] == EINVAL and b'column 4' in L.lib().nagp_last_error()
    Wn = W0.copy(); Wn[0, 0] = -0.5
    assert call(A, v, Wn, H0)[0] == EINVAL
    Hz = H0.copy(); Hz[256, 2] = 0.0
    assert call(A, v, W0, Hz)[0] == EINVAL and b'H0[' in L.lib().nagp_last_error()
    for bad in (np.nan, np.inf):
        Hb = H0.copy(); Hb[0, 0] = bad
        assert call(A, v, W0, Hb)[0] == EINVAL
        Ab = A.copy(); Ab[0, 0] = bad
        assert call(Ab, None, W0, H0)[0] == EINVAL
    st, W, H = call(A, v, W0, H0, n_its=0)                      # n_its = 0 copies the inputs through (no device needed)
    assert st == 0 and np.array_equal(W, W0) and np.array_equal(H, H0)
    with pytest.raises(ValueError):
        nagp.nmf_run(A, v, W0, H0[:-1], 2)


def test_argument_checks_under_the_address_sanitizer():
    """tests/c/abi_nmf_errors.c: a stand-alone C program on exactly-sized heap blocks against libnagp_asan.so (the host code of the C
    ABI built with AddressSanitizer), on the CPU only: every invalid call returns its status and ASan reports nothing."""
    import tempfile
    lib = nagp.build(asan=True)
    clang = '/opt/rocm/lib/llvm/bin/clang'
    rt = glob.glob('/opt/rocm/lib/llvm/lib/clang/*/lib/linux') + glob.glob('/opt/rocm/lib/llvm/lib/clang/*/lib/x86_64-unknown-linux-gnu')
    with tempfile.TemporaryDirectory() as td:
        exe = os.path.join(td, 'abi_nmf_errors')
        r = subprocess.run([clang, '-fsanitize=address', '-shared-libsan', '-g', '-O1', '-std=c99', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'include'),
                            '-o', exe, os.path.join(ROOT, 'tests', 'c', 'abi_nmf_errors.c'), lib, '-Wl,-rpath,/opt/rocm/lib',
                            '-Wl,-rpath-link,/opt/rocm/lib'] + ['-Wl,-rpath,' + d for d in rt], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        env = dict(os.environ, ASAN_OPTIONS='detect_leaks=0:abort_on_error=0:exitcode=66', LD_LIBRARY_PATH=':'.join(rt + [os.environ.get('LD_LIBRARY_PATH', '')]))
        r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
        assert r.returncode == 0 and 'all error paths returned their status' in r.stdout, r.stdout + r.stderr
        assert 'AddressSanitizer' not in r.stderr, r.stderr
