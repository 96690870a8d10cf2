"""Host tests (no GPU) of the Laplace step of GPPAD: the NumPy restatement tests/gppad_lap_ref.py against the 60-digit fixture
tests/golden/gppad_lap_multiprecision.npz (tools/make_gppad_lap_fixture.py), the stability of the Lanczos cases, the checks of a Lanczos
run that do not depend on its decisions, the tridiagonal eigen-solver and the kernel bodies as stand-alone programs under the host
sanitizers, the refusals of the ABI, and the drivers of nagp.gppad_lap with the restatement injected."""
import atexit
import functools
import os
import re
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nagp
from nagp import _lib as L
from nagp import gppad_lap as gl
import gppad_lap_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXED = sorted(ref.FIXED)
STABLE = sorted(ref.STABLE)
HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
SAN = ['-x', 'hip', '--offload-host-only', '-O1', '-g', '-std=c++17', '-Xarch_host', '-fsanitize=address,undefined', '-Xarch_host', '-fno-sanitize-recover=undefined',
       '-I', L.CSRC]
SAN_ENV = dict(os.environ, ASAN_OPTIONS='detect_leaks=0:exitcode=66')


@functools.lru_cache(maxsize=None)
def fixture():
    return dict(np.load(os.path.join(ROOT, 'tests', 'golden', 'gppad_lap_multiprecision.npz')))


@functools.lru_cache(maxsize=None)
def clean(name):
    return ref.solve(ref.stable_case(name))


@pytest.mark.parametrize('name', FIXED)
def test_restatement_matches_the_multiprecision_fixture(name):
    """d, A v, Varx from given pairs and the three terms of the objective, forward and reverse, within 1e-12 of the 60-digit values; the
    extended-precision form (the GPU tests' reference at the sizes the fixture does not hold) within 1e-15"""
    f = fixture(); c = ref.fixed_case(name)
    for ext in (False, True):
        for reverse in ((False,) if ext else (False, True)):
            d = ref.hessian(c['x'], c['y'], c['varc'], c['vary'], ext=ext); hs = ref.hhalf(c['len'], c['Tx'], c['varx'], ext=ext)
            got = dict(d=d, Av=ref.apply(c['v'], d, hs, reverse, ext), Varx=ref.varx_from(c['xv'], c['lmb'], hs, c['varx'], reverse, ext))
            O = ref.obj_terms(c['x'], c['y'], c['len'], c['varx'], c['mux'], c['varc'], c['vary'], c['lmb'], reverse, ext)
            for k, v in got.items():
                assert ref.dist(np.asarray(v, float), f['%s_%s' % (name, k)]) < (1e-15 if ext else 1e-12), (name, k, ext, reverse)
            assert np.all(np.abs(np.asarray(O, float) - f[name + '_Obj']) <= (1e-15 if ext else 1e-12) * np.abs(f[name + '_Obj'])), (name, ext, reverse, O)


def test_fixture_covers_what_it_must():
    f = fixture()
    assert {ref.FIXED[n][:2] for n in FIXED} >= {(20, 32), (200, 256), (256, 256)}
    for n in FIXED:                                          # the three branches of GetAmp and both forms of vary are among the cases
        assert f[n + '_d'].shape == (ref.FIXED[n][0],) and f[n + '_Av'].shape == f[n + '_Varx'].shape == (ref.FIXED[n][1],) and f[n + '_Obj'].shape == (3,)
    x = ref.fixed_case('f50_64')['x'][:50]
    assert np.any(x > 500) and np.any(x < -30) and np.any(np.abs(x) < 30) and np.ndim(ref.fixed_case('f50_64')['vary']) == 1
    assert np.ndim(ref.fixed_case('f200_256')['vary']) == 0
    assert np.any(ref.LMB_GIVEN < 0) and np.any(ref.LMB_GIVEN == 0)
    assert {ref.STABLE[n][1] for n in STABLE} >= {32, 256, 512, 4096, 8192, 16384}
    assert any(ref.STABLE[n][0] == ref.STABLE[n][1] for n in STABLE) and any(ref.STABLE[n][0] % 64 for n in STABLE)


@pytest.mark.parametrize('name', STABLE)
def test_the_lanczos_cases_are_stable(name):
    """the clean run gives the stored counts, lmb and Varx; four runs with every operator product times 1 + 1e-15 g and the run with
    every sum reversed give the same (steps, reorthogonalisations, nconv), and the perturbed runs stay within the stored self-deviation"""
    f = fixture(); c = ref.stable_case(name); run = clean(name)
    assert ref.counts(run) == tuple(f[name + '_counts']) and run['status'] == 0
    assert np.array_equal(run['lmb'], f[name + '_lmb']) or ref.dist(run['lmb'], f[name + '_lmb']) < 1e-13
    assert ref.dist(run['Varx'], f[name + '_Varx']) < 1e-10
    assert ref.counts(ref.solve(c, reverse=True)) == ref.counts(run)
    for k in range(4):
        p = ref.solve(c, perturb=np.random.default_rng(7700 + k))
        assert ref.counts(p) == ref.counts(run), (name, k)
        if run['nconv']:
            assert ref.dist(p['lmb'], run['lmb']) <= 1.01 * f[name + '_selfdev'][0] + 1e-18 and ref.dist(p['Varx'], run['Varx']) <= 1.01 * f[name + '_selfdev'][1] + 1e-18


def test_the_edge_cases_end_where_they_should():
    assert ref.counts(clean('s200_256_short'))[0] == 16 and clean('s200_256_short')['nconv'] <= 1          # the run ends at jmax
    j2 = clean('s200_256_j2')
    assert ref.counts(j2) == (2, 0, 0) and j2['lmb'].size == 0 and np.all(j2['Varx'] == ref.VARX)


@pytest.mark.parametrize('name', STABLE)
def test_every_returned_pair_is_an_eigenpair(name):
    """|A xv_k - lmb_k xv_k| <= 2 tolconv anorm: in exact arithmetic the Lanczos bound is this residual, rounding adds about eps j anorm"""
    run = clean(name)
    if run['nconv']:
        assert np.max(ref.residuals(run, run['d'], run['hs'])) <= 2 * ref.TOLCONV * run['anorm']


def test_lmb_are_the_leading_eigenvalues_of_the_dense_matrix():
    run = clean('s200_256')
    ev = np.linalg.eigvalsh(ref.dense(run['d'], run['hs']))[::-1]
    assert np.max(np.abs(run['lmb'] - ev[:run['nconv']])) <= 2 * ref.TOLCONV * run['anorm']


# ---------------------------------------------------------------------------------------------------------------- stand-alone programs
@functools.lru_cache(maxsize=None)
def program(src):
    td = tempfile.mkdtemp(prefix='nagp_lap_')
    atexit.register(shutil.rmtree, td, True)
    exe = os.path.join(td, os.path.splitext(src)[0])
    r = subprocess.run([HIPCC] + SAN + ['-o', exe, os.path.join(ROOT, 'tests', 'c', src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def run_program(exe, data):
    with tempfile.TemporaryDirectory() as td:
        fi, fo = os.path.join(td, 'in.bin'), os.path.join(td, 'out.bin')
        np.asarray(data, float).tofile(fi)
        r = subprocess.run([exe, fi, fo], capture_output=True, text=True, timeout=600, env=SAN_ENV)
        assert r.returncode == 0 and r.stdout.rstrip().endswith('ok'), r.stdout + r.stderr
        assert 'Sanitizer' not in r.stderr and 'runtime error' not in r.stderr, r.stderr
        return np.fromfile(fo), r.stdout


@pytest.mark.parametrize('n', [1, 2, 37, 200])
def test_tridiagonal_eigen_solver(n):
    """tests/c/tridiag_check.cpp: the implicit QL of csrc/nagp_tridiag.hpp against numpy.linalg.eigh on a drawn matrix (eigenvalues to
    1e-13 of the largest, every vector an eigenvector to the same, the one-row run equal to the last row of the full run) and against
    2 - 2 cos(k pi / (n + 1)) inside the program"""
    rng = np.random.default_rng(50 + n)
    d = rng.standard_normal(n) * 3; e = np.concatenate([[0.0], rng.standard_normal(n - 1)])
    out, text = run_program(program('tridiag_check.cpp'), np.concatenate([[n], d, e]))
    ev, last, Z = out[:n], out[n:2 * n], out[2 * n:].reshape(n, n)
    Tm = np.diag(d) + np.diag(e[1:], 1) + np.diag(e[1:], -1)
    want = np.linalg.eigvalsh(Tm); scale = max(np.max(np.abs(want)), 1.0)
    assert np.max(np.abs(ev - want)) <= 1e-13 * scale and np.all(np.diff(ev) >= 0)
    assert np.max(np.abs(Tm @ Z - Z * ev)) <= 1e-13 * scale * n and np.max(np.abs(Z.T @ Z - np.eye(n))) <= 1e-13 * n
    assert np.array_equal(last, Z[n - 1])
    assert 'toeplitz error' in text


@pytest.mark.parametrize('name', ['s20_32', 's200_256', 's333_512', 's5000_8192', 's200_256_short', 's200_256_j2'])
def test_kernel_bodies_on_the_host_under_the_sanitizers(name):
    """tests/c/gppad_lap_host_check.cpp: the kernel bodies, one "thread" per workgroup, in the sequence the entry points launch them, a
    batch of two problems that stop at different steps, host code only, under AddressSanitizer and UndefinedBehaviorSanitizer (a stand-alone
    program: nothing of it is loaded into Python).  Problem 0 is the stable case: the counts of the restatement, d and A vstart within
    1e-12, lmb and Varx within 32 x the stored self-deviation (floor 1e-15), every pair an eigenpair of the restatement's operator."""
    f = fixture(); c = ref.stable_case(name); run = clean(name); T, Tx, jmax = c['T'], c['Tx'], c['jmax']
    head = [T, Tx, c['nev'], jmax, c['len'], c['varx'], c['mux'], c['varc'], c['vary']]
    out, text = run_program(program('gppad_lap_host_check.cpp'), np.concatenate([head, c['x'], c['y'], c['vstart']]))
    info = out[:5]; lmb = out[5:5 + jmax]; p = 2 * (5 + jmax); nc = int(info[2])
    assert tuple(int(q) for q in info[:3]) == ref.counts(run) and info[3] == 0 and np.all(np.isnan(lmb[nc:]))
    assert abs(info[4] - run['anorm']) <= 1e-12 * run['anorm']
    d, Av, Varx, xv = out[p:p + T], out[p + T:p + T + Tx], out[p + T + Tx:p + T + 2 * Tx], out[p + T + 2 * Tx:].reshape(nc, Tx)
    assert ref.dist(d, run['d']) < 1e-12 and ref.dist(Av, ref.apply(c['vstart'], run['d'], run['hs'])) < 1e-12
    if nc:
        sd = f[name + '_selfdev']
        assert ref.dist(lmb[:nc], run['lmb']) <= 32 * max(sd[0], 1e-15) and ref.dist(Varx, run['Varx']) <= 32 * max(sd[1], 1e-15)
        assert np.max(ref.residuals(dict(xv=xv, lmb=lmb[:nc]), run['d'], run['hs'])) <= 2 * ref.TOLCONV * run['anorm']
    else:
        assert np.all(Varx == c['varx'])


def test_exported_and_bound():
    nagp.build()
    out = subprocess.run(['nm', '-D', '--defined-only', L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    names = {'nagp_gppad_lap_' + k for k in ('create', 'hess', 'apply', 'eig', 'varx', 'obj', 'destroy', 'timings')}
    assert names <= set(re.findall(r' T (nagp_[a-z0-9_]+)', out)) and names <= set(L.EXPORTS)
    hdr = open(os.path.join(ROOT, 'include', 'nagp.h')).read()
    assert all(re.search(r'\b%s\(' % n, hdr) for n in names)
    for n in ('GppadLapHandle', 'GetHessian', 'SigDSigTimesV', 'LanczosGPPAD', 'GetEigSigDSig', 'GetErrorBarGPPAD', 'GetLaplaceObjGPPADOneChunk',
              'GetLaplaceObjGPPAD', 'InferAmplitudeErrorBarsGPMAP', 'LoadLearnLenGradAscentGPPADOpts', 'LoadErrorBarsLapOpts'):
        assert hasattr(nagp, n), n


def test_argument_checks_in_plain_c():
    """tests/c/abi_gppad_lap_errors.c: a stand-alone C program on exactly-sized heap blocks against libnagp_asan.so (the host code of the C
    ABI built with AddressSanitizer), on the CPU only: every invalid call returns its status and ASan reports nothing."""
    lib = nagp.build(asan=True)
    clang = '/opt/rocm/llvm/bin/clang'
    rt = sorted({os.path.dirname(p) for p in subprocess.run([clang, '-print-file-name=libclang_rt.asan-x86_64.so'], capture_output=True, text=True).stdout.split()})
    with tempfile.TemporaryDirectory() as td:
        exe = os.path.join(td, 'abi_gppad_lap_errors')
        r = subprocess.run([clang, '-fsanitize=address', '-shared-libsan', '-g', '-O1', '-std=c99', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'include'),
                            '-o', exe, os.path.join(ROOT, 'tests', 'c', 'abi_gppad_lap_errors.c'), lib, '-lm', '-Wl,-rpath,/opt/rocm/lib',
                            '-Wl,-rpath-link,/opt/rocm/lib'] + ['-Wl,-rpath,' + d for d in rt], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        env = dict(os.environ, ASAN_OPTIONS='detect_leaks=0:exitcode=66')
        r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
        assert r.returncode == 0 and 'all error paths returned their status' in r.stdout, r.stdout + r.stderr
        assert 'AddressSanitizer' not in r.stderr, r.stderr


# ---------------------------------------------------------------------------------------------------------------- the drivers
def test_option_loaders():
    o = nagp.LoadErrorBarsLapOpts(dict(nev=16))
    assert (o['Overlap'], o['nev'], o['tol'], o['TruncPoint'], o['MinLength'], o['NumIts'], o['NumItsLL'], o['m']) == (5, 16, 8, 8, 8, 2000, 30, 0.5)
    assert o['loglenLR0'] == np.log(1.2) and 'Overlap' not in nagp.LoadLearnLenGradAscentGPPADOpts()


OPTS = dict(nev=8, TruncPoint=8, tol=1, Overlap=1, NumIts=4, MinLength=8)


def test_chunk_plan():
    """len = 4, nev = 8, TruncPoint = 8, tol = 1, Overlap = 1: TxCh = 2^floor(log2(floor(2 pi 8 4 / 8))) = 16, TCh = 12, Overlap = 4, a new
    chunk every 8 samples; T = 8, 14 and 30 need 1, 2 and 4 chunks, the last of T = 30 six samples short"""
    p = gl.chunk_plan(8, 4.0, OPTS)
    assert (p['TxCh'], p['TCh'], p['Overlap'], p['NumChunks'], p['bounds']) == (16, 12, 4, 1, [(0, 8)])
    assert gl.chunk_plan(14, 4.0, OPTS)['bounds'] == [(0, 12), (8, 14)]
    p = gl.chunk_plan(30, 4.0, OPTS)
    assert p['bounds'] == [(0, 12), (8, 20), (16, 28), (24, 30)]
    taper = np.cos(2 * np.pi * np.array([1, 2, 3, 4]) / 16.0) ** 2
    assert np.array_equal(p['WindowStart'], np.r_[np.ones(8), taper]) and np.array_equal(p['WindowEnd'], np.r_[taper[::-1], np.ones(8)])
    assert np.array_equal(p['Window'], np.r_[taper[::-1], np.ones(4), taper]) and p['Window'].size == 12
    with pytest.raises(ValueError, match='TCh'):
        gl.chunk_plan(100, 4.0, dict(OPTS, tol=8))


@pytest.mark.parametrize('T', [8, 14, 30])
def test_InferAmplitudeErrorBarsGPMAP_on_the_restatement(T):
    """the driver with the MAP objective and the Laplace step of the restatements injected: x and Varx are the windowed sums of the
    chunks' results (InferAmplitudeErrorBarsGPMAP.m:118-140), a = log(1 + exp(x)), Borders = tend - Overlap / 2, the chunks of equal T
    are solved together and the start vectors are drawn chunk by chunk"""
    y, _ = ref.g1.envelope_signal(T, 4.0, 17)
    Params = dict(len=4.0, varx=1.0, mux=0.0, varc=1.0, vary=np.linspace(0.0, 0.2, T))
    rec = []; calls = []
    inner = ref.laplace()

    def solver(chunks, nev, rng, vstart):
        calls.append([c['y'].size for c in chunks])
        return inner(chunks, nev, rng, vstart)
    a, x, Varx, Info = nagp.InferAmplitudeErrorBarsGPMAP(y, Params, OPTS, rng=np.random.default_rng(3), evaluator=ref.g1.evaluator(), laplace=solver, record=rec)
    plan = gl.chunk_plan(T, 4.0, OPTS); N = plan['NumChunks']
    assert len(rec) == N == Info['NumChunks'] and sorted(sum(calls, [])) == sorted(b - a_ for a_, b in plan['bounds'])
    assert all(len(set(c)) == 1 for c in calls) and len(calls) == len({b - a_ for a_, b in plan['bounds']})
    rng = np.random.default_rng(3)
    draws = [rng.standard_normal(16) for _ in range(N)]
    by_start = {c['y'][0]: (c, r) for c, r in rec}
    xs = np.zeros(T); Vs = np.zeros(T)
    for ch, (t0, t1) in enumerate(plan['bounds']):
        c, r = by_start[y[t0]]; n = t1 - t0
        assert np.array_equal(r['vstart'], draws[ch]) and np.array_equal(c['Params']['vary'], Params['vary'][t0:t1]) and c['x'].size == 16
        W = np.ones(n) if N == 1 else (plan['WindowStart'] if ch == 0 else plan['WindowEnd'] if ch == N - 1 else plan['Window'])[:n]
        xs[t0:t1] += c['x'][:n] * W; Vs[t0:t1] += r['Varx'][:n] * W
    assert np.array_equal(x, xs) and np.array_equal(Varx, Vs) and np.array_equal(a, np.log(1 + np.exp(x)))
    assert np.array_equal(Info['Borders'], np.array([t1 - 2.0 for _, t1 in plan['bounds']])) and Info['steps'].shape == (N,)
    with pytest.raises(ValueError, match='rng'):
        nagp.InferAmplitudeErrorBarsGPMAP(y, Params, OPTS, evaluator=ref.g1.evaluator(), laplace=solver)


def test_GetLaplaceObjGPPAD_on_the_restatement():
    """chunks of TCh samples, the last one shorter, every chunk an independent data set: the sum of Obj0 + Obj1 + Obj2 in chunk order"""
    y, _ = ref.g1.envelope_signal(30, 4.0, 19)
    Params = dict(len=4.0, varx=1.0, mux=0.0, varc=1.0, vary=0.05)
    info = {}; rec = []
    Obj = nagp.GetLaplaceObjGPPAD(y, Params, dict(OPTS, TCh=12, TxCh=16), rng=np.random.default_rng(4), evaluator=ref.g1.evaluator(), laplace=ref.laplace(),
                                  record=rec, info=info)
    assert info['NumChunks'] == 3 and info['Obj'].shape == (3, 3) and sorted(c['y'].size for c, _ in rec) == [6, 12, 12]
    want = 0.0
    for row in info['Obj']:
        want = want + float(row[0] + row[1] + row[2])
    assert Obj == want and np.isfinite(Obj) and np.all(info['Obj'][:, 0] <= 0)
    one = {}
    c, r = rec[0]
    O1 = nagp.GetLaplaceObjGPPADOneChunk(c['x'], c['y'], c['Params'], c['Dims'], OPTS, vstart=r['vstart'], laplace=ref.laplace(), info=one)
    assert O1 == float(r['Obj'][0] + r['Obj'][1] + r['Obj'][2]) and np.array_equal(one['Obj'], r['Obj'])
    V = nagp.GetErrorBarGPPAD(c['x'], c['y'], c['Params'], c['Dims'], OPTS, vstart=r['vstart'], laplace=ref.laplace())
    assert np.array_equal(V, r['Varx'])


def test_GetLaplaceObjGPPADMulti_on_the_restatement():
    """Len = [4, 5], nev = 8, TruncPoint = 8, tol = 1: TxMax = 2^ceil(log2(2 pi 4)) = 32, TCh = 28, TxCh = GetTx(28, 5) = 64; T = 60 gives
    three chunks per time-scale, all six through the solver, the start vectors drawn time-scale by time-scale; Objs are the chunk sums"""
    y, _ = ref.g1.envelope_signal(60, 4.0, 29)
    Params = dict(len=99.0, varx=1.0, mux=0.0, varc=1.0, vary=0.05)
    rec = []
    Len, Objs, Info = nagp.GetLaplaceObjGPPADMulti([4.0, 5.0], y, Params, OPTS, rng=np.random.default_rng(9), evaluator=ref.g1.evaluator(), laplace=ref.laplace(), record=rec)
    assert (Info['TCh'], Info['TxCh'], Info['NumChunks']) == (28, nagp.GetTx(28, 5.0), 3) and len(rec) == 6
    rng = np.random.default_rng(9)
    by = {(c['Params']['len'], c['y'].size, c['y'][0]): r for c, r in rec}
    want = np.zeros(2)
    for l, ell in enumerate((4.0, 5.0)):
        for a in (0, 28, 56):
            r = by[(ell, min(60, a + 28) - a, y[a])]
            assert np.array_equal(r['vstart'], rng.standard_normal(Info['TxCh']))
            want[l] = want[l] + float(r['Obj'][0] + r['Obj'][1] + r['Obj'][2])
    assert np.array_equal(Objs, want) and Info['MaxLoc'] == (-1 if Objs[0] >= Objs[1] else 1) and np.array_equal(Len, [4.0, 5.0])


def test_stitching_offsets_and_LenMax():
    """a hand-made objective f(len) that every call of `multi` returns with another offset (as another set of chunks would): the stitched
    curve is f up to the first segment's offset; MaxLoc of three points; LenMax lists both local optima of a two-humped f"""
    f = lambda L_: -np.sin(2.2 * np.log(L_)) - 0.05 * np.log(L_)
    calls = []

    def multi(Len, y, Params, Opts):
        calls.append(np.array(Len))
        return Len, f(np.asarray(Len)) + 10.0 * len(calls), {}
    Objs, Lens = nagp.GetLaplaceObjGPPADStitched([2.0, 200.0], 13, None, {}, {}, multi=multi)
    step = np.log(100.0) / 12; per = int(np.sum(np.arange(13) * step < np.log(3.0)))
    assert np.allclose(Lens, 2.0 * np.exp(step * np.arange(13))) and all(c.size <= per for c in calls) and len(calls) == int(np.ceil(12 / (per - 1)))
    assert all(calls[k][0] == calls[k - 1][-1] for k in range(1, len(calls)))          # neighbouring segments share one time-scale
    assert np.max(np.abs(Objs - (f(Lens) + 10.0))) < 1e-12
    ell, Info = nagp.GetLenGridSearch([2.0, 200.0], None, {}, dict(NumLens=13), multi=multi)
    k = int(np.argmax(f(Lens)))
    assert ell == Lens[k] and not Info['AtEdge']
    inner = [Lens[i] for i in range(1, 12) if f(Lens)[i] > f(Lens)[i - 1] and f(Lens)[i] > f(Lens)[i + 1]]
    assert len(Info['LenMax']) == 2 == len(inner) and np.array_equal(Info['LenMax'], inner)
    Objs2, Lens2 = nagp.GetLaplaceObjGPPADStitched([2.0, 50.0], None, None, {}, {}, multi=multi)          # NumLens = ceil(log(25) / log 3) + 1 = 4
    assert Lens2.size == 4
    with pytest.raises(ValueError, match='separation'):
        nagp.GetLaplaceObjGPPADStitched([2.0, 200.0], 3, None, {}, {}, multi=multi)
    for objs, loc in (([3.0, 1.0, 2.0], -1), ([1.0, 3.0, 2.0], 0), ([1.0, 2.0, 3.0], 1)):
        y, _ = ref.g1.envelope_signal(20, 4.0, 2)
        it = iter(objs)
        sol = lambda chunks, nev, rng, vstart: [dict(lmb=np.zeros(0), Varx=np.ones(32), Obj=np.array([0.0, next(it), 0.0]), steps=1, reorths=0, nconv=0, n_negative=0,
                                                     vstart=vstart[i]) for i in range(len(chunks))]
        _, O, I = nagp.GetLaplaceObjGPPADMulti([4.0, 4.5, 5.0], y, dict(len=1.0, varx=1.0, mux=0.0, varc=1.0, vary=0.0), OPTS, rng=np.random.default_rng(1),
                                               evaluator=ref.g1.evaluator(), laplace=sol)
        assert I['MaxLoc'] == loc and np.array_equal(O, objs)


def test_sign_ascent_trajectory():
    """GetLenGradAscent on a hand-made objective with its maximum at len = 20, from len = 5: the trajectory of the .m's update, restated
    here step by step; the prior term mulen / varlen; the stretches (Ts) from tstart= and from rng"""
    opts = nagp.LoadLearnLenGradAscentGPPADOpts(dict(NumItsLL=12, nev=8, TruncPoint=8, tol=1))
    seen = []

    def multi(Len, y, Params, Opts):
        seen.append((np.array(Len), y.size))
        return Len, -(np.log(Len) - np.log(20.0)) ** 2, {}
    y = np.arange(5000.0)
    ell, Info = nagp.GetLenGradAscent(5.0, y, dict(vary=0.0), opts, rng=np.random.default_rng(2), multi=multi)
    L_ = 5.0; last = 0.0; rng = np.random.default_rng(2)
    lr = np.log(1.2) / (1 + np.arange(13) / 6.0)
    for it in range(12):
        TMax = int(np.floor(2 ** np.ceil(np.log2(2 * np.pi * L_)) - L_))
        t0 = 1 + int(np.floor(rng.random() * (5000 - TMax)))
        assert tuple(Info['Ts'][it]) == (t0, t0 - 1 + TMax) and seen[it][1] == TMax and np.array_equal(seen[it][0], [L_, max(L_ + 1, 1.01 * L_)])
        g = lambda q: -(np.log(q) - np.log(20.0)) ** 2
        up = float(np.sign(g(max(L_ + 1, 1.01 * L_)) - g(L_)))
        d = up * lr[it] + 0.5 * last
        last = d; L_ = float(np.exp(np.log(L_) + d))
        assert abs(Info['LenHist'][it] - L_) <= 1e-12 * L_
    assert abs(ell - L_) <= 1e-12 * L_ and np.array_equal(Info['loglenLR'], lr) and abs(np.log(ell / 20.0)) < 0.3
    _, I2 = nagp.GetLenGradAscent(5.0, y, dict(vary=0.0, mulen=3.0, varlen=1e-3), dict(opts, NumItsLL=2), tstart=[7, 9], multi=multi)
    assert I2['Ts'][0, 0] == 7 and I2['Ts'][1, 0] == 9 and np.all(I2['dObjHist'] < 0) and I2['LenHist'][1] < I2['LenHist'][0] < 5.0
    with pytest.raises(ValueError, match='rng'):
        nagp.GetLenGradAscent(5.0, y, dict(vary=0.0), opts, multi=multi)


def test_FBGPMAPLearnLen_on_the_restatement():
    """two channels with given parameters and nout = 8, in lock-step: every channel is InferAmplitudeErrorBarsGPMAP on it with the
    channel's child stream, A carries sqrt(varc), the bands are the envelopes at x +- 3 sqrt(Varx); the chunks of both channels reach the
    solver together; nout = 5 is the plain MAP step; LearnLengths = 1 and 2 move len, in lock-step as one channel at a time"""
    y, _ = ref.g1.envelope_signal(30, 4.0, 31)
    Y = np.stack([y, 0.5 * y[::-1]], axis=1)
    P = dict(len=4.0, varx=1.0, varc=np.array([1.0, 0.25]), mux=0.0, vary=0.01)
    calls = []; inner = ref.laplace()

    def solver(chunks, nev, rng, vstart):
        calls.append(len(chunks))
        return inner(chunks, nev, rng, vstart)
    kw = dict(evaluator=ref.g1.evaluator(), laplace=solver)
    A, X, C, Params, Info, Varx, Au, Al = nagp.FBGPMAPLearnLen(Y, P, OPTS, nout=8, rng=np.random.default_rng(11), **kw)
    assert sorted(calls) == [2, 6]                           # T = 30: three chunks of 12 and one of 6 per channel, both channels together
    kids = np.random.default_rng(11).spawn(2)
    for d in range(2):
        a, x, vx, _ = nagp.InferAmplitudeErrorBarsGPMAP(Y[:, d], dict(len=4.0, varx=1.0, varc=P['varc'][d], mux=0.0, vary=0.01), OPTS, rng=kids[d], **kw)
        s = np.sqrt(P['varc'][d])
        assert np.array_equal(X[:, d], x) and np.array_equal(Varx[:, d], vx) and np.array_equal(A[:, d], s * a) and np.array_equal(C[:, d], Y[:, d] / (s * a))
        assert np.array_equal(Au[:, d], s * np.log(1 + np.exp(x + 3 * np.sqrt(vx)))) and np.all(Al[:, d] <= A[:, d]) and np.all(A[:, d] <= Au[:, d])
    assert np.array_equal(Params['len'], [4.0, 4.0]) and np.array_equal(Params['varc'], P['varc']) and len(Info) == 2
    out = nagp.FBGPMAPLearnLen(Y[:, 0], dict(P, varc=1.0), OPTS, evaluator=ref.g1.evaluator())
    assert len(out) == 5 and out[0].shape == (30, 1)
    y, _ = ref.g1.envelope_signal(58, 4.0, 37)             # 58 samples: two whole chunks of TCh = 29 at min(Len) = 3
    Y = np.stack([y, 0.5 * y[::-1]], axis=1)
    for opts in (dict(OPTS, LearnLengths=1, NumItsLL=2), dict(OPTS, LearnLengths=2, LenRng=[3.0, 6.0], NumLens=3)):
        both = nagp.FBGPMAPLearnLen(Y, P, opts, rng=np.random.default_rng(1), **kw)
        kids = np.random.default_rng(1).spawn(2)
        for d in range(2):
            alone = nagp.FBGPMAPLearnLen(Y[:, d], dict(P, varc=P['varc'][d]), opts, rng=[kids[d]], **kw)
            assert both[3]['len'][d] == alone[3]['len'][0] and np.array_equal(both[1][:, d], alone[1][:, 0]) and np.array_equal(both[0][:, d], alone[0][:, 0]), (opts, d)
        assert np.all(both[3]['len'] != 4.0) or opts['LearnLengths'] == 2
    assert both[4][0][1]['Lens'].shape == (3,)
