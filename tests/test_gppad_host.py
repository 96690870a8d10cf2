"""nagp_gppad_obj (the objective of experiments/gppad/GPModelFast/MAPGPFast.m: GetGPObjFast.m) and the host mirrors around it, without a
GPU: the yardstick -- tests/gppad_ref.py against the multi-precision fixture tests/golden/gppad_multiprecision.npz --, its gradient
against central differences, GetDSs, GetTx, resample2, InitPADSampleNonStat, LearnMarginalParams, the drivers InferAmplitudeGPMAP and
GPPAD on the restatement objective, the export and its binding, and the argument checks of include/nagp.h, which answer on a machine with
no device (they run before any device call).  Distances are the project's norm max|d| / max|ref| per array.

Bound of the restatement against the fixture: the division by c, which spans 1e-6 .. sqrt(2 pi) len, amplifies the rounding of the
forward transform by up to max(c) / min(c) (2.6e9 at len = 1024), so 1e-7, the TOL of the GPU tests, is what float64 can promise
on every case; measured on the CPU: Obj within 3.0e-15, dObj within 4.0e-11 (the smooth draws with len = Tx / 8), 5.9e-15 on the white ones."""
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
from nagp import gppad as gp
import gppad_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EUNSUPPORTED = -1, -2
CASES = sorted(ref.CASES)


@functools.lru_cache(maxsize=None)
def fixture():
    return dict(np.load(os.path.join(ROOT, 'tests', 'golden', 'gppad_multiprecision.npz')))


@pytest.mark.parametrize('name', CASES)
def test_restatement_matches_the_multiprecision_fixture(name):
    f = fixture(); c = ref.case(name)
    assert np.array_equal([c['x'].sum(), c['y'].sum()], f[name + '_sums'])
    for reverse in (False, True):
        Obj, dObj = ref.objective(c, reverse=reverse)
        e = ref.dist(Obj, f[name + '_Obj']), ref.dist(dObj, f[name + '_dObj'])
        print('e_ref %s reverse %d: Obj %.2e dObj %.2e' % (name, reverse, e[0], e[1]))
        assert dObj.shape == (c['Tx'],) and max(e) < 1e-7, e
        assert ref.objective(c, reverse=reverse, grad=False) == Obj


def test_fixture_covers_what_it_must():
    shapes = {ref.CASES[n][:2] for n in CASES}
    assert shapes >= {(2, 2), (3, 8), (50, 64), (64, 64), (257, 1024), (657, 1024), (3000, 4096), (4095, 4096), (5000, 8192), (20000, 32768)}
    assert {ref.CASES[n][2] for n in CASES} == {'smooth', 'white'} and {ref.CASES[n][6] for n in CASES} == {'given', 'len'}
    assert {type(ref.case(n)['vary']) for n in CASES} == {float, np.ndarray}
    assert any(ref.case(n)['vary'] == 0.0 for n in CASES if ref.CASES[n][5] != 'gap') and any(ref.CASES[n][5] not in (0.0, 'gap') for n in CASES)
    assert any(ref.CASES[n][4] is not None and ref.CASES[n][4] < 1 for n in CASES) and any(ref.CASES[n][4] is None for n in CASES)
    f = fixture()
    assert set(f) == {n + s for n in CASES for s in ('_Obj', '_dObj', '_sums')}                  # results (and two checksums) only
    for n in CASES:
        c = ref.case(n)
        assert f[n + '_dObj'].shape == (c['Tx'],) and np.isfinite(f[n + '_Obj']) and np.all(np.isfinite(f[n + '_dObj']))
        if ref.CASES[n][3]:
            assert {800.0, 501.0, -31.0, -40.0} <= set(c['x'][:c['T']])
    for n in CASES:                                            # x = 800: a = 800 and s = 1, not inf
        if ref.CASES[n][3]:
            assert np.isfinite(ref.objective(ref.case(n))[0])
    a = gp.GetAmp(np.array([800.0, 501.0, 500.0, -30.0, -31.0, -40.0]))
    assert a[0] == 800.0 and a[1] == 501.0 and a[2] == np.log1p(np.exp(500.0)) == 500.0 and a[4] == np.exp(-31.0) and a[5] == np.exp(-40.0)
    white = ref.case('c4095_4096')
    assert ref.objective(white, grad=False) > 1e3 and os.path.getsize(os.path.join(ROOT, 'tests', 'golden', 'gppad_multiprecision.npz')) < 1400000


@pytest.mark.parametrize('name', ['c3_8', 'c50_64', 'c257_1024'])
def test_gradient_against_central_differences(name):
    """every entry of dObj (the 64 first, the boundary at T and the last ones of the larger case) against a central difference of the
    restatement's Obj, step 1e-5 |x| + 1e-6, relative to the largest entry of dObj: the truncation error of the difference is
    h^2 f''' / 6 and its rounding error eps |Obj| / h, together of the order of 1e-7 on these shapes"""
    c = ref.case(name)
    Obj, dObj = ref.objective(c)
    T, Tx = c['T'], c['Tx']
    idx = sorted(set(range(min(Tx, 64))) | {T - 1, T, Tx - 1} & set(range(Tx)))
    worst = 0.0
    for i in idx:
        if abs(c['x'][i]) > 100:                             # the branch a = x: a kink of the restated link at 500, skipped
            continue
        h = 1e-5 * abs(c['x'][i]) + 1e-6
        cp = dict(c); cm = dict(c)
        cp['x'] = c['x'].copy(); cp['x'][i] += h; cm['x'] = c['x'].copy(); cm['x'][i] -= h
        fd = (ref.objective(cp, grad=False) - ref.objective(cm, grad=False)) / (cp['x'][i] - cm['x'][i])
        worst = max(worst, abs(fd - dObj[i]) / np.max(np.abs(dObj)))
    print('central differences %s: %.2e' % (name, worst))
    assert worst < 1e-5


def test_GetDSs_GetTx_GetFFTCovFast_and_packing():
    assert np.array_equal(gp.GetDSs(1600, 8), [128, 64, 32, 16, 8, 4, 2, 1]) and np.array_equal(gp.GetDSs(32, 8), [4, 2, 1])
    assert np.array_equal(gp.GetDSs(8, 8), [1]) and np.array_equal(gp.GetDSs(3, 8), [1]) and np.array_equal(gp.GetDSs(17, 8), [2, 1])
    assert gp.GetTx(84010, 5 * 1600) == 131072 and gp.GetTx(1500, 5 * 32) == 2048 and gp.GetTx(1024, 0) == 1024 and gp.GetTx(1025, 0) == 2048
    for Tx in (2, 8, 64):
        assert np.array_equal(gp.GetFFTCovFast(3.0, Tx), ref.fft_cov(3.0, Tx))
    c = gp.GetFFTCovFast(4.0, 64)
    assert c.shape == (64,) and np.allclose(c[1:], c[:0:-1]) and abs(c[0] - (np.sqrt(2 * np.pi) * 4 + 1e-6)) < 1e-12 and c.min() >= 1e-6
    P = gp.PackParamsGP(1.0, 2.0, 3.0, 4.0, 5.0)
    assert P == dict(varx=1.0, len=2.0, mux=3.0, varc=4.0, vary=5.0)


def test_resample2_is_the_default_design():
    h = gp.resample2_taps()
    assert h.shape == (41,) and np.allclose(h, h[::-1], atol=1e-15) and abs(h.sum() - 2.0) < 1e-14
    assert np.allclose(h[19:22], [0.6334, 1.0005, 0.6334], atol=5e-5)
    assert np.max(np.abs(h[20 + 2::2])) < 2e-3                   # a half-band design: the even taps off the centre nearly vanish
    n = np.arange(400)
    x = np.sin(2 * np.pi * n / 80.0)
    yy = gp.resample2(x)
    assert yy.shape == (800,)
    want = np.sin(2 * np.pi * np.arange(800) / 160.0)
    assert np.max(np.abs(yy[40:-40] - want[40:-40])) < 2e-3      # a slow sinusoid is reproduced away from the ends
    assert np.max(np.abs(yy[::2][20:-20] - x[20:-20])) < 2e-3
    assert np.allclose(gp.resample2(np.ones(64))[30:-30], 1.0, atol=2e-3)


def test_InitPADSampleNonStat_both_branches():
    rng = np.random.default_rng(3)
    T = 200
    a0 = 1.0 + 0.5 * np.sin(2 * np.pi * np.arange(T) / 100.0)
    y = a0 * rng.standard_normal(T)
    P = gp.PackParamsGP(1.0, 10.0, 0.0, 1.0, 0.0)
    z, a, c = gp.InitPADSampleNonStat(y, P, 8)
    assert z.shape == a.shape == c.shape == (T,) and np.all(a >= 1e-8) and np.allclose(np.log(np.exp(a) - 1), z) and np.allclose(c * a, y)
    W = 8                                                        # the window as the .m lays it out: the mean of |y| over t - W + 1 .. t + W
    for t in (50, 120):
        assert abs(a[t] - np.mean(np.abs(y[t - W + 1:t + W + 1]))) < 1e-12
    P['vary'] = np.zeros(T); P['vary'][60:80] = 1e3                  # per-sample noise, zeros replaced by 1e-5
    z2, a2, c2 = gp.InitPADSampleNonStat(y, P, 8)
    assert np.all(np.isfinite(z2)) and np.all(a2 >= 1e-8) and a2[70] < 0.1 * a2[150]       # inside the gap |y| is divided by sigy = sqrt(1e3)
    assert abs(a2[150] / a[150] - 1) < 1e-4                          # outside, sigy = 1e-5 gives mean|y| 1e5 / (1e5 + 1)
    z3, a3, _ = gp.InitPADSampleNonStat(y[:6], gp.PackParamsGP(1.0, 10.0, 0.0, 4.0, 0.0), 50)   # WinSz >= T - 1 -> T - 2; 1 / varc scales a^2
    assert a3.shape == (6,) and np.all(np.isfinite(z3))
    P4 = gp.PackParamsGP(1.0, 10.0, 0.0, 4.0, 0.0)
    assert np.allclose(gp.InitPADSampleNonStat(y, P4, 8)[1], 0.5 * a)


def test_LearnMarginalParams_recovers_drawn_parameters():
    """a drawn signal y = sqrt(varc) log(1 + exp(x)) n with x ~ N(mux, varx): the grid pick is a grid point, the conjugate-gradient
    result improves on it, and the implied envelope scale E[a^2] varc is that of the draw within 15 %; varc, varx and mux themselves are
    only weakly identified from 500 samples (the .m says so and adds a prior for it), so they are held to a factor of 3 and +-1.5"""
    rng = np.random.default_rng(11)
    T = 20000
    varc, varx, mux = 0.8, 1.5, 0.5
    x = mux + np.sqrt(varx) * ref.se_draw(rng, 40.0, 32768)[:T] * 1.0
    y = np.sqrt(varc) * np.log(1 + np.exp(x)) * rng.standard_normal(T)
    vc, vx, mu, Info = gp.LearnMarginalParams(y)
    sig2 = np.var(y, ddof=1)
    grid_c = np.logspace(-1, 1, 5) , np.logspace(-1, 1, 5), np.linspace(-3, 3, 5)
    assert np.min(np.abs(Info['varcGrid'] - grid_c[0])) < 1e-12 and Info['varxGrid'] in grid_c[1] and Info['muxGrid'] in grid_c[2]
    assert np.all(np.diff(Info['CG']['Obj']) <= 0) and Info['CG']['Obj'][0] <= -Info['Grid']['Obj'] + 0.5 * (np.log(Info['varcGrid'] / sig2)) ** 2 / 10 + 1e-9
    print('LearnMarginalParams: varc %.3f varx %.3f mux %.3f (drawn %.1f %.1f %.1f)' % (vc, vx, mu, varc, varx, mux))
    assert varc / 3 < vc < varc * 3 and varx / 3 < vx < varx * 3 and abs(mu - mux) < 1.5
    z = np.linspace(-6, 6, 2001); w = np.exp(-0.5 * z ** 2); w /= w.sum()
    scale = lambda c_, x_, m_: c_ * np.sum(w * np.log(1 + np.exp(m_ + np.sqrt(x_) * z)) ** 2)
    assert abs(scale(vc, vx, mu) / scale(varc, varx, mux) - 1) < 0.15
    # GetObjNumericalInt2 is minus GetObjNumericalInt plus the prior, and its gradient is that of a central difference
    Opts = gp.LoadLearnMargGPPADOpts(); Opts['logvarcMn'] = 0.3; Opts['logvarcVar'] = 10.0
    th = np.array([0.1, 0.4, -0.2]); yy = y[:500] / np.sqrt(sig2)
    O, dO = gp.GetObjNumericalInt2(th, yy, Opts)
    assert abs(O - (-gp.GetObjNumericalInt(yy, np.exp(0.4), np.exp(0.1), -0.2, Opts) + 0.5 * (0.1 - 0.3) ** 2 / 10)) < 1e-9 * abs(O)
    for k in range(3):
        e = np.zeros(3); e[k] = 1e-6
        fd = (gp.GetObjNumericalInt2(th + e, yy, Opts)[0] - gp.GetObjNumericalInt2(th - e, yy, Opts)[0]) / 2e-6
        assert abs(fd - dO[k]) < 1e-5 * max(1.0, abs(dO[k])), (k, fd, dO[k])


@functools.lru_cache(maxsize=None)
def host_gppad():
    y, a = ref.envelope_signal(1500, 32.0, 21)
    Y = np.stack([y, 0.5 * y[::-1]], axis=1)
    return Y, a, nagp.GPPAD(Y, 32.0, 0, dict(NumIts=30), evaluator=ref.evaluator())


def test_GPPAD_on_the_restatement_objective():
    Y, a, (A, Cc, Params, Info, X) = host_gppad()
    T, D = Y.shape
    assert A.shape == Cc.shape == X.shape == (T, D) and np.all(A > 0) and np.all(np.isfinite(X))
    assert np.allclose(A * Cc, Y, rtol=1e-12, atol=0)
    assert np.array_equal(Params['len'], [32.0, 32.0]) and all(Params[k].shape == (D,) and np.all(Params[k] > 0) for k in ('varx', 'varc'))
    assert Params['vary'].shape == (T, D) and not Params['vary'].any()                               # FBGPMAP.m:51
    for d in range(D):
        I1, I2 = Info[d]
        assert np.array_equal(I2['DSs'], [4, 2, 1]) and I2['Tx'] == 2048 and np.array_equal(I2['NumIts'], [10, 10, 10])
        assert len(I2['ObjLevels']) == 3 and all(np.all(np.diff(o) <= 0) for o in I2['ObjLevels']) and 'varcGrid' in I1
    assert np.corrcoef(A[:, 0], a)[0, 1] > 0.8
    # Params given: nothing is learned; Long returns the Tx circular samples; Tx and DSLength as the .m reads them
    P = dict(len=32.0, varx=1.0, varc=1.0, mux=0.0)
    A2, C2, P2, I2, X2 = nagp.GPPAD(Y[:, :1], P, 0, dict(NumIts=6, Long=1, Tx=4096, DSLength=16.0), evaluator=ref.evaluator())
    assert A2.shape == X2.shape == (4096, 1) and C2.shape == (T, 1) and I2[0][0] is None and np.array_equal(I2[0][1]['DSs'], [2, 1])
    assert np.array_equal(A2[:, 0], np.log(1 + np.exp(X2[:, 0])))
    a1, x1, i1 = nagp.InferAmplitudeGPMAP(Y[:, 0], gp.PackParamsGP(1.0, 32.0, 0.0, 1.0, np.zeros(T)), dict(NumIts=6), evaluator=ref.evaluator())
    a0, x0, i0 = nagp.InferAmplitudeGPMAP(Y[:, 0], gp.PackParamsGP(1.0, 32.0, 0.0, 1.0, 0.0), dict(NumIts=6), evaluator=ref.evaluator())
    assert a1.shape == a0.shape == (T,) and i1['Obj'].size >= 6 and i0['Obj'].size >= 6                # (the two InitPADSampleNonStat branches start them apart)
    xs, Obj = nagp.MAPGPFast(np.zeros(64), Y[:40, 0], gp.PackParamsGP(1.0, 4.0, 0.0, 1.0, 0.0), dict(T=40, Tx=64), 5, evaluator=ref.evaluator())
    assert xs.shape == (64,) and np.all(np.diff(Obj) <= 0) and Obj.size >= 2


def test_refused_forms_name_the_reference_file():
    Y = np.ones((64, 1))
    for kw, name in ((dict(LrnLen=1), 'FBGPMAPLearnLen.m'), (dict(LrnLen=2), 'FBGPMAPLearnLen.m'), (dict(nout=6), 'FBGPMAPLearnLen.m'), (dict(nout=8), 'LoadErrorBarsLapOpts.m')):
        with pytest.raises(NotImplementedError, match=re.escape(name)):
            nagp.GPPAD(Y, 8.0, **kw)
    with pytest.raises(NotImplementedError, match=r'FBCasGPMAP\.m'):
        nagp.GPPAD(Y, np.array([[8.0], [30.0]]))
    with pytest.raises(NotImplementedError, match=r'FBCasGPMAP\.m'):
        nagp.GPPAD(Y, dict(len=np.array([[8.0], [30.0]]), varx=1.0, varc=1.0, mux=0.0))
    with pytest.raises(ValueError):
        nagp.GPPAD(np.ones((64, 2)), [8.0, 9.0, 10.0])


def test_nmf_init_takes_the_envelopes():
    """mods=None keeps the arguments nmf_fp was given; mods replaces abs(Z).T; a wrong shape or a negative entry is refused"""
    import inspect
    from nagp import nmf
    assert inspect.signature(nagp.nmf_init).parameters['mods'].default is None
    seen = []
    orig = nmf.nmf_fp
    def spy(A, W0, H0, *a, **k):
        seen.append((A.copy(), W0.copy(), H0.copy())); raise RuntimeError('stop')
    nmf.nmf_fp = spy
    try:
        rng = np.random.default_rng(0)
        Z = rng.standard_normal((3, 50)) + 1j * rng.standard_normal((3, 50)); mods = rng.random((50, 3))
        for kw in ({}, dict(mods=mods)):
            with pytest.raises(RuntimeError, match='stop'):
                nagp.nmf_init(Z, 2, **kw)
    finally:
        nmf.nmf_fp = orig
    assert np.array_equal(seen[0][0], np.abs(Z).T) and np.array_equal(seen[1][0], mods) and np.array_equal(seen[0][2], seen[1][2])
    assert all(any(np.array_equal(w, r) for r in mods) for w in seen[1][1])                           # WInit = mods(ks, :)
    for bad in (mods[:-1], -mods):
        with pytest.raises(ValueError):
            nagp.nmf_init(Z, 2, mods=bad)


def test_exported_and_bound():
    nagp.build()
    out = subprocess.run(['nm', '-D', '--defined-only', L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    names = {'nagp_gppad_obj', 'nagp_gppad_create', 'nagp_gppad_eval', 'nagp_gppad_destroy', 'nagp_gppad_timings'}
    assert names <= set(re.findall(r' T (nagp_[a-z0-9_]+)', out)) and names <= set(L.EXPORTS)
    hdr = open(os.path.join(ROOT, 'include', 'nagp.h')).read()
    assert re.search(r'^int nagp_gppad_obj\(int32_t n_problems, int64_t T, int64_t Tx,', hdr, re.M)
    assert re.search(r'^int nagp_gppad_timings\(double\* ms /\* 1 \*/\);', hdr, re.M) and re.search(r'^void nagp_gppad_destroy\(nagp_gppad\* handle\);', hdr, re.M)
    fn = L.lib().nagp_gppad_obj
    assert len(fn.argtypes) == 16 and fn.restype is C.c_int and len(L.lib().nagp_gppad_create.argtypes) == 14
    ms = C.c_double(-1.0)
    assert L.lib().nagp_gppad_timings(C.byref(ms)) == 0 and ms.value >= 0.0 and L.lib().nagp_gppad_timings(None) == EINVAL
    for name in ('gppad_obj', 'GetGPObjFast', 'GetFFTCovFast', 'GetTx', 'GetDSs', 'GetAmp', 'PackParamsGP', 'InitPADSampleNonStat', 'LearnMarginalParams',
                 'GridMargParams', 'GetObjNumericalInt', 'GetObjNumericalInt2', 'ConjGradMargParams', 'MAPGPFast', 'InferAmplitudeGPMAP',
                 'InferAmplitudeGPMAP_many', 'FBGPMAP', 'GPPAD', 'resample2'):
        assert getattr(nagp, name) is getattr(gp, name)


def call(P=1, T=5, Tx=8, x=True, y=None, vary=(0.0,), vs=0, ln=(3.0,), cov=None, cs=0, varx=(1.0,), mux=(0.0,), varc=(1.0,), Obj=True):
    f = lambda v: L.f64(np.asarray(v, float), 'C') if v is not None else None
    xx = f(np.zeros(max(P, 1) * max(Tx, 1))) if x else None
    yy = f(np.ones(max(P, 1) * max(T, 1)) if y is None else y) if y is not False else None
    O = np.zeros(max(P, 1)); d = np.zeros(max(P, 1) * max(Tx, 1))
    return L.lib().nagp_gppad_obj(P, T, Tx, L.dptr(xx), L.dptr(yy), L.dptr(f(vary)), vs, L.dptr(f(ln)), L.dptr(f(cov)), cs, L.dptr(f(varx)), L.dptr(f(mux)),
                                  L.dptr(f(varc)), L.dptr(O) if Obj else None, L.dptr(d), 0)


def test_argument_errors_answer_without_a_device(monkeypatch):
    nagp.build()
    err = lambda: L.lib().nagp_last_error()
    assert call(x=False) == EINVAL and call(y=False) == EINVAL and call(Obj=False) == EINVAL
    assert call(vary=None) == EINVAL and call(varx=None) == EINVAL and call(mux=None) == EINVAL and call(varc=None) == EINVAL
    assert call(ln=None) == EINVAL and b'one of len and fftCov' in err() and call(cov=np.ones(8)) == EINVAL and b'one of len and fftCov' in err()
    assert call(P=0) == EINVAL and call(T=0) == EINVAL and call(T=9) == EINVAL and b'T=9 > Tx=8' in err()
    assert call(vs=3) == EINVAL and b'vary_stride' in err() and call(ln=None, cov=np.ones(8), cs=4) == EINVAL and b'cov_stride' in err()
    for Tx in (0, 1, 3, 6, 12, 2 ** 20 + 2, 2 ** 21):
        assert call(Tx=Tx, T=1) == EUNSUPPORTED and b'power of two' in err(), Tx
    for bad in (np.nan, np.inf, -np.inf):
        y = np.ones(5); y[-1] = bad
        assert call(y=y) == EINVAL
        assert call(vary=[bad]) == EINVAL and call(vary=[0, 0, 0, 0, bad], vs=5) == EINVAL
        assert call(ln=[bad]) == EINVAL and call(varx=[bad]) == EINVAL and call(mux=[bad]) == EINVAL and call(varc=[bad]) == EINVAL
        cv = np.ones(8); cv[-1] = bad
        assert call(ln=None, cov=cv) == EINVAL and call(P=2, ln=None, cov=np.r_[np.ones(8), cv], cs=8, vary=[0, 0], varx=[1, 1], mux=[0, 0], varc=[1, 1]) == EINVAL
    assert call(vary=[-1e-9]) == EINVAL and b'>= 0' in err()
    for kw in (dict(varx=[0.0]), dict(varx=[-1.0]), dict(varc=[0.0]), dict(varc=[-1.0]), dict(ln=[0.0]), dict(ln=[-2.0])):
        assert call(**kw) == EINVAL and b'> 0' in err(), kw
    cv = np.ones(8); cv[3] = 0.0
    assert call(ln=None, cov=cv) == EINVAL and b'fftCov[3]' in err()
    h = C.c_void_p(1)
    assert L.lib().nagp_gppad_create(C.byref(h), 1, 5, 8, None, None, 0, None, None, 0, None, None, None, 0) == EINVAL and not h.value
    assert L.lib().nagp_gppad_eval(None, None, None, None) == EINVAL
    # one problem beyond the budget of the per-evaluation buffers (lowered to 1 MiB behind NAGP_DEVELOPER, which tests/conftest.py sets)
    monkeypatch.setenv('NAGP_GPPAD_BUDGET_MB', '1')
    assert call(Tx=65536) == EUNSUPPORTED and b'budget' in err()


def test_argument_checks_in_plain_c():
    """tests/c/abi_gppad_errors.c: a stand-alone C program on exactly-sized heap blocks against libnagp_asan.so (the host code of the C ABI
    built with AddressSanitizer), on the CPU only: every invalid call returns its status and ASan reports nothing."""
    import tempfile
    lib = nagp.build(asan=True)
    clang = '/opt/rocm/lib/llvm/bin/clang'
    rt = glob.glob('/opt/rocm/lib/llvm/lib/clang/*/lib/linux') + glob.glob('/opt/rocm/lib/llvm/lib/clang/*/lib/x86_64-unknown-linux-gnu')
    with tempfile.TemporaryDirectory() as td:
        exe = os.path.join(td, 'abi_gppad_errors')
        r = subprocess.run([clang, '-fsanitize=address', '-shared-libsan', '-g', '-O1', '-std=c99', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'include'),
                            '-o', exe, os.path.join(ROOT, 'tests', 'c', 'abi_gppad_errors.c'), lib, '-lm', '-Wl,-rpath,/opt/rocm/lib',
                            '-Wl,-rpath-link,/opt/rocm/lib'] + ['-Wl,-rpath,' + d for d in rt], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        env = dict(os.environ, ASAN_OPTIONS='detect_leaks=0:abort_on_error=0:exitcode=66', LD_LIBRARY_PATH=':'.join(rt + [os.environ.get('LD_LIBRARY_PATH', '')]))
        r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
        assert r.returncode == 0 and 'all error paths returned their status' in r.stdout, r.stdout + r.stderr
        assert 'AddressSanitizer' not in r.stderr, r.stderr
