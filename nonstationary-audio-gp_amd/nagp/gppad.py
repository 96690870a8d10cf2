"""Host-side mirror of the GPPAD envelope initialisation, the step GPPAD(real(Z)', fs/10) of the reference's training drivers
(experiments/train_model.m:113, train_GTFNMF.m:73, train_GTFNMF_gaps.m) in the form the drivers call -- GPPAD(Y, len) and
GPPAD(Y, Params), both through FBGPMAP:

    [A,C,Params,Info,X] = GPPAD(Y,len,LrnLen,Opts)                             experiments/gppad/GPPAD.m
    [A,X,C,Params,Info] = FBGPMAP(Y,len,Opts)                                  gppad/GPModelFast/FBGPMAP.m
    [varc,varx,mux,Info] = LearnMarginalParams(y,Opts)                         gppad/MarginalModel/LearnMarginalParams.m
    [a,x,Info] = InferAmplitudeGPMAP(y,Params,Opts)                            gppad/GPModelFast/InferAmplitudeGPMAP.m
    [x,Obj] = MAPGPFast(x,y,Params,Dims,NumIts)                                gppad/GPModelFast/MAPGPFast.m
    [Obj,dObjdx] = GetGPObjFast(x,y,fftCov,Params,Dims)                        gppad/GPModelFast/GetGPObjFast.m

The objective and its gradient -- an FFT, a division by the prior spectrum, an inverse FFT and the likelihood pass, Tx = 131072 for
speech_74 -- run on the GPU (nagp_gppad_obj and the resident nagp_gppad_create / _eval / _destroy, include/nagp.h).  The marginal
parameters (500 samples x 250 grid points), the first-level initialisation, resample(x, 2, 1) between the levels and the
conjugate-gradient line search (minimize.minimize_steps) stay on the host.  There is no CPU fallback: the `evaluator` argument exists so
that the tests can put the float64 restatement through the same driver.

Refused here with the name of the reference file that serves them: length-scale learning (LrnLen = 1, 2: FBGPMAPLearnLen.m) and the
Laplace error bars (outputs 6-8: FBGPMAPLearnLen.m with LoadErrorBarsLapOpts.m).  Both are built in gppad_lap.py under the names of their
own .m files (FBGPMAPLearnLen, InferAmplitudeErrorBarsGPMAP, GetLenGradAscent, GetLenGridSearch, ...), with explicit randomness.  Cascades (a column of
length-scales) are built, in gppad_cas.py under the names of their own .m files (FBCasGPMAP, CasGPMAP, MAPGPCasFast, GetObjCasGPFAST);
GPPAD and FBGPMAP keep refusing a column of length-scales with the name FBCasGPMAP.m.
"""
import math

import numpy as np

from . import _lib as L
from ._drive import ResidentHandle, close, forward, lock_step_rows, run
from .minimize import minimize, minimize_steps


# ---------------------------------------------------------------------------------------------------------------- small helpers
def GetAmp(x):
    """a = GetAmp(x) (GetAmp.m): log(1 + exp(x)), x itself above 500 and exp(x) below -30"""
    x = np.asarray(x, float)
    with np.errstate(over='ignore'):
        a = np.log(1 + np.exp(x))
    return np.where(x > 500, x, np.where(x < -30, np.exp(np.minimum(x, 0.0)), a))


def GetTx(T, tau):
    """Tx = 2^ceil(log2(T + tau)) (GetTx.m)"""
    return int(2 ** math.ceil(math.log2(T + tau)))


def GetDSs(len, MinLength):
    """DSs = GetDSs(len, MinLength) (GetDSs.m): the down-sampling rates 2^floor(log2(len / MinLength)) ... 2, 1"""
    if len > MinLength:
        log2MaxDS = int(math.floor(math.log2(len) - math.log2(MinLength)))
        return np.round(np.logspace(math.log10(2.0 ** log2MaxDS), 0.0, log2MaxDS + 1)).astype(int)
    return np.array([1])


def GetFFTCovFast(len, T):
    """fftCov = GetFFTCovFast(len, T) (GetFFTCovFast.m:10-16) in host NumPy"""
    T = int(T)
    omega = 2 * np.pi * np.concatenate([np.arange(0, T // 2 + 1), np.arange(-(T // 2) + 1, 0)]) / T
    return np.sqrt(2 * np.pi * len ** 2) * np.exp(-omega ** 2 * len ** 2 / 2) + 1e-6


def PackParamsGP(varx, len, mux, varc, vary):
    """Params = PackParamsGP(varx, len, mux, varc, vary) (PackParamsGP.m) as a dict"""
    return {'varx': varx, 'len': len, 'mux': mux, 'vary': vary, 'varc': varc}


def PackDimsGPFast(T, Tx):
    return {'T': int(T), 'Tx': int(Tx)}


_RESAMPLE2 = None


def resample2_taps():
    """the 41 taps of MATLAB's resample(x, 2, 1) in its default design (resample.m with N = 10, bta = 5):
    firls(40, [0 .5 .5 1], [1 1 0 0]) .* kaiser(41, 5)', scaled to sum 2"""
    global _RESAMPLE2
    if _RESAMPLE2 is None:
        from scipy.signal import firls
        h = firls(41, [0, .5, .5, 1], [1, 1, 0, 0]) * np.kaiser(41, 5)
        _RESAMPLE2 = 2 * h / np.sum(h)
    return _RESAMPLE2


def resample2(x):
    """resample(x, 2, 1): the zero-stuffed sequence through resample2_taps, centred (the filter's delay of 20 removed), 2 numel(x) long"""
    x = np.asarray(x, float).reshape(-1)
    up = np.zeros(2 * x.size); up[::2] = x
    return np.convolve(up, resample2_taps(), 'full')[20:20 + 2 * x.size]


# ---------------------------------------------------------------------------------------------------------------- the objective
def _per_problem(v, P, name):
    a = np.asarray(v, float)
    if a.ndim == 0:
        a = np.full(P, float(a))
    if a.shape != (P,):
        raise ValueError('%s must be a scalar or hold one entry per problem' % name)
    return L.f64(a, 'C')


def _shaped(y, Tx, vary, varx, mux, varc, len, fftCov, one=False):
    """the data arguments of nagp_gppad_create / nagp_gppad_obj from NumPy arrays, in the order of the C signatures: y (P, T), vary,
    vary_stride, len, fftCov, cov_stride, varx, mux, varc.  one: a (T,) vary is the per-sample vary of the one problem."""
    P, T = y.shape
    vy = np.asarray(vary, float)
    if one and vy.shape == (T,) and T != 1:
        vy = vy[None, :]
    if vy.ndim == 0:
        vy = np.full(P, float(vy))
    if vy.shape not in ((P,), (P, T)):
        raise ValueError('vary must be a scalar, (P,) or (P, T): got %s' % (vy.shape,))
    vy = L.f64(vy, 'C')
    if (len is None) == (fftCov is None):
        raise ValueError('exactly one of len and fftCov is given')
    ln = _per_problem(len, P, 'len') if len is not None else None
    cov = None
    if fftCov is not None:
        cov = L.f64(np.asarray(fftCov, float), 'C')
        if cov.shape not in ((Tx,), (P, Tx)):
            raise ValueError('fftCov must be (Tx,) or (P, Tx): got %s' % (cov.shape,))
    return [L.dptr(y), L.dptr(vy), T if vy.ndim == 2 else 0, L.dptr(ln), L.dptr(cov), Tx if cov is not None and cov.ndim == 2 else 0,
            L.dptr(_per_problem(varx, P, 'varx')), L.dptr(_per_problem(mux, P, 'mux')), L.dptr(_per_problem(varc, P, 'varc'))]


class GppadHandle(ResidentHandle):
    """The resident form (nagp_gppad_create): y (P, T), vary (P,) or (P, T), 1 / c, the parameters and the twiddles stay on the
    device; eval(x) moves x (P, Tx) in and Obj (P,), dObj (P, Tx) out.  The prior spectrum is fftCov ((Tx,) shared or (P, Tx)) or
    is formed on the device from len."""
    _eval, _destroy = 'nagp_gppad_eval', 'nagp_gppad_destroy'

    def __init__(self, y, Tx, vary, varx, mux, varc, len=None, fftCov=None, device=0):
        import ctypes as C
        y = L.f64(np.atleast_2d(np.asarray(y, float)), 'C')
        self.P, self.T = y.shape; self.Tx = self.nx = int(Tx)
        h = C.c_void_p()
        L.check(L.lib().nagp_gppad_create(C.byref(h), self.P, self.T, self.Tx, *_shaped(y, self.Tx, vary, varx, mux, varc, len, fftCov), int(device)))
        self._h = h


def gppad_obj(x, y, vary, varx, mux, varc, len=None, fftCov=None, grad=True, device=0):
    """nagp_gppad_obj with NumPy arrays.  x (Tx,) or (P, Tx); y (T,) or (P, T); vary a scalar, (P,) or (P, T) (for one problem also
    (T,)); varx, mux, varc scalars or (P,); the prior spectrum as fftCov ((Tx,) shared or (P, Tx)) or formed on the device from len
    (a scalar or (P,)).  Returns Obj and, with grad, dObj, with the leading problem axis of x."""
    x = np.asarray(x, float); single = x.ndim <= 1
    xx = L.f64(np.atleast_2d(x), 'C'); yy = L.f64(np.atleast_2d(np.asarray(y, float)), 'C')
    if xx.ndim != 2 or yy.ndim != 2 or yy.shape[0] != xx.shape[0]:
        raise ValueError('x must be (Tx,) or (P, Tx) and y (T,) or (P, T): got %s, %s' % (x.shape, np.shape(y)))
    P, Tx = xx.shape; T = yy.shape[1]
    Obj = np.zeros(P); dObj = np.zeros((P, Tx)) if grad else None
    L.check(L.lib().nagp_gppad_obj(P, T, Tx, L.dptr(xx), *_shaped(yy, Tx, vary, varx, mux, varc, len, fftCov, one=single), L.dptr(Obj), L.dptr(dObj),
                                   int(device)))
    if single:
        return (Obj[0], dObj[0]) if grad else Obj[0]
    return (Obj, dObj) if grad else Obj


def GetGPObjFast(x, y, fftCov, Params, Dims, nout=2, device=0):
    """[Obj,dObjdx] = GetGPObjFast(x,y,fftCov,Params,Dims) (GetGPObjFast.m:1) on the device: Params a dict with varx, mux, varc and vary
    (a scalar or T entries; len is not read, the spectrum is given), Dims a dict with T and Tx.  nout stands for nargout."""
    T, Tx = int(Dims['T']), int(Dims['Tx'])
    x = np.asarray(x, float).reshape(-1); y = np.asarray(y, float).reshape(-1)
    if x.size != Tx or y.size != T:
        raise ValueError('x holds Dims.Tx = %d and y Dims.T = %d entries: got %d, %d' % (Tx, T, x.size, y.size))
    vary = np.asarray(Params['vary'], float).reshape(-1)
    return gppad_obj(x, y, vary[0] if vary.size == 1 else vary, Params['varx'], Params['mux'], Params['varc'],
                     fftCov=np.asarray(fftCov, float).reshape(-1), grad=nout > 1, device=device)


# ---------------------------------------------------------------------------------------------------------------- initialisation
def InitPADSampleNonStat(y, Params, WinSz):
    """[z,a,c] = InitPADSampleNonStat(y,Params,WinSz) (InitPADSampleNonStat.m): the moving average of |y| over 2 WinSz samples by
    circular convolution, with scalar vary (:36-37) or weighted by 1 / sqrt(vary) per sample, zeros replaced by 1e-5 (:39-42)"""
    y = np.asarray(y, float).reshape(-1)
    T = y.size
    WinSz = int(WinSz)
    if WinSz >= T - 1:
        WinSz = T - 2
    if WinSz < 1:
        raise ValueError('InitPADSampleNonStat needs at least 3 samples (T = %d)' % T)
    C = 1.0 / float(Params['varc'])
    Win = np.concatenate([np.ones(WinSz), np.zeros(2 * T - 2 * WinSz - 2), np.ones(WinSz)]) / (2 * WinSz)
    fftWin = np.fft.fft(Win)
    sigy = np.sqrt(np.asarray(Params['vary'], float).reshape(-1))
    pad = np.zeros(T - 2)
    if sigy.size == 1:
        a = np.fft.ifft(fftWin * np.fft.fft(np.concatenate([np.abs(y), pad]))) * np.sqrt(C)
    else:
        sigy = np.where(sigy == 0, 1e-5, sigy)
        fftAbsysigy = np.fft.fft(np.concatenate([np.abs(y) / sigy, pad]))
        fftsigy = np.fft.fft(np.concatenate([1.0 / sigy, pad]))
        a = np.fft.ifft(fftWin * fftAbsysigy) * np.sqrt(C) / (np.fft.ifft(fftsigy * fftWin) + 1)
    a = np.real(a[:T])
    a = np.where(a < 1e-8, 1e-8, a)
    z = np.log(np.exp(a) - 1)
    return z, a, y / a


# ---------------------------------------------------------------------------------------------------------------- marginal parameters
def LoadLearnMargGPPADOpts(Opts=None):
    """the defaults of LoadLearnMargGPPADOpts.m and LoadInferenceGPMAPOpts.m under the entries of Opts (ModifyOpts)"""
    d = {'NumXs': 250, 'zUpper': 5.0, 'zLower': -5.0, 'ChSz': 1000, 'NumRetain': 500, 'varcRng': (0.1, 10.0), 'varxRng': (0.1, 10.0),
         'muxRng': (-3.0, 3.0), 'NumGridPoints': 5, 'NumItsMM': 20, 'tol': 5, 'MinLength': 8, 'NumIts': 2000}
    d.update(Opts or {})
    return d


def _marg_terms(y, varx, varc, mux, Opts):
    z = np.linspace(Opts['zLower'], Opts['zUpper'], int(Opts['NumXs']))
    a = GetAmp(z * np.sqrt(varx) + mux)
    vary = varc * a ** 2 + 1e-9
    return z, a, vary, -0.5 * z ** 2


def GetObjNumericalInt(y, varx, varc, mux, Opts):
    """Obj = GetObjNumericalInt(y,varx,varc,mux,Opts) (GetObjNumericalInt.m): log p(y | theta) with x integrated on a grid of NumXs
    points, in chunks of ChSz samples"""
    y = np.asarray(y, float).reshape(-1)
    z, a, vary, logpz = _marg_terms(y, varx, varc, mux, Opts)
    T = y.size; ChSz = int(Opts['ChSz'])
    Obj = 0.0
    for t0 in range(0, T, ChSz):
        yc = y[t0:t0 + ChSz]
        logpxys = -np.outer(yc ** 2, 1.0 / (2 * vary)) + (logpz - 0.5 * np.log(vary))[None, :]
        m = np.max(logpxys, axis=1)
        Obj += np.sum(np.log(np.sum(np.exp(logpxys - m[:, None]), axis=1)) + m)
    return Obj + T * (np.log(z[1] - z[0]) - np.log(2 * np.pi))


def GetObjNumericalInt2(theta, y, Opts):
    """[Obj,dObj] = GetObjNumericalInt2(theta,y,Opts) (GetObjNumericalInt2.m): the negative of GetObjNumericalInt at
    theta = [log varc, log varx, mux] with its gradient and the weak prior on log varc (Opts.logvarcMn, Opts.logvarcVar)"""
    theta = np.asarray(theta, float).reshape(-1)
    y = np.asarray(y, float).reshape(-1)
    varc, varx, mux = np.exp(theta[0]), np.exp(theta[1]), theta[2]
    z, a, vary, logpz = _marg_terms(y, varx, varc, mux, Opts)
    with np.errstate(over='ignore'):
        dadmux = 1.0 / (1 + np.exp(-(z * np.sqrt(varx) + mux)))
    dadlogvarx = 0.5 * np.sqrt(varx) * z * dadmux
    T = y.size; ChSz = int(Opts['ChSz'])
    Obj = 0.0; dObj = np.zeros(3)
    for t0 in range(0, T, ChSz):
        y2 = y[t0:t0 + ChSz] ** 2
        logpxys = -np.outer(y2, 1.0 / (2 * vary)) + (logpz - 0.5 * np.log(vary))[None, :]
        m = np.max(logpxys, axis=1)
        e = np.exp(logpxys - m[:, None]); se = np.sum(e, axis=1)
        Obj += np.sum(np.log(se) + m)
        A1 = np.outer(y2, a ** 2 / vary ** 2) - (a ** 2 / vary)[None, :]
        dObj[0] += 0.5 * varc * np.sum(np.sum(e * A1, axis=1) / se)
        A2 = np.outer(y2, a / vary ** 2 * dadlogvarx) - (a * dadlogvarx / vary)[None, :]
        dObj[1] += varc * np.sum(np.sum(e * A2, axis=1) / se)
        A3 = np.outer(y2, a / vary ** 2 * dadmux) - (a * dadmux / vary)[None, :]
        dObj[2] += varc * np.sum(np.sum(e * A3, axis=1) / se)
    Obj = -(Obj + T * (np.log(z[1] - z[0]) - np.log(2 * np.pi))); dObj = -dObj
    Obj += 0.5 * (theta[0] - Opts['logvarcMn']) ** 2 / Opts['logvarcVar']
    dObj[0] += (theta[0] - Opts['logvarcMn']) / Opts['logvarcVar']
    return Obj, dObj


def GridMargParams(y, Opts):
    """[varc,varx,mux,Info] = GridMargParams(y,Opts) (GridMargParams.m): the best of NumGridPoints^3 grid points, the first one on ties"""
    N = int(Opts['NumGridPoints'])
    varcs = np.logspace(np.log10(Opts['varcRng'][0]), np.log10(Opts['varcRng'][1]), N)
    varxs = np.logspace(np.log10(Opts['varxRng'][0]), np.log10(Opts['varxRng'][1]), N)
    muxs = np.linspace(Opts['muxRng'][0], Opts['muxRng'][1], N)
    Obj = -np.inf; best = None
    for vx in varxs:
        for vc in varcs:
            for mu in muxs:
                ObjCur = GetObjNumericalInt(y, vx, vc, mu, Opts)
                if ObjCur > Obj:
                    Obj = ObjCur; best = (vc, vx, mu)
    if best is None:
        raise ValueError('GridMargParams: the objective is not finite at any grid point')
    return best[0], best[1], best[2], {'Obj': Obj}


def ConjGradMargParams(y, varc, varx, mux, Opts):
    """[varc,varx,mux,Info] = ConjGradMargParams(y,varc,varx,mux,Opts) (ConjGradMargParams.m): NumItsMM line searches of minimize on
    GetObjNumericalInt2"""
    theta, Obj, _ = minimize(np.array([np.log(varc), np.log(varx), mux]), GetObjNumericalInt2, int(Opts['NumItsMM']), y, Opts)
    return float(np.exp(theta[0])), float(np.exp(theta[1])), float(theta[2]), {'Obj': Obj}


def LearnMarginalParams(y, Opts=None):
    """[varc,varx,mux,Info] = LearnMarginalParams(y,Opts) (LearnMarginalParams.m): NumRetain samples at stride floor(T / NumRetain),
    scaled to unit variance, the grid search, then conjugate gradients under the weak prior on log varc; host NumPy"""
    Opts = LoadLearnMargGPPADOpts(Opts)
    y = np.asarray(y, float).reshape(-1)
    NumRetain = int(Opts['NumRetain']); T = y.size
    DS = T // NumRetain
    if DS < 1:
        raise ValueError('LearnMarginalParams needs at least NumRetain = %d samples (T = %d)' % (NumRetain, T))
    sigy = max(np.sqrt(np.var(y, ddof=1)), 1e-12)
    yDS = y[0:NumRetain * DS:DS] / sigy
    Opts['varcRng'] = (Opts['varcRng'][0] / sigy ** 2, Opts['varcRng'][1] / sigy ** 2)
    varc, varx, mux, InfoGrid = GridMargParams(yDS, Opts)
    Info = {'varcGrid': varc * sigy ** 2, 'varxGrid': varx, 'muxGrid': mux}
    Opts['logvarcMn'] = -np.log(sigy ** 2); Opts['logvarcVar'] = 10.0
    varc, varx, mux, InfoCG = ConjGradMargParams(yDS, varc, varx, mux, Opts)
    Info['Grid'] = InfoGrid; Info['CG'] = InfoCG
    return varc * sigy ** 2, varx, mux, Info


# ---------------------------------------------------------------------------------------------------------------- inference
def _device_evaluator(device):
    """evaluator(y, Params, Dims) -> f(x) -> (Obj, dObj): one resident handle per level; f.close() releases it"""
    def open_level(y, Params, Dims):
        vary = np.asarray(Params['vary'], float).reshape(-1)
        h = GppadHandle(y[None, :], Dims['Tx'], vary[0] if vary.size == 1 else vary[None, :], Params['varx'], Params['mux'], Params['varc'],
                        len=Params['len'], device=device)

        def f(x):
            Obj, dObj = h.eval(x)
            return Obj[0], dObj[0]
        f.close = h.close
        return f
    return open_level


def MAPGPFast(x, y, Params, Dims, NumIts, evaluator=None, device=0):
    """[x,Obj] = MAPGPFast(x,y,Params,Dims,NumIts) (MAPGPFast.m): NumIts line searches of minimize on GetGPObjFast with the spectrum
    GetFFTCovFast(Params.len, Dims.Tx), formed on the device.  evaluator(y, Params, Dims) returns the objective f(x) -> (Obj, dObj)
    of that level (by default a resident nagp_gppad handle)."""
    y = np.asarray(y, float).reshape(-1)
    f = (evaluator or _device_evaluator(device))(y, Params, Dims)
    try:
        x, Obj, _ = run(minimize_steps(np.asarray(x, float).reshape(-1), int(NumIts)), f)
    finally:
        close(f)
    return x, Obj


def infer_steps(y, Params, Opts):
    """InferAmplitudeGPMAP as a generator.  At the start of every resolution it yields ('level', yDS, ParamsCur, DimsCur) and is sent
    anything; then it yields ('x', x) and is sent (Obj, dObj) there; its return value is (a, x, Info)."""
    Opts = LoadLearnMargGPPADOpts(Opts)
    y = np.asarray(y, float).reshape(-1)
    T = y.size
    len_, mux = float(Params['len']), float(Params['mux'])
    vary = np.asarray(Params['vary'], float).reshape(-1)
    if vary.size not in (1, T):
        raise ValueError('Params.vary is a scalar or holds T = %d entries: got %d' % (T, vary.size))
    Tx = int(Opts['Tx']) if 'Tx' in Opts else GetTx(T, len_ * Opts['tol'])                          # :53-57
    DSs = GetDSs(Opts['DSLength'], Opts['MinLength']) if 'DSLength' in Opts else GetDSs(len_, Opts['MinLength'])   # :65-71
    if Tx % int(DSs[0]) or Tx < T:
        raise ValueError('Tx = %d must hold the T = %d samples and be a multiple of the coarsest rate %d' % (Tx, T, DSs[0]))
    Lens = len_ / DSs
    NumDSs = DSs.size
    NumIts = np.full(NumDSs, int(math.ceil(Opts['NumIts'] / NumDSs)))
    Info = {'Obj': [], 'NumIts': NumIts, 'DSs': DSs, 'Tx': Tx}
    xDS = None
    for n in range(NumDSs):
        DS = int(DSs[n])
        yDS = y[0:T:DS]
        TCur = yDS.size; TxCur = Tx // DS
        ParamsCur = dict(Params); ParamsCur['len'] = float(Lens[n])
        ParamsCur['vary'] = vary[0:T:DS] if vary.size > 1 else float(vary[0])                    # :98-100
        if n == 0:                                                                               # :104-113
            if np.max(ParamsCur['vary']) > 5 * np.var(yDS, ddof=1):
                WinSz = max(int(math.floor(Lens[0] * 2)), 4)
            else:
                WinSz = max(int(math.floor(Lens[0] / 2)), 2)
            xDS, _, _ = InitPADSampleNonStat(yDS, ParamsCur, WinSz)
            xDS = np.concatenate([xDS, mux * np.ones(TxCur - TCur)])
        yield ('level', yDS, ParamsCur, PackDimsGPFast(TCur, TxCur))
        xDS, Obj, _ = yield from forward(minimize_steps(xDS, int(NumIts[n])), lambda x: ('x', x))
        if n < NumDSs - 1:
            xDS = resample2(xDS)                                                                 # :128-130
        Info['Obj'].append(Obj / Tx)                                                             # :133
    Info['ObjLevels'] = Info['Obj']
    Info['Obj'] = np.concatenate(Info['Obj'])
    if 'Long' in Opts:
        return np.log(1 + np.exp(xDS)), xDS, Info
    return np.log(1 + np.exp(xDS[:T])), xDS[:T], Info


def InferAmplitudeGPMAP(y, Params, Opts=None, evaluator=None, device=0):
    """[a,x,Info] = InferAmplitudeGPMAP(y,Params,Opts) (InferAmplitudeGPMAP.m:1): MAP inference of the transformed envelope x and the
    envelope a = log(1 + exp(x)) of one channel over the resolutions DSs = GetDSs(len, MinLength), coarsest first:
    ceil(NumIts / numel(DSs)) line searches per resolution, the first initialised by InitPADSampleNonStat, the next by resample2 of the
    result.  Options: the defaults of LoadInferenceGPMAPOpts.m (tol = 5, MinLength = 8, NumIts = 2000) and Long, Tx, DSLength as in
    the .m.  Info['Obj'] is the objective history over Tx, Info['ObjLevels'] the same per resolution, Info['NumIts'], Info['DSs'].
    evaluator(y, Params, Dims) -> f(x) -> (Obj, dObj): the objective of one resolution, by default a resident nagp_gppad handle on
    `device` (f.close(), when there, is called at the end of the resolution)."""
    ev = evaluator or _device_evaluator(device)
    level = [None]                                           # the objective of the resolution the generator stands at

    def answer(req):
        if req[0] == 'x':
            return level[0](req[1])
        close(level[0])
        level[0] = ev(req[1], req[2], req[3])
    try:
        return run(infer_steps(y, Params, Opts), answer)
    finally:
        close(level[0])


def InferAmplitudeGPMAP_many(ys, Params, Opts=None, device=0):
    """InferAmplitudeGPMAP on several channels in lock-step.  ys: a list of signals (or the columns of a T x D array); Params: one dict
    per channel.  One generator per channel; the channels that stand at a resolution of equal (T, Tx) share one resident handle, and a
    round of the line searches is one batched nagp_gppad_eval (a channel whose search has ended rides along with its last point).  A
    problem's bits do not depend on its batch mates, so the results equal the one-at-a-time runs to the bit.  Returns a list of
    (a, x, Info)."""
    if isinstance(ys, np.ndarray) and ys.ndim == 2:
        ys = [ys[:, d] for d in range(ys.shape[1])]
    n = len(ys)
    if isinstance(Params, dict) or len(Params) != n:
        raise ValueError('one Params dict per channel')
    gens = [infer_steps(ys[k], Params[k], Opts) for k in range(n)]
    out = [None] * n; pending = {}
    for k, g in enumerate(gens):
        pending[k] = next(g)                                 # every channel has at least one resolution
    while pending:
        groups = {}
        for k, r in pending.items():                         # all requests are ('level', ...) here
            groups.setdefault((r[3]['T'], r[3]['Tx']), []).append(k)
        nxt = {}
        for (T, Tx), ks in groups.items():
            per_sample = any(np.ndim(pending[k][2]['vary']) > 0 for k in ks)
            vary = np.stack([np.broadcast_to(np.asarray(pending[k][2]['vary'], float), (T,)) for k in ks]) if per_sample \
                else np.array([float(pending[k][2]['vary']) for k in ks])
            h = GppadHandle(np.stack([pending[k][1] for k in ks]), Tx, vary, np.array([float(pending[k][2]['varx']) for k in ks]),
                            np.array([float(pending[k][2]['mux']) for k in ks]), np.array([float(pending[k][2]['varc']) for k in ks]),
                            len=np.array([float(pending[k][2]['len']) for k in ks]), device=device)
            try:                                             # a channel leaves with the ('level', ...) of its next resolution
                done, left = lock_step_rows(h.eval, [gens[k] for k in ks], Tx, lambda r: r[1] if r[0] == 'x' else None)
            finally:
                h.close()
            for j, k in enumerate(ks):
                if j in left:
                    nxt[k] = left[j]
                else:
                    out[k] = done[j]
        pending = nxt
    return out


# ---------------------------------------------------------------------------------------------------------------- top level
def FBGPMAP(Y, len, Opts=None, evaluator=None, device=0):
    """FBGPMAP(Y,len,Opts) (FBGPMAP.m): GPPAD down the columns of Y (T x D).  len: a scalar or D length-scales -- the marginal
    parameters varc, varx, mux of every channel are learned (LearnMarginalParams) -- or a Params dict with len, varx, varc, mux
    (scalars or D entries) and optionally vary (T x D, T x 1 or a scalar; default zeros(T, D) as :51), which fixes them.  The envelopes of
    all channels are inferred in lock-step (InferAmplitudeGPMAP_many); with an `evaluator` channel by channel through InferAmplitudeGPMAP.
    Returns (A, C, Params, Info, X), the order of GPPAD's outputs (the .m's own order is [A,X,C,Params,Info]): A = sqrt(varc) a (T x D, or Tx x D with
    Opts.Long), C = Y ./ A(1:T, :), Info[d] = (LearnMarginalParams' Info or None, InferAmplitudeGPMAP's Info)."""
    Opts = LoadLearnMargGPPADOpts(Opts)
    Y = np.asarray(Y, float)
    if Y.ndim == 1:
        Y = Y[:, None]
    T, D = Y.shape
    if isinstance(len, dict):
        Params = dict(len); LrnPar = False
        lens = np.asarray(Params['len'], float)
    else:
        Params = {}; LrnPar = True
        lens = np.asarray(len, float)
    if lens.ndim == 2 and lens.shape[0] > 1 and (LrnPar or D == 1):
        raise NotImplementedError('a column of length-scales asks for a cascade of modulators: FBCasGPMAP.m is not built')
    lens = lens.reshape(-1)
    if lens.size == 1:
        lens = np.full(D, lens[0])
    if lens.size != D:
        raise ValueError('len is a scalar or holds one length-scale per column of Y (D = %d): got %d' % (D, lens.size))
    vary = np.asarray(Params['vary'], float) if 'vary' in Params else np.zeros((T, D))
    if vary.ndim == 0:
        vary = np.full((1, D), float(vary))
    if vary.ndim == 1:
        vary = vary[:, None]
    if vary.shape[1] < D:
        vary = vary @ np.ones((1, D)) if vary.shape[1] == 1 else vary
    if vary.shape[0] not in (1, T) or vary.shape[1] != D:
        raise ValueError('Params.vary is a scalar, T x 1 or T x D: got %s' % (vary.shape,))
    if LrnPar:
        varx, varc, mux = np.zeros(D), np.zeros(D), np.zeros(D)
    else:
        varx, varc, mux = (np.broadcast_to(np.asarray(Params[k], float).reshape(-1), (D,)).copy() for k in ('varx', 'varc', 'mux'))
    Info1 = [None] * D
    for d in range(D):
        if LrnPar:
            varc[d], varx[d], mux[d], Info1[d] = LearnMarginalParams(Y[:, d], Opts)
    Ps = [PackParamsGP(varx[d], lens[d], mux[d], varc[d], vary[:, d] if vary.shape[0] > 1 else float(vary[0, d])) for d in range(D)]
    if evaluator is None:
        res = InferAmplitudeGPMAP_many([Y[:, d] for d in range(D)], Ps, Opts, device=device)
    else:
        res = [InferAmplitudeGPMAP(Y[:, d], Ps[d], Opts, evaluator=evaluator) for d in range(D)]
    A = np.stack([np.sqrt(varc[d]) * res[d][0] for d in range(D)], axis=1)
    X = np.stack([res[d][1] for d in range(D)], axis=1)
    C = Y / A[:T, :]
    Params = {'len': lens, 'varx': varx, 'varc': varc, 'mux': mux, 'vary': vary}
    return A, C, Params, [(Info1[d], res[d][2]) for d in range(D)], X


def GPPAD(Y, len, LrnLen=0, Opts=None, nout=5, evaluator=None, device=0):
    """[A,C,Params,Info,X] = GPPAD(Y,len,LrnLen,Opts) (GPPAD.m) in the form the training drivers call: GPPAD(Y, len) -- a time-scale,
    the remaining parameters learned per column -- and GPPAD(Y, Params).  Opts modifies the defaults of LoadLearnMargGPPADOpts.m and
    LoadInferenceGPMAPOpts.m.  nout stands for nargout: more than 5 outputs are the error bars."""
    if LrnLen != 0:
        raise NotImplementedError('LrnLen = %r: learning the time-scale is FBGPMAPLearnLen.m, which this call does not run (LrnLen = 0 is served here; nagp.FBGPMAPLearnLen serves the learning)' % (LrnLen,))
    if nout > 5:
        raise NotImplementedError('outputs 6-8 (VarX, Aupper, Alower) are the Laplace error bars of FBGPMAPLearnLen.m / LoadErrorBarsLapOpts.m, which this call does not run (nagp.FBGPMAPLearnLen with nout=8 serves them)')
    return FBGPMAP(Y, len, Opts, evaluator=evaluator, device=device)
