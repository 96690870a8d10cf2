"""Host-side mirror of the modulator prior fit, the block of the reference's training drivers between nmf_fp and the initial parameter
vector (experiments/train_model.m:132-149, train_GTFNMF.m:91-108, train_GTFNMF_gaps.m:91-108):

    [lenx,varx,info] = trainSEGP_RS(x,opts,lenx,varx,vary)                     experiments/toolsGP/trainSEGP_RS.m
    [obj,dobj] = getObjSEGP(param,specy,vary,varx)                             experiments/toolsGP/getObjSEGP.m
    [fftCov,dfftCov] = getGPSESpec(len,T)                                      experiments/toolsGP/getGPSESpec.m

The objective and its gradient -- every sum over the T frequencies of the periodogram -- run on the GPU (nagp_segp_obj, include/nagp.h);
the FFT of the signal (arbitrary length), the conjugate-gradient line search (minimize.minimize_steps) and the 201-tap smoothing of
modulator_prior_init stay on the host.  There is no CPU fallback: the `evaluator` argument of the fit exists so that the tests can
put the float64 restatement through the same driver.
"""
import math
import warnings

import numpy as np

from . import _lib as L
from ._drive import forward, lock_step, opt as _opt, run
from .minimize import minimize_steps


def segp_obj(param, specy, vary=None, varx=None, grad=True, device=0):
    """nagp_segp_obj with NumPy arrays.  param (n_param,) or (P, n_param) with n_param = 1 (log len), 2 (and log varx) or 3 (and
    log vary); specy (T,) shared by the problems or (P, T); vary (needed when n_param <= 2) and varx (needed when n_param = 1) scalars
    or (P,).  Returns Obj and, with grad, dObj, with the leading problem axis of param."""
    param = np.asarray(param, float); single = param.ndim <= 1
    pa = L.f64(param.reshape(1, -1) if single else param, 'C')
    spec = np.asarray(specy, float)
    if pa.ndim != 2 or spec.ndim not in (1, 2) or (spec.ndim == 2 and spec.shape[0] != pa.shape[0]):
        raise ValueError('param must be (n_param,) or (P, n_param) and specy (T,) or (P, T): got %s, %s' % (param.shape, spec.shape))
    P, n_param = pa.shape
    if n_param not in (1, 2, 3):
        raise ValueError('param holds log(len) [, log(varx) [, log(vary)]]: got %d entries' % n_param)
    if (n_param <= 2 and vary is None) or (n_param == 1 and varx is None):
        raise ValueError('n_param = %d needs vary%s' % (n_param, ' and varx' if n_param == 1 else ''))
    T = spec.shape[-1]
    spec = L.f64(spec, 'C')
    vy = L.f64(np.broadcast_to(np.asarray(vary, float), (P,)), 'C') if n_param <= 2 else None
    vx = L.f64(np.broadcast_to(np.asarray(varx, float), (P,)), 'C') if n_param == 1 else None
    Obj = np.zeros(P); dObj = np.zeros((P, n_param)) if grad else None
    L.check(L.lib().nagp_segp_obj(P, n_param, T, L.dptr(pa), L.dptr(spec), T if spec.ndim == 2 else 0, L.dptr(vy), L.dptr(vx),
                                  L.dptr(Obj), L.dptr(dObj), int(device)))
    if single:
        return (Obj[0], dObj[0]) if grad else Obj[0]
    return (Obj, dObj) if grad else Obj


def getObjSEGP(param, specy, *varargin, nout=2, device=0):
    """[obj,dobj] = getObjSEGP(param,specy,vary,varx) (getObjSEGP.m:1), the reference's argument order: no further argument -- param
    holds log(len), log(varx), log(vary); vary -- param holds log(len), log(varx); vary and varx -- param(1) = log(len) is used.
    nout stands for nargout (1: obj alone)."""
    if len(varargin) > 2:
        raise ValueError('getObjSEGP(param, specy [, vary [, varx]])')
    n_param = 3 - len(varargin)
    p = np.asarray(param, float).reshape(-1)
    if p.size < n_param:
        raise ValueError('param must hold %d entries with %d further arguments' % (n_param, len(varargin)))
    vary = varargin[0] if len(varargin) >= 1 else None
    varx = varargin[1] if len(varargin) == 2 else None
    return segp_obj(p[:n_param], np.asarray(specy, float).reshape(-1), vary=vary, varx=varx, grad=nout > 1, device=device)


def getGPSESpec(len, T, nout=1):
    """[fftCov,dfftCov] = getGPSESpec(len,T) (getGPSESpec.m:1) in host NumPy: the spectrum of a unit-variance squared-exponential GP on
    the frequency list [0:ceil(T/2), -floor(T/2)+1:-1] * 2 pi / T, one column per length-scale, and (nout = 2) its derivative in len,
    column d with the length-scale of column d (the .m's line is written for one length-scale)."""
    ell = np.asarray(len, float).reshape(-1); T = int(T)
    f = np.concatenate([np.arange(0, -(-T // 2) + 1), np.arange(-(T // 2) + 1, 0)]).astype(float)
    omega = (2 * np.pi * f / T)[:, None]
    fftCov = np.sqrt(2 * np.pi * ell ** 2)[None, :] * np.exp(-omega ** 2 * ell[None, :] ** 2 / 2)
    if nout < 2:
        return fftCov
    return fftCov, fftCov * (1.0 / ell[None, :] - omega ** 2 * ell[None, :])


def train_steps(x, opts=None, lenx=None, varx=None, vary=None):
    """trainSEGP_RS as a generator: it yields a request (param, specx, vary, varx) and is sent (obj, dobj); its return value is
    (lenx, varx, info)."""
    given = [v is not None for v in (lenx, varx, vary)]
    if any(given) and not all(given):
        raise ValueError('lenx, varx and vary are given together or not at all')
    if opts is not None and not all(given):
        raise ValueError('opts without lenx, varx and vary: trainSEGP_RS.m:66-68 reads all three once a second argument is there')
    numIts = _opt(opts, 'numIts', 100); progress_chunk = _opt(opts, 'progress_chunk', 100)            # :29-39
    x = np.asarray(x, float).reshape(-1)
    T = x.size
    if T < 2:
        raise ValueError('a signal of at least 2 samples is needed')
    specx = np.abs(np.fft.fft(x)) ** 2                                                               # :41
    if not all(given):                                                                               # :45-62
        varx = np.var(x, ddof=1)
        n = T // 2 + 1                                       # linspace(0,1/2,T/2+1): a fractional count is floored
        om = np.linspace(0, 0.5, n)
        om = np.concatenate([om, om[-2:0:-1]]) if T % 2 == 0 else np.concatenate([om, om[:0:-1]])
        ave_om_sq = (om ** 2 @ specx) / np.sum(specx)
        lenx = 1 / (2 * np.pi * np.sqrt(ave_om_sq))
        vary = 0.1
    lenx, varx, vary = float(lenx), float(varx), float(vary)
    n_chunks = int(math.ceil(numIts / progress_chunk))                                               # :77-78
    Obj, it = [], []
    params = np.array([np.log(lenx)])                                                                # :82: log(lenx) alone is optimised
    for _ in range(n_chunks):
        params, ObjCur, itCur = yield from forward(minimize_steps(params, progress_chunk), lambda p: (p, specx, vary, varx))
        lenx = float(np.exp(params[0]))
        Obj.append(ObjCur); it.append(itCur)
    info = {'Obj': np.concatenate(Obj) if Obj else np.zeros(0), 'it': np.array(it, int)}
    if lenx > 100:                                                                                   # :181-183
        warnings.warn('trainSEGP_RS: lenx > 100, might be over-fitting and underestimating lenx')
    return lenx, varx, info


def _device_evaluator(device):
    def ev(param, specy, vary, varx):
        return segp_obj(param, specy, vary=vary, varx=varx, device=device)
    return ev


def trainSEGP_RS(x, opts=None, lenx=None, varx=None, vary=None, evaluator=None, device=0):
    """[lenx,varx,info] = trainSEGP_RS(x,opts,lenx,varx,vary) (trainSEGP_RS.m:1): a squared-exponential GP plus white noise fitted to
    the regularly sampled x by conjugate gradients on the spectral-domain likelihood.  Kept: specx = |fft(x)|^2, varx = var(x) (n - 1),
    the initial lenx from the spectrum-weighted mean square frequency (:51-60; for odd T linspace(0,1/2,T/2+1) has floor(T/2+1)
    points), vary = 0.1, log(lenx) as the only optimised parameter, L = ceil(numIts / progress_chunk) calls of minimize with
    progress_chunk line searches each (defaults 100 and 100), info['Obj'] and info['it'] concatenated over the chunks, the warning for
    lenx > 100 (a Python warning).  opts without lenx, varx and vary is a ValueError (the .m indexes past varargin there); the
    progress lines are not printed.  The FFT of x stays on the host (arbitrary lengths, once per fit); every objective evaluation is
    one nagp_segp_obj call.
    evaluator(param, specy, vary, varx) -> (obj, dobj): the objective, by default nagp_segp_obj on `device`."""
    ev = evaluator or _device_evaluator(device)
    return run(train_steps(x, opts, lenx, varx, vary), lambda req: ev(*req))


def _per_signal(v, n, name):
    if v is None:
        return [None] * n
    a = np.asarray(v, float)
    if a.ndim == 0:
        return [float(a)] * n
    if a.shape != (n,):
        raise ValueError('%s must be a scalar or hold one entry per signal' % name)
    return [float(e) for e in a]


def trainSEGP_RS_many(xs, opts=None, lenx=None, varx=None, vary=None, device=0):
    """trainSEGP_RS on several signals in lock-step: one generator per signal, the pending evaluation requests of a round gathered and
    issued as one nagp_segp_obj call per group of equal T.  A problem's bits do not depend on its batch mates, so the results equal the
    one-at-a-time fits to the bit.  lenx, varx, vary: scalars or one entry per signal.  Returns a list of (lenx, varx, info)."""
    n = len(xs)
    ls, vxs, vys = _per_signal(lenx, n, 'lenx'), _per_signal(varx, n, 'varx'), _per_signal(vary, n, 'vary')
    def issue(rs):
        return list(zip(*segp_obj(np.stack([r[0] for r in rs]), np.stack([r[1] for r in rs]), vary=np.array([r[2] for r in rs]),
                                  varx=np.array([r[3] for r in rs]), device=device)))
    return lock_step([train_steps(x, opts, ls[k], vxs[k], vys[k]) for k, x in enumerate(xs)], lambda r: r[1].size, issue)


def conv_same(u, v):
    """conv(u,v,'same'): the central numel(u) entries of the full convolution, also when u is the shorter of the two"""
    u = np.asarray(u, float).reshape(-1); v = np.asarray(v, float).reshape(-1)
    start = int(math.ceil((v.size - 1) / 2))
    return np.convolve(u, v, 'full')[start:start + u.size]


def smoothed_log_envelopes(HEst):
    """train_model.m:137-146 for every column of HEst (T x N): the inverse softplus of HEst + 1e-8, smoothed with the normalised 201-tap
    filter log(1 + exp(-k^2 / 2)), k = -100 .. 100, and its mean.  Returns (logHsm (T x N), mux (N,))."""
    H = np.asarray(HEst, float)
    if H.ndim == 1:
        H = H[:, None]
    if H.ndim != 2 or H.shape[0] < 2:
        raise ValueError('HEst must be T x N with T >= 2')
    k = np.arange(-100, 101, dtype=float)
    filt = np.log(1 + np.exp(-0.5 * k ** 2))
    filt = filt / np.sum(filt)
    logHthresh = np.log(np.exp(H + 1e-8) - 1)
    logHsm = np.stack([conv_same(logHthresh[:, n], filt) for n in range(H.shape[1])], axis=1)
    return logHsm, np.mean(logHsm, axis=0)


def modulator_prior_init(HEst, device=0):
    """The block train_model.m:136-149 (train_GTFNMF.m:95-108) on the NMF activations HEst (T x N): per component the thresholded,
    smoothed, mean-free log-envelope (smoothed_log_envelopes) and its trainSEGP_RS fit, all components as one trainSEGP_RS_many.
    Returns (lenx_nmf (N,), varx_nmf (N,), mux (N,), infos); the driver's len_slow = 5 lenx_nmf, var_slow = varx_nmf and their clamps
    stay with the caller."""
    logHsm, mux = smoothed_log_envelopes(HEst)
    fits = trainSEGP_RS_many([logHsm[:, n] - mux[n] for n in range(logHsm.shape[1])], device=device)
    return np.array([f[0] for f in fits]), np.array([f[1] for f in fits]), mux, [f[2] for f in fits]
