"""Host-side mirror of the filterbank spectrum fit, the first call of the reference's real-audio drivers after the audio is loaded
(demo_nonstationary_filterbank.m:56, experiments/train_GTFNMF.m:56):

    [varx,lamx,om,Info] = fit_probSTFT_SD(y,D,kernel,Opts)                     unifying_prob_tf/fit_probSTFT_SD.m
    [Obj,dObj] = get_Obj_pSTFT_<exp|matern32|matern52|all>(theta,vary,specTar,minVar,limOm,limLam,bet,kernel)
    [pg,varpg] = welchMethod(y,numFreq,ovLp)                                   prob_filterbank/welchMethod.m
    [om,lamx,varx] = freq2probSpec(fmax,df,varMa)                              prob_filterbank/freq2probSpec.m
    [X,fX,i] = minimize(X,f,length,P1,...)                                     prob_filterbank/minimize.m

The objective and its gradient -- every sum over the frequencies -- run on the GPU (nagp_pstft_obj, include/nagp.h); the level loop, the
line search and the periodograms (FFTs of arbitrary length) stay on the host.  There is no CPU fallback: the `evaluator` argument of
the fit exists so that the tests can put the float64 restatement through the same driver.
"""
import math

import numpy as np

from . import _lib as L
from ._drive import forward, lock_step, opt as _opt, run
from .minimize import minimize, minimize_steps, INT, EXT, MAX, RATIO, SIG, RHO, REALMIN  # noqa: F401  (their home is minimize.py)

KERNEL_ID = {'exp': 0, 'matern32': 1, 'matern52': 2, 'matern72': 3}
CLOSED = ('exp', 'matern32', 'matern52')                     # the kernels with a get_Obj_pSTFT_<kernel>.m (fit_probSTFT_SD.m:285-289)


def _kernel_id(kernel):
    if kernel not in KERNEL_ID:
        raise ValueError('unsupported kernel %r (supported: exp, matern32, matern52, matern72)' % (kernel,))
    return KERNEL_ID[kernel]


def pstft_obj(theta, vary, specTar, minVar, limOm, limLam, bet, kernel, form=None, grad=True, device=0):
    """nagp_pstft_obj with NumPy arrays.  theta (3D,) or (P, 3D); specTar (N,) shared by the problems or (P, N); vary, bet scalars or
    (P,); minVar (D,), limOm, limLam (D, 2) shared.  form: 0 the kernel-specific file, 1 get_Obj_pSTFT_all.m, None: what
    fit_probSTFT_SD.m:285-289 picks.  Returns Obj and, with grad, dObj, with the leading problem axis of theta."""
    kid = _kernel_id(kernel)
    if form is None:
        form = 0 if kernel in CLOSED else 1
    theta = np.asarray(theta, float); single = theta.ndim == 1
    th = L.f64(theta[None] if single else theta, 'C'); P = th.shape[0]; D = th.shape[1] // 3
    spec = np.asarray(specTar, float)
    if th.shape[1] != 3 * D or D < 1 or spec.ndim not in (1, 2) or (spec.ndim == 2 and spec.shape[0] != P):
        raise ValueError('theta must be (3D,) or (P, 3D) and specTar (N,) or (P, N): got %s, %s' % (theta.shape, spec.shape))
    N = spec.shape[-1]
    spec = L.f64(spec, 'C')
    vary = L.f64(np.broadcast_to(np.asarray(vary, float), (P,)), 'C'); bet = L.f64(np.broadcast_to(np.asarray(bet, float), (P,)), 'C')
    minVar = L.f64(np.asarray(minVar, float).reshape(-1), 'C')
    limOm = L.f64(np.asarray(limOm, float).reshape(-1, 2)); limLam = L.f64(np.asarray(limLam, float).reshape(-1, 2))     # column-major
    if minVar.size != D or limOm.shape[0] != D or limLam.shape[0] != D:
        raise ValueError('minVar must hold D = %d entries and limOm, limLam be (D, 2)' % D)
    Obj = np.zeros(P); dObj = np.zeros((P, 3 * D)) if grad else None
    L.check(L.lib().nagp_pstft_obj(P, kid, int(form), D, N, L.dptr(th), L.dptr(spec), N if spec.ndim == 2 else 0, L.dptr(vary), L.dptr(bet),
                                   L.dptr(minVar), L.dptr(limOm), L.dptr(limLam), L.dptr(Obj), L.dptr(dObj), int(device)))
    if single:
        return (Obj[0], dObj[0]) if grad else Obj[0]
    return (Obj, dObj) if grad else Obj


def _get_obj(kernel, form, theta, vary, specTar, minVar, limOm, limLam, bet, nout, device):
    """theta and specTar come as MATLAB columns; nout = 1 asks for the objective alone"""
    return pstft_obj(np.asarray(theta, float).reshape(-1), vary, np.asarray(specTar, float).reshape(-1), minVar, limOm, limLam, bet, kernel, form=form,
                     grad=nout > 1, device=device)


def get_Obj_pSTFT_exp(theta, vary, specTar, minVar, limOm, limLam, bet, dummy=None, nout=2, device=0):
    """[Obj,dObj] = get_Obj_pSTFT_exp(theta,vary,specTar,minVar,limOm,limLam,bet,dummy); nout stands for nargout (1: Obj alone)."""
    return _get_obj('exp', 0, theta, vary, specTar, minVar, limOm, limLam, bet, nout, device)


def get_Obj_pSTFT_matern32(theta, vary, specTar, minVar, limOm, limLam, bet, dummy=None, nout=2, device=0):
    """[Obj,dObj] = get_Obj_pSTFT_matern32(...)"""
    return _get_obj('matern32', 0, theta, vary, specTar, minVar, limOm, limLam, bet, nout, device)


def get_Obj_pSTFT_matern52(theta, vary, specTar, minVar, limOm, limLam, bet, dummy=None, nout=2, device=0):
    """[Obj,dObj] = get_Obj_pSTFT_matern52(...)"""
    return _get_obj('matern52', 0, theta, vary, specTar, minVar, limOm, limLam, bet, nout, device)


def get_Obj_pSTFT_all(theta, vary, specTar, minVar, limOm, limLam, bet, kernel, nout=2, device=0):
    """[Obj,dObj] = get_Obj_pSTFT_all(theta,vary,specTar,minVar,limOm,limLam,bet,kernel): exp, matern32, matern52, matern72 (with the
    file's len = sqrt(5) / lam for matern72); se is refused as everywhere in this library."""
    return _get_obj(kernel, 1, theta, vary, specTar, minVar, limOm, limLam, bet, nout, device)


def welchMethod(y, numFreq, ovLp):
    """[pg,varpg] = welchMethod(y,numFreq,ovLp) (welchMethod.m:43-66): chunks of numFreq samples with overlap ovLp, each extended evenly
    to [y; y(end-1:-1:2)], |fft|^2 / (2 (numFreq - 1))^2, averaged over the K = floor((T - ovLp) / (Tc - ovLp)) chunks."""
    y = np.asarray(y, float).reshape(-1); numFreq = int(numFreq); ovLp = int(ovLp)
    if ovLp > numFreq:
        return np.nan, np.nan                                # :36-41
    T = y.size; Tc = numFreq
    K = (T - ovLp) // (Tc - ovLp)
    pg = np.zeros(numFreq); Epg2 = np.zeros(numFreq)
    for k in range(K):
        yCur = y[(Tc - ovLp) * k:(Tc - ovLp) * k + Tc]
        specCur = np.abs(np.fft.fft(np.concatenate([yCur, yCur[-2:0:-1]]))) ** 2
        specCur = specCur[:numFreq] / (2 * (numFreq - 1)) ** 2
        pg = pg + specCur / K
        Epg2 = Epg2 + specCur ** 2 / K
    return pg, (Epg2 - pg ** 2) / K


def freq2probSpec(fmax, df, varMa):
    """[om,lamx,varx] = freq2probSpec(fmax,df,varMa) (freq2probSpec.m:19-23)"""
    fmax = np.asarray(fmax, float); df = np.asarray(df, float)
    om = 2 * np.pi * fmax
    c = np.cos(2 * np.pi * df)
    lamx = 2 - c - np.sqrt(c ** 2 - 4 * c + 3)
    return om, lamx, np.asarray(varMa, float) * (1 - lamx ** 2)


def _mirror(pg, T):
    """fit_probSTFT_SD.m:265-271: the two-sided spectrum, its length chosen by the parity of the SIGNAL length T"""
    return np.concatenate([pg, pg[-2:0:-1]]) if T % 2 == 0 else np.concatenate([pg, pg[:0:-1]])


def fit_steps(y, D, kernel, opts=None):
    """fit_probSTFT_SD as a generator: it yields a request (theta, vary, specTar, minVar, limOm, limLam, bet, grad) and is sent
    (Obj, dObj) (grad) or Obj; its return value is (varx, lamx, om, Info)."""
    _kernel_id(kernel)
    if _opt(opts, 'reassign', 0) == 1:
        raise NotImplementedError('opts.reassign = 1 (the get_pSTFT_spec_cts_* helpers) is not built; every driver sets 0')
    D = int(D)
    y = np.asarray(y, float).reshape(-1)
    y = y - np.mean(y)                                                           # :80-82
    varSig = np.var(y, ddof=1)
    y = y / np.sqrt(varSig)
    theta_init = _opt(opts, 'theta_init', None)
    if theta_init is None:                                                       # :85-101
        mVar = np.ones(D) / D
        fmax = np.linspace(1 / 40, 0.35, D)
        om, lamx, _ = freq2probSpec(fmax, fmax * (1 / 20), 1)
        cvar_d = mVar * (1 - lamx ** 2)
        lam_c = -np.log(lamx)
        lamLim = np.ones((D, 1)) * np.array([[0.0, 0.4]])
        cvar_c = cvar_d / (1 - np.exp(-2 * lam_c))
        mVar_c = cvar_c / (1 - lam_c ** 2)
    else:                                                                        # :104-128
        theta_init = np.asarray(theta_init, float).reshape(-1)
        if theta_init.size != 3 * D:
            raise ValueError('theta_init must hold 3 D = %d entries' % (3 * D))
        cvar_c = theta_init[:D]
        lam_c = theta_init[D:2 * D] * {'exp': 1.0, 'matern32': math.sqrt(3.0)}.get(kernel, math.sqrt(5.0))
        om = theta_init[2 * D:]
        lam_max = np.minimum(lam_c * _opt(opts, 'bandwidth_lim', 2), 1 - 1e-5)
        mVar_c = np.maximum(cvar_c / (1 - lam_c ** 2), 1e-3)
        lamLim = np.stack([np.zeros(D), lam_max], axis=1)
    minVar = np.maximum(mVar_c / 400, 1e-5)                                      # :134-135
    omLim = np.ones((D, 1)) * np.array([[0.0, np.pi]])
    if not (np.all(om > omLim[:, 0]) and np.all(om < omLim[:, 1]) and np.all(lam_c > lamLim[:, 0]) and np.all(lam_c < lamLim[:, 1])
            and np.all(mVar_c > minVar)):
        raise ValueError('the initial om, lam or marginal variance lies outside its limits (om in (0, pi), lam in (0, lam_max)): '
                         'om = %s, lam = %s, lam limits = %s' % (om, lam_c, lamLim[:, 1]))
    numLevels = int(_opt(opts, 'numLevels', 40)); numIts = _opt(opts, 'numIts', 10)
    minT = _opt(opts, 'minT', 200); maxT = _opt(opts, 'maxT', 1000)
    vary_an = np.asarray(_opt(opts, 'vary_an', np.logspace(np.log10(1e-6), np.log10(1e-10), numLevels)), float).reshape(-1)
    bet = np.logspace(np.log10(_opt(opts, 'bet', 100)), 0, numLevels)
    T = y.size
    numFreq = np.floor(np.logspace(np.log10(min(minT, T)), np.log10(min(maxT, T)), numLevels)).astype(int)
    ovLp = numFreq // 10
    yHO = _opt(opts, 'yHO', None)
    if yHO is not None:                                                          # :204-229
        yHO = np.asarray(yHO, float).reshape(-1) / np.sqrt(varSig)
        THO = yHO.size
        pgHO = welchMethod(yHO, THO, 0)[0] / (1 / 2 / THO)
        specHO = _mirror(pgHO, THO)
        likeHO = np.full(numLevels, np.nan)
    likeUnReg = np.full(numLevels, np.nan)                                       # :236-247
    specUR = _mirror(welchMethod(y, T, 0)[0] / (1 / 2 / T), T)
    Objs = []; ins = []
    for c2f in range(numLevels):
        pg = welchMethod(y, numFreq[c2f], ovLp[c2f])[0] / (1 / 2 / numFreq[c2f])
        specTar = _mirror(pg, T)
        theta = np.concatenate([np.log(mVar_c - minVar), np.log(om - omLim[:, 0]) - np.log(omLim[:, 1] - om),
                                np.log(lam_c - lamLim[:, 0]) - np.log(lamLim[:, 1] - lam_c)])
        vary = np.max(specTar) * vary_an[c2f]
        b = bet[c2f] * numFreq[c2f] / numFreq[c2f]                                # :299
        theta, ObjCur, inCur = yield from forward(minimize_steps(theta, numIts), lambda x: (x, vary, specTar, minVar, omLim, lamLim, b, True))
        if yHO is not None:
            likeHO[c2f] = yield (theta, 0.0, specHO, minVar, omLim, lamLim, 0.0, False)
        likeUnReg[c2f] = yield (theta, 0.0, specUR, minVar, omLim, lamLim, 0.0, False)
        Objs.append(ObjCur); ins.append(inCur)
        mVar_c = minVar + np.exp(theta[:D])                                       # :322-324
        om = omLim[:, 0] + (omLim[:, 1] - omLim[:, 0]) / (1 + np.exp(-theta[D:2 * D]))
        lam_c = lamLim[:, 0] + (lamLim[:, 1] - lamLim[:, 0]) / (1 + np.exp(-theta[2 * D:]))
    Info = {'Objs': np.concatenate(Objs) if Objs else np.zeros(0), 'ins': np.array(ins, int), 'likeUnReg': likeUnReg,
            'nObjs': np.array([o.size for o in Objs], int)}          # (nObjs: the entries of Objs per level; not in the .m)
    if yHO is not None:
        Info['likeHO'] = likeHO
    lamx = lam_c                                                                  # :486-490
    varx = (varSig / np.sum(mVar_c)) * (mVar_c * (1 - lamx ** 2))
    return varx, lamx, om, Info


def _device_evaluator(kernel, device):
    def ev(theta, vary, specTar, minVar, limOm, limLam, bet, grad):
        return pstft_obj(theta, vary, specTar, minVar, limOm, limLam, bet, kernel, grad=grad, device=device)
    return ev


def fit_probSTFT_SD(y, D, kernel, opts=None, evaluator=None, device=0):
    """[varx,lamx,om,Info] = fit_probSTFT_SD(y,D,kernel,Opts) (fit_probSTFT_SD.m:1): the coarse-to-fine spectrum match.  Kept: the
    rescaling of y and of varx, both initialisation branches (theta_init with its sqrt(3) / sqrt(5) factors, bandwidth_lim, the
    1 - 1e-5 cap, max(., 1e-3)), minVar, omLim, numFreq, ovLp, vary_an, bet as a logspace, the mirror of pg by the parity of T, the
    weight bet(c2f) numFreq(c2f) / numFreq(c2f(1)) = bet(c2f), Info.Objs / ins / likeUnReg / likeHO (with opts['yHO']); Info['nObjs'], the entries of Objs per level, is added.  matern72 goes
    through get_Obj_pSTFT_all as in :285-289.  Refused: an initial om or lam outside its limits (ValueError; the .m would take the
    log of a negative number), opts['reassign'] = 1 (NotImplementedError); verbose plotting is ignored.
    evaluator(theta, vary, specTar, minVar, limOm, limLam, bet, grad): the objective, by default nagp_pstft_obj on `device`."""
    ev = evaluator or _device_evaluator(kernel, device)
    return run(fit_steps(y, D, kernel, opts), lambda req: ev(*req))


def fit_probSTFT_SD_many(ys, D, kernel, opts=None, device=0):
    """fit_probSTFT_SD on several signals in lock-step: one generator per signal, the pending evaluation requests of a round gathered
    and issued as one nagp_pstft_obj call per group of equal N (and equal shared arguments).  A problem's bits do not depend on its
    batch mates, so the results equal the one-at-a-time fits to the bit.  Returns a list of (varx, lamx, om, Info)."""
    def issue(rs):
        grad = rs[0][7]
        res = pstft_obj(np.stack([r[0] for r in rs]), np.array([r[1] for r in rs]), np.stack([r[2] for r in rs]),
                        rs[0][3], rs[0][4], rs[0][5], np.array([r[6] for r in rs]), kernel, grad=grad, device=device)
        return list(zip(*res)) if grad else res
    return lock_step([fit_steps(y, D, kernel, opts) for y in ys], lambda r: (r[2].size, r[7], r[3].tobytes(), r[4].tobytes(), r[5].tobytes()), issue)
