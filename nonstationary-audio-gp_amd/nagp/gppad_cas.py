"""Host-side mirror of the GPPAD cascade, GPPAD(Y,[len1;...;lenM]): a signal as a carrier times M modulators of increasing time-scale,

    [A,X,C,Params,Info] = FBCasGPMAP(Y,Len,Opts)                               experiments/gppad/Cascade/FBCasGPMAP.m
    [A,X,c,Params,Info] = CasGPMAP(y,len,Opts)                                 gppad/Cascade/CasGPMAP.m
    [X,Obj] = MAPGPCasFast(X,y,Params,Dims,NumIts)                             gppad/Cascade/MAPGPCasFast.m
    [Obj,dObjdx] = GetObjCasGPFAST(x,y,fftCovs,Params,Dims)                    gppad/Cascade/GetObjCasGPFAST.m
    Dims = PackDimsCas(T,Tx,M), [T,Tx,M] = UnpackDimsCas(Dims)

Every level of a cascade is an FBGPMAP call with Opts.Long and Opts.Tx (gppad.py); the joint objective of the fine tuning and its
gradient -- M transforms tied by a product likelihood at every sample -- run on the GPU (nagp_gppad_cas_obj and the resident
nagp_gppad_cas_create / _eval / _destroy, include/nagp.h).  The line searches (minimize.minimize_steps) stay on the host.  There is no CPU
fallback: the `evaluator` argument exists so that the tests can put the float64 restatement through the same drivers.

What the reference's statements compute is reproduced, and said here once:
  1. The fine-tuning result is discarded.  MAPGPCasFast.m:15-20 minimises into `x` and returns reshape(X, ...), its input.  So CasGPMAP
     returns the level-by-level estimate and the fine tuning shows only in Info['ObjFT'].  That is the default (fine_tuned=False, the
     literal form); fine_tuned=True returns the minimiser's x instead (the consistent form).
  2. Levels (CasGPMAP.m:30-76): y / sqrt(var(y)) with the n - 1 variance; Tx = GetTx(T, max(len) tol); level 1 is FBGPMAP(y, len(1)) with
     Long = 1 and Tx; level m is FBGPMAP(A(1:Tx - len(m) tol, m-1), len(m)) -- the colon's end floored when len(m) tol is no integer --,
     then A(:,m-1) ./= A(:,m); varc is multiplied, varx and mux are appended.
  3. X = log(exp(A) - 1) is used raw as the starting point (:81).  A(:,1) carries sqrt(varc) while varc also enters the likelihood.
  4. Outputs as :86-93: A = log(1 + exp(X(1:T,:))), c = (y / sigy) ./ prod(A,2), X(1:T,:), Params.varc multiplied by sigy^2 at the end.
  5. FBCasGPMAP.m: Len (M x 1) or (M x D); A and X are (T, D, M) squeezed; Params.len (M x D), varc (D), varx and mux (M x D) as :19-37.
     The .m keeps only the last channel's Info; the list of all of them is returned.
  6. Options: the defaults of gppad.py (tol = 5, MinLength = 8, NumIts = 2000) and NumItsCas = 500 (CASGPMAPOpts.m).
"""
import math

import numpy as np

from . import _lib as L
from ._drive import ResidentHandle, close, forward, lock_step_rows, run
from .gppad import FBGPMAP, GetTx, LoadLearnMargGPPADOpts
from .minimize import minimize_steps

MAX_M = 8


def PackDimsCas(T, Tx, M):
    """Dims = PackDimsCas(T,Tx,M) (PackDimsCas.m) as a dict"""
    return {'T': int(T), 'Tx': int(Tx), 'M': int(M)}


def UnpackDimsCas(Dims):
    """[T,Tx,M] = UnpackDimsCas(Dims) (UnpackDimsCas.m)"""
    return int(Dims['T']), int(Dims['Tx']), int(Dims['M'])


def LoadCasGPMAPOpts(Opts=None):
    """the defaults of LoadLearnMargGPPADOpts.m, LoadInferenceGPMAPOpts.m and CASGPMAPOpts.m (NumItsCas = 500) under the entries of Opts"""
    d = {'NumItsCas': 500}
    d.update(Opts or {})
    return LoadLearnMargGPPADOpts(d)


# ---------------------------------------------------------------------------------------------------------------- the objective
def _per_column(v, P, M, name):
    a = np.asarray(v, float)
    if a.ndim <= 1:
        a = np.broadcast_to(a.reshape(-1), (P, M)) if a.size in (1, M) else a
    if a.shape != (P, M):
        raise ValueError('%s must hold one entry per column (M,) or per cascade and column (P, M): got %s' % (name, np.shape(v)))
    return L.f64(a, 'C')


def _shaped(y, M, Tx, varx, mux, varc, len, fftCovs):
    """the data arguments of nagp_gppad_cas_create / nagp_gppad_cas_obj from NumPy arrays, in the order of the C signatures: y (P, T), len,
    fftCovs, cov_stride, varx, mux, varc"""
    P = y.shape[0]
    if (len is None) == (fftCovs is None):
        raise ValueError('exactly one of len and fftCovs is given')
    ln = _per_column(len, P, M, 'len') if len is not None else None
    cov = None
    if fftCovs is not None:
        cov = L.f64(np.asarray(fftCovs, float), 'C')
        if cov.shape not in ((M, Tx), (P, M, Tx)):
            raise ValueError('fftCovs must be (M, Tx) or (P, M, Tx): got %s' % (cov.shape,))
    vc = np.asarray(varc, float)
    vc = np.full(P, float(vc)) if vc.ndim == 0 else vc
    if vc.shape != (P,):
        raise ValueError('varc must be a scalar or hold one entry per cascade')
    return [L.dptr(y), L.dptr(ln), L.dptr(cov), M * Tx if cov is not None and cov.ndim == 3 else 0, L.dptr(_per_column(varx, P, M, 'varx')),
            L.dptr(_per_column(mux, P, M, 'mux')), L.dptr(L.f64(vc, 'C'))]


class GppadCasHandle(ResidentHandle):
    """The resident form (nagp_gppad_cas_create): y (P, T), 1 / c, the parameters and the twiddles stay on the device; eval(x) moves x
    (P, M Tx) -- per cascade the .m's X(:) -- in and Obj (P,), dObj (P, M Tx) out.  The spectra are fftCovs ((M, Tx) shared or (P, M, Tx))
    or are formed on the device from len ((M,) or (P, M))."""
    _eval, _destroy = 'nagp_gppad_cas_eval', 'nagp_gppad_cas_destroy'

    def __init__(self, y, M, Tx, varx, mux, varc, len=None, fftCovs=None, device=0):
        import ctypes as C
        y = L.f64(np.atleast_2d(np.asarray(y, float)), 'C')
        self.P, self.T = y.shape; self.M = int(M); self.Tx = int(Tx); self.nx = self.M * self.Tx
        h = C.c_void_p()
        L.check(L.lib().nagp_gppad_cas_create(C.byref(h), self.P, self.M, self.T, self.Tx, *_shaped(y, self.M, self.Tx, varx, mux, varc, len, fftCovs), int(device)))
        self._h = h


def gppad_cas_obj(x, y, varx, mux, varc, len=None, fftCovs=None, grad=True, device=0):
    """nagp_gppad_cas_obj with NumPy arrays.  x (M, Tx) or (P, M, Tx) -- row m is column m of the .m's X --; y (T,) or (P, T); varx, mux (M,)
    or (P, M); varc a scalar or (P,); the spectra as fftCovs ((M, Tx) shared or (P, M, Tx)) or formed on the device from len ((M,) or
    (P, M)).  Returns Obj and, with grad, dObj, shaped as x."""
    x = np.asarray(x, float); single = x.ndim == 2
    xx = L.f64(x[None] if single else x, 'C'); yy = L.f64(np.atleast_2d(np.asarray(y, float)), 'C')
    if xx.ndim != 3 or yy.ndim != 2 or yy.shape[0] != xx.shape[0]:
        raise ValueError('x must be (M, Tx) or (P, M, Tx) and y (T,) or (P, T): got %s, %s' % (x.shape, np.shape(y)))
    P, M, Tx = xx.shape; T = yy.shape[1]
    Obj = np.zeros(P); dObj = np.zeros((P, M, Tx)) if grad else None
    L.check(L.lib().nagp_gppad_cas_obj(P, M, T, Tx, L.dptr(xx), *_shaped(yy, M, Tx, varx, mux, varc, len, fftCovs), L.dptr(Obj), L.dptr(dObj), int(device)))
    if single:
        return (Obj[0], dObj[0]) if grad else Obj[0]
    return (Obj, dObj) if grad else Obj


def GetObjCasGPFAST(x, y, fftCovs, Params, Dims, nout=2, device=0):
    """[Obj,dObjdx] = GetObjCasGPFAST(x,y,fftCovs,Params,Dims) (GetObjCasGPFAST.m:1) on the device: x the M Tx entries of X(:) (or X itself,
    Tx x M), fftCovs Tx x M, Params a dict with varx, mux (M each) and varc (len and vary are not read), Dims a dict with T, Tx and M.
    dObjdx has the M Tx entries of the .m's column.  nout stands for nargout."""
    T, Tx, M = UnpackDimsCas(Dims)
    x = np.asarray(x, float); y = np.asarray(y, float).reshape(-1)
    x = x.T.reshape(-1) if x.shape == (Tx, M) and M > 1 else x.reshape(-1)                          # X(:)
    cov = np.asarray(fftCovs, float).reshape(Tx, M) if np.ndim(fftCovs) < 2 else np.asarray(fftCovs, float)
    if x.size != M * Tx or y.size != T or cov.shape != (Tx, M):
        raise ValueError('x holds Dims.M Dims.Tx = %d, y Dims.T = %d entries and fftCovs is Tx x M: got %d, %d, %s' % (M * Tx, T, x.size, y.size, cov.shape))
    out = gppad_cas_obj(x.reshape(M, Tx), y, np.asarray(Params['varx'], float).reshape(-1), np.asarray(Params['mux'], float).reshape(-1),
                        float(np.asarray(Params['varc'], float).reshape(-1)[0]), fftCovs=cov.T, grad=nout > 1, device=device)
    return (out[0], out[1].reshape(-1)) if nout > 1 else out


# ---------------------------------------------------------------------------------------------------------------- fine tuning
def _device_evaluator(device):
    """evaluator(y, Params, Dims) -> f(x) -> (Obj, dObj) for the joint objective: one resident cascade handle; f.close() releases it"""
    def open_cascade(y, Params, Dims):
        h = GppadCasHandle(np.asarray(y, float).reshape(1, -1), Dims['M'], Dims['Tx'], Params['varx'], Params['mux'], Params['varc'], len=Params['len'],
                           device=device)

        def f(x):
            Obj, dObj = h.eval(x)
            return Obj[0], dObj[0]
        f.close = h.close
        return f
    return open_cascade


def MAPGPCasFast(X, y, Params, Dims, NumIts, evaluator=None, device=0, fine_tuned=False):
    """[X,Obj] = MAPGPCasFast(X,y,Params,Dims,NumIts) (MAPGPCasFast.m): NumIts line searches of minimize on GetObjCasGPFAST from X(:), with
    the spectra GetFFTCovFast(Params.len(m), Dims.Tx) formed on the device.  As the .m's last statement reshapes X, its input, the
    first output is the starting point and the minimisation shows in Obj alone (item 1 of the module docstring); fine_tuned=True
    returns the minimiser's x, reshaped, instead.  X is Tx x M.  evaluator(y, Params, Dims) returns the joint objective f(x) -> (Obj,
    dObj) on x = X(:) (by default a resident nagp_gppad_cas handle); Dims carries M."""
    T, Tx, M = UnpackDimsCas(Dims)
    X = np.asarray(X, float).reshape(Tx, M)
    f = (evaluator or _device_evaluator(device))(np.asarray(y, float).reshape(-1), Params, Dims)
    try:
        x, Obj, _ = run(minimize_steps(X.T.reshape(-1), int(NumIts)), f)
    finally:
        close(f)
    return (x.reshape(M, Tx).T if fine_tuned else X), Obj


def cas_steps(y, len, Opts=None, fine_tuned=False):
    """CasGPMAP as a generator.  For every level it yields ('fbgpmap', signal, len_m, Opts) and is sent (a (Tx,), Params_m, Info_m) of
    FBGPMAP on that one column; then it yields ('cas', y, Params, Dims) and is sent anything, then ('x', x) and is sent (Obj, dObj)
    there; its return value is (A, X, c, Params, Info)."""
    Opts = LoadCasGPMAPOpts(Opts)
    y = np.asarray(y, float).reshape(-1)
    lens = np.asarray(len, float).reshape(-1)
    M, T = lens.size, y.size
    if not 1 <= M <= MAX_M:
        raise ValueError('a cascade has 1 to %d modulators: got %d length-scales' % (MAX_M, M))
    sigy = np.sqrt(np.var(y, ddof=1))                                                                # :30-31
    y = y / sigy
    Tx = GetTx(T, np.max(lens) * Opts['tol'])                                                        # :42
    OptsL = dict(Opts); OptsL['Long'] = 1; OptsL['Tx'] = Tx
    A = np.zeros((Tx, M))
    a, P1, I1 = yield ('fbgpmap', y, float(lens[0]), OptsL)                                          # :54
    A[:, 0] = a
    varc = float(P1['varc']); varx = [float(P1['varx'])]; mux = [float(P1['mux'])]; levels = [I1]
    for m in range(1, M):                                                                            # :59-76
        Tm = int(math.floor(Tx - lens[m] * Opts['tol']))
        a, Pm, Im = yield ('fbgpmap', A[:Tm, m - 1].copy(), float(lens[m]), OptsL)
        A[:, m] = a
        A[:, m - 1] = A[:, m - 1] / A[:, m]
        varc = varc * float(Pm['varc']); varx.append(float(Pm['varx'])); mux.append(float(Pm['mux'])); levels.append(Im)
    Params = {'len': lens, 'varx': np.array(varx), 'mux': np.array(mux), 'varc': varc}
    Dims = PackDimsCas(T, Tx, M)
    with np.errstate(over='ignore', divide='ignore'):
        X = np.log(np.exp(A) - 1)                                                                    # :81
    yield ('cas', y, Params, Dims)
    x, Obj, _ = yield from forward(minimize_steps(X.T.reshape(-1), int(Opts['NumItsCas'])), lambda x: ('x', x))
    if fine_tuned:
        X = x.reshape(M, Tx).T
    with np.errstate(over='ignore'):
        A = np.log(1 + np.exp(X[:T]))                                                                # :86-88
    c = y / np.prod(A, axis=1)
    Params = dict(Params); Params['varc'] = varc * sigy ** 2                                         # :93
    return A, X[:T].copy(), c, Params, {'ObjFT': Obj, 'Levels': levels, 'Tx': Tx, 'sigy': sigy}


def _fbgpmap_column(req, evaluator, device):
    A, C, P, Info, X = FBGPMAP(req[1][:, None], req[2], req[3], evaluator=evaluator, device=device)
    return A[:, 0], {k: P[k][0] for k in ('varc', 'varx', 'mux')}, Info[0]


def CasGPMAP(y, len, Opts=None, fine_tuned=False, evaluator=None, device=0):
    """[A,X,c,Params,Info] = CasGPMAP(y,len,Opts) (CasGPMAP.m): y (T,) as a carrier c times the M modulators A (T x M) of the time-scales
    len (M, in samples, shortest first), level by level through FBGPMAP and then jointly fine-tuned by NumItsCas line searches
    (MAPGPCasFast).  Items 1-4 and 6 of the module docstring say what is kept of the .m: by default A and X are the level-by-level
    estimate and the fine tuning shows only in Info['ObjFT']; fine_tuned=True returns the fine-tuned cascade.  Params: len, varx, mux
    (M each), varc.  Info: ObjFT, Levels (FBGPMAP's Info of every level), Tx, sigy.  evaluator(y, Params, Dims) -> f(x) -> (Obj, dObj)
    serves the levels (Dims without M: the objective of gppad.py) and the fine tuning (Dims with M); by default the device does."""
    ev = evaluator or _device_evaluator(device)
    joint = [None]

    def answer(req):
        if req[0] == 'fbgpmap':
            return _fbgpmap_column(req, evaluator, device)
        if req[0] == 'cas':
            joint[0] = ev(req[1], req[2], req[3])
            return None
        return joint[0](req[1])
    try:
        return run(cas_steps(y, len, Opts, fine_tuned), answer)
    finally:
        close(joint[0])


def _cas_many(ys, lens, Opts, fine_tuned, device):
    """CasGPMAP on several channels in lock-step on the device: the channels' FBGPMAP calls of a level whose (T_m, Tx) agree are one FBGPMAP
    call (InferAmplitudeGPMAP_many inside), and the channels whose (T, Tx, M) agree share one cascade handle for the fine tuning
    (lock_step_rows).  A cascade's bits do not depend on its batch mates: the results equal the one-at-a-time runs to the bit."""
    n = len(ys)
    gens = [cas_steps(ys[k], lens[k], Opts, fine_tuned) for k in range(n)]
    out = [None] * n
    pending = {k: next(g) for k, g in enumerate(gens)}
    while pending:
        groups = {}
        for k, r in pending.items():
            key = ('fbgpmap', r[1].size, r[3]['Tx']) if r[0] == 'fbgpmap' else ('cas', r[3]['T'], r[3]['Tx'], r[3]['M'])
            groups.setdefault(key, []).append(k)
        nxt = {}
        for key, ks in groups.items():
            if key[0] == 'fbgpmap':
                A, C, P, Info, X = FBGPMAP(np.stack([pending[k][1] for k in ks], axis=1), np.array([pending[k][2] for k in ks]), pending[ks[0]][3], device=device)
                for j, k in enumerate(ks):
                    nxt[k] = gens[k].send((A[:, j], {q: P[q][j] for q in ('varc', 'varx', 'mux')}, Info[j]))
                continue
            _, T, Tx, M = key
            st = lambda q: np.stack([np.asarray(pending[k][2][q], float) for k in ks])
            h = GppadCasHandle(np.stack([pending[k][1] for k in ks]), M, Tx, st('varx'), st('mux'), st('varc'), len=st('len'), device=device)
            try:
                done, left = lock_step_rows(h.eval, [gens[k] for k in ks], M * Tx, lambda r: r[1] if r[0] == 'x' else None)
            finally:
                h.close()
            for j, k in enumerate(ks):
                out[k] = done[j]
        pending = nxt
    return out


def FBCasGPMAP(Y, Len, Opts=None, fine_tuned=False, evaluator=None, device=0):
    """[A,X,C,Params,Info] = FBCasGPMAP(Y,Len,Opts) (FBCasGPMAP.m): CasGPMAP down the columns of Y (T x D).  Len: the M time-scales, (M,) or
    (M x 1) for every column, or (M x D).  Returns A and X (T, D, M) squeezed as the .m does ((T, M) for D = 1), C (T x D), Params with len
    (M x D), varc (D), varx and mux (M x D), and the list of the channels' Info (the .m keeps the last one).  On the device the channels
    run in lock-step (channels whose (T, Tx, M) agree share their handles), bit-equal to one channel at a time; with an `evaluator`
    channel by channel.  fine_tuned: as CasGPMAP."""
    Y = np.asarray(Y, float)
    if Y.ndim == 1:
        Y = Y[:, None]
    T, D = Y.shape
    Len = np.asarray(Len, float)
    if Len.ndim < 2:
        Len = Len.reshape(-1, 1)
    if Len.shape[1] == 1:                                                                            # :11-13
        Len = Len @ np.ones((1, D))
    if Len.shape[1] != D:
        raise ValueError('Len is (M x 1) or (M x D) with D = %d columns of Y: got %s' % (D, Len.shape))
    M = Len.shape[0]
    if evaluator is None:
        res = _cas_many([Y[:, d] for d in range(D)], [Len[:, d] for d in range(D)], Opts, fine_tuned, device)
    else:
        res = [CasGPMAP(Y[:, d], Len[:, d], Opts, fine_tuned=fine_tuned, evaluator=evaluator) for d in range(D)]
    A = np.stack([r[0] for r in res], axis=1); X = np.stack([r[1] for r in res], axis=1)             # (T, D, M)
    C = np.stack([r[2] for r in res], axis=1)
    Params = {'len': Len, 'varc': np.array([r[3]['varc'] for r in res]), 'varx': np.stack([r[3]['varx'] for r in res], axis=1),
              'mux': np.stack([r[3]['mux'] for r in res], axis=1)}
    sq = lambda Z: Z[:, 0, :] if D == 1 else (Z[:, :, 0] if M == 1 else Z)                           # squeeze (:41-42)
    return sq(A), sq(X), C, Params, [r[4] for r in res]
