"""Host-side mirror of the temporal NMF of the reference's NMF toolbox whose activations are exp(mux + a squared-exponential GP) in its
basis-function form (experiments/nmf/, experiments/toolsGP/):

    Y          = basis2SEGP(Z,lenx,varx,tol)                                   experiments/toolsGP/basis2SEGP.m
    [obj,dobj] = getObj_fitSE_basis_func(z,x,lenx,varx,tol)                    experiments/toolsGP/getObj_fitSE_basis_func.m
    [obj,dobj] = getObj_nmf_log_norm(xlogW,A,vary,lenx,mux,varx,tol)           experiments/nmf/getObj_nmf_log_norm.m
    [obj,dobj] = getObj_nmf_log_norm_inf(x,A,W,vary,lenx,mux,varx,tol)         experiments/nmf/getObj_nmf_log_norm_inf.m
    [z,info]   = fitSEGP_BF(y,lenx,varx,opts)                                  experiments/toolsGP/fitSEGP_BF.m
    [W,H,info] = tnmf(A,W,H,lenx,mux,varx,vary,Opts)                           experiments/nmf/tnmf.m
    [H,info]   = tnmf_inf(A,W,H,lenx,mux,varx,vary,Opts)                       experiments/nmf/tnmf_inf.m
    [A,H]      = randtnmf(W,lenx,mux,varx,T)                                   experiments/nmf/randtnmf.m

The convolution with the 2 tau + 1 taps of the basis, the objectives and their gradients run on the GPU (nagp_sebf_conv, nagp_sebf_fit_*,
nagp_tnmf_*, include/nagp.h); the Polak-Ribiere line search (minimize.minimize_steps) stays on the host.  The searches of a driver run as
one lock-step batch on one resident handle, a generator per search.  There is no CPU fallback: the `evaluator` argument exists so that
the tests can put the float64 restatement through the same drivers.  lenx and varx are what nagp.trainSEGP_RS returns.

Kept from the reference as written:
  * fitSEGP_BF.m:41-45 reads opts.tol only when opts has the field progress_chunk, and then requires it; otherwise tol = 9.
  * every driver runs ceil(numIts / progress_chunk) chunks, each a FRESH minimize of progress_chunk line searches (:52-53, tnmf.m:74-75),
    so ceil(numIts / progress_chunk) * progress_chunk line searches at the most.
  * tnmf / tnmf_inf convert H with the DEFAULTS of fitSEGP_BF (100 line searches in chunks of 50, tol = 9) whatever their own opts say,
    and optimise with their own tol (default 11).
  * tnmf normalises W to unit row sums when it pulls it out (tnmf.m:107-108); tnmf_inf uses W as given and never normalises it.
  * H is T x K (the help texts say K x T).
  * z = randn(T,1)/1000 (fitSEGP_BF.m:50) cannot be reproduced: the start is `init` or drawn from np.random.default_rng(seed).
  * randtnmf: tol = 20, X = randn(T,K) -- here from np.random.default_rng(seed) -- and the convolution on the device.
An empty vary ([] or None) stands for zeros.
"""
import numpy as np

from . import _lib as L
from ._drive import ResidentHandle, close, lock_step_rows, opt as _opt
from .nmf_temp import _data, _weights, _check_WH, chunked_steps


def _empty(v):
    return v is None or np.size(v) == 0


def tau_of(lenx, tol):
    """tau = ceil(lenx / sqrt(2) * tol) (basis2SEGP.m:21), per entry of lenx"""
    return np.ceil(np.asarray(lenx, float) / np.sqrt(2) * tol).astype(np.int64)


def _per(v, n, name):
    a = np.asarray(v, float).reshape(-1)
    if a.size == 1 and n > 1:
        a = np.full(n, a[0])
    if a.size != n:
        raise ValueError('%s holds one entry per column (%d): got %d' % (name, n, a.size))
    return L.f64(a, 'C')


def _cols(Z, name):
    """(T,) or (T, n) -> (n, T) C-contiguous (column-major T x n), and whether it was a vector"""
    Z = np.asarray(Z, float)
    if Z.ndim not in (1, 2):
        raise ValueError('%s must be (T,) or (T, n): got %s' % (name, Z.shape))
    return L.f64(np.atleast_2d(Z.T), 'C'), Z.ndim == 1


def basis2SEGP(Z, lenx, varx, tol, device=0):
    """Y = basis2SEGP(Z,lenx,varx,tol) (basis2SEGP.m:1): the basis-function coefficients Z (T, K) to the GP, column k with lenx[k], varx[k]"""
    zz, vec = _cols(Z, 'Z')
    n, T = zz.shape
    Y = np.zeros((n, T))
    L.check(L.lib().nagp_sebf_conv(n, T, L.dptr(zz), L.dptr(_per(lenx, n, 'lenx')), L.dptr(_per(varx, n, 'varx')), float(tol), L.dptr(Y), int(device)))
    return Y[0] if vec else np.ascontiguousarray(Y.T)


# ---------------------------------------------------------------------------------------------------------------- the fit
class SebfFitHandle(ResidentHandle):
    """The resident form of getObj_fitSE_basis_func (nagp_sebf_fit_create): the targets x (P, T), the taps of every problem's own lenx,
    varx and the intermediates stay on the device; eval(z) moves z (P, T) in and Obj (P,), dObj (P, T) out."""
    _eval, _destroy = 'nagp_sebf_fit_eval', 'nagp_sebf_fit_destroy'

    def __init__(self, x, lenx, varx, tol, device=0):
        import ctypes as C
        xx = L.f64(np.atleast_2d(np.asarray(x, float)), 'C')
        if xx.ndim != 2:
            raise ValueError('x must be (T,) or (P, T): got %s' % (np.shape(x),))
        self.P, self.T = xx.shape
        self.nx = self.T
        h = C.c_void_p()
        L.check(L.lib().nagp_sebf_fit_create(C.byref(h), self.P, self.T, L.dptr(xx), L.dptr(_per(lenx, self.P, 'lenx')), L.dptr(_per(varx, self.P, 'varx')),
                                             float(tol), int(device)))
        self._h = h


def sebf_fit_obj(z, x, lenx, varx, tol, grad=True, device=0):
    """nagp_sebf_fit_obj with NumPy arrays: z and the targets x (T,) or (P, T), lenx and varx per problem.  Returns Obj and, with grad, dObj"""
    z = np.asarray(z, float); single = z.ndim <= 1
    zz = L.f64(np.atleast_2d(z), 'C'); xx = L.f64(np.atleast_2d(np.asarray(x, float)), 'C')
    if zz.ndim != 2 or xx.shape != zz.shape:
        raise ValueError('z and x must both be (T,) or (P, T): got %s and %s' % (z.shape, np.shape(x)))
    P, T = zz.shape
    Obj = np.zeros(P); dObj = np.zeros((P, T)) if grad else None
    L.check(L.lib().nagp_sebf_fit_obj(P, T, L.dptr(zz), L.dptr(xx), L.dptr(_per(lenx, P, 'lenx')), L.dptr(_per(varx, P, 'varx')), float(tol), L.dptr(Obj),
                                      L.dptr(dObj), int(device)))
    if single:
        return (Obj[0], dObj[0]) if grad else Obj[0]
    return (Obj, dObj) if grad else Obj


def getObj_fitSE_basis_func(z, x, lenx, varx, tol, nout=2, device=0):
    """[obj,dobj] = getObj_fitSE_basis_func(z,x,lenx,varx,tol) (getObj_fitSE_basis_func.m:1) on the device; nout stands for nargout"""
    return sebf_fit_obj(np.asarray(z, float).reshape(-1), np.asarray(x, float).reshape(-1), lenx, varx, tol, grad=nout > 1, device=device)


# ---------------------------------------------------------------------------------------------------------------- the NMF objectives
def _shaped(A, vary, W, P, lenx, mux, varx, pick_K):
    """the arguments of nagp_tnmf_create / nagp_tnmf_obj from NumPy arrays: (T, D, K, [A, vary, W, lenx, mux, varx])"""
    A, vary = _data(A, None if _empty(vary) else vary)
    T, D = A.shape
    w, k = _weights(W, P, D) if W is not None else (None, None)
    K = int(pick_K(T, D, k))
    par = []
    for v, name in ((lenx, 'lenx'), (mux, 'mux'), (varx, 'varx')):
        a = np.asarray(v, float).reshape(-1)
        if a.size != K:
            raise ValueError('%s holds one entry per component (K = %d): got %d' % (name, K, a.size))
        par.append(L.f64(a, 'C'))
    return T, D, K, [A, vary, w] + par


class TnmfHandle(ResidentHandle):
    """The resident form (nagp_tnmf_create): A, vary, a given W, the taps and every intermediate stay on the device; eval(x) moves x
    (P, nx) in and Obj (P,), dObj (P, nx) out.  W = None: the learning form, nx = T K + K D (K = len(lenx)); W (K, D) or (P, K, D): the
    inference form, nx = T K."""
    _eval, _destroy = 'nagp_tnmf_eval', 'nagp_tnmf_destroy'

    def __init__(self, A, vary, W, lenx, mux, varx, tol, n_problems=1, device=0):
        import ctypes as C
        Kp = np.size(lenx)

        def pick_K(T, D, k):
            if k is not None and k != Kp:
                raise ValueError('lenx holds %d entries but W has %d rows' % (Kp, k))
            return Kp
        self.P = int(n_problems)
        self.T, self.D, self.K, arrays = _shaped(A, vary, W, self.P, lenx, mux, varx, pick_K)
        self.learn = W is None
        self.nx = self.T * self.K + (self.K * self.D if self.learn else 0)
        h = C.c_void_p()
        L.check(L.lib().nagp_tnmf_create(C.byref(h), self.P, self.T, self.D, self.K, *map(L.dptr, arrays), float(tol), int(device)))
        self._h = h


def tnmf_obj(x, A, vary, W, lenx, mux, varx, tol, grad=True, device=0):
    """nagp_tnmf_obj with NumPy arrays.  A (T, D); vary (T, D), a scalar, None or [] (= zeros).  W = None: the learning form, x
    (T K + K D,) or (P, T K + K D) = [X(:); log W(:)] per problem, K = numel / (T + D) as the .m; W (K, D) or (P, K, D): the inference
    form, x (T K,) or (P, T K).  lenx, mux, varx: K each.  Returns Obj and, with grad, dObj, with the leading problem axis of x."""
    x = np.asarray(x, float); single = x.ndim <= 1
    xx = L.f64(np.atleast_2d(x), 'C')
    if xx.ndim != 2:
        raise ValueError('x must be (nx,) or (P, nx): got %s' % (x.shape,))
    P, nx = xx.shape

    def pick_K(T, D, k):
        if k is None:
            k = nx // (T + D)
            if k < 1 or k * (T + D) != nx:
                raise ValueError('x holds T K + K D entries per problem (T = %d, D = %d): got %d' % (T, D, nx))
        elif nx != T * k:
            raise ValueError('x holds T K = %d entries per problem: got %d' % (T * k, nx))
        return k
    T, D, K, arrays = _shaped(A, vary, W, P, lenx, mux, varx, pick_K)
    Obj = np.zeros(P); dObj = np.zeros((P, nx)) if grad else None
    L.check(L.lib().nagp_tnmf_obj(P, T, D, K, L.dptr(xx), *map(L.dptr, arrays), float(tol), L.dptr(Obj), L.dptr(dObj), int(device)))
    if single:
        return (Obj[0], dObj[0]) if grad else Obj[0]
    return (Obj, dObj) if grad else Obj


def getObj_nmf_log_norm(xlogW, A, vary, lenx, mux, varx, tol, nout=2, device=0):
    """[obj,dobj] = getObj_nmf_log_norm(xlogW,A,vary,lenx,mux,varx,tol) (getObj_nmf_log_norm.m:1) on the device; nout stands for nargout"""
    return tnmf_obj(np.asarray(xlogW, float).reshape(-1), A, vary, None, lenx, mux, varx, tol, grad=nout > 1, device=device)


def getObj_nmf_log_norm_inf(x, A, W, vary, lenx, mux, varx, tol, nout=2, device=0):
    """[obj,dobj] = getObj_nmf_log_norm_inf(x,A,W,vary,lenx,mux,varx,tol) (getObj_nmf_log_norm_inf.m:1) on the device: W is used as given"""
    W = np.asarray(W, float)
    if W.ndim != 2:
        raise ValueError('W must be K x D: got %s' % (W.shape,))
    return tnmf_obj(np.asarray(x, float).reshape(-1), A, vary, W, lenx, mux, varx, tol, grad=nout > 1, device=device)


# ---------------------------------------------------------------------------------------------------------------- drivers
class _Closing:
    def __init__(self, f, close):
        self.f = f; self.close = close

    def __call__(self, X):
        return self.f(X)


class DeviceEvaluator:
    """what the drivers evaluate on: fit(x, lenx, varx, tol) and tnmf(A, vary, W, lenx, mux, varx, tol, n_problems) each open a resident
    handle and return f(X) -> (Obj, dObj), f.close() releases it; basis2SEGP(Z, lenx, varx, tol) is the convolution.  tests/tnmf_ref.py
    has the same methods on the restatement."""
    def __init__(self, device=0):
        self.device = device

    def basis2SEGP(self, Z, lenx, varx, tol):
        return basis2SEGP(Z, lenx, varx, tol, device=self.device)

    def fit(self, x, lenx, varx, tol):
        h = SebfFitHandle(x, lenx, varx, tol, device=self.device)
        return _Closing(h.eval, h.close)

    def tnmf(self, A, vary, W, lenx, mux, varx, tol, n_problems):
        h = TnmfHandle(A, vary, W, lenx, mux, varx, tol, n_problems=n_problems, device=self.device)
        return _Closing(h.eval, h.close)


def fit_options(opts):
    """(numIts, progress_chunk, tol) of fitSEGP_BF.m:29-45: tol is read from opts only when opts has progress_chunk, and is then required"""
    numIts = _opt(opts, 'numIts', 100); chunk = _opt(opts, 'progress_chunk', 50)
    if opts and 'progress_chunk' in opts:
        if 'tol' not in opts:
            raise ValueError('fitSEGP_BF.m:41-42 reads opts.tol whenever opts has progress_chunk: opts has no tol')
        tol = opts['tol']
    else:
        tol = 9
    return numIts, chunk, tol


def _starts(init, seed, n, T):
    if init is not None:
        z0 = [np.asarray(z, float).reshape(-1) for z in init]
        if len(z0) != n or any(z.size != T for z in z0):
            raise ValueError('init holds one start of %d samples per signal (%d)' % (T, n))
        return z0
    rng = np.random.default_rng(seed)
    return [rng.standard_normal(T) / 1000 for _ in range(n)]                                       # fitSEGP_BF.m:50


def fitSEGP_BF_many(ys, lenx, varx, opts=None, init=None, seed=None, evaluator=None, device=0):
    """fitSEGP_BF for several signals of one length, each with its own lenx, varx, in lock-step on one resident handle.  ys: a list of
    (T,) arrays or (n, T).  init: n starts (n, T), else drawn from np.random.default_rng(seed) as randn(T) / 1000.  Returns a list of (z, info)."""
    Y = np.stack([np.asarray(y, float).reshape(-1) for y in ys])
    n, T = Y.shape
    numIts, chunk, tol = fit_options(opts)
    gens = [chunked_steps(z0, numIts, chunk) for z0 in _starts(init, seed, n, T)]
    f = (evaluator or DeviceEvaluator(device)).fit(Y, _per(lenx, n, 'lenx'), _per(varx, n, 'varx'), tol)
    try:
        res, _ = lock_step_rows(f, gens, T)
    finally:
        close(f)
    return [(z, {'Obj': Obj, 'it': it}) for z, Obj, it in res]


def fitSEGP_BF(y, lenx, varx, opts=None, init=None, seed=None, evaluator=None, device=0):
    """[z,info] = fitSEGP_BF(y,lenx,varx,opts) (fitSEGP_BF.m:1): the basis-function coefficients z whose GP basis2SEGP(z,lenx,varx,tol)
    fits the signal y, by conjugate gradients on getObj_fitSE_basis_func.  opts: numIts (default 100), progress_chunk (default 50), tol
    (see the module docstring).  info: Obj, it."""
    (z, info), = fitSEGP_BF_many([y], [float(np.asarray(lenx).reshape(-1)[0])], [float(np.asarray(varx).reshape(-1)[0])], opts,
                                 None if init is None else [init], seed, evaluator, device)
    return z, info


def _convert(H, lenx, mux, varx, init, seed, evaluator, device, convert_opts=None):
    """tnmf.m:61-72: X(:, k) = fitSEGP_BF(log(H(:, k)) - mux(k), lenx(k), varx(k)) with the defaults of fitSEGP_BF
    (convert_opts = None), the K fits as one batch"""
    T, K = H.shape
    with np.errstate(divide='ignore'):
        ys = [np.log(H[:, k]) - mux[k] for k in range(K)]
    fits = fitSEGP_BF_many(ys, lenx, varx, convert_opts, None if init is None else np.asarray(init, float).reshape(T, K, order='F').T, seed, evaluator, device)
    return np.stack([z for z, _ in fits], axis=1)


def _model(A, W, H, lenx, mux, varx):
    A, W, H = _check_WH(A, W, H)
    K = W.shape[0]
    par = [np.asarray(v, float).reshape(-1) for v in (lenx, mux, varx)]
    if any(p.size != K for p in par):
        raise ValueError('lenx, mux and varx hold one entry per component (K = %d)' % K)
    return (A, W, H) + tuple(par)


def _activations(X, lenx, mux, varx, tol, evaluator, device):
    """H(:, k) = exp(conv(X(:, k)) + mux(k)) (tnmf.m:99-106)"""
    return np.exp((evaluator or DeviceEvaluator(device)).basis2SEGP(X, lenx, varx, tol) + mux[None, :])


def tnmf_inf(A, W, H, lenx, mux, varx, vary, opts=None, init=None, seed=None, evaluator=None, device=0, convert_opts=None):
    """[H,info] = tnmf_inf(A,W,H,lenx,mux,varx,vary,Opts) (tnmf_inf.m:1): inference of the activations with W fixed and used as given.
    opts: numIts (default 100), progress_chunk (default 25), tol (default 11).  init (T, K): the starts of the K conversions, else drawn
    from np.random.default_rng(seed).  convert_opts: the opts of the K fitSEGP_BF conversions (None: its defaults, as the .m).  evaluator: an object with the methods of DeviceEvaluator and basis2SEGP (host tests).
    Returns (H (T, K), info) with info Obj, it."""
    A, W, H, lenx, mux, varx = _model(A, W, H, lenx, mux, varx)
    T, K = H.shape
    numIts = _opt(opts, 'numIts', 100); chunk = _opt(opts, 'progress_chunk', 25); tol = _opt(opts, 'tol', 11)
    X = _convert(H, lenx, mux, varx, init, seed, evaluator, device, convert_opts)
    f = (evaluator or DeviceEvaluator(device)).tnmf(A, vary, W[None], lenx, mux, varx, tol, 1)
    try:
        ((x, Obj, it),), _ = lock_step_rows(f, [chunked_steps(X.reshape(-1, order='F'), numIts, chunk)], T * K)
    finally:
        close(f)
    return _activations(x.reshape(T, K, order='F'), lenx, mux, varx, tol, evaluator, device), {'Obj': Obj, 'it': it}


def tnmf(A, W, H, lenx, mux, varx, vary, opts=None, init=None, seed=None, evaluator=None, device=0, convert_opts=None):
    """[W,H,info] = tnmf(A,W,H,lenx,mux,varx,vary,Opts) (tnmf.m:1): temporal NMF by conjugate gradients on [X(:); log W(:)], the
    activations and the spectral rows learned jointly.  opts: numIts (default 1000), progress_chunk (default 100), tol (default 11).
    init, seed, evaluator: as tnmf_inf.  Returns (W (K, D) with unit row sums, H (T, K), info) with info Obj, it."""
    A, W, H, lenx, mux, varx = _model(A, W, H, lenx, mux, varx)
    T, K = H.shape; D = A.shape[1]
    numIts = _opt(opts, 'numIts', 1000); chunk = _opt(opts, 'progress_chunk', 100); tol = _opt(opts, 'tol', 11)
    X = _convert(H, lenx, mux, varx, init, seed, evaluator, device, convert_opts)
    with np.errstate(divide='ignore'):
        x0 = np.concatenate([X.reshape(-1, order='F'), np.log(W).reshape(-1, order='F')])
    f = (evaluator or DeviceEvaluator(device)).tnmf(A, vary, None, lenx, mux, varx, tol, 1)
    try:
        ((x, Obj, it),), _ = lock_step_rows(f, [chunked_steps(x0, numIts, chunk)], T * K + K * D)
    finally:
        close(f)
    H = _activations(x[:T * K].reshape(T, K, order='F'), lenx, mux, varx, tol, evaluator, device)
    W = np.exp(x[T * K:].reshape(K, D, order='F'))
    W = (1.0 / np.sum(W, axis=1))[:, None] * W                                                    # tnmf.m:108
    return W, H, {'Obj': Obj, 'it': it}


def randtnmf(W, lenx, mux, varx, T, seed=None, device=0):
    """[A,H] = randtnmf(W,lenx,mux,varx,T) (randtnmf.m:1): a draw from the generative model, tol = 20, X = randn(T, K) from
    np.random.default_rng(seed), H = exp(conv(X) + mux) on the device, A = H W"""
    W = np.asarray(W, float)
    lenx, mux, varx = (np.asarray(v, float).reshape(-1) for v in (lenx, mux, varx))
    K = lenx.size
    X = np.random.default_rng(seed).standard_normal((int(T), K))
    H = np.exp(basis2SEGP(X, lenx, varx, 20, device=device) + mux[None, :])
    return H @ W, H
