"""Host-side mirror of the conjugate-gradient NMF of the reference's NMF toolbox (experiments/nmf/), the alternative the training
drivers keep next to their nmf_fp call (train_model.m:123) and the only form of the factorisation with temporal priors on the activations:

    [obj,dobj] = getObj_nmf_temp(logHW,A,vary[,muinf],[varinf,lam])            experiments/nmf/getObj_nmf_temp.m
    [obj,dobj] = getObj_nmf_temp_inf(logH,A,W,vary[,muinf],[varinf,lam])       experiments/nmf/getObj_nmf_temp_inf.m
    [H,info]   = nmf_inf(A,W,H,muinf,varinf,lam,vary,Opts)                     experiments/nmf/nmf_inf.m
    [W,H,info] = nmf(A,W,H,muinf,varinf,lam,vary,Opts)                         experiments/nmf/nmf.m

The objective and its gradient run on the GPU (nagp_nmf_temp_obj and the resident nagp_nmf_temp_create / _eval / _destroy,
include/nagp.h); the Polak-Ribiere line search (minimize.minimize_steps) stays on the host.  The restarts of a driver run as one lock-step
batch on one resident handle, a generator per restart.  There is no CPU fallback: the `evaluator` argument exists so that the tests can
put the float64 restatement through the same drivers.

The priors are selected as nmf.m:119-131 does: varinf empty (None or []) -- none; muinf empty -- the truncated-Gaussian chain (varinf,
lam); none empty -- the inverse-gamma chain (muinf, varinf, lam).

The squared-exponential basis-function variant (tnmf.m, tnmf_inf.m on getObj_nmf_log_norm*.m and fitSEGP_BF.m) and the sampler
randtnmf.m live in nagp.tnmf; the names tnmf, tnmf_inf and randtnmf of THIS module still refuse and name the reference file.  Not built:
the sampler randnmf.m.
"""
import math

import numpy as np

from . import _lib as L
from ._drive import ResidentHandle, close, lock_step_rows, opt as _opt
from .minimize import minimize_steps

PRIORS = {'none': L.NMFT_NONE, 'tg': L.NMFT_TG, 'ig': L.NMFT_IG}


def _empty(v):
    return v is None or np.size(v) == 0


def prior_of(muinf, varinf, lam):
    """the dispatch of nmf.m:119-131 / nmf_inf.m:106-119 -> (name, muinf, varinf, lam) with the arrays the prior does not read as None"""
    if _empty(varinf):
        return 'none', None, None, None
    if _empty(lam):
        raise ValueError('lam is empty but varinf is not')
    if _empty(muinf):
        return 'tg', None, varinf, lam
    return 'ig', muinf, varinf, lam


def _prior_args(args, where):
    """the positional convention of the objectives: () none, (varinf, lam) TG, (muinf, varinf, lam) IG"""
    if len(args) == 0:
        return 'none', None, None, None
    if len(args) == 2:
        return 'tg', None, args[0], args[1]
    if len(args) == 3:
        return 'ig', args[0], args[1], args[2]
    raise TypeError('%s takes no prior argument, (varinf, lam) or (muinf, varinf, lam): got %d (the .m fails on varargin{2} with one)' % (where, len(args)))


def _vec(v, K, name):
    if v is None:
        return None
    a = np.asarray(v, float).reshape(-1)
    if a.size != K:
        raise ValueError('%s holds one entry per component (K = %d): got %d' % (name, K, a.size))
    return L.f64(a, 'C')


def _data(A, vary):
    A = np.asarray(A, float)
    if A.ndim != 2:
        raise ValueError('A must be T x D: got %s' % (A.shape,))
    if vary is not None:
        vary = np.asarray(vary, float)
        if vary.ndim == 0:
            vary = np.full(A.shape, float(vary))
        if vary.shape != A.shape:
            raise ValueError('vary must be a scalar, None or shaped as A %s: got %s' % (A.shape, vary.shape))
        vary = L.f64(vary, 'F')
    return L.f64(A, 'F'), vary


def _weights(W, P, D):
    """W (K, D) shared or (P, K, D) -> P blocks of K x D column-major"""
    W = np.asarray(W, float)
    if W.ndim == 2:
        W = np.broadcast_to(W, (P,) + W.shape)
    if W.ndim != 3 or W.shape[0] != P or W.shape[2] != D:
        raise ValueError('W must be (K, D) or (P, K, D) with P = %d, D = %d: got %s' % (P, D, W.shape))
    return L.f64(np.ascontiguousarray(np.transpose(W, (0, 2, 1))), 'C'), W.shape[1]


def _shaped(A, vary, W, P, prior, muinf, varinf, lam, pick_K):
    """the arguments of nagp_nmf_temp_create / nagp_nmf_temp_obj from NumPy arrays: (T, D, K, [A, vary, W, muinf, varinf, lam]).
    pick_K(T, D, k) settles K, k being the rows of a given W (None in the learning form)."""
    if prior not in PRIORS:
        raise ValueError('prior is one of %s: got %r' % (sorted(PRIORS), prior))
    A, vary = _data(A, vary)
    T, D = A.shape
    w, k = _weights(W, P, D) if W is not None else (None, None)
    K = int(pick_K(T, D, k))
    need = {'none': (), 'tg': ('varinf', 'lam'), 'ig': ('muinf', 'varinf', 'lam')}[prior]
    given = dict(muinf=muinf, varinf=varinf, lam=lam)
    for name in need:
        if _empty(given[name]):
            raise ValueError('the %s prior reads %s' % (prior, name))
    return T, D, K, [A, vary, w] + [_vec(given[name], K, name) if name in need else None for name in ('muinf', 'varinf', 'lam')]


class NmfTempHandle(ResidentHandle):
    """The resident form (nagp_nmf_temp_create): A, vary, a given W, the prior parameters and the partial-sum buffers stay on the
    device; eval(x) moves x (P, nx) in and Obj (P,), dObj (P, nx) out.  W = None: the learning form, nx = T K + K D (K is then
    required); W (K, D) or (P, K, D): the inference form, nx = T K."""
    _eval, _destroy = 'nagp_nmf_temp_eval', 'nagp_nmf_temp_destroy'

    def __init__(self, A, vary, W=None, prior='none', muinf=None, varinf=None, lam=None, K=None, n_problems=1, device=0):
        import ctypes as C

        def pick_K(T, D, k):
            if k is not None and K is not None and int(K) != k:
                raise ValueError('K = %d but W has %d rows' % (K, k))
            if k is None and K is None:
                raise ValueError('the learning form needs K')
            return K if k is None else k
        self.P = int(n_problems)
        self.T, self.D, self.K, arrays = _shaped(A, vary, W, self.P, prior, muinf, varinf, lam, pick_K)
        self.learn = W is None
        self.nx = self.T * self.K + (self.K * self.D if self.learn else 0)
        h = C.c_void_p()
        L.check(L.lib().nagp_nmf_temp_create(C.byref(h), self.P, self.T, self.D, self.K, PRIORS[prior], *map(L.dptr, arrays), int(device)))
        self._h = h


def nmf_temp_obj(x, A, vary, W=None, prior='none', muinf=None, varinf=None, lam=None, grad=True, device=0):
    """nagp_nmf_temp_obj with NumPy arrays.  A (T, D); vary (T, D), a scalar or None (= zeros).  W = None: the learning form, x
    (T K + K D,) or (P, T K + K D) = [log H(:); log W(:)] per problem, K = numel / (T + D) as the .m; W (K, D) or (P, K, D): the inference
    form, x (T K,) or (P, T K).  muinf, varinf, lam: K each, as the prior reads them.  Returns Obj and, with grad, dObj, with the leading
    problem axis of x."""
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
    T, D, K, arrays = _shaped(A, vary, W, P, prior, muinf, varinf, lam, pick_K)
    Obj = np.zeros(P); dObj = np.zeros((P, nx)) if grad else None
    L.check(L.lib().nagp_nmf_temp_obj(P, T, D, K, PRIORS[prior], L.dptr(xx), *map(L.dptr, arrays), L.dptr(Obj), L.dptr(dObj), int(device)))
    if single:
        return (Obj[0], dObj[0]) if grad else Obj[0]
    return (Obj, dObj) if grad else Obj


def getObj_nmf_temp(logHW, A, vary, *prior_args, nout=2, device=0):
    """[obj,dobj] = getObj_nmf_temp(logHW,A,vary[,muinf],[varinf,lam]) (getObj_nmf_temp.m:1) on the device; nout stands for nargout"""
    prior, muinf, varinf, lam = _prior_args(prior_args, 'getObj_nmf_temp')
    return nmf_temp_obj(np.asarray(logHW, float).reshape(-1), A, vary, None, prior, muinf, varinf, lam, grad=nout > 1, device=device)


def getObj_nmf_temp_inf(logH, A, W, vary, *prior_args, nout=2, device=0):
    """[obj,dobj] = getObj_nmf_temp_inf(logH,A,W,vary[,muinf],[varinf,lam]) (getObj_nmf_temp_inf.m:1) on the device: W is used as given"""
    prior, muinf, varinf, lam = _prior_args(prior_args, 'getObj_nmf_temp_inf')
    W = np.asarray(W, float)
    if W.ndim != 2:
        raise ValueError('W must be K x D: got %s' % (W.shape,))
    return nmf_temp_obj(np.asarray(logH, float).reshape(-1), A, vary, W, prior, muinf, varinf, lam, grad=nout > 1, device=device)


# ---------------------------------------------------------------------------------------------------------------- drivers
def _device_evaluator(device):
    """evaluator(A, vary, W, K, prior, muinf, varinf, lam, n_problems) -> f(X) -> (Obj, dObj) on a resident handle; f.close() releases it"""
    def open_batch(A, vary, W, K, prior, muinf, varinf, lam, n_problems):
        h = NmfTempHandle(A, vary, W, prior, muinf, varinf, lam, K=K, n_problems=n_problems, device=device)
        f = h.eval
        return _Closing(f, h.close)
    return open_batch


class _Closing:
    def __init__(self, f, close):
        self.f = f; self.close = close

    def __call__(self, X):
        return self.f(X)


def chunked_steps(x0, numIts, progress_chunk):
    """the loop of nmf.m:111-169 / nmf_inf.m:99-152 as a generator: ceil(numIts / progress_chunk) chunks, each a fresh minimize of
    progress_chunk line searches from the result of the one before.  It yields a point and is sent (f, df) there; its return value is
    (x, Obj, it): Obj the concatenated objective histories, it the count of every chunk."""
    Lc = int(math.ceil(numIts / progress_chunk))
    x = np.asarray(x0, float).reshape(-1)
    Obj = []; it = []
    for _ in range(Lc):
        x, fX, i = yield from minimize_steps(x, int(progress_chunk))
        Obj.append(fX); it.append(i)
    return x, (np.concatenate(Obj) if Obj else np.zeros(0)), np.array(it, int)


def _check_WH(A, W, H):
    A = np.asarray(A, float); W = np.asarray(W, float); H = np.asarray(H, float)
    if A.ndim != 2 or W.ndim != 2 or H.ndim != 2 or W.shape[1] != A.shape[1] or H.shape != (A.shape[0], W.shape[0]):
        raise ValueError('A is T x D, W is K x D and H is T x K: got %s, %s, %s' % (A.shape, W.shape, H.shape))
    return A, W, H


def nmf_inf_many(A, Ws, Hs, muinf, varinf, lam, vary, numIts=1000, progress_chunk=50, evaluator=None, device=0):
    """the optimisation loop of nmf_inf.m:97-158 for several (W, H) pairs on one data matrix, in lock-step on one resident handle.
    Returns a list of (H, info)."""
    prior, mu, vi, la = prior_of(muinf, varinf, lam)
    n = len(Hs)
    T, K = np.shape(Hs[0])
    with np.errstate(divide='ignore'):
        gens = [chunked_steps(np.log(np.asarray(H, float)).reshape(-1, order='F'), numIts, progress_chunk) for H in Hs]
    f = (evaluator or _device_evaluator(device))(A, vary, np.stack([np.asarray(W, float) for W in Ws]), K, prior, mu, vi, la, n)
    try:
        res, _ = lock_step_rows(f, gens, T * K)
    finally:
        close(f)
    return [(np.exp(x.reshape(T, K, order='F')), {'Obj': Obj, 'it': it}) for x, Obj, it in res]


def _rng_inits(inits, seed, n, make):
    if inits is not None:
        if len(inits) < n:
            raise ValueError('%d restarts need %d initialisations beside the caller\'s: got %d' % (n + 1, n, len(inits)))
        return list(inits[:n])
    rng = np.random.default_rng(seed)
    return [make(rng) for _ in range(n)]


def nmf_inf(A, W, H, muinf, varinf, lam, vary, opts=None, inits=None, seed=None, evaluator=None, device=0):
    """[H,info] = nmf_inf(A,W,H,muinf,varinf,lam,vary,Opts) (nmf_inf.m:1): inference of H by conjugate gradients with W fixed (used as
    given) and vary per sample -- the temporal-NMF baseline of the missing-data and denoising experiments.  opts: numIts (default 1000),
    progress_chunk (default 50): ceil(numIts / progress_chunk) chunks, each a fresh minimize; restarts: the loop of :76-93 -- every
    restart runs numIts = 500, the first from the caller's H, the others from exp(randn(T, K)); the one with the smallest last Obj is
    kept.  The restarts run as one lock-step batch.  MATLAB's randn stream cannot be reproduced: the candidates are `inits` (a list of
    T x K arrays) or drawn from np.random.default_rng(seed).  info: Obj, it.
    evaluator(A, vary, W, K, prior, muinf, varinf, lam, n_problems) -> f(X) -> (Obj, dObj) replaces the device (host tests)."""
    A, W, H = _check_WH(A, W, H)
    T, K = H.shape
    numIts = _opt(opts, 'numIts', 1000); chunk = _opt(opts, 'progress_chunk', 50)
    info = {}
    if opts and 'restarts' in opts:
        R = int(opts['restarts'])
        cands = [H] + _rng_inits(inits, seed, R - 1, lambda rng: np.exp(rng.standard_normal((T, K))))
        runs = nmf_inf_many(A, [W] * R, cands[:R], muinf, varinf, lam, vary, 500, 50, evaluator, device) if R > 0 else []
        best = np.inf
        for r, (Hr, inf_r) in enumerate(runs):
            if inf_r['Obj'][-1] < best:
                H = Hr; best = inf_r['Obj'][-1]; info['restart'] = r
        info['restart_Obj'] = np.array([i['Obj'][-1] for _, i in runs])
    (H, run), = nmf_inf_many(A, [W], [H], muinf, varinf, lam, vary, numIts, chunk, evaluator, device)
    info.update(run)
    return H, info


def nmf(A, W, H, muinf, varinf, lam, vary, opts=None, inits=None, seed=None, evaluator=None, device=0):
    """[W,H,info] = nmf(A,W,H,muinf,varinf,lam,vary,Opts) (nmf.m:1): NMF by conjugate gradients on [log H(:); log W(:)], W and H learned
    jointly, W normalised to unit row sums.  opts: numIts (default 1000), progress_chunk (default 1000); restarts: the initialisation of
    :78-102 -- the caller's (W, H) first, then (W = A(ks, :) with K random rows, H = exp(randn(T, K))), each refined by nmf_inf with 1000
    iterations (opts['restart_numIts'] overrides the count), all as one lock-step batch; the candidate with the smallest last Obj wins.
    nmf_inf returns only H, so the winner keeps its INITIAL W (kept).  Candidates: `inits`, a list of (W, H), or drawn from
    np.random.default_rng(seed).  Returns (W, H, info) with info Obj, it."""
    A, W, H = _check_WH(A, W, H)
    T, K = H.shape; D = A.shape[1]
    numIts = _opt(opts, 'numIts', 1000); chunk = _opt(opts, 'progress_chunk', 1000)
    prior, mu, vi, la = prior_of(muinf, varinf, lam)
    info = {}
    if opts and 'restarts' in opts:
        R = int(opts['restarts'])
        cands = [(W, H)] + _rng_inits(inits, seed, R - 1, lambda rng: (A[rng.integers(0, T, K), :], np.exp(rng.standard_normal((T, K)))))
        cands = [_check_WH(A, w, h)[1:] for w, h in cands[:R]]
        runs = nmf_inf_many(A, [c[0] for c in cands], [c[1] for c in cands], muinf, varinf, lam, vary, _opt(opts, 'restart_numIts', 1000), 50,
                            evaluator, device) if R > 0 else []
        best = np.inf
        for r, (Hr, inf_r) in enumerate(runs):
            if inf_r['Obj'][-1] < best:
                W = cands[r][0]; H = Hr; best = inf_r['Obj'][-1]; info['restart'] = r
        info['restart_Obj'] = np.array([i['Obj'][-1] for _, i in runs])
    with np.errstate(divide='ignore'):
        x0 = np.concatenate([np.log(H).reshape(-1, order='F'), np.log(W).reshape(-1, order='F')])
    f = (evaluator or _device_evaluator(device))(A, vary, None, K, prior, mu, vi, la, 1)
    try:
        ((x, Obj, it),), _ = lock_step_rows(f, [chunked_steps(x0, numIts, chunk)], T * K + K * D)
    finally:
        close(f)
    H = np.exp(x[:T * K].reshape(T, K, order='F'))
    W = np.exp(x[T * K:].reshape(K, D, order='F'))
    W = (1.0 / np.sum(W, axis=1))[:, None] * W                                                    # :138
    info.update({'Obj': Obj, 'it': it})
    return W, H, info


def tnmf(*a, **k):
    raise NotImplementedError('tnmf.m / tnmf_inf.m (squared-exponential basis functions: getObj_nmf_log_norm*.m, fitSEGP_BF.m) are not built')


tnmf_inf = tnmf


def randnmf(*a, **k):
    raise NotImplementedError('randnmf.m / randtnmf.m (the samplers of the NMF toolbox) are not built')


randtnmf = randnmf
