"""Host-side mirror of the chain that takes the reference's real-audio drivers from audio to W (demo_nonstationary_filterbank.m:93-97,
experiments/train_GTFNMF.m:64-89):

    [Z,covZ,Zfull,covZfull] = kernel_ss_probFB(y,A,Q,C,P0,K,vary,tau,verbose,KF,slow)      unifying_prob_tf/kernel_ss_probFB.m
    [S,covS,Sfull,covSfull] = getFBLDSOutput_tau(Xfin,Pfin,tau)                            unifying_prob_tf/getFBLDSOutput_tau.m
    [H,info]   = nmf_inf_fp(A,W,H,vary,opts)                                               experiments/nmf/nmf_inf_fp.m
    [W,H,info] = nmf_fp(A,W,H,vary,opts)                                                   experiments/nmf/nmf_fp.m

Everything O(T) of the factorisation runs on the GPU (nagp_nmf_fp, include/nagp.h); the host marshals arguments, normalises W where
the .m does, draws the restart candidates and picks among them.  The filterbank wrappers select and pair rows of what
kernel_ss_kalmanFastFB / kernel_ss_kalmanSlowFB return.  There is no CPU fallback.
"""
import numpy as np

from . import _lib as L
from ._drive import opt as _opt
from .fastfb import kernel_ss_kalmanFastFB
from .slowfb import kernel_ss_kalmanSlowFB


def nmf_run(A, vary, W0, H0, n_its, update_w=True, device=0):
    """nagp_nmf_fp with NumPy arrays.  A (T, D); vary (T, D), a scalar or None (= zeros); W0 (K, D) or (P, K, D); H0 (T, K) or
    (P, T, K).  W0 is used as given (not normalised).  Returns W, H, Obj with the leading problem axis of the inputs
    (Obj: (P, (2 if update_w else 1) * n_its))."""
    A = L.f64(A); T, D = A.shape
    W0 = np.asarray(W0, float); H0 = np.asarray(H0, float)
    single = W0.ndim == 2
    if single:
        W0 = W0[None]; H0 = H0[None] if H0.ndim == 2 else H0
    P, K = W0.shape[0], W0.shape[1]
    if W0.shape != (P, K, D) or H0.shape != (P, T, K):
        raise ValueError('W0 must be (P, K, D) and H0 (P, T, K) with A (T, D): got %s, %s, %s' % (W0.shape, H0.shape, A.shape))
    if vary is not None:
        vary = np.asarray(vary, float)
        vary = L.f64(np.broadcast_to(vary, (T, D)) if vary.size == 1 else vary.reshape(T, D))
    w0 = L.f64(W0.transpose(0, 2, 1), 'C')                      # problem-major blocks of K x D column-major
    h0 = L.f64(H0.transpose(0, 2, 1), 'C')                      # ... of T x K column-major
    n_its = int(n_its); n_obj = (2 if update_w else 1) * n_its
    W = np.zeros_like(w0); H = np.zeros_like(h0); Obj = np.zeros((P, n_obj))
    L.check(L.lib().nagp_nmf_fp(P, T, D, K, L.dptr(A), L.dptr(vary), L.dptr(w0), L.dptr(h0), n_its, 1 if update_w else 0,
                                L.dptr(W), L.dptr(H), L.dptr(Obj) if n_obj else L.c_dp(), int(device)))
    W = W.transpose(0, 2, 1); H = H.transpose(0, 2, 1)
    return (W[0], H[0], Obj[0]) if single else (W, H, Obj)


def _row_normalise(W):
    """diag(1 ./ sum(W,2)) * W"""
    W = np.asarray(W, float)
    return (1.0 / W.sum(axis=-1))[..., None] * W


def inf_normalise(W):
    """nmf_inf_fp.m:37-40, literally: `if sum(W,2)~=ones(K,1)` holds only when EVERY row sum differs from 1; a W with one row sum
    exactly 1 is left as it is."""
    W = np.asarray(W, float)
    return _row_normalise(W) if np.all(W.sum(axis=1) != 1) else W


def pick_restart(last):
    """nmf_fp.m:48-52: the candidate with the smallest last objective, strict <, so the earliest wins a tie"""
    best, ObjBest = 0, np.inf
    for r, o in enumerate(last):
        if o < ObjBest:
            best, ObjBest = r, o
    return best


def nmf_inf_fp(A, W, H, vary, opts=None, device=0):
    """[H,info] = nmf_inf_fp(A,W,H,vary,opts) (nmf_inf_fp.m:1): opts['numIts'] iterations (default 100) of the H update with W fixed.
    The condition of :37 is kept literally: MATLAB's `if` on a vector is true only when every element is, so W is normalised only
    when EVERY row sum differs from 1.  W (K, D), H (T, K); with a leading problem axis on both, a batch (each W under :37 by itself).
    info['Obj']: one objective per iteration."""
    W = np.asarray(W, float); single = W.ndim == 2
    Wb = np.stack([inf_normalise(w) for w in (W[None] if single else W)])
    Hb = np.asarray(H, float)
    _, Hn, Obj = nmf_run(A, vary, Wb, Hb[None] if single else Hb, _opt(opts, 'numIts', 100), update_w=False, device=device)
    return [Hn[0], {'Obj': Obj[0]}] if single else [Hn, {'Obj': Obj}]


def restart_candidates(A, K, R, seed=None):
    """Candidates 2..R of nmf_fp.m:53-55: ks = ceil(T*rand(K,1)), W = A(ks,:), H = exp(randn(T,K)), drawn per candidate in the
    reference's order (ks, then H) from numpy.random.default_rng(seed) -- NumPy's stream, not MATLAB's."""
    A = np.asarray(A, float); T = A.shape[0]
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(R - 1):
        ks = np.ceil(T * rng.random(K)).astype(int)
        out.append((A[np.maximum(ks, 1) - 1, :], np.exp(rng.standard_normal((T, K)))))
    return out


def nmf_fp(A, W, H, vary, opts=None, inits=None, seed=None, device=0):
    """[W,H,info] = nmf_fp(A,W,H,vary,opts) (nmf_fp.m:1): opts['numIts'] iterations (default 1000) of the H and W updates;
    info['Obj'] has 2*numIts entries.  With opts['restarts'] = R (:34-57) candidate 1 is the caller's (W, H) and candidates 2..R are
    W = A[ks, :], H = exp(randn(T, K)), drawn from numpy.random.default_rng(seed) in the reference's order (ks, then H) for each
    candidate -- this is NumPy's stream, not MATLAB's (matlab/nmf_fp.m draws with MATLAB's own rand / randn) -- or taken from `inits`,
    a list of R - 1 pairs (W, H).  Every candidate's W is row-normalised (:45), all R candidates run their 10 iterations of
    nmf_inf_fp as ONE batched call, and the smallest last Obj wins with strict <, so the earliest wins a tie (:48-52).
    info['restart'] is the winner's 0-based index, info['restartObj'] the candidates' last objectives."""
    A = np.asarray(A, float); W = np.asarray(W, float); H = np.asarray(H, float)
    K = W.shape[0]
    info = {}
    R = _opt(opts, 'restarts', None)
    if R is not None:
        R = int(R)
        cands = [(W, H)] + list(inits if inits is not None else restart_candidates(A, K, R, seed))
        if len(cands) != R:
            raise ValueError('inits must hold restarts - 1 = %d pairs (W, H)' % (R - 1))
        Wc = np.stack([_row_normalise(c[0]) for c in cands])                                  # :45
        Hc, inf = nmf_inf_fp(A, Wc, np.stack([np.asarray(c[1], float) for c in cands]), vary, {'numIts': 10}, device=device)   # :46
        last = inf['Obj'][:, -1]
        best = pick_restart(last)                                                             # :48-52
        # (nmf_inf_fp may have normalised the candidate's W once more under :37; :49 keeps Wtest as :45 left it)
        W, H = Wc[best], Hc[best]
        info['restart'] = best; info['restartObj'] = last
    W = _row_normalise(W)                                                                      # :63
    W, H, Obj = nmf_run(A, vary, W, H, _opt(opts, 'numIts', 1000), update_w=True, device=device)
    info['Obj'] = Obj
    return [W, H, info]


def _quad(P, a, b):
    """[P(a,a,:), P(a,b,:); P(b,a,:), P(b,b,:)]"""
    return np.concatenate([np.concatenate([P[np.ix_(a, a)], P[np.ix_(a, b)]], axis=1),
                           np.concatenate([P[np.ix_(b, a)], P[np.ix_(b, b)]], axis=1)], axis=0)


def getFBLDSOutput_tau(Xfin, Pfin, tau, nout=1):
    """[S,covS,Sfull,covSfull] = getFBLDSOutput_tau(Xfin,Pfin,tau) (getFBLDSOutput_tau.m:1); nout stands for nargout.
    Xfin 1 x 2Dtau x T, Pfin 2Dtau x 2Dtau x T (not read when nout = 1).  S: D x T complex (the first-order term of every
    sub-band), covS: 2D x 2D x T ([Re; Im] ordering), Sfull: tau D x T, covSfull: 2 tau D x 2 tau D x T.  Returns a list of nout items."""
    Xfin = np.asarray(Xfin); n2 = Xfin.shape[1]; tau = int(tau)
    X = Xfin[0]
    re, im = np.arange(0, n2 - 1, 2 * tau), np.arange(1, n2, 2 * tau)               # indRe = 1:2*tau:TwoDtau-1, indIm = 2:2*tau:TwoDtau
    if nout <= 2:
        out = [X[re] + 1j * X[im]]
        if nout == 2:
            out.append(_quad(np.asarray(Pfin), re, im))
        return out
    fre, fim = np.arange(0, n2 - 1, 2), np.arange(1, n2, 2)
    Sfull = X[fre] + 1j * X[fim]
    out = [Sfull[::tau], _quad(np.asarray(Pfin), re, im), Sfull]
    if nout > 3:
        out.append(_quad(np.asarray(Pfin), fre, fim))
    return out


def covS_rows(S, tau):
    """the rows of the state that covS needs, ascending: [0, 2 tau, ...] and their odd partners"""
    return np.sort(np.concatenate([np.arange(0, S - 1, 2 * tau), np.arange(1, S, 2 * tau)]))


def kernel_ss_probFB(y, A, Q, C_, P0, K, vary, tau, verbose=0, KF=0, slow=0, nout=1, device=0):
    """[Z,covZ,Zfull,covZfull] = kernel_ss_probFB(y,A,Q,C,P0,K,vary,tau,verbose,KF,slow) (kernel_ss_probFB.m:1); nout stands for
    nargout and a list of nout items is returned.  slow = 0: the steady-state filterbank (kernel_ss_kalmanFastFB), slow = 1: the exact
    smoother (kernel_ss_kalmanSlowFB).  With slow = 1 covZ asks the exact smoother only for the rows it needs (cov='sub'); covZfull
    goes through cov='full' and its memory guard; without a covariance output none is computed."""
    S = np.asarray(A).shape[0]; tau = int(tau)
    if slow == 1:
        if nout in (2, 3):
            rows = covS_rows(S, tau)
            _, Xfin, Psub = kernel_ss_kalmanSlowFB(A, Q, C_, P0, K, vary, y, verbose, KF, cov='sub', sub_idx=rows, device=device)
            re, im = np.searchsorted(rows, np.arange(0, S - 1, 2 * tau)), np.searchsorted(rows, np.arange(1, S, 2 * tau))
            covS = _quad(Psub, re, im)
            if nout == 2:
                return [getFBLDSOutput_tau(Xfin, None, tau, 1)[0], covS]
            Sfull = Xfin[0][0::2] + 1j * Xfin[0][1::2]
            return [Sfull[::tau], covS, Sfull]
        _, Xfin, Pfin = kernel_ss_kalmanSlowFB(A, Q, C_, P0, K, vary, y, verbose, KF, cov=('full' if nout > 3 else None), device=device)
    else:
        lik, Xfin, Pfin = kernel_ss_kalmanFastFB(A, Q, C_, P0, K, vary, y, verbose, KF, device=device)
    return getFBLDSOutput_tau(Xfin, Pfin, tau, nout)


def nmf_init(Z, N, restarts=20, numIts=500, seed=0, device=0, mods=None):
    """The W of experiments/train_GTFNMF.m:64-89 from the sub-bands Z (D x T complex): A = abs(Z).T, W0 = A[ks, :], H0 = exp(randn)
    (NumPy's stream from `seed`: H0, then ks as in :76-77, then the restart candidates), nmf_fp with `restarts` and `numIts`, and the components
    ordered by fastness = mean(diff(H)**2) / var(H), descending (:85-89).  mods (T x D): the demodulated envelopes of GPPAD(real(Z)', fs/10),
    which the drivers factorise in place of abs(Z)' (:73, :78-83); Z then only gives the shape.  Returns WEst (N x D), HEst (T x N), info."""
    A = np.abs(np.asarray(Z)).T; T = A.shape[0]; N = int(N)
    if mods is not None:
        mods = np.asarray(mods, float)
        if mods.shape != A.shape or not np.all(np.isfinite(mods)) or np.any(mods < 0):
            raise ValueError('mods must be T x D = %s, finite and >= 0: got %s' % (A.shape, mods.shape))
        A = mods
    rng = np.random.default_rng(seed)
    H0 = np.exp(rng.standard_normal((T, N)))                                                 # :76
    ks = np.ceil(T * rng.random(N)).astype(int)                                              # :77
    W0 = A[np.maximum(ks, 1) - 1, :]
    W, H, info = nmf_fp(A, W0, H0, None, {'restarts': restarts, 'numIts': numIts}, seed=rng.integers(0, 2 ** 63), device=device)
    fastness = np.mean(np.diff(H, axis=0) ** 2, axis=0) / np.var(H, axis=0, ddof=1)
    order = np.argsort(-fastness, kind='stable')
    info['fastness'] = fastness[order]; info['order'] = order
    return W[order], H[:, order], info
