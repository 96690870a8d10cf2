"""Host-side mirror of the exact branch of the stationary filterbank (kernel_ss_probFB.m with slow = 1):

    [lik,Xfin,Pfin] = kernel_ss_kalmanSlowFB(A,Q,C,P0,K,vary,y,verbose,KF)        unifying_prob_tf/kernel_ss_kalmanSlowFB_rewrite.m

the Kalman filter and RTS smoother with a time-varying covariance and an observation variance per step.  Everything O(T) runs
on the GPU (nagp_slowfb_run, include/nagp.h); the host marshals arguments and detects the block size.  There is no CPU fallback.
"""
import numpy as np

from . import _lib as L


def detect_block(A, Q, max_block=8):
    """The smallest divisor b <= max_block of S outside whose b x b diagonal blocks both A and Q vanish; None when there is none."""
    A = np.asarray(A); Q = np.asarray(Q); S = A.shape[0]
    nz = (A != 0) | (Q != 0)
    idx = np.arange(S)
    for b in range(1, max_block + 1):
        if S % b == 0 and not np.any(nz & ((idx[:, None] // b) != (idx[None, :] // b))):
            return b
    return None


def slowfb_run(A, Q, H, P0, y, vary, filter_only=False, want_ms=True, want_diag=False, sub_idx=None, block=None, device=0):
    """nagp_slowfb_run with NumPy arrays: y, vary (n_series, T).  Returns lik (n_series), MS (n_series, S, T) or None,
    Pdiag (n_series, S, T) or None, Psub (n_series, n_sub, n_sub, T) or None."""
    A = L.f64(A); Q = L.f64(Q); P0 = L.f64(P0); S = A.shape[0]
    H = L.f64(np.asarray(H, float).ravel(), 'C')
    y = L.f64(np.atleast_2d(np.asarray(y, float)), 'C'); n, T = y.shape
    vary = L.f64(np.broadcast_to(np.asarray(vary, float), (n, T)), 'C')
    if block is None:
        block = detect_block(A, Q)
        if block is None:
            block = max(b for b in range(1, 9) if S % b == 0)     # no block structure: the library names the stray entry (NAGP_EUNSUPPORTED)
    sub = None if sub_idx is None else np.ascontiguousarray(np.asarray(sub_idx).ravel(), dtype=np.int32)
    n_sub = 0 if sub is None else sub.size
    lik = np.zeros(n)
    MS = np.zeros((n, T, S)) if want_ms else None                 # series-major blocks of S x T column-major
    Pd = np.zeros((n, T, S)) if want_diag else None
    Ps = np.zeros((n, T, n_sub, n_sub)) if n_sub else None        # blocks of n_sub x n_sub x T column-major
    st = L.lib().nagp_slowfb_run(S, int(block), L.dptr(A), L.dptr(Q), L.dptr(H), L.dptr(P0), n, L.dptr(y), L.dptr(vary), T,
                                 1 if filter_only else 0, n_sub, sub.ctypes.data_as(L.c_ip) if n_sub else L.c_ip(),
                                 L.dptr(lik), L.dptr(MS), L.dptr(Pd), L.dptr(Ps), int(device))
    L.check(st)
    tr = lambda a: None if a is None else a.transpose(0, 2, 1)
    return lik, tr(MS), tr(Pd), (None if Ps is None else Ps.transpose(0, 3, 2, 1))


def kernel_ss_kalmanSlowFB(A, Q, C_, P0, K, vary, y, verbose=0, KF=0, cov='full', sub_idx=None, device=0):
    """[lik,Xfin,Pfin] = kernel_ss_kalmanSlowFB(A,Q,C,P0,K,vary,y,verbose,KF) (kernel_ss_kalmanSlowFB_rewrite.m:1).
    vary: a scalar or a T-vector (2-D (n_series, T) with a batch); y: 1-D, or 2-D (n_series, T) for a batch of series on one model.
    NaN in y = missing (the .m has no such guard).  Xfin is 1 x S x T; Pfin by `cov`: 'full' S x S x T, 'diag' S x T (marginal
    variances), 'sub' the rows and columns sub_idx (0-based, ascending), None: no covariance.  With a batch every output gains a
    leading n_series axis.  KF = 1: the filtered moments."""
    y = np.asarray(y, float); batch = y.ndim == 2
    y2 = np.atleast_2d(y); n, T = y2.shape
    S = np.asarray(A).shape[0]
    vary = np.asarray(vary, float)
    if vary.size == 1:
        vary = np.full((n, T), float(vary.ravel()[0]))
    elif vary.size == T:
        vary = np.broadcast_to(vary.reshape(1, T), (n, T))
    elif vary.shape != (n, T):
        raise ValueError('vary must be a scalar, a T-vector or (n_series, T)')
    if cov not in ('full', 'diag', 'sub', None):
        raise ValueError("cov must be 'full', 'diag', 'sub' or None")
    sub = None
    if cov == 'full':
        if n * S * S * T * 8 > (1 << 30):
            raise MemoryError("Pfin would take %.1f GiB; pass cov='diag', cov='sub' with sub_idx, or cov=None" % (n * S * S * T * 8 / 2 ** 30))
        sub = np.arange(S)
    elif cov == 'sub':
        if sub_idx is None:
            raise ValueError("cov='sub' needs sub_idx")
        sub = np.asarray(sub_idx).ravel()
    lik, MS, Pd, Ps = slowfb_run(A, Q, C_, P0, y2, vary, filter_only=(KF == 1), want_diag=(cov == 'diag'), sub_idx=sub, device=device)
    Xfin = MS.reshape(n, 1, S, T)
    Pfin = Pd if cov == 'diag' else Ps
    if batch:
        return [lik, Xfin, Pfin]
    return [float(lik[0]), Xfin[0], None if Pfin is None else Pfin[0]]
