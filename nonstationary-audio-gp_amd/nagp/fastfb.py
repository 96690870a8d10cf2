"""Host-side mirror of the stationary filterbank path:

    [A,Q,H,Pinf,K,tau1] = get_disc_model(lamx,varx,omega,D,kernel,se_approx_order)     unifying_prob_tf/get_disc_model.m
    [lik,Xfin,Pfin]     = kernel_ss_kalmanFastFB(A,Q,C,P0,K,vary,y,verbose,KF)         unifying_prob_tf/kernel_ss_kalmanFastFB.m

The set-up (`dare`, stationary gain, smoother gain) stays on the host where the .m has it -- float64 doubling iterations stand
for the Control-System-Toolbox `dare` (_steady_state; pinned to a 60-digit solution in tests/test_fastfb_host.py) -- and the two
O(T) loops run on the GPU (nagp_fastfb_run).  There is no CPU fallback.
`kernel_ss_sampleFastFB` draws whole posterior trajectories on the same model (nagp_fastfb_sample).
"""
import ctypes as C

import numpy as np
import scipy.linalg as sla

from . import _lib as L
from . import ss as ssm


def get_disc_model(lamx, varx, omega, D, kernel, se_approx_order=6):
    """get_disc_model.m:1-72.  Sub-band d = `kernel`(varx_d, lengthscale(lamx_d)) x cosine(omega_d); the observation row H
    sums the real parts of all sub-bands.  Returns A, Q, H (1 x S), Pinf, K (= D*tau1), tau1."""
    lamx = np.asarray(lamx, float).ravel(); varx = np.asarray(varx, float).ravel(); omega = np.asarray(omega, float).ravel()
    if kernel not in ('exp', 'matern32', 'matern52'):
        raise ValueError("kernel must be 'exp', 'matern32' or 'matern52'")
    ls = {'exp': 1.0, 'matern32': np.sqrt(3.0), 'matern52': np.sqrt(5.0)}[kernel] / lamx     # :9-20
    Ab, Qb, Pb, Hb = [], [], [], []
    for d in range(D):
        F1, L1, Qc1, P1 = ssm.kernel_block(kernel, varx[d], ls[d])
        tau1 = F1.shape[0]
        F = np.kron(F1, np.eye(2)) + np.kron(np.eye(tau1), np.array([[0.0, -omega[d]], [omega[d], 0.0]]))     # :53-62
        Lm = np.kron(L1, np.eye(2)); LQL = Qc1 * (Lm @ Lm.T)
        A_d, Q_d = ssm.lti_disc_block(F, LQL, 1.0)                                                             # :69, block-wise
        H1 = np.zeros((1, tau1)); H1[0, 0] = 1.0
        Ab.append(A_d); Qb.append(Q_d); Pb.append(np.kron(P1, np.eye(2))); Hb.append(np.kron(H1, np.array([[1.0, 0.0]])))
    return sla.block_diag(*Ab), sla.block_diag(*Qb), np.hstack(Hb), sla.block_diag(*Pb), D * tau1, tau1


def _dare_doubling(A, H, Q, R, iters=60, tol=1e-15):
    """PP = dare(A', H', Q, R) by the structure-preserving doubling iteration of ihgp_tables._dare_batch, one equation:
    W = I + G H ; A+ = A W^-1 A ; G+ = G + A W^-1 G A' ; H+ = H + A' H W^-1 A  ->  H_k -> PP.  None unless it converges
    (and for R = 0, where G_0 = H' R^-1 H does not exist)."""
    if not R > 0:
        return None
    S = A.shape[0]; eye = np.eye(S)
    Ak = np.array(A.T); Gk = H.T @ H / R; Hk = (Q + Q.T) / 2
    with np.errstate(all='ignore'):
        for _ in range(iters):
            W = eye + Gk @ Hk
            WiA = np.linalg.solve(W, Ak); WiG = np.linalg.solve(W, Gk)
            Hn = Hk + Ak.T @ Hk @ WiA
            d = np.max(np.abs(Hn - Hk)) / max(np.max(np.abs(Hn)), 1e-300)
            Ak, Gk, Hk = Ak @ WiA, Gk + Ak @ WiG @ Ak.T, (Hn + Hn.T) / 2
            if d < tol:
                break
    return Hk if np.all(np.isfinite(Hk)) and d < tol else None


def _stein_doubling(G, QQ, iters=60, tol=1e-15):
    """X = G X G' + QQ (dare(G', 0, QQ)) by doubling: X <- X + G_k X G_k', G_k <- G_k^2."""
    X = QQ; Gk = G
    for _ in range(iters):
        Xn = X + Gk @ X @ Gk.T
        d = np.max(np.abs(Xn - X)) / max(np.max(np.abs(Xn)), 1e-300)
        X = (Xn + Xn.T) / 2; Gk = Gk @ Gk
        if d < tol:
            break
    return X


def _steady_state(A, Q, C_, vary, KF=0):
    """The set-up lines of kernel_ss_kalmanFastFB.m (:46-77, :127-132): DARE, stationary gain, smoother gain and covariance.
    Returns A (Fortran order), H (1 x S), R, Sinn, Kg, HA, AKHA, PF2, G and Psm (both None when KF == 1).
    The steady-state covariances of Matern-5/2 filterbanks are conditioned 1e8 and worse, so the equations of the .m are solved in
    forms that hold PF2 and Psm to 1e-12 of a 60-digit solution (tests/test_fastfb_host.py) where the QZ / Bartels-Stewart route
    is 1e-9 .. 1e-7 away: the DARE by doubling; G = PF2*A'/PP by a Cholesky solve against PP = A*PF2*A' + Q formed from the
    symmetrised PF2 (the same matrix in exact arithmetic; its rounding is then consistent with the right-hand side, which
    cond(PP) would otherwise amplify); QQ = PF2 - G*PP*G' as the equal sum (I-GA)*PF2*(I-GA)' + G*Q*G' of positive
    semi-definite terms; the Stein equation by doubling.  A DARE the doubling iteration does not serve -- vary = 0 (kernel_ss_probFB
    calls with it), or no convergence -- goes to SciPy's QZ solver, as in ihgp_tables; when that fails too the error of the .m is raised."""
    A = L.f64(A)
    H = np.asarray(C_, float).reshape(1, -1); R = float(np.ravel(vary)[0]); Q = np.asarray(Q, float)
    try:
        PP = _dare_doubling(A, H, Q, R)                                                    # :46
        if PP is None:
            PP = sla.solve_discrete_are(A.T, H.T, Q, np.array([[R]]))
        Sinn = float((H @ PP @ H.T)[0, 0]) + R
        if not Sinn > 0:
            raise ArithmeticError('innovation variance %g' % Sinn)
    except Exception as e:                                                                 # :51-53
        raise L.NagpError('Unstable DARE solution!') from e
    Kg = (PP @ H.T / Sinn).ravel()                                                         # :56
    HA = (H @ A).ravel()
    AKHA = L.f64(A - np.outer(Kg, HA))                                                     # :59
    PF2 = PP - np.outer(Kg, (H @ PP).ravel()); PF2 = (PF2 + PF2.T) / 2                     # :73
    G = None; Psm = None
    if KF != 1:
        PPc = A @ PF2 @ A.T + (Q + Q.T) / 2; PPc = (PPc + PPc.T) / 2
        try:
            G = sla.cho_solve(sla.cho_factor(PPc), A @ PF2).T                              # :127  PF2*A'/PP
        except np.linalg.LinAlgError:                                                      # PP not numerically positive definite
            G = sla.solve(PPc, A @ PF2, assume_a='sym').T
        IGA = np.eye(A.shape[0]) - G @ A
        QQ = IGA @ PF2 @ IGA.T + G @ Q @ G.T; QQ = (QQ + QQ.T) / 2                         # :130-131
        Psm = _stein_doubling(G, QQ)                                                       # :132  dare(G',0,QQ)
        G = L.f64(G)
    return A, H, R, Sinn, Kg, HA, AKHA, PF2, G, Psm


def kernel_ss_kalmanFastFB(A, Q, C_, P0, K, vary, y, verbose=0, KF=0, steady=False, device=0):
    """[lik,Xfin,Pfin] = kernel_ss_kalmanFastFB(A,Q,C,P0,K,vary,y,verbose,KF) (kernel_ss_kalmanFastFB.m:1).
    Xfin is 1 x S x T, Pfin S x S x T (every slice the steady-state covariance, the last one the filter's -- as the .m
    stores them); steady=True returns Pfin = (P_smoother or None, P_filter) instead of the T-fold copy."""
    A, H, R, Sinn, Kg, HA, AKHA, PF2, G, Psm = _steady_state(A, Q, C_, vary, KF)
    S = A.shape[0]
    y = L.f64(np.asarray(y, float).ravel(), 'C'); T = y.size
    MS = np.zeros((S, T), order='F'); sv2 = C.c_double(0.0)
    L.check(L.lib().nagp_fastfb_run(S, L.dptr(A), L.dptr(AKHA), L.dptr(L.f64(HA, 'C')), L.dptr(L.f64(Kg, 'C')), L.dptr(G),
                                    L.dptr(y), T, L.dptr(MS), C.byref(sv2), int(device)))
    n_obs = T                                                                              # :80 counts every step, observed or not
    lik = -(0.5 * np.log(2 * np.pi) * n_obs + 0.5 * np.log(Sinn) * n_obs + 0.5 * sv2.value / Sinn)
    Xfin = MS.reshape(1, S, T, order='F')
    if steady:
        return lik, Xfin, (Psm, PF2)
    if S * S * T * 8 > (1 << 30):
        raise MemoryError('Pfin would take %.1f GiB (the reference stores the same S x S matrix T times); pass steady=True'
                          % (S * S * T * 8 / 2 ** 30))
    Pfin = np.empty((S, S, T), order='F')
    Pfin[:] = (PF2 if Psm is None else Psm)[:, :, None]
    Pfin[:, :, T - 1] = PF2
    return lik, Xfin, Pfin


def _lower_factor(P):
    """F with F F' = P: the Cholesky factor, or -- when P is not numerically positive definite -- the symmetric eigen-factor with
    negative eigenvalues clipped to 0."""
    P = np.asarray(P, float); P = (P + P.T) / 2
    try:
        return np.linalg.cholesky(P)
    except np.linalg.LinAlgError:
        w, V = np.linalg.eigh(P)
        return V * np.sqrt(np.clip(w, 0.0, None))


def kernel_ss_sampleFastFB(A, Q, C_, P0, K, vary, y, n_draws, seed=0, return_states=False, Lq=None, Lp=None, device=0):
    """Joint posterior draws of the stationary filterbank (nagp_fastfb_sample, include/nagp.h): the simulation smoother on the
    steady-state filter / smoother of kernel_ss_kalmanFastFB, same arguments (P0 = Pinf; NaN in y = missing).
    Draw i:  x* ~ prior (x*_0 = Lp z_0, x*_t = A x*_{t-1} + Lq z_t),  y* = H x* + sqrt(vary) e where y is observed,
    X_i = x* + S_y(y - y*),  Ydraw_i = H X_i, with S_y(.) the smoothed means of kernel_ss_kalmanFastFB and z, e from the
    counter-based generator keyed by `seed` (draw i does not depend on n_draws).  The covariance over draws is the error covariance of
    the steady-state smoother under the model: Psm away from the ends and from gaps, larger inside gaps.
    Lq, Lp: factors with Lq Lq' = Q, Lp Lp' = P0 (default: Cholesky; eigen-factor with clipped eigenvalues when that fails).
    Returns Ydraw (n_draws, T), Xdraw (n_draws, S, T) or None, Xmean (S, T) = S_y(y)."""
    A, H, R, Sinn, Kg, HA, AKHA, PF2, G, Psm = _steady_state(A, Q, C_, vary, 0)
    S = A.shape[0]; n_draws = int(n_draws)
    y = L.f64(np.asarray(y, float).ravel(), 'C'); T = y.size
    Lq = L.f64(_lower_factor(Q) if Lq is None else Lq); Lp = L.f64(_lower_factor(P0) if Lp is None else Lp)
    if Lq.shape != (S, S) or Lp.shape != (S, S):
        raise ValueError('Lq and Lp must be S x S')
    Yd = np.zeros((max(n_draws, 0), T)); MS = np.zeros((S, T), order='F')
    Xd = np.zeros((max(n_draws, 0), T, S)) if return_states else None                      # draw-major blocks of S x T column-major
    L.check(L.lib().nagp_fastfb_sample(S, L.dptr(A), L.dptr(AKHA), L.dptr(L.f64(HA, 'C')), L.dptr(L.f64(Kg, 'C')), L.dptr(G),
                                       L.dptr(L.f64(H.ravel(), 'C')), R, L.dptr(Lp), L.dptr(Lq), L.dptr(y), T, n_draws, int(seed) & (2 ** 64 - 1),
                                       L.dptr(Yd), L.dptr(Xd), L.dptr(MS), int(device)))
    return Yd, (Xd.transpose(0, 2, 1) if return_states else None), MS
