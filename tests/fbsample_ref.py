"""TEST INFRASTRUCTURE ONLY -- plain NumPy restatement of a joint posterior draw of the stationary filterbank
(nagp_fastfb_sample, include/nagp.h): the simulation smoother, statement by statement, with sequential loops, the variates of
oracle.recon.normals and the steady-state filter / smoother of oracle.fastfb for S_y.

    z[t][j] = normals(T, j, n_draws, seed)[t, i]   j = 0..S-1         e[t] = normals(T, S, n_draws, seed)[t, i]
    x*_0 = Lp z[0];   x*_t = A x*_{t-1} + Lq z[t]
    y*_t = H x*_t + sqrt(R) e[t] where y_t is observed, NaN where y_t is NaN
    X_i = x* + S_y(y - y*);   Ydraw_i[t] = H X_i[:, t]
"""
import numpy as np

from oracle import fastfb as offb, recon as orec


def matern32_model(D, seed, ls_range=(20.0, 400.0), kernel='matern32'):
    """A filterbank of D sub-bands as tests/test_gpu_parity.py builds it; returns A, Q, H (1 x S), Pinf."""
    rng = np.random.default_rng(seed)
    lam = 1.0 / rng.uniform(ls_range[0], ls_range[1], D); var = rng.uniform(0.1, 1.0, D); om = np.linspace(np.pi / 3, np.pi / 50, D)
    A, Q, H, Pinf, _, _ = offb.get_disc_model(lam, var, om, D, kernel, 6)
    return A, Q, H, Pinf


def factors(Q, Pinf):
    S = Q.shape[0]
    return np.linalg.cholesky(Q + 1e-14 * np.eye(S)), np.linalg.cholesky(Pinf)


def simulate_y(A, Lq, Lp, H, R, T, seed):
    rng = np.random.default_rng(seed); S = A.shape[0]
    x = Lp @ rng.normal(size=S); y = np.zeros(T)
    for k in range(T):
        x = A @ x + Lq @ rng.normal(size=S); y[k] = (H @ x)[0] + np.sqrt(R) * rng.normal()
    return y


def smooth(st, A, y):
    """S_y(y): the two loops of oracle.fastfb.kernel_ss_kalmanFastFB (filter from m = 0, smoother with G, NaN = missing) on its set-up
    `st` = oracle.fastfb.steady_state(...).  y is (T,) -> (S, T), or (T, n) with one NaN pattern -> (n, S, T): the loops over time
    stay sequential, the n sequences go through them side by side (tests/test_fbsample_host.py pins this to the oracle's function)."""
    y = np.asarray(y, float); one = y.ndim == 1
    Y = y[:, None] if one else y
    T, n = Y.shape; S = A.shape[0]
    m = np.zeros((S, n)); MS = np.zeros((T, S, n))
    for k in range(T):
        if not np.isnan(Y[k, 0]):
            m = st['AKHA'] @ m + st['K'][:, None] * Y[k][None, :]
        else:
            m = A @ m
        MS[k] = m
    for k in range(T - 2, -1, -1):
        m = MS[k] + st['G'] @ (m - A @ MS[k])
        MS[k] = m
    return MS[:, :, 0].T.copy() if one else MS.transpose(2, 1, 0).copy()


def prior_draws(A, Lq, Lp, T, n_draws, seed, which=None):
    """x* of the draws `which` (default all) of an n_draws call: (len(which), S, T)."""
    S = A.shape[0]
    which = np.arange(n_draws) if which is None else np.asarray(which)
    z = np.stack([orec.normals(T, j, n_draws, seed)[:, which] for j in range(S)])      # (S, T, n)
    X = np.zeros((T, S, which.size))
    x = Lp @ z[:, 0, :]; X[0] = x
    for t in range(1, T):
        x = A @ x + Lq @ z[:, t, :]; X[t] = x
    return X.transpose(2, 1, 0).copy()


def sample(A, Q, H, Pinf, R, y, n_draws, seed, Lq, Lp, which=None):
    """-> Ydraw (n, T), Xdraw (n, S, T), MS = S_y(y) (S, T) for the draws `which` (default all) of an n_draws call."""
    y = np.asarray(y, float).ravel(); T = y.size
    H = np.asarray(H, float).reshape(1, -1)
    st = offb.steady_state(A, Q, H, R)
    which = np.arange(n_draws) if which is None else np.asarray(which)
    xs = prior_draws(A, Lq, Lp, T, n_draws, seed, which)                                # (n, S, T)
    e = orec.normals(T, A.shape[0], n_draws, seed)[:, which]                            # (T, n)
    ystar = np.einsum('s,nst->tn', H[0], xs) + np.sqrt(R) * e
    ystar[np.isnan(y), :] = np.nan
    X = xs + smooth(st, A, y[:, None] - ystar)
    Y = np.einsum('s,nst->nt', H[0], X)
    return Y, X, smooth(st, A, y)
