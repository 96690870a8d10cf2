"""NumPy float64 restatement of unifying_prob_tf/kernel_ss_kalmanSlowFB_rewrite.m (the exact filterbank filter / RTS smoother with an
observation variance per step), statement by statement with sequential loops and the Cholesky-based gain of :114-124, plus the
library's NaN guard (a NaN y_k skips the update and the lik term).  It is the yardstick of the GPU tests of nagp_slowfb_run; its own
distance to the multi-precision fixture (tests/golden/slowfb_multiprecision.npz, tools/make_slowfb_fixture.py) is pinned in
tests/test_slowfb_host.py.  The jitter retry of :117-121 must never trigger here: it is asserted."""
import numpy as np


def model(kernel, D):
    """The test models: get_disc_model with fixed, spread hyper-parameters.  Returns A, Q, H (S), P0 = Pinf, tau1."""
    from nagp import get_disc_model
    d = np.arange(D)
    lamx = 0.05 + 0.25 * (d + 1.0) / D
    varx = 0.5 + 1.0 * ((d * 7) % 5) / 4.0
    omega = 0.15 + 2.6 * (d + 0.5) / D
    A, Q, H, Pinf, K, tau1 = get_disc_model(lamx, varx, omega, D, kernel)
    return np.asarray(A), np.asarray(Q), np.asarray(H).ravel(), np.asarray(Pinf), tau1


def sample_y(A, Q, H, P0, T, seed, noise=1e-2):
    """A series drawn from the model"""
    rng = np.random.default_rng(seed)
    S = A.shape[0]
    w, V = np.linalg.eigh((P0 + P0.T) / 2); Lp = V * np.sqrt(np.clip(w, 0, None))
    w, V = np.linalg.eigh((Q + Q.T) / 2); Lq = V * np.sqrt(np.clip(w, 0, None))
    x = Lp @ rng.standard_normal(S); y = np.zeros(T)
    for k in range(T):
        if k:
            x = A @ x + Lq @ rng.standard_normal(S)
        y[k] = H @ x + noise * rng.standard_normal()
    return y


def gap_pattern(y, g0, g1, n0, n1):
    """The missing-data pattern of the fixture: vary = 1e-4, 1e5 and y = 0 on [g0, g1), NaN on [n0, n1) and at T-2."""
    T = y.size; y = y.copy(); vary = np.full(T, 1e-4)
    vary[g0:g1] = 1e5; y[g0:g1] = 0.0
    y[n0:n1] = np.nan; y[T - 2] = np.nan
    return y, vary


def case(name):
    """Inputs of the two fixture cases (the fixture stores them; this is how tools/make_slowfb_fixture.py builds them)."""
    if name == 'm32':
        A, Q, H, P0, tau = model('matern32', 2); T = 120
        y, vary = gap_pattern(sample_y(A, Q, H, P0, T, 11), 20, 40, 45, 50)
        steps = [0, 19, 20, 30, 39, 40, 47, T - 2, T - 1]
    elif name == 'm52':
        A, Q, H, P0, tau = model('matern52', 3); T = 60
        y, vary = gap_pattern(sample_y(A, Q, H, P0, T, 12), 10, 20, 22, 25)
        steps = [0, 9, 10, 15, 19, 20, 23, T - 2, T - 1]
    else:
        raise ValueError(name)
    return dict(A=A, Q=Q, H=H, P0=P0, y=y, vary=vary, steps=np.array(steps), block=2 * tau, tau=tau)


def slowfb(A, Q, H, P0, y, vary, KF=0):
    """[lik, MS (S x T), PS (S x S x T)] of kernel_ss_kalmanSlowFB_rewrite.m; NaN in y = missing."""
    A = np.asarray(A, float); Q = np.asarray(Q, float); H = np.asarray(H, float).reshape(1, -1)
    y = np.asarray(y, float).ravel(); T = y.size
    vary = np.full(T, float(np.ravel(vary)[0])) if np.size(vary) == 1 else np.asarray(vary, float).ravel()
    S = A.shape[0]
    m = np.zeros((S, 1)); P = np.array(P0, float)
    MS = np.zeros((S, T)); PS = np.zeros((S, S, T)); lik = 0.0
    for k in range(T):                                             # :55-84
        R = vary[k]
        if k > 0:
            m = A @ m
            P = A @ P @ A.T + Q
        if not np.isnan(y[k]):
            Sk = (H @ P @ H.T)[0, 0] + R
            K = P @ H.T / Sk
            v = y[k] - (H @ m)[0, 0]
            m = m + K * v
            P = P - K @ H @ P
            lik = lik + .5 * np.log(2 * np.pi) + .5 * np.log(Sk) + .5 * v / Sk * v
        MS[:, k] = m[:, 0]; PS[:, :, k] = P
    if KF != 1:
        for k in range(T - 2, -1, -1):                             # :100-134
            PSk = PS[:, :, k]
            PSkp = A @ PSk @ A.T + Q
            try:
                Lc = np.linalg.cholesky(PSkp)
            except np.linalg.LinAlgError:
                raise AssertionError('the jitter retry of kernel_ss_kalmanSlowFB_rewrite.m:117-121 would be needed at step %d' % k)
            G = np.linalg.solve(Lc.T, np.linalg.solve(Lc, (PSk @ A.T).T)).T      # PSk*A'/L'/L
            m = MS[:, k:k + 1] + G @ (m - A @ MS[:, k:k + 1])
            P = PSk + G @ (P - PSkp) @ G.T
            MS[:, k] = m[:, 0]; PS[:, :, k] = P
    return -lik, MS, PS


def dist(a, ref):
    """the project's norm: max|a - ref| / max|ref|"""
    ref = np.asarray(ref, float)
    return float(np.max(np.abs(np.asarray(a, float) - ref)) / np.max(np.abs(ref)))
