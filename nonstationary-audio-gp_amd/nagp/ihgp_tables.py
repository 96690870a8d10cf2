"""Host-side steady-state look-up tables of the IHGP path (once per call, before the C ABI).

Replaces matlab/ihgp_ep_modulator_nmf.m:99-141 (forward DARE per channel on ro=logspace(-2,4,32),
linear interpolation to r=logspace(-2,4,200) -- apxGrid('interp') on a non-equispaced grid is
linear, SURVEY C-12) and :148-191 (steady-state smoother gain G and covariance PS2 per grid point).
MATLAB's Control-System-Toolbox `dare` is stood in for by a structure-preserving doubling iteration that solves all
(channel, grid point) Riccati equations of one block size in one batched NumPy sweep (1 216 equations at cfg3: 0.03 s
instead of 1.0 s with one scipy.linalg.solve_discrete_are call each); any equation the doubling does not converge on
falls back to SciPy's QZ solver, and a point that fails there is dropped as the reference drops it (:118-126).  One Newton
step on the residual follows.  The steady-state covariances of 6- and 8-state sub-band blocks are conditioned 1e8 .. 1e12, and
the smoother's QQ = P - G*PP*G' (:167) is down to 1e-12 of P there: QQ is formed from a sum of positive semi-definite terms
that equals it in exact arithmetic, not by that subtraction.  tests/test_dare_fixture.py holds PP, G and PS2 to a
60-digit solution of the same equations (tests/golden/dare_sixeight_states.npz).
"""
import numpy as np
import scipy.linalg as sla


def _interp_rows(ro, tab, r):
    """piece-wise linear in r between bracketing ro knots, clamped at the ends (apxGrid.m:555-565)."""
    out = np.empty((r.size, tab.shape[1]))
    for c in range(tab.shape[1]):
        out[:, c] = np.interp(r, ro, tab[:, c])
    return out


def _dare_batch(At, h, Q, rr, iters=60, tol=1e-15):
    """X = dare(A', H', Q, r) for a batch: At (B,b,b) = A', h (B,b) = H (row vector), Q (B,b,b), rr (B,).
    Doubling (SDA):  W = I + G H ; A+ = A W^-1 A ; G+ = G + A W^-1 G A' ; H+ = H + A' H W^-1 A  ->  H_k -> X."""
    B, b, _ = At.shape
    A = At.copy()                                   # the `a` argument of dare
    G = h[:, :, None] * h[:, None, :] / rr[:, None, None]
    H = Q.copy()
    eye = np.broadcast_to(np.eye(b), (B, b, b))
    ok = np.ones(B, bool)
    for _ in range(iters):
        W = eye + G @ H
        WiA = np.linalg.solve(W, A)
        WiG = np.linalg.solve(W, G)
        An = A @ WiA
        Gn = G + A @ WiG @ np.swapaxes(A, 1, 2)
        Hn = H + np.swapaxes(A, 1, 2) @ H @ WiA
        d = np.max(np.abs(Hn - H), axis=(1, 2)) / np.maximum(np.max(np.abs(Hn), axis=(1, 2)), 1e-300)
        A, G, H = An, Gn, Hn
        if np.all(d < tol):
            break
    H = (H + np.swapaxes(H, 1, 2)) / 2
    ok &= np.isfinite(H).all(axis=(1, 2)) & (d < 1e-10)
    return H, ok


def _stein_batch(F, C):
    """X = F X F' + C for a batch, as the b^2 x b^2 linear system (I - F (x) F) vec X = vec C."""
    B, b, _ = F.shape
    KK = np.einsum('qij,qkl->qikjl', F, F).reshape(B, b * b, b * b)
    return np.linalg.solve(np.broadcast_to(np.eye(b * b), (B, b * b, b * b)) - KK, C.reshape(B, b * b, 1)).reshape(B, b, b)


def _dare_residual(A, Q, h, rr, P):
    """R = A (P - P h'(h P h' + r)^-1 h P) A' + Q - P and the predictor gain L = A P h' / (h P h' + r)."""
    Ph = np.einsum('qij,qj->qi', P, h)
    S = np.einsum('qi,qi->q', h, Ph) + rr
    R = A @ (P - Ph[:, :, None] * Ph[:, None, :] / S[:, None, None]) @ np.swapaxes(A, 1, 2) + Q - P
    return R, np.einsum('qij,qj->qi', A, Ph) / S[:, None]


def _newton_dare(A, Q, h, rr, P):
    """One Newton step on the predictive DARE: E = Ac E Ac' + R(P) with Ac = A - L h, P + E kept where its residual is smaller."""
    with np.errstate(all='ignore'):
        R, Lg = _dare_residual(A, Q, h, rr, P)
        Ac = A - Lg[:, :, None] * h[:, None, :]
        fin = np.isfinite(R).all(axis=(1, 2)) & np.isfinite(Ac).all(axis=(1, 2))
        try:
            E = _stein_batch(np.where(fin[:, None, None], Ac, 0.0), np.where(fin[:, None, None], R, 0.0))
        except np.linalg.LinAlgError:
            return P
        Pn = P + (E + np.swapaxes(E, 1, 2)) / 2
        Rn, _ = _dare_residual(A, Q, h, rr, Pn)
        better = np.isfinite(Rn).all(axis=(1, 2)) & (np.abs(Rn).max(axis=(1, 2)) < np.abs(R).max(axis=(1, 2)))
    return np.where(better[:, None, None], Pn, P)


def build_knots(A, Q, offsets, h_val, n_knots=32):
    """The solved level of the tables (PPlisto of ihgp_ep_modulator_nmf.m:107-127 and its smoother counterpart): returns
    (ro, PPs, PGs, good) with PPs[n] (len(good[n]) x b^2) and PGs[n] (len(good[n]) x 2 b^2, rows [PS2(:)' G(:)']) on the knots
    ro[good[n]] of block n.  build_tables interpolates these to the look-up grid."""
    M = len(h_val)
    ro = np.logspace(-2, 4, n_knots)
    sizes = [int(offsets[n + 1]) - int(offsets[n]) for n in range(M)]
    PPs = [None] * M; PGs = [None] * M; good = [None] * M
    for b in sorted(set(sizes)):
        idx = [n for n in range(M) if sizes[n] == b]
        nb = len(idx); B = nb * n_knots
        Ab = np.stack([A[int(offsets[n]):int(offsets[n]) + b, int(offsets[n]):int(offsets[n]) + b] for n in idx])
        Qb = np.stack([Q[int(offsets[n]):int(offsets[n]) + b, int(offsets[n]):int(offsets[n]) + b] for n in idx])
        hv = np.array([h_val[n] for n in idx])
        Ar = np.repeat(Ab, n_knots, axis=0); Qr = np.repeat(Qb, n_knots, axis=0)
        hr = np.zeros((B, b)); hr[:, 0] = np.repeat(hv, n_knots)
        rr = np.tile(ro, nb)
        PP, ok = _dare_batch(np.swapaxes(Ar, 1, 2), hr, Qr, rr)
        for q in np.where(~ok)[0]:                                      # rare: fall back to the QZ solver
            try:
                PP[q] = sla.solve_discrete_are(Ar[q].T, hr[q][:, None], Qr[q], np.array([[rr[q]]])); ok[q] = True
            except Exception:
                pass
        PP = _newton_dare(Ar, Qr, hr, rr, PP)
        S = hr[:, 0] ** 2 * PP[:, 0, 0] + rr                              # H PP H' + r
        K = PP[:, :, 0] * hr[:, 0][:, None] / S[:, None]                  # PP H' / S
        P = PP - rr[:, None, None] * (K[:, :, None] * K[:, None, :])      # :163  (C-23: K r K', not K S K')
        PSkp = Ar @ P @ np.swapaxes(Ar, 1, 2) + Qr
        PSkp = np.tril(PSkp) + np.swapaxes(np.tril(PSkp, -1), 1, 2)       # chol(.,'lower') reads the lower triangle
        PAt = P @ np.swapaxes(Ar, 1, 2)
        with np.errstate(all='ignore'):
            try:
                G = np.swapaxes(np.linalg.solve(PSkp, np.swapaxes(PAt, 1, 2)), 1, 2)    # P*A'/L'/L
            except np.linalg.LinAlgError:
                G = np.full_like(P, np.nan)
        # QQ = P - G PP G' (:167) without the subtraction: G PSkp = P A' gives P - G PSkp G' = (I - G A) P (I - G A)' + G Q G',
        # and the DARE gives PSkp - PP = (S - r) A K K' A', so QQ = (I - G A) P (I - G A)' + G Q G' + (S - r) (G A K)(G A K)'
        with np.errstate(all='ignore'):
            GA = G @ Ar
            IGA = np.eye(b) - GA
            GAK = np.einsum('qij,qj->qi', GA, K)
            QQ = IGA @ P @ np.swapaxes(IGA, 1, 2) + G @ Qr @ np.swapaxes(G, 1, 2) + (S - rr)[:, None, None] * (GAK[:, :, None] * GAK[:, None, :])
        QQ = (QQ + np.swapaxes(QQ, 1, 2)) / 2
        fin = np.isfinite(QQ).all(axis=(1, 2))
        QQ[~fin] = 0.0
        lam, V = np.linalg.eigh(QQ)                                        # cholcov-style projection on the PSD cone (:169-175)
        lam = np.where(lam > 0, lam, 0.0)
        QQ = (V * lam[:, None, :]) @ np.swapaxes(V, 1, 2)
        # PS2 = dare(G',0,QQ): the Stein equation X = G X G' + QQ as a b^2 x b^2 linear system
        Gs = np.where(np.isfinite(G), G, 0.0)
        try:
            PS2 = _stein_batch(Gs, QQ)
        except np.linalg.LinAlgError:
            PS2 = np.full_like(P, np.nan)
        ok &= fin & np.isfinite(G).all(axis=(1, 2)) & np.isfinite(PS2).all(axis=(1, 2))
        ok &= np.linalg.eigvalsh(PSkp).min(axis=1) > 0                     # chol of PSkp must exist
        for ii, n in enumerate(idx):
            sl = slice(ii * n_knots, (ii + 1) * n_knots)
            g = np.where(ok[sl])[0]
            good[n] = g
            # MATLAB column-major flattening PP(:)'
            PPs[n] = np.stack([PP[sl][j].flatten(order='F') for j in g])
            PGs[n] = np.stack([np.concatenate([PS2[sl][j].flatten(order='F'), G[sl][j].flatten(order='F')]) for j in g])
    return ro, PPs, PGs, good


def build_tables(A, Q, offsets, h_val, n_grid=200, n_knots=32):
    """Returns (r, PPlist, pp_offsets, PGlist, pg_offsets) in the flat layout of nagp_ihgp_tables."""
    M = len(h_val)
    r = np.logspace(-2, 4, n_grid)
    ro, PPs, PGs, good = build_knots(A, Q, offsets, h_val, n_knots)
    pp_parts, pg_parts, pp_off, pg_off = [], [], [], []
    npp = npg = 0
    for n in range(M):
        pp = _interp_rows(ro[good[n]], PPs[n], r)
        pg = _interp_rows(ro[good[n]], PGs[n], r)
        pp_off.append(npp); pg_off.append(npg)
        pp_parts.append(pp.ravel()); pg_parts.append(pg.ravel())
        npp += pp.size; npg += pg.size
    return (r, np.concatenate(pp_parts), np.array(pp_off, dtype=np.int64),
            np.concatenate(pg_parts), np.array(pg_off, dtype=np.int64))
