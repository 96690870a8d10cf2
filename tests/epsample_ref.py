"""NumPy restatement (FP64, dense, step by step) of nagp_ep_sample (include/nagp.h): joint posterior draws of a full-covariance
EP run by forward filtering with the returned sites and backward sampling.  Test infrastructure: the GPU tests compare the library
with it, tests/test_epsample_host.py pins it to the oracle's run_predict (MF, PF, MS) and to the exact law of the smoother.

A model is a dict {A, Q, Pinf (S x S), offsets (M+1), h_val (M)}; row n of H has its non-zero h_val[n] at column offsets[n]."""
import math

import numpy as np

from oracle import recon as orec

JITTER = math.sqrt(1e-4) * 0.5          # the reference's retry, rand -> 0.5 (SURVEY C-7)


def dense_H(model):
    off = np.asarray(model['offsets']); M = off.size - 1
    H = np.zeros((M, model['A'].shape[0])); H[np.arange(M), off[:-1]] = model['h_val']
    return H


def model_of(A, Q, Pinf, H):
    """the dict of this module from dense matrices (the oracle's assembled model)"""
    H = np.asarray(H, float); M, S = H.shape
    starts = np.array([int(np.nonzero(H[n])[0][0]) for n in range(M)])
    return dict(A=np.asarray(A, float), Q=np.asarray(Q, float), Pinf=np.asarray(Pinf, float), offsets=np.concatenate([starts, [S]]).astype(np.int32),
                h_val=H[np.arange(M), starts].copy())


def fixed_site_filter(model, y, ttau, tnu, predict_at_k1=False):
    """the last forward pass of a run as a recursion in its sites: MF (S x T), PF (T x S x S)"""
    A, Q = model['A'], model['Q']; S = A.shape[0]; T = y.size
    c = np.asarray(model['offsets'])[:-1]; h = np.asarray(model['h_val'], float)
    m = np.zeros(S); P = np.array(model['Pinf'], float)
    MF = np.zeros((S, T)); PF = np.zeros((T, S, S))
    for k in range(T):
        if k > 0 or predict_at_k1:
            m = A @ m; P = A @ P @ A.T + Q
        if not np.isnan(y[k]):
            tt, tn = ttau[:, k], tnu[:, k]
            fmu = h * m[c]; W = P[:, c] * h[None, :]; HPH = h * P[c, c] * h
            z0 = tt == 0
            with np.errstate(all='ignore'):
                # sites with ttau = 0: K = W ttau / (ttau HPH + 1), P - K W';  the others: K = W / (HPH + 1 / ttau), P - (K H) P
                cm = np.where(z0, -(tt * fmu - tn) / (tt * HPH + 1.0), (tn / tt - fmu) / (HPH + 1.0 / tt))
                K0 = W * np.where(z0, tt / (tt * HPH + 1.0), 0.0)[None, :]
                K1 = np.where(z0[None, :], 0.0, W / (HPH + 1.0 / tt)[None, :])
            m = m + W @ cm
            if np.any(z0):
                P = P - K0[:, z0] @ W[:, z0].T
            if np.any(~z0):
                P = P - (K1 * h[None, :])[:, ~z0] @ P[c[~z0], :]
        MF[:, k] = m; PF[k] = P
    return MF, PF


def chol_clamped(C):
    """lower Cholesky factor of the lower triangle of C; a pivot <= 0 (or NaN) zeroes its column and is counted"""
    n = C.shape[0]; Lc = np.tril(C).astype(float); clamped = 0
    for j in range(n):
        d = Lc[j, j]
        if not d > 0.0:
            Lc[j:, j] = 0.0; clamped += 1
            continue
        r = math.sqrt(d)
        Lc[j, j] = r; Lc[j + 1:, j] /= r
        v = Lc[j + 1:, j]
        Lc[j + 1:, j + 1:] -= np.tril(np.outer(v, v))
    return Lc, clamped


def chol_retry(P):
    """chol(P, 'lower') of the lower triangle with the reference's jitter retry; (L, retries, ok)"""
    Ls = np.tril(P); Ls = Ls + np.tril(Ls, -1).T
    Lc, bad = chol_clamped(Ls)
    if bad == 0:
        return Lc, 0, True
    Lc, bad = chol_clamped(Ls + JITTER * np.eye(P.shape[0]))
    return Lc, 1, bad == 0


def backward_factors(model, PF, retry_steps=None):
    """per step k < T-1: G_k = PF_k A' / L' / L with L = chol(A PF_k A' + Q), Lc_k = chol((I - G A) PF_k (I - G A)' + G Q G');
    Lc_{T-1} = chol(PF_{T-1}).  Returns G (T x S x S, G[T-1] = 0), Lc (T x S x S), counters [retries, clamped]; the steps that took
    the jitter retry are appended to retry_steps."""
    A, Q = model['A'], model['Q']; T, S, _ = PF.shape
    G = np.zeros((T, S, S)); Lc = np.zeros((T, S, S)); cnt = np.zeros(2, np.int64); I = np.eye(S)
    for k in range(T - 1):
        L, r, _ = chol_retry(A @ PF[k] @ A.T + Q); cnt[0] += r
        if r and retry_steps is not None:
            retry_steps.append(k)
        B = PF[k] @ A.T
        X = np.linalg.solve(L, B.T).T                      # B / L'
        G[k] = np.linalg.solve(L.T, X.T).T                 # X / L
        M1 = I - G[k] @ A
        C = M1 @ PF[k] @ M1.T + G[k] @ Q @ G[k].T
        Lc[k], c = chol_clamped(C); cnt[1] += c
    Lc[T - 1], c = chol_clamped(PF[T - 1]); cnt[1] += c
    return G, Lc, cnt


def generator_normals(T, S, n_draws, seed):
    """z[i, k, j] = normals(T, j, n_draws, seed)[k, i]"""
    return np.stack([orec.normals(T, j, n_draws, seed) for j in range(S)], axis=2).transpose(1, 0, 2).copy()


def link(kind, shift, g):
    return np.log(1.0 + np.exp(g - shift)) if kind == 0 else np.exp(g)


def signal(F, D, Wnmf, amp_kind, link_kind, shift):
    """Sdraw[i, k] = sum_d a_d z_d on Fdraw (n x M x T): a_d = W_d.link(g) or its square root"""
    lk = link(link_kind, shift, F[:, D:, :])
    a = np.einsum('dn,int->idt', np.asarray(Wnmf, float), lk)
    if amp_kind == 1:
        with np.errstate(invalid='ignore'):
            a = np.sqrt(a)
    return np.einsum('idt,idt->it', a, F[:, :D, :])


def sample(model, ttau, tnu, y, predict_at_k1, n_draws, seed=0, z=None, sig=None):
    """(Xdraw n x S x T, Fdraw n x M x T, Sdraw n x T or None, MS S x T, counters, parts) of nagp_ep_sample.
    z: n x T x S caller's normals or None = the generator.  sig = (Wnmf, amp_kind, link_kind, shift) or None."""
    y = np.asarray(y, float).ravel(); T = y.size
    A = model['A']; S = A.shape[0]
    c = np.asarray(model['offsets'])[:-1]; h = np.asarray(model['h_val'], float)
    MF, PF = fixed_site_filter(model, y, ttau, tnu, predict_at_k1)
    steps = []
    G, Lc, cnt = backward_factors(model, PF, steps)
    if z is None:
        z = generator_normals(T, S, n_draws, seed)
    z = np.concatenate([np.asarray(z, float).reshape(n_draws, T, S), np.zeros((1, T, S))])      # the last one is the mean chain
    X = np.zeros((n_draws + 1, S, T))
    x = MF[:, T - 1][None, :] + z[:, T - 1, :] @ Lc[T - 1].T
    X[:, :, T - 1] = x
    for k in range(T - 2, -1, -1):
        x = MF[:, k][None, :] + (x - (A @ MF[:, k])[None, :]) @ G[k].T + z[:, k, :] @ Lc[k].T
        X[:, :, k] = x
    MS = X[n_draws]; X = X[:n_draws]
    F = h[None, :, None] * X[:, c, :]
    Sd = None if sig is None else signal(F, len(c) - np.asarray(sig[0]).shape[1], *sig)
    return X, F, Sd, MS, cnt, dict(MF=MF, PF=PF, G=G, Lc=Lc, retry_steps=np.array(steps, np.int64))
