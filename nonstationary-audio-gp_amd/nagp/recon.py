"""Posterior reconstruction of the signal and the modulator amplitudes from the marginals the hot path returns
(matlab/demo_toy_modulators_nmf.m:119-158): nagp_reconstruct of the C ABI, and the experiment scripts' form
of it with the square-root amplitude, sources and envelopes (experiments/source_sep_piano.m:165-244): nagp_reconstruct_sources."""
import numpy as np

from . import _lib as L
from .cubature import gauher, sigma_points


def reconstruct_signal(Eft, Varft, Wnmf, link='softplus', link_shift=0.0, n_samples=0, seed=0, n_gh=32, device=0):
    """Eft, Varft: (D+N) x T as returned by gf_ep_modulator_nmf & co; Wnmf: D x N.
    n_samples = 0: population means / variances (Gauss-Hermite, closed-form combination);
    n_samples = s >= 2: the reference's sampling estimator (s = 250 in the demos) with a reproducible counter-based generator.
    Returns dict(Esig (T,), Vsig (T,), Eft_mod (N,T), Varft_mod (N,T))."""
    W = L.f64(Wnmf); D, N = W.shape
    E = L.f64(Eft); V = L.f64(Varft)
    if E.shape != V.shape or E.shape[0] != D + N:
        raise ValueError('Eft / Varft must be (D+N) x T')
    T = E.shape[1]
    gx, gw = gauher(int(n_gh))
    gx = L.f64(gx, 'C'); gw = L.f64(gw, 'C')
    Esig = np.zeros(T); Vsig = np.zeros(T); Em = np.zeros((N, T), order='F'); Vm = np.zeros((N, T), order='F')
    L.check(L.lib().nagp_reconstruct(D, N, T, L.dptr(E), L.dptr(V), L.dptr(W), L.LINK_SOFTPLUS if link == 'softplus' else L.LINK_EXP,
                                     float(link_shift), gx.size, L.dptr(gx), L.dptr(gw), int(n_samples), int(seed),
                                     L.dptr(Esig), L.dptr(Vsig), L.dptr(Em), L.dptr(Vm), int(device)))
    return dict(Esig=Esig, Vsig=Vsig, Eft_mod=Em, Varft_mod=Vm)


RECON_OUTPUTS = ('Esig', 'Vsig', 'Esrc', 'Vsrc', 'Eenv', 'Eft_mod', 'Varft_mod')


def stack_sources(Ws):
    """W_all = blkdiag(Wnmf{:}) (source_sep_piano.m:210) and the sub-band offsets of the sources."""
    Ws = [np.atleast_2d(np.asarray(w, dtype=np.float64)) for w in Ws]
    W = np.zeros((sum(w.shape[0] for w in Ws), sum(w.shape[1] for w in Ws)))
    off = [0]; c = 0
    for w in Ws:
        W[off[-1]:off[-1] + w.shape[0], c:c + w.shape[1]] = w
        off.append(off[-1] + w.shape[0]); c += w.shape[1]
    return W, off


def reconstruct_sources(Eft, Varft, Wnmf, amplitude='sqrt', sources=None, link='softplus', link_shift=0.0, n_samples=0, seed=0, n_gh=32,
                        p_cubature=5, device=0, outputs=None):
    """sig = sum_d a_d z_d, sig_j = its part over the sub-bands of source j, env_d = a_d with a_d = sqrt(W_d.link(g)) (amplitude='sqrt',
    the model of likModulatorPreCalcwn and of every experiment script) or W_d.link(g) ('linear', the demos) under the independent marginals.
    Eft, Varft: (D+N) x T; Wnmf: D x N, or a list of per-source matrices (stacked block-diagonally, the sources taken from them).
    sources: None (one source), J (J equal blocks of sub-bands, source_sep_piano.m:221-223) or the J+1 offsets.
    n_samples = s >= 2: the scripts' sampling estimator on the reproducible draws of reconstruct_signal; 0: the population values
    (1-D Gauss-Hermite rule of n_gh points; amplitude='sqrt': sigma_points(p_cubature, N) over the modulators).
    outputs: the names wanted (default all).  Returns dict(Esig (T,), Vsig (T,), Esrc (J,T), Vsrc (J,T), Eenv (D,T), Eft_mod (N,T), Varft_mod (N,T))."""
    off = None
    if isinstance(Wnmf, (list, tuple)):
        if sources is not None:
            raise ValueError('a list of per-source matrices defines the sources')
        Wnmf, off = stack_sources(Wnmf)
    W = L.f64(Wnmf); D, N = W.shape
    E = L.f64(Eft); V = L.f64(Varft)
    if E.ndim != 2 or E.shape != V.shape or E.shape[0] != D + N:
        raise ValueError('Eft / Varft must be (D+N) x T')
    T = E.shape[1]
    if off is None:
        if sources is None:
            off = [0, D]
        elif np.ndim(sources) == 0:
            J = int(sources)
            if J < 1 or D % J:
                raise ValueError('sources = J needs J equal blocks of sub-bands')
            off = [j * (D // J) for j in range(J + 1)]
        else:
            off = [int(x) for x in sources]
    J = len(off) - 1
    offs = np.ascontiguousarray(off, dtype=np.int32)
    amp = {'linear': L.AMP_LINEAR, 'sqrt': L.AMP_SQRT}.get(amplitude, amplitude)
    lk = {'softplus': L.LINK_SOFTPLUS, 'exp': L.LINK_EXP}.get(link, link)
    o = L.ReconOpts(amp_kind=int(amp), link_kind=int(lk), link_shift=float(link_shift), n_sources=J, source_offsets=offs.ctypes.data_as(L.c_ip),
                    n_samples=int(n_samples), seed=int(seed), device=int(device))
    keep = [offs]
    if not n_samples:
        gx, gw = gauher(int(n_gh))
        gx = L.f64(gx, 'C'); gw = L.f64(gw, 'C'); keep += [gx, gw]
        o.n_gh = gx.size; o.gh_x = L.dptr(gx); o.gh_w = L.dptr(gw)
        if amp == L.AMP_SQRT:
            wn, xn = sigma_points(p_cubature, N)
            wn = L.f64(wn, 'C'); xn = L.f64(xn); keep += [wn, xn]
            o.n_pts = wn.size; o.wn = L.dptr(wn); o.xn_unscaled = L.dptr(xn)
    shapes = dict(Esig=(T,), Vsig=(T,), Esrc=(J, T), Vsrc=(J, T), Eenv=(D, T), Eft_mod=(N, T), Varft_mod=(N, T))
    want = RECON_OUTPUTS if outputs is None else tuple(outputs)
    res = {k: np.zeros(shapes[k], order='F') for k in want}
    out = L.ReconOut(**{k: L.dptr(a) for k, a in res.items()})
    L.check(L.lib().nagp_reconstruct_sources(D, N, T, L.dptr(E), L.dptr(V), L.dptr(W), L.C.byref(o), L.C.byref(out)))
    del keep
    return res
