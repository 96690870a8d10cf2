"""Joint posterior draws of a full-covariance EP run (nagp_ep_sample, include/nagp.h): whole state paths, correlated in time, from
the sites a predict-mode run of gf_ep_modulator / gf_ep_modulator_nmf / gf_ep_modulator_nmf_constraints returned.  The forward
filter with fixed sites, the per-step factorisation and the backward sampling run in libnagp.so on the GPU; there is no CPU
fallback.  The mixture drivers, the EKF family and the infinite-horizon family are not served (see the header)."""
import ctypes as C

import numpy as np

from . import _lib as L
from . import ss as ssm
from .api import Mom, _Problem, _blocks_from_dense, _merge_inputs, _unpack_constraints, _unpack_log


def _signal_opts(signal):
    """signal: a Mom (sqrt amplitudes for likModulatorPreCalcwn, its link and shift) or a dict(amp='linear'|'sqrt', link='softplus'|'exp',
    link_shift=0.0) -> (amp_kind, link_kind, link_shift)"""
    if isinstance(signal, Mom):
        return (L.AMP_SQRT if signal.kind == L.LIK_POWER_NMF_SQRT else L.AMP_LINEAR,
                L.LINK_SOFTPLUS if signal.link == 'softplus' else L.LINK_EXP, float(signal.link_shift))
    amp = signal.get('amp', 'linear'); link = signal.get('link', 'softplus')
    if amp not in ('linear', 'sqrt') or link not in ('softplus', 'exp'):
        raise ValueError("signal: amp must be 'linear' or 'sqrt', link 'softplus' or 'exp'")
    return (L.AMP_SQRT if amp == 'sqrt' else L.AMP_LINEAR, L.LINK_SOFTPLUS if link == 'softplus' else L.LINK_EXP, float(signal.get('link_shift', 0.0)))


def ep_sample(prob, ttau, tnu, yall, n_draws, seed=0, predict_at_k1=0, states=False, signal=None, Wnmf=None, z=None, fdraw=True, device=0,
              return_counters=False):
    """nagp_ep_sample on one problem (a _Problem: the discrete model as the driver built it).  ttau, tnu: M x T as the run returned them;
    yall: T, NaN = missing.  z: optional n_draws x T x S normals of the caller in place of the generator.
    Returns (Fdraw n x M x T, Xdraw n x S x T or None, Sdraw n x T or None, MS S x T)[, counters (2,)]."""
    blk = prob.blk; S, M = blk.S, blk.M
    yall = L.f64(np.asarray(yall, float).ravel(), 'C'); T = yall.size
    tt = L.f64(ttau); tn = L.f64(tnu)
    if tt.shape != (M, T) or tn.shape != (M, T):
        raise ValueError('ttau and tnu must be %d x %d (the sites of the run on these inputs)' % (M, T))
    n = int(n_draws)
    zc = None
    if z is not None:
        zc = L.f64(z, 'C')
        if zc.shape != (n, T, S):
            raise ValueError('z must be n_draws x T x S')
    sig = None; keep = None
    if signal is not None:
        W = prob.W if Wnmf is None else L.f64(Wnmf)
        if W is None:
            W = L.f64(np.eye(blk.D))                      # gf_ep_modulator: one modulator per sub-band
        amp, link, shift = _signal_opts(signal)
        keep = W
        sig = L.EpSampleSig(Wnmf=L.dptr(W), amp_kind=amp, link_kind=link, link_shift=shift)
    nn = max(n, 0)
    X = np.zeros((nn, T, S)) if states else None
    F = np.zeros((nn, T, M)) if fdraw else None
    Sd = np.zeros((nn, T)) if signal is not None else None
    MS = np.zeros((S, T), order='F')
    cnt = np.zeros(2, dtype=np.int64)
    L.check(L.lib().nagp_ep_sample(C.byref(prob.model), L.dptr(tt), L.dptr(tn), L.dptr(yall), T, int(predict_at_k1), n, int(seed) & (2 ** 64 - 1),
                                   L.dptr(zc), C.byref(sig) if sig is not None else None, L.dptr(X), L.dptr(F), L.dptr(Sd), L.dptr(MS),
                                   cnt.ctypes.data_as(L.c_lp), int(device)))
    del keep
    res = (None if F is None else F.transpose(0, 2, 1), None if X is None else X.transpose(0, 2, 1), Sd, MS)
    return res + (cnt,) if return_counters else res


def ep_sample_timings():
    """device time of the three parts of the last nagp_ep_sample on this thread, in ms: filter, factor, draw"""
    ms = np.zeros(3)
    L.check(L.lib().nagp_ep_sample_timings(L.dptr(ms)))
    return dict(filter=ms[0], factor=ms[1], draw=ms[2])


def gf_ep_sample(w, x, y, ss, kernel1, kernel2, num_lik_params, D, N, out, n_draws, seed=0, states=False, signal=None, constraints=None,
                 w_fixed=None, tune_hypers=None, xt=None, z=None, device=0, return_counters=False):
    """Joint draws from the posterior a predict-mode run left in `out` (its ttau, tnu).  The arguments are those of the driver that made
    `out`, the model is unpacked and balanced as that driver does:
      constraints given          gf_ep_modulator_nmf_constraints (sigmoid-constrained parameters with w_fixed, tune_hypers; balance on)
      N given                    gf_ep_modulator_nmf (log parameters; balance off)
      N None                     gf_ep_modulator (one modulator per sub-band; balance on; predicts at the first step)
    xt as passed to the driver (None: xt = x).  signal: None, the driver's Mom, or dict(amp=, link=, link_shift=) -- asks for Sdraw.
    Returns (Fdraw n x M x T, Xdraw n x S x T or None (states), Sdraw n x T or None, MS S x T) over the merged inputs, like out['MS']."""
    yall, _ = _merge_inputs(x, y, x if xt is None else xt)
    pk1 = 0
    if constraints is not None:
        lik_param, p1, p2, Wnmf = _unpack_constraints(w, w_fixed, tune_hypers, constraints, num_lik_params, D, N)
        blk = ssm.balance_blocks(_blocks_from_dense(*ss(x, p1, p2, kernel1, kernel2), D, N))
    elif N is not None:
        lik_param, p1, p2, Wnmf = _unpack_log(w, num_lik_params, D, N)
        blk = _blocks_from_dense(*ss(x, p1, p2, kernel1, kernel2), D, N)
    else:
        w = np.asarray(w, float).ravel()
        lik_param = w[:num_lik_params]; param = np.exp(w[num_lik_params:])
        D = param.size // 5
        blk = ssm.balance_blocks(_blocks_from_dense(*ss(x, param, kernel1, kernel2), D, D))
        Wnmf = None; pk1 = 1
    prob = _Problem(blk, Wnmf, lik_param)
    return ep_sample(prob, out['ttau'], out['tnu'], yall, n_draws, seed, pk1, states, signal, z=z, device=device, return_counters=return_counters)
