"""CPU restatement (test infrastructure) of the post-processing block of the experiment scripts -- experiments/source_sep_piano.m:165-244,
noise_reduction_speech.m:142 (the same line in missing_data_music.m:173, test_missing_data.m:159, synthetic_data_experiment.m:221):
draws of the independent posterior marginals, amplitude a_d = sqrt(W_d.link(g)) ('sqrt') or W_d.link(g) ('linear', the toy demo),
sig = sum_d a_d z_d, sig_j = the same sum over the sub-bands of source j, envs = mean over the draws of a_d.  `sampling` follows the .m
statement by statement on the draws of the library's counter-based generator (oracle.recon.normals); `population` gives the values those
sample statistics estimate."""
import numpy as np

from oracle.recon import normals


def amp_of(kind):
    if kind == 'sqrt':
        def amp(x):
            with np.errstate(invalid='ignore'):
                return np.sqrt(x)          # negative argument: NaN (MATLAB goes complex)
        return amp
    return lambda x: x


def draws(Eft, Varft, D, N, s, seed):
    """sub_samp (D, T, s), mod_samp (N, T, s): source_sep_piano.m:177-178, :196"""
    T = Eft.shape[1]
    sub = np.stack([normals(T, d, s, seed) * np.sqrt(Varft[d])[:, None] + Eft[d][:, None] for d in range(D)])
    mod = np.stack([normals(T, D + n, s, seed) * np.sqrt(Varft[D + n])[:, None] + Eft[D + n][:, None] for n in range(N)])
    return sub, mod


def sampled_signals(Eft, Varft, W, offsets, link, kind, s, seed):
    """the per-draw arrays: lm (N, T, s), envs (D, T, s), sig (T, s), sig_j (J, T, s)"""
    D, N = W.shape
    sub, mod = draws(Eft, Varft, D, N, s, seed)
    lm = link(mod)
    envs = amp_of(kind)(np.einsum('dn,nts->dts', W, lm))                                   # :218
    chan = envs * sub                                                                      # :219
    sig = chan.sum(axis=0)                                                                 # :220
    sigj = np.stack([chan[offsets[j]:offsets[j + 1]].sum(axis=0) for j in range(len(offsets) - 1)])   # :221-223
    return lm, envs, sig, sigj


def sampling(Eft, Varft, W, offsets, link, kind, s, seed):
    lm, envs, sig, sigj = sampled_signals(Eft, Varft, W, offsets, link, kind, s, seed)
    return dict(Esig=sig.mean(axis=1), Vsig=sig.var(axis=1, ddof=1),                       # :226-227
                Esrc=sigj.mean(axis=2), Vsrc=sigj.var(axis=2, ddof=1),                     # :229-234
                Eenv=envs.mean(axis=2),                                                    # :225
                Eft_mod=lm.mean(axis=2), Varft_mod=lm.var(axis=2, ddof=1))                 # :197-198


def population(Eft, Varft, W, offsets, link, kind, gh_x, gh_w, exp_link=False, wn=None, xn=None):
    """Population values.  Eft_mod / Varft_mod: 1-D Gauss-Hermite rule (exp link: closed form).  'linear': closed forms per source.
    'sqrt': E a_d^2 = W_d.E lk from the 1-D rule; E a_d and the moments of u_j(g) = sum_{d in j} a_d(g) Eft_d from the N-dimensional rule
    (wn, xn: unit points), the variance of u_j accumulated about its value c_j at the centre g = Eft:
        E u_j = c_j sw + S1,  Var u_j = S2 - S1^2 + (1 - sw)(c_j^2 sw + 2 c_j S1),  S1 = sum w (u_j - c_j), S2 = sum w (u_j - c_j)^2, sw = sum w."""
    D, N = W.shape
    mg, vg = Eft[D:], Varft[D:]
    if exp_link:
        e1 = np.exp(mg + 0.5 * vg); e2 = np.exp(2 * mg + 2 * vg)
    else:
        l = link(mg[:, :, None] + np.sqrt(vg)[:, :, None] * gh_x[None, None, :])
        e1 = l @ gh_w; e2 = (l * l) @ gh_w
    var = e2 - e1 * e1
    m, v = Eft[:D], Varft[:D]
    ranges = [slice(offsets[j], offsets[j + 1]) for j in range(len(offsets) - 1)] + [slice(0, D)]     # the sources, then the total
    if kind == 'linear':
        a = W @ e1
        E = [np.sum(a[r] * m[r], axis=0) for r in ranges]
        Vv = [np.sum(a[r] ** 2 * v[r], axis=0) + np.sum(var * ((W[r].T @ m[r]) ** 2 + (W[r].T ** 2) @ v[r]), axis=0) for r in ranges]
        env = a
    else:
        amp = amp_of('sqrt')
        g = mg[:, :, None] + np.sqrt(vg)[:, :, None] * xn[:, None, :]                      # (N, T, P)
        ap = amp(np.einsum('dn,ntp->dtp', W, link(g)))                                     # (D, T, P)
        ac = amp(W @ link(mg))                                                             # (D, T)
        env = ap @ wn
        a2 = W @ e1                                                                        # E a_d^2
        sw = np.sum(wn)
        E, Vv = [], []
        for r in ranges:
            u = np.einsum('dtp,dt->tp', ap[r], m[r]); c = np.sum(ac[r] * m[r], axis=0)
            x = u - c[:, None]
            S1 = x @ wn; S2 = (x * x) @ wn
            E.append(c * sw + S1)
            Vv.append(np.sum(a2[r] * v[r], axis=0) + ((S2 - S1 * S1) + (1.0 - sw) * (c * c * sw + 2.0 * c * S1)))
    return dict(Esig=E[-1], Vsig=Vv[-1], Esrc=np.stack(E[:-1]), Vsrc=np.stack(Vv[:-1]), Eenv=env, Eft_mod=e1, Varft_mod=var)
