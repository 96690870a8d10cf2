"""NumPy float64 restatement of the four objectives of the filterbank spectrum fit, unifying_prob_tf/get_Obj_pSTFT_exp.m, _matern32.m,
_matern52.m (form 0, written from the .m text statement by statement) and get_Obj_pSTFT_all.m (form 1).  The generic file's complex
solves H ((F - i w I) \\ L) are stated here through what they equal for a Matern companion system under the rotation,
S_d = (Qc / 2) ((lambda^2 + (w - om)^2)^-p + (lambda^2 + (w + om)^2)^-p), and its gradient through the derivatives in (mVar, len, om)
that _all.m:194-209 forms, chained with dl_dlam as there; `generic_literal` keeps the solves themselves, in float64, for a cross-check.
The 60-digit fixture (tools/make_pstft_fixture.py -> tests/golden/pstft_multiprecision.npz) follows the .m files literally, solves
included, and is what this file and the device are measured against (tests/test_pstft_host.py, tests/test_pstft_gpu.py).
`reverse` forms every sum over the frequencies in the opposite order."""
import math

import numpy as np

KERNELS = ['exp', 'matern32', 'matern52', 'matern72']
ORDER = {'exp': 1, 'matern32': 2, 'matern52': 3, 'matern72': 4}

# name: (kernel, N, D, vary (None: max(specTar) 1e-4; 0: with limLam = [0.05, 0.9]), bet, flavour)
CASES = {
    'n4': ('exp', 4, 1, None, 0.0, ''),                      # even grid, less than a wave
    'n5': ('matern32', 5, 3, None, 750.0, ''),               # odd grid
    'n63': ('matern52', 63, 1, None, 3.0, ''),
    'n64': ('exp', 64, 3, 0.0, 3.0, ''),                     # one wave exactly; vary = 0 with lam bounded away from 0
    'n65': ('matern32', 65, 12, None, 0.0, ''),
    'n255': ('matern52', 255, 3, None, 3.0, 'saturated'),    # theta = +-30 in the om and in the lam part
    'n256': ('exp', 256, 3, None, 750.0, 'edges'),           # one workgroup exactly; om within 1e-3 of 0 and of pi
    'n257': ('matern32', 257, 3, 0.0, 3.0, ''),              # one frequency in the second workgroup
    'n1998': ('matern52', 1998, 12, None, 750.0, ''),        # a level's size
    'n1999': ('exp', 1999, 64, None, 3.0, ''),               # the component limit
    'n70001': ('exp', 70001, 2, None, 3.0, ''),              # 274 workgroups: several runs of the finish order
    'g5': ('matern72', 5, 1, None, 0.0, ''),
    'g64': ('matern72', 64, 3, 0.0, 3.0, ''),
    'g65': ('matern72', 65, 3, None, 750.0, 'saturated'),
    'g257': ('matern72', 257, 3, None, 3.0, 'edges'),
}


def forms(name):
    """the forms a case is stored for: the generic form wherever the 60-digit solves stay within minutes (N <= 257, D <= 3)"""
    kernel, N, D = CASES[name][:3]
    if kernel == 'matern72':
        return (1,)
    return (0, 1) if N <= 257 and D <= 3 else (0,)


def omegas(N):
    """:72-74"""
    h = -(-N // 2)
    om = np.arange(h) * np.pi / (h - 1)                      # linspace(0,pi,ceil(N/2))
    return np.concatenate([om, -om[N // 2 - 1::-1]])


def transforms(theta, minVar, limOm, limLam):
    """:61-67 -> dVar, mVar, om, lam"""
    D = theta.size // 3
    dVar = np.exp(theta[:D]); mVar = minVar + dVar
    om = limOm[:, 0] + (limOm[:, 1] - limOm[:, 0]) / (1 + np.exp(-theta[D:2 * D]))
    lam = limLam[:, 0] + (limLam[:, 1] - limLam[:, 0]) / (1 + np.exp(-theta[2 * D:]))
    return dVar, mVar, om, lam


def case(name):
    """Seeded inputs of a fixture case: limOm = [0, pi]; limLam = [0, 0.4] ([0.05, 0.9] with vary = 0); specTar = the exp-kernel model
    spectrum of a second draw of the parameters times Exp(1) noise, as a periodogram would be."""
    kernel, N, D, vary, bet, flavour = CASES[name]
    rng = np.random.default_rng(4100 + sorted(CASES).index(name))
    limOm = np.tile([0.0, np.pi], (D, 1))
    limLam = np.tile([0.05, 0.9] if vary == 0.0 else [0.0, 0.4], (D, 1))
    minVar = 1e-3 * (0.5 + rng.random(D))

    def draw():
        return np.concatenate([rng.normal(-1.0, 1.0, D), rng.normal(0.0, 1.5, D), rng.normal(-1.0, 1.0, D)])
    theta, truth = draw(), draw()
    if flavour == 'saturated':                               # D = 3: om -> pi with lam -> its upper limit, om -> 0, lam -> 0
        theta[D:2 * D] = [30.0, -30.0, 0.3]                  # (lam -> 0 keeps its om in the interior: at om = pi (1 - 1e-13) the grid
        theta[2 * D:] = [30.0, -0.5, -30.0]                  # point pi - om is known to 1e-3 only, in the .m as here)
    if flavour == 'edges':
        theta[D] = np.log(1e-3 / np.pi) - np.log1p(-1e-3 / np.pi)          # om = 1e-3
        theta[D + 1] = -theta[D]                                             # om = pi - 1e-3
    _, mV, om, lam = transforms(truth, minVar, limOm, limLam)
    w = omegas(N)
    spec = 1e-4 + sum(mV[d] * (1 - lam[d] ** 2) * lam[d] * (1 / (lam[d] ** 2 + (w - om[d]) ** 2) + 1 / (lam[d] ** 2 + (w + om[d]) ** 2)) for d in range(D))
    specTar = spec * rng.exponential(1.0, N)
    v = float(specTar.max() * 1e-4) if vary is None else vary
    return dict(kernel=kernel, N=N, D=D, theta=theta, vary=v, specTar=specTar, minVar=minVar, limOm=limOm, limLam=limLam, bet=bet)


def _fsum(x, reverse):
    """a sum over the frequencies, one term after the other (reverse: from the last)"""
    return np.cumsum(x[::-1] if reverse else x)[-1]


def _tail(theta, D, N, bet, dVar, mVar, limOm, limLam, spec, specTar, dspec, reverse, grad):
    """Obj and dObj from spec and the per-component d spec / d (transVar, om, lam): the common end of the four files"""
    Obj = (_fsum(np.log(spec), reverse) + _fsum(specTar / spec, reverse) + bet * np.sum(mVar)) / N
    if not grad:
        return Obj
    dObjdspec = 1 / spec - specTar / spec ** 2
    dV, dO, dL = np.zeros(D), np.zeros(D), np.zeros(D)
    for d in range(D):
        dspecdtransVar, dspecdom, dspecdlam = dspec(d)
        dV[d] = _fsum(dObjdspec * dspecdtransVar, reverse)
        domdtransOm = (limOm[d, 1] - limOm[d, 0]) * (1 / 4) / np.cosh(theta[D + d] / 2) ** 2
        dO[d] = _fsum(dObjdspec * dspecdom, reverse) * domdtransOm
        dlamdtransLam = (limLam[d, 1] - limLam[d, 0]) * (1 / 4) / np.cosh(theta[2 * D + d] / 2) ** 2
        dL[d] = _fsum(dObjdspec * dspecdlam, reverse) * dlamdtransLam
    dObj = (np.concatenate([dV, dO, dL]) + np.concatenate([bet * dVar, np.zeros(2 * D)])) / N
    return Obj, dObj


def closed(kernel, theta, vary, specTar, minVar, limOm, limLam, bet, reverse=False, grad=True):
    """get_Obj_pSTFT_exp.m / _matern32.m / _matern52.m"""
    theta = np.asarray(theta, float); specTar = np.asarray(specTar, float); D = theta.size // 3; N = specTar.size
    dVar, mVar, om, lam = transforms(theta, minVar, limOm, limLam)
    w = omegas(N); cVar = mVar * (1 - lam ** 2)
    spec = np.ones(N) * vary
    for d in range(D):
        a1 = lam[d] ** 2 + (w - om[d]) ** 2; a2 = lam[d] ** 2 + (w + om[d]) ** 2
        if kernel == 'exp':
            spec = spec + cVar[d] * lam[d] * (a1 ** -1 + a2 ** -1)
        elif kernel == 'matern32':
            spec = spec + 2 * cVar[d] * lam[d] ** 3 * (a1 ** -2 + a2 ** -2)
        elif kernel == 'matern52':
            spec = spec + (8 / 3) * cVar[d] * lam[d] ** 5 * (a1 ** -3 + a2 ** -3)
        else:
            raise ValueError('no closed-form file for %r' % kernel)

    def dspec(d):
        l = lam[d]; a1 = l ** 2 + (w - om[d]) ** 2; a2 = l ** 2 + (w + om[d]) ** 2; wm = w - om[d]; wp = w + om[d]
        if kernel == 'exp':
            return ((mVar[d] - minVar[d]) * (1 - l ** 2) * l * (a1 ** -1 + a2 ** -1),
                    2 * mVar[d] * (1 - l ** 2) * l * (a1 ** -2 * wm - a2 ** -2 * wp),
                    mVar[d] * ((1 - 3 * l ** 2) * (a1 ** -1 + a2 ** -1) - 2 * l ** 2 * (1 - l ** 2) * (a1 ** -2 + a2 ** -2)))
        if kernel == 'matern32':
            return ((mVar[d] - minVar[d]) * 2 * (1 - l ** 2) * l ** 3 * (a1 ** -2 + a2 ** -2),
                    8 * mVar[d] * (1 - l ** 2) * l ** 3 * (a1 ** -3 * wm - a2 ** -3 * wp),
                    2 * mVar[d] * l ** 2 * ((3 * (1 - l ** 2) - 2 * l ** 2) * (a1 ** -2 + a2 ** -2) - 4 * (1 - l ** 2) * l ** 2 * (a1 ** -3 + a2 ** -3)))
        return ((mVar[d] - minVar[d]) * (8 / 3) * (1 - l ** 2) * l ** 5 * (a1 ** -3 + a2 ** -3),
                16 * mVar[d] * (1 - l ** 2) * l ** 5 * (a1 ** -4 * wm - a2 ** -4 * wp),
                (8 / 3) * mVar[d] * l ** 4 * ((5 - 7 * l ** 2) * (a1 ** -3 + a2 ** -3) - 6 * (1 - l ** 2) * l ** 2 * (a1 ** -4 + a2 ** -4)))
    return _tail(theta, D, N, bet, dVar, mVar, limOm, limLam, spec, specTar, dspec, reverse, grad)


def ss_scalars(kernel, mVar, ell):
    """lambda, Qc of cf_<kernel>_to_ss(mVar, ell) and their derivatives in ell (dF's last row is the derivative of the powers of lambda)"""
    p = ORDER[kernel]
    c = {1: 1.0, 2: math.sqrt(3.0), 3: math.sqrt(5.0), 4: math.sqrt(7.0)}[p]
    q = {1: 2.0, 2: 12.0 * math.sqrt(3.0), 3: 400.0 * math.sqrt(5.0) / 3.0, 4: 10976.0 * math.sqrt(7.0) / 5.0}[p]
    lamb = c / ell
    Qc = mVar * q / ell ** (2 * p - 1)
    return lamb, Qc, -lamb / ell, -(2 * p - 1) * Qc / ell


def generic(kernel, theta, vary, specTar, minVar, limOm, limLam, bet, reverse=False, grad=True):
    """get_Obj_pSTFT_all.m with its solves in closed form (module docstring)"""
    theta = np.asarray(theta, float); specTar = np.asarray(specTar, float); D = theta.size // 3; N = specTar.size
    p = ORDER[kernel]
    dVar, mVar, om, lam = transforms(theta, minVar, limOm, limLam)
    w = omegas(N)
    cl = {'exp': 1.0, 'matern32': math.sqrt(3.0)}.get(kernel, math.sqrt(5.0))           # _all.m:81-94
    ell = cl / lam; dl_dlam = -cl * lam ** -2.0
    spec = np.ones(N) * vary; spec_om = [None] * D
    for d in range(D):
        lamb, Qc, _, _ = ss_scalars(kernel, mVar[d], ell[d])
        a1 = lamb ** 2 + (w - om[d]) ** 2; a2 = lamb ** 2 + (w + om[d]) ** 2
        spec_om[d] = (Qc / 2) * (a1 ** -p + a2 ** -p)
        spec = spec + (1 - lam[d] ** 2) * spec_om[d]

    def dspec(d):
        lamb, Qc, dlamb_dl, dQc_dl = ss_scalars(kernel, mVar[d], ell[d])
        wm = w - om[d]; wp = w + om[d]; a1 = lamb ** 2 + wm ** 2; a2 = lamb ** 2 + wp ** 2
        dS_dvar = (Qc / mVar[d] / 2) * (a1 ** -p + a2 ** -p)
        dS_dl = (dQc_dl / 2) * (a1 ** -p + a2 ** -p) - (Qc / 2) * p * 2 * lamb * dlamb_dl * (a1 ** -(p + 1) + a2 ** -(p + 1))
        dS_dom = (Qc / 2) * 2 * p * (a1 ** -(p + 1) * wm - a2 ** -(p + 1) * wp)
        dS_dlam = dS_dl * dl_dlam[d]
        return ((mVar[d] - minVar[d]) * (1 - lam[d] ** 2) * dS_dvar, (1 - lam[d] ** 2) * dS_dom,
                (1 - lam[d] ** 2) * dS_dlam - 2 * lam[d] * spec_om[d])
    return _tail(theta, D, N, bet, dVar, mVar, limOm, limLam, spec, specTar, dspec, reverse, grad)


def generic_literal(kernel, theta, vary, specTar, minVar, limOm, limLam, bet):
    """get_Obj_pSTFT_all.m line by line, the 2 tau x 2 tau complex solves included, in float64 (a cross-check of `generic`; its
    accuracy is that of the solves)"""
    theta = np.asarray(theta, float); specTar = np.asarray(specTar, float); D = theta.size // 3; N = specTar.size
    p = ORDER[kernel]
    dVar, mVar, om, lam = transforms(theta, minVar, limOm, limLam)
    w = omegas(N)
    cl = {'exp': 1.0, 'matern32': math.sqrt(3.0)}.get(kernel, math.sqrt(5.0))
    ell = cl / lam; dl_dlam = -cl * lam ** -2.0
    I2 = np.eye(2); binom = [math.comb(p, k) for k in range(p)]
    spec = np.ones(N) * vary
    parts = []
    for d in range(D):
        lamb, Qc1, dlamb_dl, dQc_dl = ss_scalars(kernel, mVar[d], ell[d])
        F1 = np.diag(np.ones(p - 1), 1); dF1 = np.zeros((p, p))
        for k in range(p):
            F1[p - 1, k] = -binom[k] * lamb ** (p - k)
            dF1[p - 1, k] = -binom[k] * (p - k) * lamb ** (p - k - 1) * dlamb_dl
        L1 = np.zeros((p, 1)); L1[-1, 0] = 1.0; H1 = np.zeros((1, p)); H1[0, 0] = 1.0
        F2 = np.array([[0.0, -om[d]], [om[d], 0.0]])
        F = np.kron(F1, I2) + np.kron(np.eye(p), F2); L = np.kron(L1, I2); H = np.kron(H1, [[1.0, 0.0]])
        dF_dl = np.kron(dF1, I2); dF_dom = np.kron(np.eye(p), np.array([[0.0, -1.0], [1.0, 0.0]]))
        B = L @ L.T
        S = np.zeros(N); dS_dvar = np.zeros(N); dS_dom = np.zeros(N); dS_dlam = np.zeros(N)
        for i in range(N):
            G = F - 1j * w[i] * np.eye(2 * p)
            J = H @ np.linalg.inv(G); JL = J @ L
            s = (JL @ JL.conj().T).real[0, 0]
            JJ = J.conj().T @ J; GB = np.linalg.solve(G, B)

            def tr(dF):
                K = dF @ GB
                return np.trace(JJ @ (K + K.conj().T)).real
            S[i] = Qc1 * s
            dS_dvar[i] = (Qc1 / mVar[d]) * s
            dS_dlam[i] = (dQc_dl * s - Qc1 * tr(dF_dl)) * dl_dlam[d]
            dS_dom[i] = -Qc1 * tr(dF_dom)
        spec = spec + (1 - lam[d] ** 2) * S
        parts.append(((mVar[d] - minVar[d]) * (1 - lam[d] ** 2) * dS_dvar, (1 - lam[d] ** 2) * dS_dom, (1 - lam[d] ** 2) * dS_dlam - 2 * lam[d] * S))
    return _tail(theta, D, N, bet, dVar, mVar, limOm, limLam, spec, specTar, lambda d: parts[d], False, True)


def objective(c, form, reverse=False, grad=True):
    """a case (or any dict with its keys) through the form's restatement"""
    f = closed if form == 0 else generic
    return f(c['kernel'], c['theta'], c['vary'], c['specTar'], c['minVar'], c['limOm'], c['limLam'], c['bet'], reverse=reverse, grad=grad)


def dist(a, ref):
    """the project's norm: max|a - ref| / max|ref|"""
    ref = np.asarray(ref, float)
    return float(np.max(np.abs(np.asarray(a, float) - ref)) / np.max(np.abs(ref)))


def evaluator(kernel, reverse=False):
    """the restatement as the `evaluator` of nagp.fit_probSTFT_SD: the kernel-specific file where there is one, else the generic"""
    f = generic if kernel == 'matern72' else closed

    def ev(theta, vary, specTar, minVar, limOm, limLam, bet, grad):
        return f(kernel, theta, vary, specTar, minVar, limOm, limLam, bet, reverse=reverse, grad=grad)
    return ev


def ar_signal(seed, T, om=(0.35, 0.9, 1.7), lam=(0.97, 0.95, 0.9), var=(1.0, 0.5, 0.25)):
    """a seeded draw of y_t = sum_d Re x_{d,t}, x_{d,t} = lam_d exp(i om_d) x_{d,t-1} + complex white noise: three AR sub-bands"""
    rng = np.random.default_rng(seed)
    y = np.zeros(T)
    for o, l, v in zip(om, lam, var):
        e = np.sqrt(v * (1 - l ** 2)) * (rng.standard_normal(T + 200) + 1j * rng.standard_normal(T + 200))
        x = np.zeros(T + 200, complex)
        for t in range(1, T + 200):
            x[t] = l * np.exp(1j * o) * x[t - 1] + e[t]
        y += x[200:].real
    return y
