"""NumPy float64 restatement of the modulator prior fit's objective, experiments/toolsGP/getObjSEGP.m on getGPSESpec.m, written from the
formulae of include/nagp.h (nagp_segp_obj):

    f_j = j (j <= ceil(T/2)) else j - T,  w_j = 2 pi f_j / T,  c_j = sqrt(2 pi len^2) exp(-w_j^2 len^2 / 2),  dc_j = c_j (1/len - w_j^2 len),
    S_j = varx c_j + vary,  g_j = 1/(2 S_j) - specy_j / (2 T S_j^2),
    Obj = (1/2 sum log S + 1/(2T) sum specy / S) / T,  dObj = [len varx sum g dc, varx sum g c, vary sum g] / T.

The 60-digit fixture (tools/make_segp_fixture.py -> tests/golden/segp_multiprecision.npz) is what this file and the device are measured
against (tests/test_segp_host.py, tests/test_segp_gpu.py).  `reverse` forms every sum over the frequencies in the opposite order (float64, pairwise: see _fsum).
`train` and `modulator_prior_init` put this objective through the driver of nagp.segp (its `evaluator` argument), the second with a
smoothing written out as a direct sum."""
import numpy as np

# name: (T, n_param, len, varx, vary)
CASES = {
    't4': (4, 3, 1.5, 1.0, 0.1),                 # even T, less than a wave
    't5': (5, 2, 1.2, 0.8, 0.1),                 # odd T: entry (T+1)/2 of the frequency list is +(T+1)/2
    't255': (255, 3, 6.0, 1.3, 0.2),             # the workgroup tail
    't256': (256, 1, 14.0, 1.0, 0.1),            # one workgroup exactly
    't257': (257, 2, 4.0, 2.0, 0.1),             # one frequency in the second workgroup
    't1998': (1998, 3, 35.0, 1.0, 0.05),
    't1999': (1999, 1, 12.0, 1.4, 0.1),
    'u4096': (4096, 3, 300.0, 1.0, 0.1),         # the spectrum underflows to 0 over most frequencies: S = vary there
    'u4097': (4097, 1, 800.0, 2.0, 0.1),
    's513': (513, 3, 0.3, 1.0, 0.01),            # a length-scale below the sampling interval: a nearly flat spectrum
    'b70001': (70001, 3, 90.0, 1.2, 0.1),        # 274 workgroups and an odd T: several runs of the finish order
}


def freqs(T):
    """getGPSESpec.m:18: [0:ceil(T/2), -floor(T/2)+1:-1]"""
    j = np.arange(T)
    return np.where(j <= -(-T // 2), j, j - T).astype(float)


def se_spec(ell, T):
    w = 2 * np.pi * freqs(T) / T
    c = np.sqrt(2 * np.pi * ell ** 2) * np.exp(-w ** 2 * ell ** 2 / 2)
    return w, c


def getGPSESpec(ell, T, nout=1):
    """[fftCov,dfftCov] = getGPSESpec(len,T): T x D, one column per length-scale"""
    ell = np.asarray(ell, float).reshape(-1)
    cols = [se_spec(l, T) for l in ell]
    fftCov = np.stack([c for _, c in cols], axis=1)
    if nout < 2:
        return fftCov
    return fftCov, np.stack([c * (1 / l - w ** 2 * l) for l, (w, c) in zip(ell, cols)], axis=1)


def case(name):
    """Seeded inputs of a fixture case: param holds the logs of the first n_param of (len, varx, vary), the others are given; specy =
    T times the model spectrum of perturbed parameters (1.3 len, 0.8 varx, 1.2 vary) times Exp(1) noise, as a periodogram would be."""
    T, n_param, ell, varx, vary = CASES[name]
    rng = np.random.default_rng(5100 + sorted(CASES).index(name))
    _, c = se_spec(1.3 * ell, T)
    specy = T * (0.8 * varx * c + 1.2 * vary) * rng.exponential(1.0, T)
    param = np.log(np.array([ell, varx, vary][:n_param]))
    return dict(T=T, n_param=n_param, param=param, specy=specy, vary=vary if n_param <= 2 else None, varx=varx if n_param == 1 else None)


def _fsum(x, reverse):
    """a sum over the frequencies in float64, from the first term or (reverse) from the last, by NumPy's pairwise summation.
    Over the frequencies where the spectrum has died away S = vary, so sum log S adds one constant thousands of times; with a single
    running float64 accumulator the rounding errors of those additions do not average out but repeat, in both orders alike (measured
    with np.cumsum against the 60-digit fixture: up to 1.1e-13 of Obj, on case b70001; tools/make_segp_fixture.py prints the figure of
    every case), which is more than the device's own distance from the 60-digit values.  Pairwise partial sums keep the yardstick's summation error below what it is
    used to measure, and the two orders still differ in their last bits."""
    x = np.ascontiguousarray(x[::-1] if reverse else x, dtype=float)
    return np.sum(x)


def obj(param, specy, vary=None, varx=None, reverse=False, grad=True):
    param = np.asarray(param, float).reshape(-1); specy = np.asarray(specy, float).reshape(-1)
    n_param = param.size; T = specy.size
    ell = np.exp(param[0])
    varx = np.exp(param[1]) if n_param >= 2 else float(varx)
    vary = np.exp(param[2]) if n_param >= 3 else float(vary)
    with np.errstate(all='ignore'):
        w, c = se_spec(ell, T)
        S = varx * c + vary
        Obj = (0.5 * _fsum(np.log(S), reverse) + 1 / (2 * T) * _fsum(specy / S, reverse)) / T
        if not grad:
            return Obj
        g = 1 / (2 * S) - 1 / (2 * T) * specy / S ** 2
        dc = c * (1 / ell - w ** 2 * ell)
        d = [_fsum(g * dc, reverse) * ell * varx, _fsum(g * c, reverse) * varx, _fsum(g, reverse) * vary]
    return Obj, np.array(d[:n_param]) / T


def objective(c, reverse=False, grad=True):
    """a case (or any dict with its keys) through the restatement"""
    return obj(c['param'], c['specy'], c['vary'], c['varx'], reverse=reverse, grad=grad)


def dist(a, ref):
    """the project's norm: max|a - ref| / max|ref|"""
    ref = np.asarray(ref, float)
    return float(np.max(np.abs(np.asarray(a, float) - ref)) / np.max(np.abs(ref)))


def evaluator(reverse=False):
    """the restatement as the `evaluator` of nagp.trainSEGP_RS"""
    def ev(param, specy, vary, varx):
        return obj(param, specy, vary, varx, reverse=reverse)
    return ev


def se_signal(T, ell, seed, noise_var=0.01):
    """a seeded draw of a unit-variance squared-exponential GP of length-scale ell on T regular samples (circulant embedding on 2T
    points, where the kernel has long died away) plus white noise of variance noise_var"""
    rng = np.random.default_rng(seed)
    n = 2 * T
    lag = np.minimum(np.arange(n), n - np.arange(n)).astype(float)
    lam = np.maximum(np.fft.fft(np.exp(-lag ** 2 / (2 * ell ** 2))).real, 0.0)
    z = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    x = np.fft.fft(np.sqrt(lam / n) * z).real[:T]
    return x + np.sqrt(noise_var) * rng.standard_normal(T)


def train(x, reverse=False, **kw):
    """trainSEGP_RS on the restatement objective -> (lenx, varx, info)"""
    import nagp
    return nagp.trainSEGP_RS(x, evaluator=evaluator(reverse), **kw)


def smooth(HEst):
    """train_model.m:137-146 with conv(.,.,'same') as the direct sum logHsm_t = sum_k filt_k u_(t-k), k = -100 .. 100, u = 0 outside"""
    H = np.asarray(HEst, float)
    T, N = H.shape
    k = np.arange(-100, 101)
    filt = np.log(1 + np.exp(-0.5 * k.astype(float) ** 2)); filt = filt / filt.sum()
    u = np.zeros((T + 200, N)); u[100:100 + T] = np.log(np.exp(H + 1e-8) - 1)
    sm = np.zeros((T, N))
    for kk, fk in zip(k, filt):
        sm += fk * u[100 - kk:100 - kk + T]
    return sm, sm.mean(axis=0)


def modulator_prior_init(HEst, reverse=False):
    """train_model.m:136-149 on the restatement objective -> (lenx_nmf, varx_nmf, mux, infos)"""
    sm, mux = smooth(HEst)
    fits = [train(sm[:, n] - mux[n], reverse=reverse) for n in range(sm.shape[1])]
    return np.array([f[0] for f in fits]), np.array([f[1] for f in fits]), mux, [f[2] for f in fits]
