"""NumPy float64 restatement of the GPPAD cascade objective, experiments/gppad/Cascade/GetObjCasGPFAST.m, written from the formulae of
include/nagp.h (nagp_gppad_cas_obj).  One cascade: X (M, Tx) -- row m is column m of the .m's X --, y (T), spectra c (M, Tx), varx, mux (M),
varc:

    A_tm = amp(X_mt) (t < T),  P_t = prod_m A_tm,  ObjA = sum_t sum_m log A_tm + (sum_t 1/2 (y_t / P_t)^2) / varc,
    D_t = 1 - y_t^2 / (varc P_t^2),  u_m = real(ifft(fft(X_m - mux_m) ./ c_m)),  ObjB = sum_m (u_m' (X_m - mux_m)) / (2 varx_m),
    dObj_mt = u_mt / varx_m + (t < T ? s_mt / A_tm D_t : 0),  Obj = ObjA + ObjB.

The 60-digit fixture (tools/make_gppad_cas_fixture.py -> tests/golden/gppad_cas_multiprecision.npz) is what this file and the device are
measured against (tests/test_gppad_cas_host.py, tests/test_gppad_cas_gpu.py).  `reverse` forms every sum and the product in the opposite
order -- the sums over t from their last term (float64, pairwise, as tests/gppad_ref.py), the columns from the last one, both transforms
on the index-reversed sequence.  `evaluator` puts this objective (and, for the levels, that of tests/gppad_ref.py) through the drivers of
nagp.gppad_cas."""
import numpy as np

import gppad_ref as g1
from gppad_ref import GetAmp, _flip, _fsum, dist, fft_cov, freqs, se_draw  # noqa: F401

# name: (M, T, Tx, lens, cov, specials)
#   lens: None stands for a geometric ladder from max(0.7, Tx / 64) to Tx / 8 (the last spectrum runs into its 1e-6 floor)
#   cov: 'given' (fftCovs passed) or 'len' (formed from len);  specials: entries of x at -35, 0 and 600 and one y_t = 0
CASES = {
    'k1_1_2': (1, 1, 2, [0.5], 'len', False),                            # the minimum
    'k2_64_64': (2, 64, 64, None, 'len', False),                         # no padding
    'k3_40_64': (3, 40, 64, None, 'len', False),                         # padding; one wave
    'k8_100_128': (8, 100, 128, None, 'len', False),                     # the M limit
    'k2_3000_4096': (2, 3000, 4096, [12.0, 300.0], 'len', False),        # the last LDS size
    'k3_5000_8192': (3, 5000, 8192, [7.5, 125.0, 600.0], 'len', False),  # the first four-step size, N1 = 2
    'k3_200_256': (3, 200, 256, [2.0, 16.0, 64.0], 'given', False),      # spectra given per column
    'k2_100_128': (2, 100, 128, [0.3, 0.5], 'len', True),                # the amp branches (short length-scales: c stays within 0.3 .. 1.3, so
}                                                                        # that the entries at 600 do not bury the likelihood under ObjB)
VARC = 0.8


def ladder(M, Tx):
    lo, hi = max(0.7, Tx / 64.0), Tx / 8.0
    return [lo] if M == 1 else [lo * (hi / lo) ** (m / (M - 1.0)) for m in range(M)]


def case(name):
    """Seeded inputs of a fixture case"""
    M, T, Tx, lens, cov, specials = CASES[name]
    rng = np.random.default_rng(9100 + sorted(CASES).index(name))
    lens = np.array(ladder(M, Tx) if lens is None else lens, float)
    varx = 1.2 - 0.1 * np.arange(M); mux = 0.5 - 0.15 * np.arange(M)
    X = np.stack([mux[m] + np.sqrt(varx[m]) * se_draw(rng, max(lens[m], 1.0), Tx) for m in range(M)])
    if specials:
        X[0, 5] = -35.0; X[1, 17] = 0.0; X[0, 40] = 600.0; X[1, 41] = 600.0
    with np.errstate(over='ignore'):
        y = np.prod(GetAmp(np.clip(X[:, :T], -20.0, 20.0)), axis=0) * np.sqrt(VARC) * rng.standard_normal(T)
    if specials:
        y[5] = 0.0                                           # P_5 of the order of 1e-16 (x = -35): with y_5 = 0 the sample's terms stay of the order of the rest
    return dict(M=M, T=T, Tx=Tx, x=X, y=y, len=lens, varx=varx, mux=mux, varc=VARC, given=cov == 'given',
                fftCovs=np.stack([fft_cov(ell, Tx) for ell in lens]))


def obj(X, y, fftCovs, varx, mux, varc, reverse=False, grad=True):
    X = np.asarray(X, float); y = np.asarray(y, float).reshape(-1); c = np.asarray(fftCovs, float)
    M, Tx = X.shape; T = y.size
    varx = np.broadcast_to(np.asarray(varx, float).reshape(-1), (M,)); mux = np.broadcast_to(np.asarray(mux, float).reshape(-1), (M,))
    order = range(M - 1, -1, -1) if reverse else range(M)
    with np.errstate(over='ignore', divide='ignore', invalid='ignore'):
        A = GetAmp(X[:, :T]); S = 1.0 / (1.0 + np.exp(-X[:, :T]))
        P = np.ones(T); la = np.zeros(T)
        for m in order:
            P = P * A[m]; la = la + np.log(A[m])
        r = y / P
        ObjA = _fsum(la, reverse) + _fsum(0.5 * (r * r), reverse) / varc
        D = 1.0 - y * y / (varc * (P * P))
        ObjB = 0.0
        d = np.zeros((M, Tx))
        for m in order:
            xe = X[m] - mux[m]
            if reverse:
                u = _flip(np.fft.ifft(np.fft.fft(_flip(xe)) / _flip(c[m])).real)
            else:
                u = np.fft.ifft(np.fft.fft(xe) / c[m]).real
            ObjB = ObjB + _fsum(u * xe, reverse) / (2.0 * varx[m])
            d[m] = u / varx[m]
            d[m, :T] += S[m] / A[m] * D
    Obj = ObjA + ObjB
    return (Obj, d) if grad else Obj


def obj_ext(X, y, lens, varx, mux, varc):
    """The objective and gradient in extended precision (np.longdouble through scipy.fft, as gppad_ref.obj_ext), the spectra formed from the
    length-scales in that precision: the reference where no 60-digit value is stored.  Returns float64 roundings."""
    import scipy.fft as sf
    LD = np.longdouble
    assert np.finfo(LD).eps < 1e-18, 'np.longdouble is no wider than float64 on this machine'
    X = np.asarray(X, float).astype(LD); y = np.asarray(y, float).reshape(-1).astype(LD)
    M, Tx = X.shape; T = y.size
    lens = np.broadcast_to(np.asarray(lens, float).reshape(-1), (M,)); varx = np.broadcast_to(np.asarray(varx, float).reshape(-1), (M,))
    mux = np.broadcast_to(np.asarray(mux, float).reshape(-1), (M,)); varc = LD(varc)
    pi = LD('3.14159265358979323846264338327950288')
    w = 2 * pi * freqs(Tx).astype(LD) / Tx
    with np.errstate(over='ignore', divide='ignore', invalid='ignore'):
        xt = X[:, :T]
        A = np.where(xt > 500, xt, np.where(xt < -30, np.exp(np.minimum(xt, LD(0))), np.log(1 + np.exp(xt))))
        S = 1 / (1 + np.exp(-xt))
        P = np.prod(A, axis=0)
        Obj = np.sum(np.log(A)) + np.sum((y / P) ** 2 / 2) / varc
        D = 1 - y * y / (varc * P * P)
        d = np.zeros((M, Tx), LD)
        for m in range(M):
            ell = LD(lens[m])
            c = np.sqrt(2 * pi * ell ** 2) * np.exp(-w ** 2 * ell ** 2 / 2) + LD('1e-6')
            xe = X[m] - LD(mux[m])
            u = sf.ifft(sf.fft(xe.astype(np.clongdouble)) / c).real
            Obj = Obj + np.sum(u * xe) / (2 * LD(varx[m]))
            d[m] = u / LD(varx[m])
            d[m, :T] += S[m] / A[m] * D
    return float(Obj), d.astype(float)


def objective(c, reverse=False, grad=True):
    """a case (or any dict with its keys) through the restatement"""
    return obj(c['x'], c['y'], c['fftCovs'], c['varx'], c['mux'], c['varc'], reverse=reverse, grad=grad)


def evaluator(reverse=False, record=None):
    """the restatement as the `evaluator` of nagp.CasGPMAP, nagp.FBCasGPMAP and nagp.MAPGPCasFast: evaluator(y, Params, Dims) -> f(x).  Dims
    with M: the joint objective on x = X(:); without: a level of FBGPMAP, served by gppad_ref.evaluator.  record: a list that receives
    (y, Params, Dims, x, Obj, dObj) of every evaluation of the joint objective."""
    level = g1.evaluator(reverse=reverse)

    def open_(y, Params, Dims):
        if 'M' not in Dims:
            return level(y, Params, Dims)
        M, Tx = Dims['M'], Dims['Tx']
        c = np.stack([fft_cov(float(ell), Tx) for ell in np.asarray(Params['len'], float).reshape(-1)])

        def f(x):
            O, d = obj(np.asarray(x, float).reshape(M, Tx), y, c, Params['varx'], Params['mux'], Params['varc'], reverse=reverse)
            if record is not None:
                record.append((y, Params, Dims, np.array(x), O, d.reshape(-1)))
            return O, d.reshape(-1)
        return f
    return open_
