"""NumPy float64 restatement of the GPPAD envelope objective, experiments/gppad/GPModelFast/GetGPObjFast.m, written from the formulae of
include/nagp.h (nagp_gppad_obj):

    a = GetAmp(x_t), s = 1/(1+exp(-x_t)), v_t = a^2 varc + vary_t + 1e-5 (t < T), xe = x - mux, c = fftCov,
    ObjA = sum_t 1/2 log v_t + 1/2 y_t^2 / v_t,  dA_t = s a / v_t (1 - y_t^2 / v_t) varc,
    u = real(ifft(fft(xe) ./ c)),  ObjB = (u' xe) / (2 varx),  Obj = ObjA + ObjB,  dObj = u / varx (+ dA on the first T entries).

The 60-digit fixture (tools/make_gppad_fixture.py -> tests/golden/gppad_multiprecision.npz) is what this file and the device are measured
against (tests/test_gppad_host.py, tests/test_gppad_gpu.py).  `reverse` forms every sum in the opposite order: the two sums of the
objective from their last term (float64, pairwise, as tests/segp_ref.py), and both transforms on the index-reversed sequence
z_n = x_(-n mod Tx), whose transform is the index-reversed transform of x, so that the FFT library meets every term at another place of its
butterflies.  `evaluator` puts this objective through the drivers of nagp.gppad."""
import numpy as np

# name: (T, Tx, x, specials, len, vary, cov)
#   x: 'smooth' -- a circular squared-exponential draw of the prior, mux + sqrt(varx) g; 'white' -- independent normal entries (ObjB of the order of 1e8)
#   specials: entries of x set to 800, 501, -31, -40 (the branches of GetAmp.m and their neighbours)
#   len: None stands for Tx / 8, where c runs into its 1e-6 floor
#   vary: 0.0 or a scalar, or 'gap' -- per sample, zero but for a block of 1e3; cov: 'given' (fftCov passed) or 'len' (formed from len)
CASES = {
    'c2_2': (2, 2, 'white', False, 0.5, 0.0, 'len'),                     # no padding, the smallest transform
    'c3_8': (3, 8, 'smooth', False, None, 0.1, 'given'),
    'c50_64': (50, 64, 'white', True, 0.7, 'gap', 'len'),
    'c64_64': (64, 64, 'smooth', False, None, 0.0, 'given'),
    'c257_1024': (257, 1024, 'smooth', False, 20.0, 0.0, 'len'),          # T one past a 256 boundary
    'c657_1024': (657, 1024, 'white', True, None, 'gap', 'given'),
    'c3000_4096': (3000, 4096, 'smooth', False, 100.0, 0.05, 'len'),      # the largest transform held in LDS
    'c4095_4096': (4095, 4096, 'white', False, 0.6, 0.0, 'given'),
    'c5000_8192': (5000, 8192, 'smooth', False, None, 'gap', 'len'),      # the smallest four-step transform, 2 x 4096
    'c20000_32768': (20000, 32768, 'white', True, 150.0, 0.0, 'given'),   # 8 x 4096
}
VARX, MUX, VARC = 1.7, -0.4, 0.6


def GetAmp(x):
    x = np.asarray(x, float)
    with np.errstate(over='ignore'):
        a = np.log(1 + np.exp(x))
    return np.where(x > 500, x, np.where(x < -30, np.exp(np.minimum(x, 0.0)), a))


def freqs(Tx):
    """GetFFTCovFast.m:12: [0:floor(Tx/2), -floor(Tx/2)+1:-1]"""
    k = np.arange(Tx)
    return np.where(k <= Tx // 2, k, k - Tx).astype(float)


def fft_cov(ell, Tx):
    """GetFFTCovFast.m:10-16"""
    w = 2 * np.pi * freqs(Tx) / Tx
    return np.sqrt(2 * np.pi * ell ** 2) * np.exp(-w ** 2 * ell ** 2 / 2) + 1e-6


def se_draw(rng, ell, Tx):
    """a circular unit-variance squared-exponential draw of Tx points"""
    c = fft_cov(ell, Tx) - 1e-6
    z = rng.standard_normal(Tx)
    return np.fft.ifft(np.sqrt(c) * np.fft.fft(z)).real


def case(name):
    """Seeded inputs of a fixture case"""
    T, Tx, kind, specials, ell, vary, cov = CASES[name]
    rng = np.random.default_rng(6200 + sorted(CASES).index(name))
    ell = Tx / 8.0 if ell is None else ell
    x = MUX + np.sqrt(VARX) * se_draw(rng, max(ell, 1.0), Tx) if kind == 'smooth' else MUX + 2.0 * rng.standard_normal(Tx)
    if specials:
        x[[1, T // 3, T // 2, T - 2]] = [800.0, 501.0, -31.0, -40.0]
    with np.errstate(over='ignore'):
        y = GetAmp(np.minimum(x[:T], 20.0)) * np.sqrt(VARC) * rng.standard_normal(T)
    if vary == 'gap':
        vy = np.zeros(T); vy[T // 4:T // 4 + max(2, T // 10)] = 1e3
    else:
        vy = float(vary)
    return dict(T=T, Tx=Tx, x=x, y=y, vary=vy, len=ell, varx=VARX, mux=MUX, varc=VARC, given=cov == 'given', fftCov=fft_cov(ell, Tx))


def _fsum(x, reverse):
    """a sum in float64 from the first term or (reverse) from the last, by NumPy's pairwise summation (see tests/segp_ref.py)"""
    return np.sum(np.ascontiguousarray(x[::-1] if reverse else x, dtype=float))


def _flip(z):
    """z_(-n mod N)"""
    return np.concatenate([z[:1], z[:0:-1]])


def obj(x, y, fftCov, varx, mux, varc, vary, reverse=False, grad=True):
    x = np.asarray(x, float).reshape(-1); y = np.asarray(y, float).reshape(-1); c = np.asarray(fftCov, float).reshape(-1)
    T = y.size
    xt = x[:T]
    with np.errstate(over='ignore'):
        a = GetAmp(xt); s = 1.0 / (1.0 + np.exp(-xt))
    v = a * a * varc + (np.asarray(vary, float) + 1e-5)
    r = y * y / v
    ObjA = _fsum(0.5 * np.log(v) + 0.5 * r, reverse)
    xe = x - mux
    if reverse:
        u = _flip(np.fft.ifft(np.fft.fft(_flip(xe)) / _flip(c)).real)
    else:
        u = np.fft.ifft(np.fft.fft(xe) / c).real
    Obj = ObjA + 1.0 / (2.0 * varx) * _fsum(u * xe, reverse)
    if not grad:
        return Obj
    d = u / varx
    d[:T] += s * a / v * (1.0 - r) * varc
    return Obj, d


def obj_ext(x, y, ell, varx, mux, varc, vary):
    """The objective and gradient in extended precision (np.longdouble, 64-bit mantissa; scipy.fft transforms in the precision of its
    input), the spectrum formed from len in that precision as well: the reference of the GPU tests where no 60-digit value is stored
    (the sweep over every size, the replay of a device run).  Returns float64 roundings."""
    import scipy.fft as sf
    LD = np.longdouble
    assert np.finfo(LD).eps < 1e-18, 'np.longdouble is no wider than float64 on this machine'
    x = np.asarray(x, float).reshape(-1).astype(LD); y = np.asarray(y, float).reshape(-1).astype(LD)
    T = y.size; Tx = x.size
    varx, mux, varc, ell = LD(varx), LD(mux), LD(varc), LD(ell)
    pi = LD('3.14159265358979323846264338327950288')
    w = 2 * pi * freqs(Tx).astype(LD) / Tx
    c = np.sqrt(2 * pi * ell ** 2) * np.exp(-w ** 2 * ell ** 2 / 2) + LD('1e-6')
    xt = x[:T]
    with np.errstate(over='ignore'):
        a = np.where(xt > 500, xt, np.where(xt < -30, np.exp(np.minimum(xt, LD(0))), np.log(1 + np.exp(xt))))
        s = 1 / (1 + np.exp(-xt))
    v = a * a * varc + (np.asarray(vary, float).astype(LD) + LD('1e-5'))
    r = y * y / v
    xe = x - mux
    u = sf.ifft(sf.fft(xe.astype(np.clongdouble)) / c).real
    Obj = np.sum(np.log(v) / 2 + r / 2) + np.sum(u * xe) / (2 * varx)
    d = u / varx
    d[:T] += s * a / v * (1 - r) * varc
    return float(Obj), d.astype(float)


def objective(c, reverse=False, grad=True):
    """a case (or any dict with its keys) through the restatement"""
    return obj(c['x'], c['y'], c['fftCov'], c['varx'], c['mux'], c['varc'], c['vary'], reverse=reverse, grad=grad)


def dist(a, ref):
    """the project's norm: max|a - ref| / max|ref|"""
    ref = np.asarray(ref, float)
    return float(np.max(np.abs(np.asarray(a, float) - ref)) / np.max(np.abs(ref)))


def evaluator(reverse=False, record=None):
    """the restatement as the `evaluator` of nagp.InferAmplitudeGPMAP, nagp.MAPGPFast and nagp.GPPAD: evaluator(y, Params, Dims) -> f(x).
    record: a list that receives (y, Params, Dims, x, Obj, dObj) of every evaluation."""
    def open_level(y, Params, Dims):
        c = fft_cov(float(Params['len']), Dims['Tx'])

        def f(x):
            out = obj(x, y, c, Params['varx'], Params['mux'], Params['varc'], Params['vary'], reverse=reverse)
            if record is not None:
                record.append((y, Params, Dims, np.array(x), out[0], out[1]))
            return out
        return f
    return open_level


def envelope_signal(T, ell, seed, varx=1.0, mux=0.0, varc=1.0):
    """a drawn envelope times white noise: (y, a) with a = sqrt(varc) log(1 + exp(x)), x a squared-exponential draw of length-scale ell"""
    rng = np.random.default_rng(seed)
    n = 2
    while n < 2 * T:
        n *= 2
    x = mux + np.sqrt(varx) * se_draw(rng, ell, n)[:T]
    a = np.sqrt(varc) * np.log(1 + np.exp(x))
    return a * rng.standard_normal(T), a
