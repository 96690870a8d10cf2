"""NumPy float64 restatement of the Laplace step of GPPAD, experiments/gppad/GPModelFast/Laplace (GetHessian.m, SigDSigTimesV.m,
LanczosGPPAD.m, GetEigSigDSig.m, GetErrorBarGPPAD.m, GetLaplaceObjGPPADOneChunk.m), written from the formulae of include/nagp.h
(nagp_gppad_lap_create):

    d_t = (c2 a + s^2)/v (1 - y^2/v) varc - s a/v^2 (1 - y^2/v) varc dv + s a/v y^2/v^2 varc dv,   hs = sqrt(c varx),
    A v = ifft(hs .* fft([d .* a(1:T); 0])),  a = ifft(hs .* fft(v)),   Varx = varx - sum_k |ifft(hs .* fft(xv_k))|^2 l_k/(l_k + 1),
    Obj0 = -1/2 sum log|1 + l|,  Obj1 = -1/2 sum_t (log v + y^2/v),  Obj2 = -(u' xe)/(2 varx).

The parts without decisions are pinned to the 60-digit fixture (tools/make_gppad_lap_fixture.py -> tests/golden/gppad_lap_multiprecision.npz)
in tests/test_gppad_lap_host.py; `reverse` forms every sum from its last term and every transform on the index-reversed sequence, as
tests/gppad_ref.py does, and ext=True evaluates in np.longdouble (the reference where no 60-digit value is stored).  The Lanczos run is
LanczosGPPAD.m statement by statement (indices 1-based as there) with the vectors kept real, as the device keeps them; `perturb`
multiplies every operator product by 1 + 1e-15 g, g standard normal, which stands in for another FFT's rounding."""
import numpy as np

import gppad_ref as g1
from gppad_ref import GetAmp, _flip, _fsum, dist, fft_cov, freqs, se_draw  # noqa: F401

EPS = np.finfo(float).eps
VARX, MUX, VARC = 1.3, -0.2, 0.7
LD = np.longdouble

# the parts without decisions.  name: (T, Tx, len, vary, specials)
#   vary: a scalar, or 'gap' -- per sample, zero but for a block of 2.0;  specials: entries of x at 800, 501, -31, -40 (the branches of GetAmp)
FIXED = {
    'f20_32': (20, 32, 2.0, 0.0, False),
    'f50_64': (50, 64, 3.0, 'gap', True),
    'f200_256': (200, 256, 10.0, 0.05, False),
    'f256_256': (256, 256, 6.0, 'gap', True),
}
LMB_GIVEN = np.array([2.5, 0.7, 0.0, -0.3])             # the pairs of the Varx and Obj0 entries of the fixture: a zero and a negative value

# the Lanczos run as a whole.  name: (T, Tx, nev, jmax, len, seed); len = None stands for 8 Tx / (2 pi nev), the reference's own chunk rule
STABLE = {
    's20_32': (20, 32, 4, 8, None, 1),                  # idle threads
    's200_256': (200, 256, 8, 16, None, 1),
    's333_512': (333, 512, 8, 16, None, 1),             # a leading radix-2 pass
    's3000_4096': (3000, 4096, 16, 32, None, 1),        # the largest single-workgroup transform, T no multiple of 64
    's4096_4096': (4096, 4096, 16, 32, None, 2),        # T = Tx
    's5000_8192': (5000, 8192, 16, 32, None, 1),        # four-step, N1 = 2
    's11111_16384': (11111, 16384, 24, 48, None, 1),    # N1 = 4
    's200_256_short': (200, 256, 8, 16, 1.5, 3),        # len far below the rule: the run ends at jmax
    's200_256_j2': (200, 256, 1, 2, 1.5, 3),            # jmax = 2: nconv = 0
}
TRESH, TOLCONV = 1e-12, 1e-8


def fixed_case(name):
    T, Tx, ell, vary, specials = FIXED[name]
    rng = np.random.default_rng(4300 + sorted(FIXED).index(name))
    x = MUX + np.sqrt(VARX) * se_draw(rng, ell, Tx)
    if specials:
        x[[1, T // 3, T // 2, T - 2]] = [800.0, 501.0, -31.0, -40.0]
    y = GetAmp(np.minimum(x[:T], 20.0)) * np.sqrt(VARC) * rng.standard_normal(T)
    if vary == 'gap':
        vy = np.zeros(T); vy[T // 4:T // 4 + max(2, T // 10)] = 2.0
    else:
        vy = float(vary)
    K = LMB_GIVEN.size
    return dict(T=T, Tx=Tx, x=x, y=y, vary=vy, len=ell, varx=VARX, mux=MUX, varc=VARC, v=rng.standard_normal(Tx),
                xv=rng.standard_normal((K, Tx)) / np.sqrt(Tx), lmb=LMB_GIVEN.copy())


def stable_case(name):
    T, Tx, nev, jmax, ell, seed = STABLE[name]
    rng = np.random.default_rng(4400 + 16 * sorted(STABLE).index(name) + seed)
    ell = 8.0 * Tx / (2 * np.pi * nev) if ell is None else ell
    x = MUX + np.sqrt(VARX) * se_draw(rng, ell, Tx)
    y = GetAmp(x[:T]) * np.sqrt(VARC) * rng.standard_normal(T)
    return dict(T=T, Tx=Tx, nev=nev, jmax=jmax, x=x, y=y, vary=0.01, len=ell, varx=VARX, mux=MUX, varc=VARC, vstart=rng.standard_normal(Tx))


# ---------------------------------------------------------------------------------------------------------------- the parts without decisions
def _f(ext):
    return LD if ext else float


def _fft(z, ext):
    if not ext:
        return np.fft.fft(z)
    import scipy.fft as sf
    assert np.finfo(LD).eps < 1e-18, 'np.longdouble is no wider than float64 on this machine'
    return sf.fft(np.asarray(z).astype(np.clongdouble))


def _ifft(z, ext):
    if not ext:
        return np.fft.ifft(z)
    import scipy.fft as sf
    return sf.ifft(np.asarray(z).astype(np.clongdouble))


def amp(x):
    """GetAmp.m in the precision of x"""
    with np.errstate(over='ignore'):
        return np.where(x > 500, x, np.where(x < -30, np.exp(np.minimum(x, 0 * x)), np.log(1 + np.exp(x))))


def hessian(x, y, varc, vary, ext=False):
    """d of GetHessian.m:28-40"""
    F = _f(ext)
    y = np.asarray(y, float).reshape(-1).astype(F); T = y.size
    xt = np.asarray(x, float).reshape(-1)[:T].astype(F)
    varc = F(varc); vy = np.asarray(vary, float).astype(F) + F('1e-5' if ext else 1e-5)
    with np.errstate(over='ignore'):
        a = amp(xt); s = 1 / (1 + np.exp(-xt)); c2 = F(1) / 4 / np.cosh(xt / 2) ** 2
    v = a ** 2 * varc + vy; dv = 2 * varc * a * s
    w = 1 - y ** 2 / v
    d = (c2 * a + s ** 2) / v * w * varc - s * a / v ** 2 * w * varc * dv + s * a / v * y ** 2 / v ** 2 * varc * dv
    return d if ext else np.asarray(d, float)


def spectrum(ell, Tx, ext=False):
    if not ext:
        return fft_cov(ell, Tx)
    pi = LD('3.14159265358979323846264338327950288'); ell = LD(ell)
    w = 2 * pi * freqs(Tx).astype(LD) / Tx
    return np.sqrt(2 * pi * ell ** 2) * np.exp(-w ** 2 * ell ** 2 / 2) + LD('1e-6')


def hhalf(ell, Tx, varx, ext=False):
    """h^(1/2) of GetHessian.m:46 and GetEigSigDSig.m:24"""
    return np.sqrt(spectrum(ell, Tx, ext) * _f(ext)(varx))


def sandwich(v, hs, reverse=False, ext=False):
    """real(ifft(hs .* fft(v)))"""
    if reverse:
        return _flip(_ifft(_flip(hs) * _fft(_flip(v), ext), ext).real)
    return _ifft(hs * _fft(v, ext), ext).real


def apply(v, d, hs, reverse=False, ext=False):
    """SigDSigTimesV.m with the real part kept after either half"""
    a = sandwich(v, hs, reverse, ext)
    b = np.zeros(hs.size, dtype=a.dtype)
    b[:d.size] = d * a[:d.size]
    return sandwich(b, hs, reverse, ext)


def dense(d, hs):
    """A as a matrix (Tx x Tx), symmetrised"""
    n = hs.size
    A = np.stack([apply(e, d, hs) for e in np.eye(n)], axis=1)
    return 0.5 * (A + A.T)


def varx_from(xv, lmb, hs, varx, reverse=False, ext=False):
    """GetErrorBarGPPAD.m:11-20, xv (K, Tx); a NaN lmb skips its pair"""
    F = _f(ext)
    V = np.full(hs.size, F(varx))
    ks = range(len(lmb))
    for k in (reversed(ks) if reverse else ks):
        if lmb[k] != lmb[k]:
            continue
        l = F(max(lmb[k], 0.0))
        b = sandwich(np.asarray(xv[k]).astype(F), hs, reverse, ext)
        V = V - b ** 2 * l / (l + 1)
    return V if ext else np.asarray(V, float)


def obj_terms(x, y, ell, varx, mux, varc, vary, lmb, reverse=False, ext=False):
    """(Obj0, Obj1, Obj2) of GetLaplaceObjGPPADOneChunk.m"""
    F = _f(ext)
    x = np.asarray(x, float).reshape(-1).astype(F); y = np.asarray(y, float).reshape(-1).astype(F); T = y.size
    l = np.maximum(np.asarray([q for q in lmb if q == q], float), 0.0).astype(F)
    sm = (lambda z: np.sum(z)) if ext else (lambda z: _fsum(z, reverse))
    Obj0 = -sm(np.log(np.abs(1 + l))) / 2 if l.size else F(0)
    a = amp(x[:T])
    v = a ** 2 * F(varc) + (np.asarray(vary, float).astype(F) + F('1e-5' if ext else 1e-5))
    Obj1 = -sm(np.log(v) + y ** 2 / v) / 2
    xe = x - F(mux); c = spectrum(ell, x.size, ext)
    u = _flip(_ifft(_fft(_flip(xe), ext) / _flip(c), ext).real) if reverse else _ifft(_fft(xe, ext) / c, ext).real
    Obj2 = -sm(u * xe) / (2 * F(varx))
    return np.array([Obj0, Obj1, Obj2], dtype=F)


# ---------------------------------------------------------------------------------------------------------------- LanczosGPPAD.m
def _dot(a, b, reverse):
    return _fsum(a * b, reverse)


def _gram_schmidt(Q, vj, rr, reverse):
    """h1 = Q' [v_j r], [v_j r] -= Q h1 (classical: every product from the vectors as they came in)"""
    idx = range(len(Q))
    h1 = np.array([[_dot(Q[i], vj, reverse), _dot(Q[i], rr, reverse)] for i in idx])
    for i in (reversed(idx) if reverse else idx):
        vj = vj - Q[i] * h1[i, 0]; rr = rr - Q[i] * h1[i, 1]
    return vj, rr, h1


def lanczos(d, hs, vstart, nev, jmax, tresh=TRESH, tolconv=TOLCONV, reverse=False, perturb=None):
    """[xv,lmb] = LanczosGPPAD(d2pxhalf,d2py,vstart,epert,nev,jmax,tresh,tolconv) with what GetEigSigDSig.m does around it.  Returns a dict:
    lmb (nconv,) descending, xv (nconv, Tx), steps, reorths, nconv, anorm, status (0 fine, 1 a tridiagonal entry that is not finite)"""
    n = hs.size
    reps = 10 * np.sqrt(EPS)
    al = np.zeros(jmax + 4); be = np.zeros(jmax + 4)
    wjm1 = np.zeros(jmax + 4); wj = np.zeros(jmax + 4); wjp1 = np.zeros(jmax + 4)
    wj[2] = wj[3] = EPS
    V = np.zeros((jmax + 1, n))                                   # row j: v_j (1-based)
    r = np.asarray(vstart, float).copy()
    be[1] = np.sqrt(_dot(r, r, reverse))
    flagreort = False; nconv = 0; reorths = 0; anorm = 0.0; status = 0
    convd = np.zeros(0, bool); ev = np.zeros(0); s = np.zeros((0, 0))
    j = 0
    with np.errstate(all='ignore'):
        while j < jmax:
            j += 1
            V[j] = r / be[j]
            r = apply(V[j], d, hs, reverse)
            if perturb is not None:
                r = r * (1 + 1e-15 * perturb.standard_normal(n))
            if j > 1:
                r = r - V[j - 1] * be[j]
            al[j] = _dot(r, V[j], reverse)
            r = r - V[j] * al[j]
            be[j + 1] = np.sqrt(_dot(r, r, reverse))
            anorm = abs(al[1] + be[2]) if j == 1 else max(anorm, be[j] + abs(al[j]) + be[j + 1])
            epert = anorm * EPS
            wjp1[1] = 0.0
            jv = np.arange(2, j + 1)
            w = be[jv] * wj[jv + 1] + (al[jv - 1] - al[j]) * wj[jv] + be[jv - 1] * wj[jv - 1] - be[j] * wjm1[jv]
            wjp1[jv] = (w + np.sign(w) * epert) / be[j + 1]
            wjp1[j + 1] = epert / be[j + 1]
            wjp1[j + 2] = EPS
            m = np.abs(wjp1[1:j + 3]); m = m[m == m]                  # max() skips NaN
            if m.size and m.max() > tresh:
                flagreort = True; reorths += 1
                vj, rr = V[j].copy(), r
                if j > 1:
                    vj, rr, h1 = _gram_schmidt(V[1:j], vj, rr, reverse)
                    if np.linalg.norm(h1, 2) > reps:
                        vj, rr, _ = _gram_schmidt(V[1:j], vj, rr, reverse)
                r = rr - vj * _dot(vj, rr, reverse)
                V[j] = vj
                wjp1[2:j + 2] = EPS
                wj[2:j + 1] = EPS
            wjm1 = wj.copy(); wj = wjp1.copy()
            if flagreort or j == jmax or be[j + 1] < epert:
                Tm = np.diag(al[1:j + 1]) + np.diag(be[2:j + 1], 1) + np.diag(be[2:j + 1], -1)
                if not np.all(np.isfinite(Tm)):
                    status = 1; nconv = 0; convd = np.zeros(j, bool)
                    break
                ev, s = np.linalg.eigh(Tm)
                convd = np.abs(be[j + 1] * s[j - 1]) < tolconv * anorm
                nconv = int(convd.sum())
                flagreort = False
            if be[j + 1] < epert or nconv >= nev:
                break
    if status or nconv == 0:
        return dict(lmb=np.zeros(0), xv=np.zeros((0, n)), steps=j, reorths=reorths, nconv=0, anorm=anorm, status=status)
    ic = np.flatnonzero(convd)
    ic = ic[np.argsort(-ev[ic], kind='stable')]
    return dict(lmb=ev[ic].copy(), xv=(V[1:j + 1].T @ s[:, ic]).T.copy(), steps=j, reorths=reorths, nconv=nconv, anorm=anorm, status=0)


def solve(c, reverse=False, perturb=None):
    """a stable case through GetHessian, the Lanczos run and GetErrorBarGPPAD: the run's dict with d, hs and Varx added"""
    d = hessian(c['x'], c['y'], c['varc'], c['vary']); hs = hhalf(c['len'], c['Tx'], c['varx'])
    out = lanczos(d, hs, c['vstart'], c['nev'], c['jmax'], reverse=reverse, perturb=perturb)
    out.update(d=d, hs=hs, Varx=varx_from(out['xv'], out['lmb'], hs, c['varx'], reverse))
    return out


def counts(run):
    return run['steps'], run['reorths'], run['nconv']


def residuals(run, d, hs):
    """|A xv_k - lmb_k xv_k| for every returned pair, A applied by this file"""
    return np.array([np.linalg.norm(apply(v, d, hs) - l * v) for v, l in zip(run['xv'], run['lmb'])])


def laplace(reverse=False):
    """the restatement as the `laplace` of the drivers of nagp.gppad_lap: solve(chunks, nev, rng, vstart) -> one dict per chunk"""
    def solve(chunks, nev, rng, vstart):
        out = []
        for i, c in enumerate(chunks):
            P = c['Params']; Tx = int(c['Dims']['Tx'])
            v = np.asarray(vstart[i], float) if vstart is not None else rng.standard_normal(Tx)
            d = hessian(c['x'], c['y'], P['varc'], P['vary']); hs = hhalf(float(P['len']), Tx, P['varx'])
            run = lanczos(d, hs, v, nev, 2 * nev, reverse=reverse)
            V = varx_from(run['xv'], run['lmb'], hs, P['varx'], reverse)
            O = obj_terms(c['x'], c['y'], float(P['len']), P['varx'], P['mux'], P['varc'], P['vary'], run['lmb'], reverse)
            out.append(dict(lmb=run['lmb'], Varx=V, Obj=O, steps=run['steps'], reorths=run['reorths'], nconv=run['nconv'], n_negative=int(np.sum(V < 0)), vstart=v))
        return out
    return solve
