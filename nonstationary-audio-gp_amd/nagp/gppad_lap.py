"""Host-side mirror of the Laplace step of GPPAD, experiments/gppad/GPModelFast/Laplace -- the error bars of the transformed envelope and the
approximate marginal likelihood that the time-scale is learnt with:

    [d,h] = GetHessian(x,y,Params,Dims)                        GetHessian.m
    b = SigDSigTimesV(v,d2py,d2pxhalf)                         SigDSigTimesV.m
    [xv,lmb] = LanczosGPPAD(d2pxhalf,d2py,vstart,epert,nev,jmax,tresh,tolconv)
    [xv,lmb] = GetEigSigDSig(d2px,d2py,Opts)                   GetEigSigDSig.m
    Varx = GetErrorBarGPPAD(x,y,Params,Dims,Opts)              GetErrorBarGPPAD.m
    Obj = GetLaplaceObjGPPADOneChunk(x,y,Params,Dims,Opts)     GetLaplaceObjGPPADOneChunk.m
    Obj = GetLaplaceObjGPPAD(y,Params,Opts)                    GetLaplaceObjGPPAD.m
    [Len,Objs,Info] = GetLaplaceObjGPPADMulti(Len,y,Params,Opts), [Objs,Lens] = GetLaplaceObjGPPADStitched(LenRng,NumLens,y,Params,Opts)
    [len,Info] = GetLenGradAscent(len,y,Params,Opts), [len,Info] = GetLenGridSearch(LenRng,y,Params,Opts)
    [a,x,Varx,Info] = InferAmplitudeErrorBarsGPMAP(y,Params,Opts)
    [A,X,C,Params,Info,Varx,Aupper,Alower] = FBGPMAPLearnLen(Y,len,Opts)

The Hessian, the operator, the Lanczos run with its selective reorthogonalisation, the Ritz vectors, Varx and the likelihood and prior
terms run on the GPU (nagp_gppad_lap_*, include/nagp.h); the Lanczos control is in the library, so one call is one batched eigen-solve.
There is no CPU fallback: `laplace=` exists so that the tests can put the float64 restatement through the same drivers, as `evaluator=`
does for the MAP step.

What differs from the .m files, said here once:
  1. Randomness is explicit.  GetEigSigDSig.m draws vstart = randn(n,1) from MATLAB's global stream, which cannot be reproduced; here
     `vstart=` gives the start vectors or `rng=` a numpy Generator that draws them (rng.standard_normal(Tx) per problem, in order).
  2. Where the .m stops in the debugger: a tridiagonal matrix that is not finite sets the problem's status, and GetEigSigDSig draws another
     vstart for it, three times at the most, then raises (with `vstart=` given it raises at once; so do the drivers above the one-chunk
     calls, which draw all their start vectors before they ask the device); Varx < 0 is counted in Info, without plots.
  3. The Lanczos vectors are kept real (the .m carries the imaginary rounding noise of ifft along and drops it with real(lmb)).
  4. The operator is given by the model (y, Params, Dims, x), not by arrays d2px, d2py: the spectrum is formed on the device from len.
     SigDSigTimesV, LanczosGPPAD and GetEigSigDSig therefore take a GppadLapHandle (or the arguments that make one).
All chunks of equal (T, Tx) go through one handle, the channels of FBGPMAPLearnLen run in lock-step; a problem's bits do not depend on its
batch mates."""
import builtins
import math

import numpy as np

from . import _lib as L
from ._drive import lock_step, run
from .gppad import InferAmplitudeGPMAP, InferAmplitudeGPMAP_many, PackDimsGPFast

TRESH, TOLCONV = 1e-12, 1e-8                # GetEigSigDSig.m:29-30
MAX_REDRAWS = 3


def LoadLearnLenGradAscentGPPADOpts(Opts=None):
    """the defaults of LoadLearnLenGradAscentGPPADOpts.m under the entries of Opts"""
    d = {'NumIts': 2000, 'nev': 100, 'tol': 8, 'MinLength': 8, 'TruncPoint': 8, 'NumItsLL': 30, 'loglenLR0': math.log(1.2), 'm': 0.5}
    d.update(Opts or {})
    return d


def LoadErrorBarsLapOpts(Opts=None):
    """the default of LoadErrorBarsLapOpts.m (Overlap = 5) on top of LoadLearnLenGradAscentGPPADOpts"""
    d = {'Overlap': 5}
    d.update(Opts or {})
    return LoadLearnLenGradAscentGPPADOpts(d)


def _rows(v, P, name):
    a = np.asarray(v, float).reshape(-1)
    if a.size == 1:
        a = np.full(P, a[0])
    if a.size != P:
        raise ValueError('%s holds one entry per problem (%d): got %d' % (name, P, a.size))
    return L.f64(a, 'C')


class GppadLapHandle:
    """The resident form (nagp_gppad_lap_create): y (P, T), vary (a scalar, (P,) or (P, T)), len, varx, mux, varc (scalars or (P,)) and the
    spectra stay on the device; hess(x) sets the MAP point (P, Tx), then apply / eig / varx / obj."""

    def __init__(self, y, Tx, vary, varx, mux, varc, len, jmax, device=0):
        import ctypes as C
        y = L.f64(np.atleast_2d(np.asarray(y, float)), 'C')
        self.P, self.T = y.shape; self.Tx = int(Tx); self.jmax = int(jmax)
        vy = np.asarray(vary, float)
        per_sample = vy.ndim == 2 or (vy.ndim == 1 and self.P == 1 and vy.size == self.T and self.T > 1)
        vy = L.f64(vy.reshape(self.P, self.T), 'C') if per_sample else _rows(vy, self.P, 'vary')
        h = C.c_void_p()
        L.check(L.lib().nagp_gppad_lap_create(C.byref(h), self.P, self.T, self.Tx, L.dptr(y), L.dptr(vy), self.T if per_sample else 0,
                                              L.dptr(_rows(len, self.P, 'len')), L.dptr(_rows(varx, self.P, 'varx')), L.dptr(_rows(mux, self.P, 'mux')),
                                              L.dptr(_rows(varc, self.P, 'varc')), self.jmax, int(device)))
        self._h = h

    def _live(self):
        if not self._h:
            raise L.NagpError('the handle is closed')
        return self._h

    def _vec(self, v):
        return L.f64(np.asarray(v, float).reshape(self.P, self.Tx), 'C')

    def hess(self, x, d=True):
        """sets the MAP point; returns d (P, T) of GetHessian.m when asked"""
        out = np.zeros((self.P, self.T)) if d else None
        L.check(L.lib().nagp_gppad_lap_hess(self._live(), L.dptr(self._vec(x)), L.dptr(out)))
        return out

    def apply(self, v):
        """A v of SigDSigTimesV.m, (P, Tx)"""
        out = np.zeros((self.P, self.Tx))
        L.check(L.lib().nagp_gppad_lap_apply(self._live(), L.dptr(self._vec(v)), L.dptr(out)))
        return out

    def eig(self, nev, vstart, tresh=TRESH, tolconv=TOLCONV, xv=False):
        """one batched LanczosGPPAD run.  Returns a dict: lmb (P, jmax) NaN beyond nconv, nconv, steps, reorths, status (P,), anorm (P,) and,
        with xv, xv (P, jmax, Tx) whose rows beyond nconv are zero"""
        import ctypes as C
        lmb = np.zeros((self.P, self.jmax)); nconv = np.zeros(self.P, np.int32); info = np.zeros((self.P, 3), np.int32); anorm = np.zeros(self.P)
        X = np.zeros((self.P, self.jmax, self.Tx)) if xv else None
        ip = lambda a: a.ctypes.data_as(L.c_ip)
        L.check(L.lib().nagp_gppad_lap_eig(self._live(), int(nev), float(tresh), float(tolconv), L.dptr(self._vec(vstart)), L.dptr(lmb), ip(nconv), ip(info),
                                           L.dptr(anorm), L.dptr(X)))
        out = dict(lmb=lmb, nconv=nconv.astype(int), steps=info[:, 0].astype(int), reorths=info[:, 1].astype(int), status=info[:, 2].astype(int), anorm=anorm)
        if xv:
            out['xv'] = X
        return out

    def varx(self, xv=None, lmb=None):
        """Varx (P, Tx) and the count of its negative entries (P,): of the last eig, or from given pairs xv (P, K, Tx), lmb (P, K)"""
        V = np.zeros((self.P, self.Tx)); neg = np.zeros(self.P, np.int64); K = 0
        if xv is not None:
            lmb = L.f64(np.asarray(lmb, float).reshape(self.P, -1), 'C'); K = lmb.shape[1]
            xv = L.f64(np.asarray(xv, float).reshape(self.P, K, self.Tx), 'C')
        L.check(L.lib().nagp_gppad_lap_varx(self._live(), K, L.dptr(xv), L.dptr(lmb), L.dptr(V), neg.ctypes.data_as(L.c_lp)))
        return V, neg

    def obj(self):
        """(P, 3): Obj0, Obj1, Obj2 of GetLaplaceObjGPPADOneChunk.m (Obj0 is NaN before an eig)"""
        O = np.zeros((self.P, 3))
        L.check(L.lib().nagp_gppad_lap_obj(self._live(), L.dptr(O)))
        return O

    def timings(self):
        ms = np.zeros(1)
        L.check(L.lib().nagp_gppad_lap_timings(L.dptr(ms)))
        return ms[0]

    def close(self):
        if self._h:
            L.lib().nagp_gppad_lap_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _handle_of(y, Params, Dims, jmax, device):
    T, Tx = int(Dims['T']), int(Dims['Tx'])
    y = np.asarray(y, float).reshape(1, T)
    vary = np.asarray(Params['vary'], float).reshape(-1)
    return GppadLapHandle(y, Tx, vary[0] if vary.size == 1 else vary[None, :], Params['varx'], Params['mux'], Params['varc'], Params['len'], jmax, device)


def GetHessian(x, y, Params, Dims, device=0):
    """[d,h] = GetHessian(x,y,Params,Dims): d (T,) on the device, h = GetFFTCovFast(len, Tx) varx (Tx,) on the host"""
    from .gppad import GetFFTCovFast
    with _handle_of(y, Params, Dims, 1, device) as h:
        d = h.hess(x)[0]
    return d, GetFFTCovFast(float(Params['len']), int(Dims['Tx'])) * float(Params['varx'])


def SigDSigTimesV(v, handle):
    """b = SigDSigTimesV(v,d2py,d2pxhalf) on a handle whose point is set (item 4 of the module docstring); v (Tx,) or (P, Tx)"""
    v = np.asarray(v, float)
    out = handle.apply(v)
    return out[0] if v.ndim == 1 else out


def LanczosGPPAD(handle, vstart, nev, tresh=TRESH, tolconv=TOLCONV):
    """[xv,lmb] = LanczosGPPAD(...) for every problem of the handle (jmax is the handle's): a list of (xv (Tx, nconv), lmb (nconv,)) and
    the dict of GppadLapHandle.eig"""
    r = handle.eig(nev, vstart, tresh, tolconv, xv=True)
    return [(r['xv'][p, :r['nconv'][p]].T.copy(), r['lmb'][p, :r['nconv'][p]].copy()) for p in range(handle.P)], r


def _starts(P, Tx, rng, vstart):
    if vstart is not None:
        return np.asarray(vstart, float).reshape(P, Tx)
    if rng is None:
        raise ValueError('give rng= (a numpy Generator) or vstart=: the start vectors of the Lanczos runs are not drawn from a hidden stream')
    return np.stack([rng.standard_normal(Tx) for _ in range(P)])


def GetEigSigDSig(handle, Opts, rng=None, vstart=None, xv=True):
    """[xv,lmb] = GetEigSigDSig(d2px,d2py,Opts) for every problem of a handle whose point is set: nev = Opts.nev, tresh = 1e-12,
    tolconv = 1e-8 (the handle's jmax is 2 nev in the drivers).  A problem whose run is not finite gets another vstart from rng,
    MAX_REDRAWS times at the most; then, or at once when vstart= was given, NagpError.  Returns the dict of GppadLapHandle.eig with
    'vstart' (the vectors every problem's returned run started from) and 'redraws'."""
    P, Tx = handle.P, handle.Tx
    v = _starts(P, Tx, rng, vstart)
    for redraw in range(MAX_REDRAWS + 1):
        r = handle.eig(int(Opts['nev']), v, xv=xv)
        bad = np.flatnonzero(r['status'] != 0)
        if bad.size == 0:
            r['vstart'] = v; r['redraws'] = redraw
            return r
        if vstart is not None or redraw == MAX_REDRAWS:
            raise L.NagpError('GetEigSigDSig: the Lanczos run of problem(s) %s is not finite (status %s)' % (bad.tolist(), r['status'][bad].tolist()))
        v = v.copy()
        for p in bad:
            v[p] = rng.standard_normal(Tx)
        # the problems that were fine run again with their vstart: their bits do not depend on their batch mates


def _device_laplace(device):
    """laplace(chunks, nev, rng, vstart) -> one dict per chunk (lmb, Varx, Obj (3,), steps, reorths, nconv, n_negative, vstart) for
    chunks (dicts with x, y, Params, Dims) of equal (T, Tx): one handle, one batched eigen-solve"""
    def solve(chunks, nev, rng, vstart):
        T, Tx = int(chunks[0]['Dims']['T']), int(chunks[0]['Dims']['Tx'])
        per_sample = any(np.size(c['Params']['vary']) > 1 for c in chunks)
        vary = np.stack([np.broadcast_to(np.asarray(c['Params']['vary'], float).reshape(-1), (T,)) for c in chunks]) if per_sample \
            else np.array([float(np.asarray(c['Params']['vary']).reshape(-1)[0]) for c in chunks])
        col = lambda k: np.array([float(c['Params'][k]) for c in chunks])
        with GppadLapHandle(np.stack([np.asarray(c['y'], float).reshape(-1) for c in chunks]), Tx, vary, col('varx'), col('mux'), col('varc'), col('len'),
                            2 * int(nev), device) as h:
            h.hess(np.stack([c['x'] for c in chunks]), d=False)
            r = GetEigSigDSig(h, {'nev': nev}, rng=rng, vstart=vstart, xv=False)
            V, neg = h.varx(); O = h.obj()
        return [dict(lmb=r['lmb'][p, :r['nconv'][p]].copy(), Varx=V[p], Obj=O[p], steps=int(r['steps'][p]), reorths=int(r['reorths'][p]),
                     nconv=int(r['nconv'][p]), n_negative=int(neg[p]), vstart=r['vstart'][p]) for p in range(len(chunks))]
    return solve


def _solve_chunks(chunks, nev, rng, vstart, laplace, device, record):
    """every chunk through the Laplace step, the chunks of equal (T, Tx) together; vstart: None or one vector per chunk.  The start
    vectors are drawn chunk by chunk in order, whatever the grouping."""
    solve = laplace or _device_laplace(device)
    if vstart is None:
        if rng is None:
            raise ValueError('give rng= (a numpy Generator) or vstart=')
        vstart_all = [rng.standard_normal(int(c['Dims']['Tx'])) for c in chunks]
        given = False
    else:
        vstart_all = [np.asarray(v, float).reshape(-1) for v in vstart]; given = True
    groups = {}
    for i, c in enumerate(chunks):
        groups.setdefault((int(c['Dims']['T']), int(c['Dims']['Tx'])), []).append(i)
    out = [None] * len(chunks)
    for key, idx in groups.items():
        res = _solve_with(solve, [chunks[i] for i in idx], nev, np.stack([vstart_all[i] for i in idx]), None if given else rng)
        for i, r in zip(idx, res):
            out[i] = r
            if record is not None:
                record.append((chunks[i], r))
    return out


def _solve_with(solve, chunks, nev, v, rng):
    """solve with given start vectors; a status failure with an rng at hand redraws inside GetEigSigDSig (device) or in the injected solver"""
    try:
        return solve(chunks, nev, None, v)
    except L.NagpError:
        if rng is None:
            raise
        return solve(chunks, nev, rng, None)


def GetErrorBarGPPAD(x, y, Params, Dims, Opts, rng=None, vstart=None, laplace=None, device=0, info=None):
    """Varx = GetErrorBarGPPAD(x,y,Params,Dims,Opts): the Laplace error bars (Tx,) of one chunk.  info: a dict that receives lmb, steps,
    reorths, nconv, n_negative and vstart."""
    c = dict(x=np.asarray(x, float).reshape(-1), y=np.asarray(y, float).reshape(-1), Params=Params, Dims=Dims)
    r = _solve_chunks([c], int(Opts['nev']), rng, None if vstart is None else [vstart], laplace, device, None)[0]
    if info is not None:
        info.update({k: r[k] for k in ('lmb', 'steps', 'reorths', 'nconv', 'n_negative', 'vstart')})
    return r['Varx']


def GetLaplaceObjGPPADOneChunk(x, y, Params, Dims, Opts, rng=None, vstart=None, laplace=None, device=0, info=None):
    """Obj = GetLaplaceObjGPPADOneChunk(x,y,Params,Dims,Opts) = Obj0 + Obj1 + Obj2; info receives the three terms as 'Obj' and the run's counts"""
    c = dict(x=np.asarray(x, float).reshape(-1), y=np.asarray(y, float).reshape(-1), Params=Params, Dims=Dims)
    r = _solve_chunks([c], int(Opts['nev']), rng, None if vstart is None else [vstart], laplace, device, None)[0]
    if info is not None:
        info.update({k: r[k] for k in ('Obj', 'lmb', 'steps', 'reorths', 'nconv', 'vstart')})
    return float(r['Obj'][0] + r['Obj'][1] + r['Obj'][2])


def _map_chunks(ys, Params, Opts, evaluator, device):
    """InferAmplitudeGPMAP with Long = 1 on every chunk: in lock-step on the device, one by one through an evaluator"""
    if evaluator is None:
        return InferAmplitudeGPMAP_many(ys, Params, Opts, device=device)
    return [InferAmplitudeGPMAP(y, P, Opts, evaluator=evaluator) for y, P in zip(ys, Params)]


def _chunk_params(Params, first, last):
    """Params of the samples [first, last) of a signal: a per-sample vary is cut with it"""
    P = dict(Params)
    vary = np.asarray(Params['vary'], float).reshape(-1)
    P['vary'] = vary[first:last].copy() if vary.size > 1 else float(vary[0])
    return P


def chunk_plan(T, len, Opts):
    """the chunks of InferAmplitudeErrorBarsGPMAP.m:41-84: TxCh, TCh, Overlap, NumChunks, the (tstart, tend) of every chunk (0-based,
    end exclusive) and the three windows"""
    TxCh = int(math.floor(2 * math.pi * Opts['nev'] * len / Opts['TruncPoint']))
    TxCh = 2 ** int(math.floor(math.log2(TxCh)))
    TCh = TxCh - int(math.ceil(len * Opts['tol']))
    Overlap = int(math.ceil(len * Opts['Overlap']))
    if TCh <= 0:
        raise ValueError('the observed chunk length TCh = %d is not positive: reduce tol or TruncPoint, or increase nev' % TCh)
    if 2 * Overlap > TCh:
        raise ValueError('Overlap = %d against the chunk length TCh = %d: reduce Overlap or TruncPoint, or increase nev' % (Overlap, TCh))
    NumChunks = int(math.ceil(T / (TCh - Overlap)))
    Taper = np.cos(2 * np.pi * np.arange(1, Overlap + 1) / (4 * Overlap)) ** 2
    bounds = [(ch * (TCh - Overlap), min(ch * (TCh - Overlap) + TCh, T)) for ch in range(NumChunks)]
    return dict(TxCh=TxCh, TCh=TCh, Overlap=Overlap, NumChunks=NumChunks, bounds=bounds,
                WindowStart=np.concatenate([np.ones(TCh - Overlap), Taper]),
                Window=np.concatenate([Taper[::-1], np.ones(TCh - 2 * Overlap), Taper]),
                WindowEnd=np.concatenate([Taper[::-1], np.ones(TCh - Overlap)]))


# The drivers are generators (as those of gppad.py and gppad_cas.py): they do the bookkeeping of the .m files and draw from their own
# stream, and they yield the device work as requests --
#     ('solve', ys, Params, OptsMAP, Tx, nev, vstarts) -> (chunks, results): the MAP step (Long = 1) and the Laplace step of every chunk
#     ('map', y, Params, Opts) -> (a, x, Info) of InferAmplitudeGPMAP
# -- so that several channels can run in lock-step (_drive.lock_step): the requests of a round whose options agree are one MAP call and one
# Laplace handle per (T, Tx).  A problem's bits do not depend on its batch mates, so a channel's results are those of the channel alone.
def _draw(rng, vstart, n, Tx):
    if vstart is not None:
        v = [np.asarray(q, float).reshape(-1) for q in vstart]
        if len(v) != n or any(q.size != Tx for q in v):
            raise ValueError('vstart holds one start vector of Tx = %d entries per problem (%d)' % (Tx, n))
        return v
    if rng is None:
        raise ValueError('give rng= (a numpy Generator) or vstart=: the start vectors of the Lanczos runs are not drawn from a hidden stream')
    return [rng.standard_normal(Tx) for _ in range(n)]


def _key(req):
    return ('solve', tuple(sorted(req[3].items())), req[5]) if req[0] == 'solve' else ('map', tuple(sorted((k, v) for k, v in req[3].items() if np.ndim(v) == 0)))


def _issuer(evaluator, laplace, device, record):
    """issue(requests) -> one answer per request, for requests of one _key"""
    def issue(reqs):
        if reqs[0][0] == 'map':
            if evaluator is None:
                return InferAmplitudeGPMAP_many([r[1] for r in reqs], [r[2] for r in reqs], reqs[0][3], device=device)
            return [InferAmplitudeGPMAP(r[1], r[2], r[3], evaluator=evaluator) for r in reqs]
        ys = [y for r in reqs for y in r[1]]; Ps = [P for r in reqs for P in r[2]]; vs = [v for r in reqs for v in r[6]]
        maps = _map_chunks(ys, Ps, reqs[0][3], evaluator, device)
        chunks = [dict(x=m[1], y=yc, Params=P, Dims=PackDimsGPFast(yc.size, r[4])) for m, yc, P, r in zip(maps, ys, Ps, [r for r in reqs for _ in r[1]])]
        res = _solve_chunks(chunks, int(reqs[0][5]), None, vs, laplace, device, record)
        out = []; at = 0
        for r in reqs:
            out.append((chunks[at:at + len(r[1])], res[at:at + len(r[1])])); at += len(r[1])
        return out
    return issue


def _run(gen, evaluator, laplace, device, record):
    issue = _issuer(evaluator, laplace, device, record)
    return run(gen, lambda req: issue([req])[0])


def errorbar_steps(y, Params, Opts, rng, vstart):
    """InferAmplitudeErrorBarsGPMAP as a generator: one 'solve' request for all chunks; returns (a, x, Varx, Info)"""
    Opts = LoadErrorBarsLapOpts(Opts)
    y = np.asarray(y, float).reshape(-1); T = y.size
    plan = chunk_plan(T, float(Params['len']), Opts)
    OptsCur = {'Tx': plan['TxCh'], 'MinLength': Opts['MinLength'], 'NumIts': Opts['NumIts'], 'Long': 1}
    ys = [y[a:b] for a, b in plan['bounds']]
    Ps = [_chunk_params(Params, a, b) for a, b in plan['bounds']]
    chunks, res = yield ('solve', ys, Ps, OptsCur, plan['TxCh'], int(Opts['nev']), _draw(rng, vstart, len(ys), plan['TxCh']))
    x = np.zeros(T); Varx = np.zeros(T); N = plan['NumChunks']
    Borders = np.zeros(N)
    for ch, ((a, b), c, r) in enumerate(zip(plan['bounds'], chunks, res)):
        n = b - a
        W = np.ones(n) if N == 1 else (plan['WindowStart'] if ch == 0 else (plan['WindowEnd'] if ch == N - 1 else plan['Window']))[:n]
        Varx[a:b] += r['Varx'][:n] * W
        x[a:b] += c['x'][:n] * W
        Borders[ch] = b - plan['Overlap'] / 2.0
    Info = {'Borders': Borders, 'TxCh': plan['TxCh'], 'TCh': plan['TCh'], 'Overlap': plan['Overlap'], 'NumChunks': N}
    for k in ('steps', 'reorths', 'nconv', 'n_negative'):
        Info[k] = np.array([r[k] for r in res])
    return np.log(1 + np.exp(x)), x, Varx, Info


def InferAmplitudeErrorBarsGPMAP(y, Params, Opts=None, rng=None, vstart=None, evaluator=None, laplace=None, device=0, record=None):
    """[a,x,Varx,Info] = InferAmplitudeErrorBarsGPMAP(y,Params,Opts): the MAP envelope and its Laplace error bars for a long signal, chunk
    by chunk with cos^2 windows over the overlaps.  The MAP step of all chunks is one InferAmplitudeGPMAP_many call, the Laplace step one
    handle per (T, Tx) (the shorter last chunk has its own).  vstart: one start vector (TxCh,) per chunk, or rng, which draws them chunk by
    chunk before the device is asked (a run that is not finite raises; GetEigSigDSig is the place that redraws).  The last chunk by the .m's
    count is windowed as the .m windows it.  Info: Borders, TxCh, TCh, Overlap, NumChunks and per chunk steps, reorths, nconv, n_negative.
    record: a list that receives (chunk, result) of every Laplace solve."""
    return _run(errorbar_steps(y, Params, Opts, rng, vstart), evaluator, laplace, device, record)


def _sum_obj(res):
    Obj = 0.0
    for r in res:
        Obj = Obj + float(r['Obj'][0] + r['Obj'][1] + r['Obj'][2])
    return Obj


def laplace_obj_steps(y, Params, Opts, rng, vstart, info=None):
    """GetLaplaceObjGPPAD as a generator"""
    y = np.asarray(y, float).reshape(-1); T = y.size
    TCh, TxCh = int(Opts['TCh']), int(Opts['TxCh'])
    N = int(math.ceil(T / TCh))
    bounds = [(ch * TCh, min(T, (ch + 1) * TCh)) for ch in range(N)]
    OptsCur = {k: Opts[k] for k in ('NumIts', 'MinLength', 'DSLength') if k in Opts}
    OptsCur['Long'] = 1; OptsCur['Tx'] = TxCh
    ys = [y[a:b] for a, b in bounds]
    Ps = [_chunk_params(Params, a, b) for a, b in bounds]
    chunks, res = yield ('solve', ys, Ps, OptsCur, TxCh, int(Opts['nev']), _draw(rng, vstart, N, TxCh))
    if info is not None:
        info.update(Obj=np.stack([r['Obj'] for r in res]), NumChunks=N, steps=np.array([r['steps'] for r in res]), nconv=np.array([r['nconv'] for r in res]))
    return _sum_obj(res)


def GetLaplaceObjGPPAD(y, Params, Opts, rng=None, vstart=None, evaluator=None, laplace=None, device=0, record=None, info=None):
    """Obj = GetLaplaceObjGPPAD(y,Params,Opts): the signal in chunks of Opts.TCh samples (transforms of Opts.TxCh), every chunk an
    independent data set; the sum of the chunks' Laplace objectives, added in chunk order.  info receives the chunks' terms ('Obj',
    NumChunks x 3) and counts."""
    return _run(laplace_obj_steps(y, Params, Opts, rng, vstart, info), evaluator, laplace, device, record)


# ---------------------------------------------------------------------------------------------------------------- learning the time-scale
def multi_steps(Len, y, Params, Opts, rng, vstart):
    """GetLaplaceObjGPPADMulti as a generator: one 'solve' request for the chunks of all time-scales"""
    from .gppad import GetTx
    Len = np.asarray(Len, float).reshape(-1); y = np.asarray(y, float).reshape(-1); T = y.size
    TxMax = 2 ** int(math.ceil(math.log2(2 * math.pi * Len.min() * Opts['nev'] / Opts['TruncPoint'])))
    TCh = int(math.floor(TxMax - Opts['tol'] * Len.min()))
    TxCh = GetTx(TCh, Len.max() * Opts['tol'])
    N = int(math.ceil(T / TCh))
    bounds = [(ch * TCh, min(T, (ch + 1) * TCh)) for ch in range(N)]
    OptsCur = {k: Opts[k] for k in ('NumIts', 'MinLength') if k in Opts}
    OptsCur.update(Long=1, Tx=TxCh, DSLength=float(Len.min()))
    ys = [y[a:b] for _ in Len for a, b in bounds]
    Ps = []
    for ell in Len:
        for a, b in bounds:
            P = _chunk_params(Params, a, b); P['len'] = float(ell)
            Ps.append(P)
    chunks, res = yield ('solve', ys, Ps, OptsCur, TxCh, int(Opts['nev']), _draw(rng, vstart, len(ys), TxCh))
    Objs = np.array([_sum_obj(res[l * N:(l + 1) * N]) for l in range(Len.size)])
    pos = int(np.argmax(Objs))
    return Len, Objs, {'TCh': TCh, 'TxCh': TxCh, 'MaxLoc': -1 if pos == 0 else (1 if pos == Len.size - 1 else 0), 'NumChunks': N}


def GetLaplaceObjGPPADMulti(Len, y, Params, Opts, rng=None, vstart=None, evaluator=None, laplace=None, device=0, record=None):
    """[Len,Objs,Info] = GetLaplaceObjGPPADMulti(Len,y,Params,Opts): the Laplace objective at several time-scales on the same chunks
    (TCh from min(Len), TxCh = GetTx(TCh, max(Len) tol), the resolutions of the MAP step from DSLength = min(Len)).  The chunks of all
    time-scales go through one MAP call and one Laplace handle per (T, Tx); the start vectors are drawn time-scale by time-scale, chunk by
    chunk, as the .m's loop would draw them.  Info: TCh, TxCh, MaxLoc (-1, 0, 1: the largest value is the first, an inner, the last)."""
    return _run(multi_steps(Len, y, Params, Opts, rng, vstart), evaluator, laplace, device, record)


def _multi(multi, Len, y, Params, Opts, rng):
    """a step of the searches: the hand-made `multi` of the tests at once, GetLaplaceObjGPPADMulti as requests"""
    if multi is not None:
        return multi(Len, y, Params, Opts)
    return (yield from multi_steps(Len, y, Params, Opts, rng, None))


def stitched_steps(LenRng, NumLens, y, Params, Opts, rng, multi=None):
    """GetLaplaceObjGPPADStitched as a generator"""
    alpha = 3.0
    if NumLens is None:
        NumLens = int(math.ceil((math.log(LenRng[1]) - math.log(LenRng[0])) / math.log(alpha))) + 1
    logLens = np.linspace(math.log(LenRng[0]), math.log(LenRng[1]), int(NumLens))
    Lens = np.exp(logLens)
    if NumLens < 2 or logLens[1] - logLens[0] > math.log(alpha):
        raise ValueError('GetLaplaceObjGPPADStitched: the separation between the points is too great: reduce LenRng or increase NumLens')
    NumPerSeg = int(np.sum(logLens < logLens[0] + math.log(alpha)))
    if NumPerSeg < 2:
        raise ValueError('GetLaplaceObjGPPADStitched: a segment must hold two time-scales: increase NumLens')
    NumSeg = int(math.ceil((NumLens - 1) / (NumPerSeg - 1)))
    Objs = np.full(int(NumLens), np.nan)
    for s in range(NumSeg):
        s0 = s * (NumPerSeg - 1); s1 = min(s0 + NumPerSeg, int(NumLens))
        _, cur, _ = yield from _multi(multi, Lens[s0:s1], y, Params, Opts, rng)
        if s == 0:
            Objs[s0:s1] = cur
        else:
            Objs[s0 + 1:s1] = cur[1:] - (cur[0] - Objs[s0])
    return Objs, Lens


def GetLaplaceObjGPPADStitched(LenRng, NumLens, y, Params, Opts, rng=None, multi=None, evaluator=None, laplace=None, device=0, record=None):
    """[Objs,Lens] = GetLaplaceObjGPPADStitched(LenRng,NumLens,y,Params,Opts): the objective on a logarithmic grid of time-scales, in
    segments that span less than a factor alpha = 3 (within one segment the chunks agree); neighbouring segments share one time-scale, and
    a segment is shifted so that it agrees with its predecessor there.  multi(Len, y, Params, Opts) -> (Len, Objs, Info) stands for
    GetLaplaceObjGPPADMulti (the tests put a hand-made objective there)."""
    return _run(stitched_steps(LenRng, NumLens, y, Params, Opts, rng, multi), evaluator, laplace, device, record)


def gridsearch_steps(LenRng, y, Params, Opts, rng, multi=None):
    """GetLenGridSearch as a generator"""
    Objs, Lens = yield from stitched_steps(LenRng, Opts.get('NumLens'), y, Params, Opts, rng, multi)
    pos = int(np.argmax(Objs)); K = Objs.size
    LenMax = [Lens[0]] if Objs[0] > Objs[1] else []
    LenMax += [Lens[k] for k in range(1, K - 1) if Objs[k] > Objs[k - 1] and Objs[k] > Objs[k + 1]]
    if Objs[K - 1] > Objs[K - 2]:
        LenMax.append(Lens[K - 1])
    return float(Lens[pos]), {'Objs': Objs, 'Lens': Lens, 'LenMax': np.array(LenMax), 'AtEdge': pos in (0, K - 1)}


def GetLenGridSearch(LenRng, y, Params, Opts, rng=None, multi=None, evaluator=None, laplace=None, device=0, record=None):
    """[len,Info] = GetLenGridSearch(LenRng,y,Params,Opts): the time-scale of the largest stitched objective; Info: Objs, Lens, LenMax (the
    local optima of the grid, the ends included) and AtEdge"""
    return _run(gridsearch_steps(LenRng, y, Params, Opts, rng, multi), evaluator, laplace, device, record)


def gradascent_steps(len, y, Params, Opts, rng, tstart=None, multi=None):
    """GetLenGradAscent as a generator"""
    y = np.asarray(y, float).reshape(-1); T = y.size
    N = int(Opts['NumItsLL']); len = float(len)
    loglenLR = Opts['loglenLR0'] / (1 + np.arange(N + 1) / (N / 2.0))
    LastUp = 0.0
    Info = {'LenHist': np.zeros(N), 'ObjHist': np.zeros(N), 'dObjHist': np.zeros(N), 'Ts': np.zeros((N, 2), int), 'loglenLR': loglenLR}
    for it in range(N):
        TxMax = 2 ** int(math.ceil(math.log2(2 * math.pi * len * Opts['nev'] / Opts['TruncPoint'])))
        TMax = int(math.floor(TxMax - Opts['tol'] * len))
        if TMax < T:
            if tstart is not None:
                t0 = int(tstart[it])
            elif rng is not None:
                t0 = 1 + int(math.floor(rng.random() * (T - TMax)))
            else:
                raise ValueError('give rng= (a numpy Generator) or tstart=: the stretches are not drawn from a hidden stream')
            t1 = t0 - 1 + TMax
        else:
            t0, t1 = 1, T
        P = _chunk_params(Params, t0 - 1, t1)
        Len, Objs, _ = yield from _multi(multi, np.array([len, max(len + 1, len * 1.01)]), y[t0 - 1:t1], P, Opts, rng)
        if 'mulen' in Params:
            Objs = Objs - (Len - Params['mulen']) ** 2 / (2 * Params['varlen'])
        dObj = float(Objs[1] - Objs[0])
        dloglen = float(np.sign(dObj)) * loglenLR[it] + Opts['m'] * LastUp
        LastUp = dloglen
        len = math.exp(math.log(len) + dloglen)
        Info['LenHist'][it] = len; Info['ObjHist'][it] = Objs[0]; Info['dObjHist'][it] = dObj; Info['Ts'][it] = (t0, t1)
    return len, Info


def GetLenGradAscent(len, y, Params, Opts, rng=None, tstart=None, multi=None, evaluator=None, laplace=None, device=0, record=None):
    """[len,Info] = GetLenGradAscent(len,y,Params,Opts): NumItsLL steps of sign ascent with momentum on log len.  Every step takes a stretch
    of TMax samples at a uniformly drawn place (tstart= gives the places, 1-based as Info.Ts holds them, or rng draws them with
    rng.random() before the step's start vectors), evaluates the Laplace objective at len and at max(len + 1, 1.01 len), subtracts the
    prior (len - mulen)^2 / (2 varlen) when Params has mulen, and moves log len by sign(dObj) loglenLR(it) + m LastUp.  Info: LenHist,
    ObjHist, dObjHist, Ts, loglenLR.  multi: as in GetLaplaceObjGPPADStitched."""
    return _run(gradascent_steps(len, y, Params, Opts, rng, tstart, multi), evaluator, laplace, device, record)


def channel_steps(y, len, given, Opts, bars, rng):
    """one channel of FBGPMAPLearnLen as a generator; given: None, or (varc, varx, mux, vary) that are then not learnt"""
    from .gppad import LearnMarginalParams, PackParamsGP
    if given is None:
        varc, varx, mux, I1 = LearnMarginalParams(y, Opts)
        vary = 1e-6
    else:
        (varc, varx, mux, vary), I1 = given, None
    P = PackParamsGP(varx, float(len), mux, varc, vary)
    I2 = None
    if Opts.get('LearnLengths') == 1:
        P['len'], I2 = yield from gradascent_steps(len, y, P, Opts, rng)
    elif Opts.get('LearnLengths') == 2:
        P['len'], I2 = yield from gridsearch_steps(Opts['LenRngCur'], y, P, Opts, rng)
    if bars:
        a, x, vx, I3 = yield from errorbar_steps(y, P, Opts, rng, None)
    else:
        a, x, I3 = yield ('map', y, P, {k: Opts[k] for k in ('NumIts', 'MinLength', 'tol')})
        vx = None
    return a, x, vx, P, (I1, I2, I3)


def FBGPMAPLearnLen(Y, len, Opts=None, nout=5, rng=None, evaluator=None, laplace=None, device=0, record=None):
    """[A,X,C,Params,Info,Varx,Aupper,Alower] = FBGPMAPLearnLen(Y,len,Opts): GPPAD down the columns of Y (T x D) with the time-scale learnt
    (Opts.LearnLengths = 1: GetLenGradAscent from len; 2: GetLenGridSearch over Opts.LenRng, (2,) or (D, 2); anything else: len as given)
    and, with nout = 8 (nargout), the Laplace error bars Varx and the envelopes at x +- 3 sqrt(Varx).  len: a time-scale, one per channel,
    or a dict of parameters (len, varx, varc, mux, vary) that are then not learnt.  vary defaults to 1e-6.  Info[d] =
    (LearnMarginalParams' Info, the time-scale search's, the inference's).
    The channels run in lock-step: the requests of a round whose options agree share one MAP call and one Laplace handle per (T, Tx).
    rng: a Generator, from which one child stream per channel is spawned (rng.spawn(D)), or the list of the channels' Generators: a
    channel's results are bit-equal to FBGPMAPLearnLen on that column alone with its child stream."""
    Opts = LoadErrorBarsLapOpts(Opts); bars = nout == 8
    Y = np.asarray(Y, float)
    if Y.ndim == 1:
        Y = Y[:, None]
    T, D = Y.shape
    given = isinstance(len, dict)
    Pin = dict(len) if given else {}
    lens = np.broadcast_to(np.asarray(Pin['len'] if given else len, float).reshape(-1), (D,)).copy()
    vary = np.asarray(Pin.get('vary', 1e-6), float)                                                  # (1 or T) x D; the .m's default is 1e-6 ones(T,D)
    vary = vary.reshape(-1, 1) if vary.ndim < 2 else vary
    if vary.shape[1] < D:
        vary = vary[:, :1] @ np.ones((1, D))
    per = lambda k, d: float(np.broadcast_to(np.asarray(Pin[k], float).reshape(-1), (D,))[d])
    rngs = list(rng) if isinstance(rng, (list, tuple)) else (rng.spawn(D) if rng is not None else [None] * D)
    if builtins.len(rngs) != D:
        raise ValueError('rng is a Generator or holds one Generator per channel (%d)' % D)
    gens = []
    for d in range(D):
        O = dict(Opts)
        if Opts.get('LearnLengths') == 2:
            R = np.asarray(Opts['LenRng'], float)
            O['LenRngCur'] = R[d] if R.ndim > 1 and R.shape[0] > 1 else R.reshape(-1)
        vy = vary[:, d]
        g = (per('varc', d), per('varx', d), per('mux', d), vy if vy.size > 1 else float(vy[0])) if given else None
        gens.append(channel_steps(Y[:, d], lens[d], g, O, bars, rngs[d]))
    res = lock_step(gens, _key, _issuer(evaluator, laplace, device, record))
    A = np.zeros((T, D)); X = np.zeros((T, D)); C = np.zeros((T, D)); Varx = np.zeros((T, D)); Au = np.zeros((T, D)); Al = np.zeros((T, D))
    Params = {'len': lens, 'varx': np.zeros(D), 'varc': np.zeros(D), 'mux': np.zeros(D), 'vary': vary}
    Info = []
    for d, (a, x, vx, P, I) in enumerate(res):
        s = math.sqrt(P['varc'])
        A[:, d] = s * a; X[:, d] = x; C[:, d] = Y[:, d] / A[:, d]
        if bars:
            Varx[:, d] = vx
            Au[:, d] = s * np.log(1 + np.exp(x + 3 * np.sqrt(vx))); Al[:, d] = s * np.log(1 + np.exp(x - 3 * np.sqrt(vx)))
        Params['varc'][d] = P['varc']; Params['varx'][d] = P['varx']; Params['mux'][d] = P['mux']; Params['len'][d] = P['len']
        Info.append(I)
    return (A, X, C, Params, Info, Varx, Au, Al) if bars else (A, X, C, Params, Info)
