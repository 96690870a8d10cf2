"""NumPy float64 restatement of the squared-exponential basis-function NMF of the reference's NMF toolbox: basis2SEGP.m,
getObj_fitSE_basis_func.m, getObj_nmf_log_norm.m (learning form) and getObj_nmf_log_norm_inf.m (inference form), written from the formulae
of include/nagp.h (nagp_sebf_conv, nagp_sebf_fit_obj, nagp_tnmf_obj):

    tau = ceil(lenx / sqrt(2) * tol),  bh = sqrt(varx sqrt(2) / (lenx sqrt(pi))),  bas(s) = bh exp(-1 / lenx^2 * s^2),  s = -tau .. tau
    conv(Z)(t) = sum_s bas(s) Z(t - s), Z = 0 outside 1 .. T;   fit: dx = conv(z) - x, obj = (1/2 sum dx^2 + 1/2 sum z^2) / T,
    dobj = (conv(dx) + z) / T;   H(:, k) = exp(conv(X(:, k)) + mux(k)), Ahat = H W + vary, obj1 = sum(A ./ Ahat + log Ahat),
    dA = (Ahat - A) ./ Ahat.^2, dX(:, k) = conv((dA W')(:, k) .* H(:, k)), dW = H' dA, dWW = dW .* W, dlogw = dWW - diag(sum(dWW,2)) W,
    obj = (obj1 + 1/2 sum X^2) / T, dobj = [dX(:) + X(:); dlogw(:)] / T.

The multi-precision fixture (tools/make_tnmf_fixture.py -> tests/golden/tnmf_multiprecision.npz) is what this file and the device are
measured against (tests/test_tnmf_host.py, tests/test_tnmf_gpu.py).  `reverse` forms every sum over t and over the taps in the opposite
order.  The case table, the seeded inputs of a case, the project's distance, the evaluator of the drivers and the planted data of the
driver tests live here as well."""
import numpy as np

TILE, CHUNK = 2048, 512                      # SEBF_TT and SEBF_C of csrc/nagp_sebf_check.hpp: outputs of a workgroup, taps of a chunk


def lenx_for(tau, tol=1.0):
    """a length scale whose tau = ceil(lenx / sqrt(2) * tol) is the given one"""
    return (tau - 0.5) * np.sqrt(2) / tol


# name: (T, D, K, lenx, mux, varx, tol, vary given)
CASES = {
    'r20': (20, 3, 2, [3, 45], [1, 2], [.1, .3], 9, True),                       # test_getObj_nmf_log_norm.m:13-27: tau = 20 and 287, both beyond T
    't1': (1, 1, 1, [2.0], [0.5], [.2], 9, True),
    't2': (2, 1, 1, [0.7], [-0.5], [.4], 9, True),
    'w257': (257, 4, 3, [1, 12.5, 40.2], [0, 1, -1], [.1, .5, 1.0], 9, True),     # tau = 7, 80, 256
    'm513': (513, 5, 2, [33, 0.5], [.3, -.2], [.6, .05], 11, True),              # tau = 257, 4
    'b1999': (1999, 7, 3, [5, 50, 100], [0, -.5, .5], [.5, 1.0, .25], 11, True),  # tau = 39, 389, 778: the batch case
    'lim70': (70, 64, 16, list(np.linspace(1, 30, 16)), list(np.linspace(-1, 1, 16)), list(np.linspace(.05, 1, 16)), 9, True),   # the limits of D and K
    'tol0': (300, 2, 2, [10, 3], [0, .2], [.5, .3], 0, True),                    # tau = 0: a single tap
    'novary': (257, 3, 2, [4, 20], [.1, -.1], [.3, .6], 9, False),               # vary = []
    # T and tau one below, at and one above the tile length; tau and the tap count 2 tau + 1 around the chunk length
    'e2047': (TILE - 1, 2, 3, [lenx_for(CHUNK - 1), lenx_for(CHUNK), lenx_for(CHUNK + 1)], [0, .1, -.1], [.2, .3, .4], 1, True),
    'e2048': (TILE, 2, 3, [lenx_for(CHUNK // 2 - 1), lenx_for(CHUNK // 2), lenx_for(TILE)], [0, .1, -.1], [.2, .3, .4], 1, True),
    'e2049': (TILE + 1, 2, 3, [lenx_for(TILE - 1), lenx_for(TILE + 1), lenx_for(3 * CHUNK)], [0, .1, -.1], [.2, .3, .4], 1, True),
}


def case(name):
    """Seeded inputs of a fixture case: x = [X(:); log W(:)] = randn (test_getObj_nmf_log_norm.m:17), A = exp(randn(T, D)) (:18), vary =
    rand(T, D) (:27); a given W = 0.1 + rand(K, D), rows NOT summing to 1; the targets of the fit y = randn(T, K)"""
    T, D, K, lenx, mux, varx, tol, has_vary = CASES[name]
    rng = np.random.default_rng(9300 + sorted(CASES).index(name))
    x = rng.standard_normal(T * K + K * D)
    A = np.exp(rng.standard_normal((T, D)))
    vary = rng.random((T, D))
    W = 0.1 + rng.random((K, D))
    y = rng.standard_normal((T, K))
    return dict(T=T, D=D, K=K, lenx=np.array(lenx, float), mux=np.array(mux, float), varx=np.array(varx, float), tol=float(tol), x=x, X=x[:T * K].reshape(T, K, order='F'),
                A=A, vary=vary if has_vary else None, W=W, y=y)


def tau_of(lenx, tol):
    return int(np.ceil(lenx / np.sqrt(2) * tol))


def taps(lenx, varx, tol):
    tau = tau_of(lenx, tol)
    bh = np.sqrt(varx * np.sqrt(2) / (lenx * np.sqrt(np.pi)))
    return bh * np.exp(-1 / (lenx ** 2) * np.arange(-tau, tau + 1.0) ** 2)


def conv1(z, lenx, varx, tol, reverse=False):
    """conv(z, bas, 'same') with 2 tau + 1 odd, for any tau; reverse: the taps meet the samples in the opposite order"""
    z = np.asarray(z, float).reshape(-1)
    bas = taps(lenx, varx, tol); tau = (bas.size - 1) // 2
    with np.errstate(all='ignore'):
        if reverse:
            return np.convolve(z[::-1], bas)[tau:tau + z.size][::-1]
        return np.convolve(z, bas)[tau:tau + z.size]


def basis2SEGP(Z, lenx, varx, tol, reverse=False):
    Z = np.asarray(Z, float)
    if Z.ndim == 1:
        return conv1(Z, float(np.reshape(lenx, -1)[0]), float(np.reshape(varx, -1)[0]), tol, reverse)
    return np.stack([conv1(Z[:, k], lenx[k], varx[k], tol, reverse) for k in range(Z.shape[1])], axis=1)


def _tsum(M, reverse):
    """sums over t (axis 0) of a T x n array, from the first row or (reverse) from the last -> (n,)"""
    M = np.asarray(M, float)
    if M.ndim == 1:
        M = M[:, None]
    return np.sum(np.ascontiguousarray((M[::-1] if reverse else M).T), axis=1)


def fit_obj(z, x, lenx, varx, tol, reverse=False, grad=True):
    """getObj_fitSE_basis_func.m:25-43, one problem"""
    z = np.asarray(z, float).reshape(-1); x = np.asarray(x, float).reshape(-1)
    T = z.size
    with np.errstate(all='ignore'):
        dx = conv1(z, lenx, varx, tol, reverse) - x
        Obj = (0.5 * _tsum(dx ** 2, reverse)[0] + 0.5 * _tsum(z ** 2, reverse)[0]) / T
        if not grad:
            return Obj
        return Obj, (conv1(dx, lenx, varx, tol, reverse) + z) / T


def obj(x, A, vary, W, lenx, mux, varx, tol, reverse=False, grad=True):
    """getObj_nmf_log_norm.m (W = None: x = [X(:); log W(:)]) or getObj_nmf_log_norm_inf.m (W given, K x D: x = X(:)), one problem"""
    x = np.asarray(x, float).reshape(-1); A = np.asarray(A, float)
    T, D = A.shape
    learn = W is None
    K = x.size // (T + D) if learn else np.shape(W)[0]
    vary = np.zeros((T, D)) if vary is None or np.size(vary) == 0 else np.broadcast_to(np.asarray(vary, float), (T, D))
    lenx, mux, varx = (np.asarray(v, float).reshape(-1) for v in (lenx, mux, varx))
    with np.errstate(all='ignore'):
        X = x[:T * K].reshape(T, K, order='F')
        H = np.exp(basis2SEGP(X, lenx, varx, tol, reverse) + mux[None, :])
        if learn:
            W = np.exp(x[T * K:]).reshape(K, D, order='F')
            W = (1.0 / np.sum(W, axis=1))[:, None] * W
        else:
            W = np.asarray(W, float)
        Ahat = np.zeros((T, D))
        for k in range(K):
            Ahat = Ahat + H[:, k:k + 1] * W[k:k + 1, :]
        Ahat = Ahat + vary
        obj1 = np.sum(_tsum(A / Ahat + np.log(Ahat), reverse))
        obj2 = 0.5 * np.sum(_tsum(X ** 2, reverse))
        Obj = (obj1 + obj2) / T
        if not grad:
            return Obj
        dA = (Ahat - A) / Ahat ** 2
        dH = np.zeros((T, K))
        for d in range(D):
            dH = dH + dA[:, d:d + 1] * W[:, d][None, :]
        dX = basis2SEGP(dH * H, lenx, varx, tol, reverse)
        out = [(dX + X).reshape(-1, order='F')]
        if learn:
            dW = np.stack([_tsum(H[:, k:k + 1] * dA, reverse) for k in range(K)])
            dWW = dW * W
            out.append((dWW - np.sum(dWW, axis=1)[:, None] * W).reshape(-1, order='F'))
    return Obj, np.concatenate(out) / T


def objective(c, learn, reverse=False, grad=True):
    """a case through the restatement: the learning form on c['x'], the inference form on its first T K entries with c['W']"""
    x = c['x'] if learn else c['x'][:c['T'] * c['K']]
    return obj(x, c['A'], c['vary'], None if learn else c['W'], c['lenx'], c['mux'], c['varx'], c['tol'], reverse=reverse, grad=grad)


def fit_objective(c, reverse=False):
    """the fit of every column of a case: z = X(:, k), target y(:, k) -> Obj (K,), dObj (K, T)"""
    res = [fit_obj(c['X'][:, k], c['y'][:, k], c['lenx'][k], c['varx'][k], c['tol'], reverse) for k in range(c['K'])]
    return np.array([r[0] for r in res]), np.stack([r[1] for r in res])


def dist(a, ref):
    """the project's norm: max|a - ref| / max|ref|"""
    ref = np.asarray(ref, float)
    return float(np.max(np.abs(np.asarray(a, float) - ref)) / np.max(np.abs(ref)))


class evaluator:
    """the restatement as the `evaluator` of nagp.fitSEGP_BF, nagp.tnmf.tnmf and nagp.tnmf.tnmf_inf (the methods of nagp.tnmf.DeviceEvaluator): a
    batch is a loop over its problems.  record: a list that receives one dict per opened batch."""
    def __init__(self, reverse=False, record=None):
        self.reverse = reverse; self.record = record

    def _note(self, **kw):
        if self.record is not None:
            self.record.append(dict(kw, evals=0))
        return self.record[-1] if self.record is not None else {'evals': 0}

    def basis2SEGP(self, Z, lenx, varx, tol):
        return basis2SEGP(Z, np.asarray(lenx, float).reshape(-1), np.asarray(varx, float).reshape(-1), tol, self.reverse)

    def fit(self, x, lenx, varx, tol):
        x = np.atleast_2d(np.asarray(x, float)); n = x.shape[0]
        note = self._note(kind='fit', n_problems=n, tol=tol, lenx=np.array(lenx), varx=np.array(varx))

        def f(Z):
            Z = np.asarray(Z, float).reshape(n, -1); note['evals'] += 1
            res = [fit_obj(Z[q], x[q], lenx[q], varx[q], tol, self.reverse) for q in range(n)]
            return np.array([r[0] for r in res]), np.stack([r[1] for r in res])
        return f

    def tnmf(self, A, vary, W, lenx, mux, varx, tol, n_problems):
        note = self._note(kind='tnmf', n_problems=n_problems, tol=tol, W=None if W is None else np.array(W))

        def f(X):
            X = np.asarray(X, float).reshape(n_problems, -1); note['evals'] += 1
            res = [obj(X[q], A, vary, None if W is None else np.asarray(W)[q], lenx, mux, varx, tol, reverse=self.reverse) for q in range(n_problems)]
            return np.array([r[0] for r in res]), np.stack([r[1] for r in res])
        return f


def planted(T=400, D=6, K=2, seed=3, lenx=(10, 25), varx=(.5, 1), mux=(0, -.5)):
    """data of the driver tests: a draw from the model itself -- X = randn(T, K), H = exp(conv(X) + mux) with tol = 11 -- times K
    spectral rows that sum to 1, under the model's multiplicative noise, plus the noise floor vary = 0.01.
    Returns (A, W, H, vary, dict(lenx, mux, varx))."""
    rng = np.random.default_rng(seed)
    lenx, varx, mux = (np.array(v, float)[:K] for v in (lenx, varx, mux))
    H = np.exp(basis2SEGP(rng.standard_normal((T, K)), lenx, varx, 11) + mux[None, :])
    W = 0.05 + rng.random((K, D)) ** 2
    W = W / W.sum(axis=1)[:, None]
    vary = np.full((T, D), 0.01)
    A = (H @ W + vary) * rng.gamma(4.0, 0.25, (T, D))
    return A, W, H, vary, dict(lenx=lenx, mux=mux, varx=varx)
