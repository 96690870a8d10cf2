"""NumPy float64 restatement of the objectives of the conjugate-gradient NMF with temporal priors, experiments/nmf/getObj_nmf_temp.m
(learning form) and getObj_nmf_temp_inf.m (inference form), written from the formulae of include/nagp.h (nagp_nmf_temp_obj):

    H = exp(logH);  learning form: W = exp(logW), W = diag(1 ./ sum(W,2)) W;  inference form: W as given;  Ahat = H W + vary
    obj1 = sum(A ./ Ahat + log(Ahat));  dA = (Ahat - A) ./ Ahat.^2;  dlogh = (dA W') .* H;  dW = H' dA, dWW = dW .* W,
    dlogw = dWW - diag(sum(dWW,2)) W;  prior none / 'tg' (varinf, lam) / 'ig' (muinf, varinf, lam): obj2 and dobj2dH with their three
    row forms;  obj = (obj1 + obj2) / T, dobj = [dlogh + dobj2dH .* H; dlogw] / T.

The 60-digit fixture (tools/make_nmf_temp_fixture.py -> tests/golden/nmf_temp_multiprecision.npz) is what this file and the device are
measured against (tests/test_nmf_temp_host.py, tests/test_nmf_temp_gpu.py).  `reverse` forms every sum over t in the opposite order
(float64, NumPy's pairwise summation along t from the first or from the last row).  The case table, the seeded inputs of a case, the
project's distance and the planted data of the driver tests live here as well."""
import numpy as np

TG1 = dict(varinf=[1 / 16, 1 / 32], lam=[.1, .3])                           # test_getObj_nmf_temp.m:21-22
IG1 = dict(muinf=[1 / 4, 1 / 4], varinf=[1 / 16, 1 / 16], lam=[.1, .1])     # :52-54
TG3 = dict(varinf=[1 / 16, 1 / 8, 1 / 4], lam=[.1, .5, .9])
IG3 = dict(muinf=[1 / 4, 1 / 2, 1.0], varinf=[1 / 16, 1 / 8, 1 / 4], lam=[.1, .5, .9])

# name: (T, D, K, prior, form ('l' learning, 'i' inference), vary given, prior parameters)
CASES = {}
for _p, _par in (('none', {}), ('tg', TG1), ('ig', IG1)):
    for _f in 'li':
        CASES['r20_%s_%s' % (_p, _f)] = (20, 3, 2, _p, _f, True, _par)       # the reference's own test shape
for _T in (2, 3):                                                             # the first, interior and last row forms meet or vanish
    for _p, _par in (('none', {}), ('tg', dict(varinf=[1 / 16], lam=[.3])), ('ig', dict(muinf=[1 / 4], varinf=[1 / 16], lam=[.1]))):
        for _f in 'li':
            CASES['t%d_%s_%s' % (_T, _p, _f)] = (_T, 1, 1, _p, _f, True, _par)
CASES['t1_none_l'] = (1, 1, 1, 'none', 'l', True, {})
CASES['t1_none_i'] = (1, 1, 1, 'none', 'i', True, {})
for _T in (255, 256, 257):                                                    # the neighbour rows across a workgroup boundary
    CASES['w%d_tg_l' % _T] = (_T, 16, 3, 'tg', 'l', True, TG3)
    CASES['w%d_ig_l' % _T] = (_T, 16, 3, 'ig', 'l', True, IG3)
CASES['m513_tg_l'] = (513, 64, 16, 'tg', 'l', True, dict(varinf=list(np.linspace(1 / 16, 1 / 2, 16)), lam=list(np.linspace(.05, .95, 16))))   # the limits of D and K
for _p, _par in (('none', {}), ('tg', TG3), ('ig', IG3)):                     # the drivers' D and K
    for _f in 'li':
        CASES['b1999_%s_%s' % (_p, _f)] = (1999, 16, 3, _p, _f, not (_p == 'tg' and _f == 'i'), _par)      # b1999_tg_i: vary = None
CASES['b1999_ig0_l'] = (1999, 16, 3, 'ig', 'l', True, dict(IG3, lam=[0.0, 0.0, 0.0]))
CASES['b1999_ig1_i'] = (1999, 16, 3, 'ig', 'i', True, dict(IG3, lam=[1.0, 1.0, 1.0]))
del _p, _par, _f, _T


def case(name):
    """Seeded inputs of a fixture case: x = randn (test_getObj_nmf_temp.m:18), A = exp(randn(T, D)) (:19), vary = rand(T, D) (:27);
    a given W = 0.1 + rand(K, D), rows NOT summing to 1"""
    T, D, K, prior, form, has_vary, par = CASES[name]
    rng = np.random.default_rng(9100 + sorted(CASES).index(name))
    learn = form == 'l'
    x = rng.standard_normal(T * K + (K * D if learn else 0))
    A = np.exp(rng.standard_normal((T, D)))
    vary = rng.random((T, D))
    W = None if learn else 0.1 + rng.random((K, D))
    return dict(T=T, D=D, K=K, prior=prior, learn=learn, x=x, A=A, vary=vary if has_vary else None, W=W,
                muinf=np.array(par['muinf'], float) if 'muinf' in par else None,
                varinf=np.array(par['varinf'], float) if 'varinf' in par else None,
                lam=np.array(par['lam'], float) if 'lam' in par else None)


def _tsum(M, reverse):
    """sums over t (axis 0) of a T' x n array, from the first row or (reverse) from the last, pairwise in float64 -> (n,)"""
    M = np.asarray(M, float)
    if M.shape[0] == 0:
        return np.zeros(M.shape[1])
    return np.sum(np.ascontiguousarray((M[::-1] if reverse else M).T), axis=1)


def obj(x, A, vary, W=None, prior='none', muinf=None, varinf=None, lam=None, reverse=False, grad=True):
    """one problem: x = [log H(:); log W(:)] (W = None) or log H(:) (W given, K x D)"""
    x = np.asarray(x, float).reshape(-1); A = np.asarray(A, float)
    T, D = A.shape
    learn = W is None
    K = x.size // (T + D) if learn else np.shape(W)[0]
    vary = np.zeros((T, D)) if vary is None else np.broadcast_to(np.asarray(vary, float), (T, D))
    with np.errstate(all='ignore'):
        logH = x[:T * K].reshape(T, K, order='F')
        H = np.exp(logH)
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
        dA = (Ahat - A) / Ahat ** 2
        dH = np.zeros((T, K))
        for d in range(D):
            dH = dH + dA[:, d:d + 1] * W[:, d][None, :]
        obj2 = 0.0; d2 = None
        if prior == 'tg':
            varinf = np.asarray(varinf, float).reshape(-1); lam = np.asarray(lam, float).reshape(-1)
            obj2 = np.sum((1 + lam ** 2) / (2 * varinf) * _tsum(H[1:T - 1] ** 2, reverse)) + np.sum(1 / (2 * varinf) * H[T - 1] ** 2) \
                + np.sum(lam ** 2 / (2 * varinf) * H[0] ** 2) - np.sum(lam / varinf * _tsum(H[1:] * H[:T - 1], reverse))
            d2 = np.zeros((T, K))
            d2[0] = lam ** 2 / varinf * H[0] - lam / varinf * H[1]
            d2[1:T - 1] = (1 + lam ** 2) / varinf * H[1:T - 1] - lam / varinf * (H[2:] + H[:T - 2])
            d2[T - 1] = 1 / varinf * H[T - 1] - lam / varinf * H[T - 2]
        elif prior == 'ig':
            muinf = np.asarray(muinf, float).reshape(-1); varinf = np.asarray(varinf, float).reshape(-1); lam = np.asarray(lam, float).reshape(-1)
            alp1 = muinf ** 2 / varinf + 2
            bet1 = (alp1 - 1) * muinf
            alp = 2 + lam ** 2 + muinf ** 2 / varinf
            a = (alp - 1) * lam
            b = (alp - 1) * (1 - lam) * muinf
            ahtpb = a * H[:T - 1] + b
            obj2 = np.sum(bet1 / H[0]) + np.sum((alp1 + 1) * logH[0]) - np.sum(alp * _tsum(np.log(ahtpb), reverse)) \
                + np.sum((alp + 1) * _tsum(logH[1:], reverse)) + np.sum(_tsum(ahtpb / H[1:], reverse))
            d2 = np.zeros((T, K))
            d2[0] = a / H[1] - bet1 / H[0] ** 2 + (alp1 + 1) / H[0] - alp * a / ahtpb[0]
            d2[1:T - 1] = a / H[2:] - ahtpb[:T - 2] / H[1:T - 1] ** 2 + (alp + 1) / H[1:T - 1] - alp * a / ahtpb[1:]
            d2[T - 1] = -ahtpb[T - 2] / H[T - 1] ** 2 + (1 + alp) / H[T - 1]
        elif prior != 'none':
            raise ValueError(prior)
        Obj = (obj1 + obj2) / T
        if not grad:
            return Obj
        dlogh = dH * H
        if d2 is not None:
            dlogh = dlogh + d2 * H
        out = [dlogh.reshape(-1, order='F')]
        if learn:
            dW = np.stack([_tsum(H[:, k:k + 1] * dA, reverse) for k in range(K)])
            dWW = dW * W
            out.append((dWW - np.sum(dWW, axis=1)[:, None] * W).reshape(-1, order='F'))
    return Obj, np.concatenate(out) / T


def objective(c, reverse=False, grad=True):
    """a case (or any dict with its keys) through the restatement"""
    return obj(c['x'], c['A'], c['vary'], c['W'], c['prior'], c['muinf'], c['varinf'], c['lam'], reverse=reverse, grad=grad)


def dist(a, ref):
    """the project's norm: max|a - ref| / max|ref|"""
    ref = np.asarray(ref, float)
    return float(np.max(np.abs(np.asarray(a, float) - ref)) / np.max(np.abs(ref)))


def evaluator(reverse=False, record=None):
    """the restatement as the `evaluator` of nagp.nmf_inf / nagp.nmf_temp.nmf: a batch is a loop over its problems"""
    def open_batch(A, vary, W, K, prior, muinf, varinf, lam, n_problems):
        if record is not None:
            record.append(dict(W=None if W is None else np.array(W), K=K, prior=prior, muinf=muinf, varinf=varinf, lam=lam, n_problems=n_problems, evals=0))

        def f(X):
            X = np.asarray(X, float).reshape(n_problems, -1)
            if record is not None:
                record[-1]['evals'] += 1
            res = [obj(X[q], A, vary, None if W is None else np.asarray(W)[q], prior, muinf, varinf, lam, reverse=reverse) for q in range(n_problems)]
            return np.array([r[0] for r in res]), np.stack([r[1] for r in res])
        return f
    return open_batch


def planted(T=400, D=6, K=2, seed=3):
    """data of the driver tests: K smooth positive activations (exp of a random walk pulled to its mean) times K spectral rows that sum
    to 1, under the model's multiplicative noise A = Ahat .* Exp(1)-like gamma(4) / 4, plus the noise floor vary = 0.01.
    Returns (A, W, H, vary, prior parameters of the IG chain that fit H loosely)."""
    rng = np.random.default_rng(seed)
    g = np.zeros((T, K))
    for t in range(1, T):
        g[t] = 0.97 * g[t - 1] + 0.15 * rng.standard_normal(K)
    H = np.exp(g) * np.array([0.5, 1.0, 0.75, 1.5][:K])
    W = 0.05 + rng.random((K, D)) ** 2
    W = W / W.sum(axis=1)[:, None]
    vary = np.full((T, D), 0.01)
    A = (H @ W + vary) * rng.gamma(4.0, 0.25, (T, D))
    par = dict(muinf=np.mean(H, axis=0), varinf=np.var(H, axis=0), lam=np.full(K, 0.9))
    return A, W, H, vary, par
