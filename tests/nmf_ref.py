"""NumPy restatement of the fixed-point NMF of experiments/nmf/nmf_fp.m, nmf_inf_fp.m and its objective getObj_nmf_temp.m (the branch
without temporal priors), written from the .m text statement by statement: both update forms, the objective with its renormalisation
of W and its exp(log(.)), and the restart selection of nmf_fp.m:44-56.  It is the yardstick of the GPU tests of nagp_nmf_fp; its own
distance to the multi-precision fixture (tests/golden/nmf_multiprecision.npz, tools/make_nmf_fixture.py) is pinned in
tests/test_nmf_host.py.  `dtype` chooses the arithmetic (float64, longdouble, or object arrays of mpmath numbers with `fn`);
`reverse` forms every sum over t in the opposite order."""
import numpy as np

CASES = {  # name: (T, D, K, its, vary)
    'a': (257, 5, 3, 5, 1e-3),      # more than one workgroup with a ragged tail
    'b': (63, 1, 1, 5, None),       # less than one wave; vary absent
    'c': (1000, 17, 4, 10, 1e-3),   # odd D, several workgroups
    'd': (300, 16, 9, 40, 1e-3),    # K beyond one MFMA k-group
    'e': (1, 3, 2, 2, 1e-3),        # a single time row
    'f': (64, 64, 16, 3, 1e-3),     # both limits
}


def case(name):
    """Inputs of a fixture case: A = (Ht Wt) .* Exp(1) noise, H0 = exp(randn), W0 = rows of A plus 1e-6, row-normalised (the caller's
    line nmf_fp.m:63); vary a constant matrix or None."""
    T, D, K, its, v = CASES[name]
    rng = np.random.default_rng(9000 + ord(name))
    Ht = np.exp(rng.standard_normal((T, K))); Wt = rng.random((K, D)) + 0.05
    Wt /= Wt.sum(axis=1, keepdims=True)
    A = (Ht @ Wt) * rng.exponential(1.0, (T, D))
    H0 = np.exp(rng.standard_normal((T, K)))
    W0 = A[rng.integers(0, T, K), :] + 1e-6
    W0 = np.diag(1.0 / W0.sum(axis=1)) @ W0
    return dict(A=A, vary=None if v is None else np.full((T, D), v), W0=W0, H0=H0, its=its)


class Fn:
    """the elementary functions of an arithmetic"""
    def __init__(self, log=np.log, exp=np.exp):
        self.log, self.exp = log, exp


def _sum_all(X, reverse):
    """sum(X(:)): column-major order (reverse: t descending inside every column)"""
    X = X[::-1] if reverse else X
    s = X[0, 0] * 0
    for d in range(X.shape[1]):
        for t in range(X.shape[0]):
            s = s + X[t, d]
    return s


def _tdot(H, G, reverse):
    """H' * G, every entry summed over t in ascending (reverse: descending) order"""
    if reverse:
        H, G = H[::-1], G[::-1]
    acc = H[0][:, None] * G[0][None, :]
    for t in range(1, H.shape[0]):
        acc = acc + H[t][:, None] * G[t][None, :]
    return acc


def normalise(W):
    """diag(1 ./ sum(W,2)) * W"""
    s = W[:, 0]
    for d in range(1, W.shape[1]):
        s = s + W[:, d]
    return (1 / s)[:, None] * W


def objective(H, W, A, vary, fn=Fn(), reverse=False):
    """getObj_nmf_temp(logHW, A, vary) with logHW = [log(H(:)); log(W(:))]: :45-54, :134"""
    H = fn.exp(fn.log(H)); W = normalise(fn.exp(fn.log(W)))
    Ahat = H.dot(W) + vary
    return _sum_all(A / Ahat + fn.log(Ahat), reverse) / A.shape[0]


def iterate(A, vary, W, H, n_its, update_w=True, dtype=np.float64, fn=Fn(), reverse=False):
    """n_its iterations of nmf_fp.m:65-87 (update_w) or nmf_inf_fp.m:42-55; W is used as given.  Returns W, H, Obj."""
    cast = (lambda x: np.asarray(x, dtype=dtype)) if dtype is not object else (lambda x: x)
    A = cast(A); W = cast(W); H = cast(H)
    vary = A * 0 if vary is None else cast(vary)
    Obj = []
    for _ in range(n_its):
        AHat = H.dot(W) + vary                                                   # :74
        H = (A * AHat ** -2).dot(W.T) / (AHat ** -1).dot(W.T) * H                # :75
        Obj.append(objective(H, W, A, vary, fn, reverse))                        # :77-79
        if update_w:
            AHat = H.dot(W)                                                      # :81
            W = _tdot(H, A * AHat ** -2, reverse) / _tdot(H, AHat ** -1, reverse) * W      # :82
            W = normalise(W)                                                     # :83
            Obj.append(objective(H, W, A, vary, fn, reverse))                    # :85-87
    return W, H, np.array(Obj, dtype=dtype)


def nmf_inf_fp(A, W, H, vary, numIts=100, **kw):
    """nmf_inf_fp.m: :37 normalises W only when EVERY row sum differs from 1 (MATLAB's `if` on a vector)"""
    if np.all(np.sum(W, axis=1) != 1):
        W = normalise(np.asarray(W))
    _, H, Obj = iterate(A, vary, W, H, numIts, update_w=False, **kw)
    return H, Obj


def select_restart(A, vary, cands, **kw):
    """nmf_fp.m:44-56 with the candidates given: each W row-normalised (:45), 10 iterations of nmf_inf_fp, the smallest last Obj
    wins with strict < (the earliest of a tie).  Returns the index, W, H and the last objectives."""
    best, ObjBest, last = None, np.inf, []
    for r, (Wt, Ht) in enumerate(cands):
        Wt = normalise(np.asarray(Wt, float))
        Hn, Obj = nmf_inf_fp(A, Wt, Ht, vary, 10, **kw)
        last.append(float(Obj[-1]))
        if Obj[-1] < ObjBest:
            best, ObjBest = (r, Wt, Hn), Obj[-1]
    return best[0], best[1], best[2], np.array(last)


def nmf_fp(A, W, H, vary, numIts=1000, cands=None, **kw):
    """nmf_fp.m with the restart candidates given (cands[0] is the caller's pair)"""
    if cands is not None:
        _, W, H, _ = select_restart(A, vary, cands, **kw)
    W = normalise(np.asarray(W, float))                                          # :63
    return iterate(A, vary, W, H, numIts, update_w=True, **kw)


def dist(a, ref):
    """the project's norm: max|a - ref| / max|ref|"""
    ref = np.asarray(ref, float)
    return float(np.max(np.abs(np.asarray(a, float) - ref)) / np.max(np.abs(ref)))
