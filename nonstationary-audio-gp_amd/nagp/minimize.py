"""The optimiser of every fit of this package, prob_filterbank/minimize.m:

    [X,fX,i] = minimize(X,f,length,P1,...)                                     prob_filterbank/minimize.m

as a generator (minimize_steps), so that the drivers can run many searches in lock-step on one batched evaluator (_drive.py).
"""
import numpy as np

from ._drive import run

INT, EXT, MAX, RATIO, SIG = 0.1, 3.0, 20, 10.0, 0.1         # minimize.m:42-46
RHO = SIG / 2
REALMIN = np.finfo(float).tiny


def minimize_steps(X, length):
    """The algorithm of minimize.m -- Polak-Ribiere conjugate gradients, a line search by cubic extrapolation and quadratic / cubic
    interpolation under the Wolfe-Powell conditions, the slope-ratio guess of the first step -- as a generator: it yields a point and
    is sent (f, df) there; its return value (StopIteration.value) is (X, fX, i).  length > 0: at most that many line searches,
    < 0: at most that many evaluations; a pair (length, red) sets the reduction expected of the first line search.  A non-finite
    f or df during extrapolation halves the step, as the .m's catch does.  An interpolation whose square root is of a negative number
    bisects (the .m would carry a complex step into max / min)."""
    red = 1.0
    if np.ndim(length) > 0:
        length, red = length[0], length[1]
    X = np.array(X, float).reshape(-1)
    with np.errstate(all='ignore'):
        i = 0; ls_failed = False
        f0, df0 = yield X.copy()
        f0 = np.float64(f0); df0 = np.asarray(df0, float).reshape(-1)
        fX = [f0]
        i += length < 0
        s = -df0; d0 = -s @ s
        x3 = np.float64(red) / (1 - d0)
        while i < abs(length):
            i += length > 0
            X0, F0, dF0 = X.copy(), f0, df0
            M = MAX if length > 0 else min(MAX, -length - i)
            while True:                                      # extrapolate
                x2, f2, d2, f3, df3 = np.float64(0), f0, d0, f0, df0
                success = False
                while not success and M > 0:
                    M -= 1; i += length < 0
                    f3, df3 = yield X + x3 * s
                    f3 = np.float64(f3); df3 = np.asarray(df3, float).reshape(-1)
                    if not np.isfinite(f3) or not np.all(np.isfinite(df3)):
                        x3 = (x2 + x3) / 2                   # bisect and try again
                        continue
                    success = True
                if f3 < F0:
                    X0, F0, dF0 = X + x3 * s, f3, df3
                d3 = df3 @ s
                if d3 > SIG * d0 or f3 > f0 + x3 * RHO * d0 or M == 0:
                    break
                x1, f1, d1 = x2, f2, d2
                x2, f2, d2 = x3, f3, d3
                A = 6 * (f1 - f2) + 3 * (d2 + d1) * (x2 - x1)
                B = 3 * (f2 - f1) - (2 * d1 + d2) * (x2 - x1)
                disc = B * B - A * d1 * (x2 - x1)
                x3 = x1 - d1 * (x2 - x1) ** 2 / (B + np.sqrt(disc)) if disc >= 0 else np.float64(np.nan)
                if not np.isfinite(x3) or x3 < 0 or x3 > x2 * EXT:
                    x3 = x2 * EXT
                elif x3 < x2 + INT * (x2 - x1):
                    x3 = x2 + INT * (x2 - x1)
            while (abs(d3) > -SIG * d0 or f3 > f0 + x3 * RHO * d0) and M > 0:      # interpolate
                if d3 > 0 or f3 > f0 + x3 * RHO * d0:
                    x4, f4, d4 = x3, f3, d3
                else:
                    x2, f2, d2 = x3, f3, d3
                if f4 > f0:
                    x3 = x2 - (0.5 * d2 * (x4 - x2) ** 2) / (f4 - f2 - d2 * (x4 - x2))
                else:
                    A = 6 * (f2 - f4) / (x4 - x2) + 3 * (d4 + d2)
                    B = 3 * (f4 - f2) - (2 * d2 + d4) * (x4 - x2)
                    disc = B * B - A * d2 * (x4 - x2) ** 2
                    x3 = x2 + (np.sqrt(disc) - B) / A if disc >= 0 else np.float64(np.nan)
                if not np.isfinite(x3):
                    x3 = (x2 + x4) / 2
                x3 = max(min(x3, x4 - INT * (x4 - x2)), x2 + INT * (x4 - x2))
                f3, df3 = yield X + x3 * s
                f3 = np.float64(f3); df3 = np.asarray(df3, float).reshape(-1)
                if f3 < F0:
                    X0, F0, dF0 = X + x3 * s, f3, df3
                M -= 1; i += length < 0
                d3 = df3 @ s
            if abs(d3) < -SIG * d0 and f3 < f0 + x3 * RHO * d0:                    # the line search succeeded
                X = X + x3 * s; f0 = f3; fX.append(f0)
                s = (df3 @ df3 - df0 @ df3) / (df0 @ df0) * s - df3                # Polak-Ribiere
                df0 = df3
                d3 = d0; d0 = df0 @ s
                if d0 > 0:
                    s = -df0; d0 = -s @ s
                x3 = x3 * min(RATIO, d3 / (d0 - REALMIN))
                ls_failed = False
            else:
                X, f0, df0 = X0, F0, dF0
                if ls_failed or i > abs(length):
                    break
                s = -df0; d0 = -s @ s
                x3 = 1 / (1 - d0)
                ls_failed = True
    return X, np.array(fX, float), int(i)


def minimize(X, f, length, *args):
    """[X, fX, i] = minimize(X, f, length, P1, P2, ...) (minimize.m:1): f(X, P1, ...) returns (value, gradient)."""
    shape = np.shape(X)
    X, fX, i = run(minimize_steps(X, length), lambda x: f(x.reshape(shape), *args))
    return X.reshape(shape), fX, i
