"""Multi-precision fixture of the infinite-horizon look-up tables of 6- and 8-state sub-band blocks:
tests/golden/dare_sixeight_states.npz.

The infinite-horizon family reads, per block and per knot r of ro = logspace(-2, 4, 32), the predictive DARE solution PP,
the steady-state smoother gain G and the steady-state smoothed covariance PS2 (matlab/ihgp_ep_modulator_nmf.m:107-191).
The product solves them in f64 with a batched doubling iteration (nagp/ihgp_tables.py), the oracle with SciPy's QZ solver
(oracle/ihgp.py).  For Matern-5/2 and Matern-7/2 sub-bands the steady-state covariances are conditioned 1e8 .. 1e12 and
the two f64 solvers do not agree to better than 1e-7 .. 1e-3, so this script solves the same equations in mpmath at
DPS decimal digits and rounds the answer to f64 once, at the end:

  inputs    A, Q, h of each block exactly as the product forms them (ss_modulators_nmf -> balance -> lti_disc with
            Q = (Q + Q')/2), taken as exact f64 numbers and stored, so the fixture does not depend on the installed expm;
  DARE      P = A (P - P h' (h P h' + r)^-1 h P) A' + Q  by structure-preserving doubling to a change below 1e-40 of |P|
            (the same iteration as the host's, in DPS digits), checked by its residual;
  smoother  the formulas of oracle/ihgp.py:smoother_tables (ihgp_ep_modulator_nmf.m:158-180) with K r K' in the filtered
            covariance (C-23), G = P A' (A P A' + Q)^-1, QQ = P - G PP G' projected on the PSD cone (mp.eigsy, eigenvalues
            <= 0 dropped) and PS2 = G PS2 G' + QQ by doubling to a change below 1e-40.

Blocks: every block of harness.nmf_problem(3, 2, *, 11, kernel1=k1) for k1 = matern52 / matern72 (three sub-band blocks of
6 or 8 states, two Matern-5/2 modulators of 3), of the constraints recipe through the constrained parameter unpacking for
k1 = matern72 (what ihgp_ep_modulator_nmf_constraints builds), and one sub-band block per kernel at each end of the
length-scale range of harness.CONSTRAINTS_DEMO (20 and 500 samples).  Stored per block i: A_i, Q_i (b x b), h_i,
PP_i / G_i / PS2_i (32 x b^2, each row the column-major flattening of one knot, as in the product's tables), and the recipe.

Run:  python tools/make_dare_fixture.py            (about 100 s of one core; --jobs 8 spreads the blocks over 8 processes: 17 s)
      python tools/make_dare_fixture.py --check    (recompute and compare with the committed file instead of writing it)
The output is bit-for-bit reproducible (fixed zip time stamps, round-to-nearest from mpmath).
"""
import argparse
import io
import math
import os
import sys
import time
import zipfile

import numpy as np
from mpmath import mp
from mpmath.libmp import round_nearest, to_float

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'nonstationary-audio-gp_amd'))

from nagp import harness, ss as pss                                        # noqa: E402
from nagp.api import SSHandle, _blocks_from_dense, _unpack_constraints, _unpack_log     # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden', 'dare_sixeight_states.npz')
DPS = 60
TOL = mp.mpf('1e-40')
SEED, D, N = 11, 3, 2
N_KNOTS = 32
# (recipe, kernel1): the product's problems; 'edge': sub-band blocks (variance, length-scale, omega) at the ends of CONSTRAINTS_DEMO's range
PROBLEMS = [('demo_nmf', 'matern52'), ('demo_nmf', 'matern72'), ('constraints', 'matern72'), ('edge', 'matern52'), ('edge', 'matern72')]
EDGE = [(0.055, 20.0, math.pi / 4), (0.055, 500.0, math.pi / 50)]


def problem_params(recipe, k1):
    """(param1, param2, D, N) of one problem, as the product's entry point unpacks them."""
    if recipe == 'edge':
        cons = harness.CONSTRAINTS_DEMO(D)
        assert all(cons[1][0] <= ell <= cons[1][1] for _, ell, _ in EDGE) and {e[1] for e in EDGE} == set(cons[1])
        return np.array([e[0] for e in EDGE] + [e[1] for e in EDGE] + [e[2] for e in EDGE]), np.zeros(0), len(EDGE), 0
    pr = harness.nmf_problem(D, N, 5, SEED, recipe, kernel1=k1)
    if recipe == 'constraints':
        cons = harness.CONSTRAINTS_DEMO(D)
        w, wf = harness.constrained_vectors(pr, cons, harness.TUNE_DEMO)
        _, p1, p2, _ = _unpack_constraints(w, wf, harness.TUNE_DEMO, cons, 1, D, N)
        return p1, p2, D, N
    _, p1, p2, _ = _unpack_log(pr['w'], 1, D, N)
    return p1, p2, D, N


def product_blocks(recipe, k1):
    """The balanced block model and its (A, Q) exactly as nagp.api.ihgp_ep_modulator_nmf{,_constraints} form them."""
    p1, p2, D_, N_ = problem_params(recipe, k1)
    if N_:
        blk = pss.balance_blocks(_blocks_from_dense(*SSHandle()(None, p1, p2, k1, 'matern52'), D_, N_))
    else:
        blk = pss.balance_blocks(pss.ss_blocks_nmf(p1, p2, k1, 'matern52'))
    A, Q, _ = pss.discretise(blk, symmetrize_Q=True)
    return blk, A, Q


def _mat(X):
    return mp.matrix([[mp.mpf(float(v)) for v in row] for row in np.asarray(X, float)])


def _amax(X):
    return max(abs(X[i, j]) for i in range(X.rows) for j in range(X.cols))


def _sym(X):
    return (X + X.T) / 2


def _f64(X):
    """column-major flattening rounded to nearest f64"""
    return [to_float(X[i, j]._mpf_, rnd=round_nearest) for j in range(X.cols) for i in range(X.rows)]


def dare(A, Q, h, r):
    """P = A (P - P h'(h P h' + r)^-1 h P) A' + Q by doubling (SDA on dare(A', h', Q, r)); raises unless converged."""
    b = A.rows; I = mp.eye(b)
    Ak = A.T; Gk = (h.T * h) / r; Hk = Q.copy()
    for it in range(200):
        Wi = mp.inverse(I + Gk * Hk)
        WiA = Wi * Ak
        An = Ak * WiA; Gn = Gk + Ak * Wi * Gk * Ak.T; Hn = Hk + Ak.T * Hk * WiA
        d = _amax(Hn - Hk) / _amax(Hn)
        Ak, Gk, Hk = An, Gn, Hn
        if d < TOL:
            break
    else:
        raise RuntimeError('DARE doubling did not converge (r = %r, last change %s)' % (float(r), mp.nstr(d, 3)))
    P = _sym(Hk)
    S = (h * P * h.T)[0, 0] + r
    res = A * (P - P * h.T * h * P / S) * A.T + Q - P
    if _amax(res) > TOL * _amax(P):
        raise RuntimeError('DARE residual %s of |P| at r = %r' % (mp.nstr(_amax(res) / _amax(P), 3), float(r)))
    return P, it + 1


def stein(G, QQ):
    """X = G X G' + QQ by doubling; raises unless converged."""
    X = QQ.copy(); Gk = G.copy()
    for it in range(200):
        Xn = X + Gk * X * Gk.T
        d = _amax(Xn - X) / _amax(Xn)
        X = Xn; Gk = Gk * Gk
        if d < TOL:
            break
    else:
        raise RuntimeError('Stein doubling did not converge (last change %s)' % mp.nstr(d, 3))
    res = G * X * G.T + QQ - X
    if _amax(res) > TOL * _amax(X):
        raise RuntimeError('Stein residual %s of |X|' % mp.nstr(_amax(res) / _amax(X), 3))
    return _sym(X), it + 1


def solve_block(job):
    """All 32 knots of one block: returns (PP, G, PS2) as (32, b^2) f64 arrays and the largest iteration counts."""
    Ab, Qb, hval = job
    mp.dps = DPS
    b = Ab.shape[0]
    A = _mat(Ab); Q = _mat(Qb); h = mp.matrix(1, b); h[0, 0] = mp.mpf(float(hval))
    out = {'PP': [], 'G': [], 'PS2': []}; its = [0, 0]
    for r in np.logspace(-2, 4, N_KNOTS):
        r = mp.mpf(float(r))
        PP, n1 = dare(A, Q, h, r)
        S = (h * PP * h.T)[0, 0] + r
        K = PP * h.T / S
        P = PP - r * (K * K.T)                                         # ihgp_ep_modulator_nmf.m:163 (C-23: K r K')
        PSkp = _sym(A * P * A.T + Q)
        G = P * A.T * mp.inverse(PSkp)
        QQ = _sym(P - G * PP * G.T)
        lam, V = mp.eigsy(QQ)
        QQ = mp.matrix(b, b)
        for k in range(b):
            if lam[k] > 0:
                QQ += lam[k] * (V[:, k] * V[:, k].T)
        PS2, n2 = stein(G, QQ)
        out['PP'].append(_f64(PP)); out['G'].append(_f64(G)); out['PS2'].append(_f64(PS2))
        its = [max(its[0], n1), max(its[1], n2)]
    return {k: np.array(v) for k, v in out.items()}, its


def build(jobs=1, verbose=True):
    t0 = time.time()
    arrays = {'ro': np.logspace(-2, 4, N_KNOTS), 'dps': np.array(DPS), 'seed': np.array(SEED),
              'problem_recipe': np.array([p[0] for p in PROBLEMS]), 'problem_kernel1': np.array([p[1] for p in PROBLEMS]),
              'edge_params': np.array(EDGE)}
    blocks, owner = [], []
    for q, (recipe, k1) in enumerate(PROBLEMS):
        blk, A, Q = product_blocks(recipe, k1)
        for n in range(blk.M):
            o, e = blk.offsets[n], blk.offsets[n + 1]
            blocks.append((np.array(A[o:e, o:e]), np.array(Q[o:e, o:e]), float(blk.h_val[n])))
            owner.append((q, n))
    if jobs > 1:
        from multiprocessing import Pool
        with Pool(jobs) as pool:
            res = pool.map(solve_block, blocks, chunksize=1)
    else:
        res = [solve_block(bl) for bl in blocks]
    for i, ((Ab, Qb, hv), (tabs, its), (q, n)) in enumerate(zip(blocks, res, owner)):
        arrays['A_%d' % i] = Ab; arrays['Q_%d' % i] = Qb; arrays['h_%d' % i] = np.array(hv)
        for k, v in tabs.items():
            arrays['%s_%d' % (k, i)] = v
        if verbose:
            print('block %2d  problem %d (%-11s %s) #%d  %d states  doubling steps DARE %d / Stein %d'
                  % (i, q, PROBLEMS[q][0], PROBLEMS[q][1], n, Ab.shape[0], its[0], its[1]))
    arrays['block_problem'] = np.array([o[0] for o in owner]); arrays['block_index'] = np.array([o[1] for o in owner])
    arrays['block_size'] = np.array([bl[0].shape[0] for bl in blocks])
    if verbose:
        print('%d blocks in %.0f s' % (len(blocks), time.time() - t0))
    return arrays


def write_npz(path, arrays):
    """np.savez_compressed with fixed member time stamps and order, so the bytes depend on the contents only."""
    tmp = path + '.tmp'
    with zipfile.ZipFile(tmp, 'w', compression=zipfile.ZIP_DEFLATED) as zf:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asarray(arrays[k]), allow_pickle=False)
            zi = zipfile.ZipInfo(k + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
            zi.compress_type = zipfile.ZIP_DEFLATED
            zf.writestr(zi, buf.getvalue())
    os.replace(tmp, path)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--jobs', type=int, default=1)
    ap.add_argument('--check', action='store_true', help='compare with the committed fixture instead of writing it')
    ap.add_argument('--out', default=OUT)
    a = ap.parse_args()
    arrays = build(a.jobs)
    if a.check:
        g = np.load(a.out)
        bad = [k for k in arrays if k not in g.files or not np.array_equal(np.asarray(arrays[k]), g[k])]
        bad += [k for k in g.files if k not in arrays]
        print('fixture matches' if not bad else 'differs in %s' % bad)
        sys.exit(1 if bad else 0)
    write_npz(a.out, arrays)
    print('wrote %s (%d bytes)' % (os.path.relpath(a.out, ROOT), os.path.getsize(a.out)))


if __name__ == '__main__':
    main()
