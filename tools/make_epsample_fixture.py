"""Multi-precision fixture of nagp_ep_sample (joint posterior draws of a full-covariance EP run): tests/golden/epsample_multiprecision.npz.

The GPU tests of the sampler compare the kernels with a float64 restatement (tests/epsample_ref.py) at 1e-7, eight decades above
what is measured, and none of them takes the jitter retry, a clamped pivot or the "not positive definite" exit.  This script restates the
algorithm of csrc/nagp_epsample.hpp from the exact f64 inputs the library is handed, in the integer fixed point of
tools/make_smoother_fixture.py (PREC = 320 bits), and rounds to f64 once at the end:

  filter    k > 0 or predict_at_k1: m = A m, P = A P A' + Q;  y_k not NaN: the update with the sites of step k, per site the ttau == 0
            branch (m += W tnu, P untouched) or K = W / (HPH + 1 / ttau), m += K (tnu / ttau - fmu), P -= (K H) P;
  factors   k < T-1: PSkp = A PF_k A' + Q (lower triangle); L = chol(PSkp), and where a pivot is not positive a second attempt on a
            RECOMPUTED PSkp with sqrt(1e-4) * 0.5 on the diagonal (counted; a pivot that is not positive there is an error);
            G = PF_k A' / L' / L;  C = (I - G A) PF_k (I - G A)' + G Q G' with the true Q;  Lc = chol(C) where a pivot <= 0 zeroes its
            column and is counted;  Lc_{T-1} = chol(PF_{T-1}) the same way;
  chain     x_{T-1} = MF_{T-1} + Lc z_{T-1};  x_k = MF_k + G_k (x_{k+1} - A MF_k) + Lc_k z_k on the stored normals z (n = 3 draws: the
            generator is not restated) and on z = 0, which gives MS;  Fdraw = H Xdraw;  Sdraw = sum_d a_d Fdraw_d with
            a = Wnmf link(Fdraw_g) or its square root (two cases).

Every run is repeated at 256 bits; the answers agree to better than 1e-60 of each field's largest entry (asserted, agree_256_bits).

The factorisations decide by the sign of a pivot, and a case is committed only where the multi-precision run decides every pivot with a
margin: per case `margins` = the smallest |pivot| / max |diag| over the first attempts (the failing pivot included), the second attempts
and the factorisations of C_k / PF_{T-1}, over the pivots that are not structurally zero (exact zeros of a state of zero variance -- exact
in fixed point and in f64, counted in `zero_pivots`); `margins_scaled` = the same with each pivot over its OWN diagonal entry of the
matrix, which does not move when a state is rescaled.  MARGIN = 1e-6: both figures on every synthetic case; the two driver models are
not balanced (variances of 1e1 .. 1e-11 side by side: the first figure is 5e-12 there for pivots that keep 6 % .. 85 % of their entry)
and are held to the scaled figure.  A synthetic case walks seeds upwards from its base seed until the margins hold and the counters are
what the case is for (seeds_skipped).  No step is excused.

err_oracle(field): tests/epsample_ref.py (model column- and row-major) on the same f64 inputs against this run, max-abs difference over
the largest entry of the field; 10 x err_oracle < 1e-7 is asserted.

Synthetic model (tests/test_epsample_gpu.py:synthetic_blocks with rho a parameter): per block A_b = rho x the Q factor of a normal
matrix, Pinf_b = u I, u ~ U(0.5, 2); Q = Pinf - A Pinf A' symmetrised from the lower triangle; h_val ~ U(0.5, 2); Wnmf ~ U(0.1, 1)
(D = M - 1, N = 1); ttau ~ U(0.5, 50) with two entries zero; tnu ~ N(0, 1); y missing at both ends and over T//3 .. T//2.  `dead` blocks
have Pinf_b = Q_b = 0: a state of exactly zero variance.  The driver cases take nagp.harness.nmf_problem through nagp.ss and the sites of
oracle.gf_ep.run_predict (two sweeps), stored as data.

Run:  python tools/make_epsample_fixture.py --jobs 8     (5 s; 15 s of one core, s80 four of them)
      python tools/make_epsample_fixture.py --check [--only s16,retry_all_T1]
The output is reproducible bit for bit (fixed zip time stamps, round-to-nearest from mpmath).
"""
import argparse
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'nonstationary-audio-gp_amd'))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

try:                                                                       # the loader below needs neither
    from mpmath import mp, mpf
    from make_smoother_fixture import Fx, link_funs, write_npz             # noqa: E402
except ImportError:                                                        # pragma: no cover
    mp = mpf = Fx = link_funs = write_npz = None

OUT = os.path.join(ROOT, 'tests', 'golden', 'epsample_multiprecision.npz')
PREC, PREC_LOW = 320, 256
JITTER = math.sqrt(1e-4) * 0.5
assert JITTER == 0.005                    # EPS_JITTER of csrc/nagp_epsample.hpp, the same double
MARGIN = 1e-6
TOL_MEAN = 1e-7
N_DRAWS = 3
FIELDS = ('Xdraw', 'Fdraw', 'MS', 'Sdraw')
MARGIN_NAMES = ('first_attempt', 'second_attempt', 'clamped_factor')
AMP_LINEAR, AMP_SQRT, LINK_SOFTPLUS, LINK_EXP = 0, 1, 0, 1

B52 = [8, 8, 8, 8, 8, 1, 6, 5]
# want: what the case is for -- 'none': no retry, no clamped pivot; 'some': 0 < retries < T-1; 'all': retries == T-1 (max(T-1, 0)) and
# clamped == dead states x T
CASES = {
    's16': dict(blocks=[4, 4, 4, 4], T=24, seed=11, want='none', sig=(AMP_LINEAR, LINK_SOFTPLUS, 1.5)),
    's32': dict(blocks=[8, 8, 8, 8], T=24, seed=11, want='none'),
    's33': dict(blocks=[8, 8, 8, 8, 1], T=24, seed=11, want='none', sig=(AMP_SQRT, LINK_EXP, 0.0)),
    's48': dict(blocks=[8] * 6, T=24, seed=11, want='none'),
    's52_pk1': dict(blocks=B52, T=24, seed=11, want='none', p0_scale=2.0, pk1=True),
    's64': dict(blocks=[8] * 8, T=24, seed=11, want='none'),
    's80': dict(blocks=[8] * 10, T=24, seed=11, want='none'),
    'drv_s18': dict(driver=dict(D=3, N=2, k1='matern32'), T=24, seed=42, want='none'),
    'drv_exp_s25': dict(driver=dict(D=8, N=3, k1='exp'), T=24, seed=42, want='none'),
    'retry_some': dict(blocks=[4, 4, 3, 2], T=24, seed=11, want='some', rho=0.999, p0_set=[(3, -0.005)]),
    'retry_all': dict(blocks=[4, 2, 3, 4], T=24, seed=11, want='all', dead=[1]),
    'retry_all_T1': dict(blocks=[4, 2, 3, 4], T=1, seed=11, want='all', dead=[1]),
    'retry_all_T2': dict(blocks=[4, 2, 3, 4], T=2, seed=11, want='all', dead=[1]),
    'retry_s52': dict(blocks=B52, T=24, seed=11, want='all', dead=[5]),
}
K2 = 'matern52'
NOTPD_P0 = (3, -0.05)                      # retry_some's model with this entry of P0: not positive definite even with the jitter


class CaseRejected(Exception):
    pass


# ---------------------------------------------------------------------------------------------
# the f64 inputs
def synthetic_inputs(c, seed):
    sizes = c['blocks']; T = c['T']; rho = c.get('rho', 0.9)
    rng = np.random.default_rng(seed)
    S = int(sum(sizes)); M = len(sizes); off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    A = np.zeros((S, S)); P = np.zeros((S, S))
    for n, b in enumerate(sizes):
        o = off[n]; q, _ = np.linalg.qr(rng.standard_normal((b, b)))
        A[o:o + b, o:o + b] = rho * q; P[o:o + b, o:o + b] = rng.uniform(0.5, 2.0) * np.eye(b)
    for n in c.get('dead', ()):
        P[off[n]:off[n + 1], off[n]:off[n + 1]] = 0.0
    Q = P - A @ P @ A.T; Q = np.tril(Q) + np.tril(Q, -1).T
    for n in c.get('dead', ()):
        assert not Q[off[n]:off[n + 1], off[n]:off[n + 1]].any()
    hv = rng.uniform(0.5, 2.0, M)
    W = rng.uniform(0.1, 1.0, (M - 1, 1))
    ttau = rng.uniform(0.5, 50.0, (M, T)); tnu = rng.standard_normal((M, T))
    if T > 3:
        ttau[0, 3] = 0.0
    if T > 7:
        ttau[M - 1, 7] = 0.0
    y = np.zeros(T); y[0] = y[T - 1] = np.nan; y[T // 3:T // 2] = np.nan
    P0 = c.get('p0_scale', 1.0) * P
    for i, v in c.get('p0_set', ()):
        P0[i, i] = v
    z = np.random.default_rng(seed + 7919).standard_normal((N_DRAWS, T, S))
    return dict(A=A, Q=Q, P0=P0, Pinf=P, h_val=hv, block_offsets=off, Wnmf=W, D=np.array(M - 1), N=np.array(1), ttau=ttau, tnu=tnu, y=y, z=z,
                predict_at_k1=np.array(bool(c.get('pk1', False))), rho=np.array(rho), seed=np.array(seed))


def driver_model(c):
    """(pr, blk, A, Q, Pinf, y) of a driver case: nagp.harness.nmf_problem through nagp.ss, as nagp.api hands it to the library"""
    from nagp import harness, ss as pss
    d = c['driver']; T = c['T']
    pr = harness.nmf_problem(d['D'], d['N'], T, c['seed'], kernel1=d['k1'], kernel2=K2)
    blk = pss.ss_blocks_nmf(pr['param1'], pr['param2'], d['k1'], K2)
    A, Q, P = pss.discretise(blk)
    y = pr['y'].copy(); y[T // 3:T // 2] = np.nan
    return pr, blk, np.array(A), np.array(Q), np.array(P), y


def driver_sites(c, A, Q, P, blk, pr, y):
    from oracle import gf_ep as ogf, lik as olik
    S = A.shape[0]
    H = np.zeros((blk.M, S)); H[np.arange(blk.M), np.asarray(blk.offsets)[:-1]] = blk.h_val
    model = dict(A=A, Q=Q, H=H, Pinf=P, Wnmf=pr['W'], lik_param=np.log(pr['w_lik']))
    with np.errstate(all='ignore'):
        res = ogf.run_predict(model, y, olik.Mom(olik.LIK_POWER_NMF, p=5), 0.5, 0.5 * np.ones(2), 2, predict_at_k1=False)
    return np.array(res['ttau'], float), np.array(res['tnu'], float)


def driver_inputs(c):
    pr, blk, A, Q, P, y = driver_model(c)
    ttau, tnu = driver_sites(c, A, Q, P, blk, pr, y)
    d = c['driver']; S = A.shape[0]
    z = np.random.default_rng(c['seed'] + 7919).standard_normal((N_DRAWS, c['T'], S))
    return dict(A=A, Q=Q, P0=P.copy(), Pinf=P, h_val=np.array(blk.h_val, float), block_offsets=np.array(blk.offsets, np.int32), Wnmf=np.array(pr['W']),
                D=np.array(d['D']), N=np.array(d['N']), ttau=ttau, tnu=tnu, y=y, z=z, predict_at_k1=np.array(False), seed=np.array(c['seed']),
                kernel1=np.array(d['k1']), kernel2=np.array(K2), param1=pr['param1'], param2=pr['param2'])


# ---------------------------------------------------------------------------------------------
# the restatement in fixed point
class Pivots:
    """the smallest |pivot| / max |diag| of one kind of factorisation and its count of structurally zero pivots"""

    def __init__(self):
        self.margin = math.inf; self.own = math.inf; self.zeros = 0

    def see(self, pivot, dmax, djj):
        if pivot == 0:
            self.zeros += 1
        else:
            self.margin = min(self.margin, abs(int(pivot)) / int(dmax))
            self.own = min(self.own, abs(int(pivot)) / abs(int(djj)))


def chol_fx(fx, a, clamp, piv):
    """lower Cholesky factor from the lower triangle of a.  clamp: a pivot <= 0 zeroes its column and is counted; not clamp: the first
    such pivot ends the attempt.  Returns (L, number of such pivots)."""
    n = a.shape[0]; L = np.zeros((n, n), dtype=object); bad = 0
    dmax = max(abs(int(a[j, j])) for j in range(n))
    for j in range(n):
        v = a[j:, j] - (np.dot(L[j:, :j], L[j, :j]) >> fx.p) if j else a[j:, j].copy()
        piv.see(v[0], dmax, a[j, j])
        if not v[0] > 0:
            bad += 1
            if not clamp:
                return L, bad
            continue                                                # the column stays zero
        d = math.isqrt(int(v[0]) << fx.p)
        L[j:, j] = (v << fx.p) // d
        L[j, j] = d
    return L, bad


def lower_sym(a):
    t = np.tril(a)
    return t + np.tril(a, -1).T


def run_case(inp, prec, sig=None):
    """nagp_ep_sample at `prec` bits -> (dict of fixed-point arrays Xdraw n x S x T, Fdraw n x M x T, MS S x T[, Sdraw n x T]), Fx,
    counters [retries, clamped], retry steps, the three Pivots"""
    mp.prec = prec + 64
    fx = Fx(prec); one = fx.one
    off = [int(o) for o in inp['block_offsets']]; M = len(off) - 1; S = off[-1]; T = inp['y'].size
    offa = np.array(off[:M])
    Ab = [fx.of(inp['A'][off[n]:off[n + 1], off[n]:off[n + 1]]) for n in range(M)]
    AbT = [b.T.copy() for b in Ab]
    QbT = [fx.of(inp['Q'][off[n]:off[n + 1], off[n]:off[n + 1]]).T.copy() for n in range(M)]
    Qd = fx.of(inp['Q']); hv = fx.of(inp['h_val'])
    tt = fx.of(inp['ttau']); tn = fx.of(inp['tnu']); yv = inp['y']
    pk1 = bool(inp['predict_at_k1'])

    def Amul(v):
        return np.concatenate([np.dot(Ab[n], v[off[n]:off[n + 1]]) >> prec for n in range(M)])

    m = np.zeros(S, dtype=object); P = fx.of(inp['P0'])
    MF = [None] * T; PF = [None] * T
    for k in range(T):
        if k > 0 or pk1:
            m = Amul(m)
            P = fx.bd_right_t(fx.bd_left(Ab, off, P), Ab, off) + Qd
        if not math.isnan(yv[k]):
            fmu = fx.mul(hv, m[offa]); W = fx.mul(P[:, offa], hv[None, :]); hph = fx.mul(fx.mul(hv, hv), P[offa, offa])
            ii = [n for n in range(M) if tt[n, k] == 0]; jj = [n for n in range(M) if tt[n, k] != 0]
            mn = m
            if ii:                                                  # -(ttau fmu - tnu) / (ttau HPH + 1) = tnu; K = 0
                mn = mn + fx.dot(W[:, ii], tn[ii, k])
            if jj:
                den = hph[jj] + fx.div(one, tt[jj, k])
                K = fx.div(W[:, jj], den[None, :])
                mn = mn + fx.dot(K, fx.div(tn[jj, k], tt[jj, k]) - fmu[jj])
                P = P - fx.dot(fx.mul(K, hv[jj][None, :]), P[offa[jj], :])
            m = mn
        MF[k] = m; PF[k] = P
    first, second, fac = Pivots(), Pivots(), Pivots()
    cnt = [0, 0]; steps = []
    G = [None] * T; Lc = [None] * T
    I = np.zeros((S, S), dtype=object)
    for i in range(S):
        I[i, i] = one
    for k in range(T - 1):
        PSkp = lower_sym(fx.bd_right_t(fx.bd_left(Ab, off, PF[k]), Ab, off) + Qd)
        L, bad = chol_fx(fx, PSkp, False, first)
        if bad:
            cnt[0] += 1; steps.append(k)
            L, bad = chol_fx(fx, PSkp + fx.mul(I, fx.of(JITTER)[()]), True, second)
            if bad:
                raise CaseRejected('PSkp is not positive definite even with the jitter at step %d' % k)
        G[k] = fx.right_solve_spd(fx.bd_right_t(PF[k], Ab, off), L)
        M1 = I - fx.bd_right_t(G[k], AbT, off)
        M1P = fx.dot(M1, PF[k])
        C = fx.dot(M1P, M1.T) + fx.dot(fx.bd_right_t(G[k], QbT, off), G[k].T)      # (G Q) G'
        Lc[k], bad = chol_fx(fx, C, True, fac); cnt[1] += bad
    Lc[T - 1], bad = chol_fx(fx, PF[T - 1], True, fac); cnt[1] += bad
    z = np.concatenate([fx.of(inp['z']), np.zeros((1, T, S), dtype=object)])       # the last one is the mean chain
    n1 = z.shape[0]
    X = np.zeros((n1, S, T), dtype=object)
    x = MF[T - 1][None, :] + fx.dot(z[:, T - 1, :], Lc[T - 1].T)
    X[:, :, T - 1] = x
    for k in range(T - 2, -1, -1):
        x = MF[k][None, :] + fx.dot(x - Amul(MF[k])[None, :], G[k].T) + fx.dot(z[:, k, :], Lc[k].T)
        X[:, :, k] = x
    out = dict(Xdraw=X[:n1 - 1], MS=X[n1 - 1])
    out['Fdraw'] = fx.mul(hv[None, :, None], out['Xdraw'][:, offa, :])
    if sig is not None:
        amp, link, shift = sig
        D = int(inp['D']); Wn = fx.of(inp['Wnmf'])
        lk, _ = link_funs(fx, 'exp' if link == LINK_EXP else 'softplus', shift)
        F = out['Fdraw']; Sd = np.zeros((n1 - 1, T), dtype=object)
        for i in range(n1 - 1):
            for t in range(T):
                a = fx.dot(Wn, np.array([lk(v) for v in F[i, D:, t]], dtype=object))
                if amp == AMP_SQRT:
                    a = np.array([math.isqrt(int(v) << prec) for v in a], dtype=object)
                Sd[i, t] = int(np.dot(a, F[i, :D, t])) >> prec
        out['Sdraw'] = Sd
    return out, fx, cnt, steps, (first, second, fac)


# ---------------------------------------------------------------------------------------------
def ref_model(inp, order='F'):
    return dict(A=np.array(inp['A'], order=order), Q=np.array(inp['Q'], order=order), Pinf=np.array(inp['P0'], order=order),
                offsets=np.asarray(inp['block_offsets']), h_val=np.asarray(inp['h_val'], float))


def ref_run(inp, sig=None, order='F', ref=None):
    """tests/epsample_ref.py on the inputs of a case -> (dict of the fixture's fields, counters, retry steps)"""
    if ref is None:
        import epsample_ref as ref
    s = None if sig is None else (inp['Wnmf'], int(sig[0]), int(sig[1]), float(sig[2]))
    with np.errstate(all='ignore'):
        X, F, Sd, MS, cnt, parts = ref.sample(ref_model(inp, order), inp['ttau'], inp['tnu'], inp['y'], bool(inp['predict_at_k1']), N_DRAWS, z=inp['z'], sig=s)
    out = dict(Xdraw=X, Fdraw=F, MS=MS)
    if Sd is not None:
        out['Sdraw'] = Sd
    return out, cnt, parts['retry_steps']


def rel_err(fx, got, ref):
    """max |got - ref| / max |ref| with got an f64 array taken exactly and ref fixed point"""
    got = np.asarray(got, float)
    assert got.shape == ref.shape and np.all(np.isfinite(got)), (got.shape, ref.shape)
    return ratio(fx, np.abs(fx.of(got) - ref).max(), np.abs(ref).max())


def ratio(fx, d, s):
    """d / s of two fixed-point numbers as a float; a field that is zero throughout (the means of a series without observations) has
    error 0 where it is met exactly"""
    if s == 0:
        return 0.0 if d == 0 else math.inf
    return float(fx.mpf(d) / fx.mpf(s))


def field_err(got, ref):
    """the suite's metric on f64 arrays: max-abs difference over the largest entry of the reference"""
    got = np.asarray(got, float); ref = np.asarray(ref, float)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert np.all(np.isfinite(got)), 'non-finite entries'
    return float(np.abs(got - ref).max() / (np.abs(ref).max() + 1e-300))


def bound(err):
    """the device bound of the sibling fixtures: min(max(10 x err_oracle, 1e-12), TOL_MEAN)"""
    return min(max(10.0 * float(err), 1e-12), TOL_MEAN)


def dead_states(c):
    return int(sum(c['blocks'][n] for n in c.get('dead', ()))) if 'blocks' in c else 0


def check_want(c, cnt, T):
    want = c['want']; r, cl = int(cnt[0]), int(cnt[1])
    if want == 'none' and (r or cl):
        raise CaseRejected('counters %s in a case without retries' % [r, cl])
    if want == 'some' and not (0 < r < T - 1 and cl > 0):
        raise CaseRejected('counters %s: not a retry at some steps only, with clamped pivots' % [r, cl])
    if want == 'all' and (r, cl) != (T - 1, dead_states(c) * T):
        raise CaseRejected('counters %s: not a retry at every step' % [r, cl])


def build_case(name, verbose=True):
    c = CASES[name]; t0 = time.time(); skipped = 0; sig = c.get('sig'); T = c['T']
    while True:
        try:
            inp = driver_inputs(c) if 'driver' in c else synthetic_inputs(c, c['seed'] + skipped)
            hi, fx, cnt, steps, piv = run_case(inp, PREC, sig)
            margins = np.array([p.margin for p in piv]); zeros = np.array([p.zeros for p in piv])
            own = np.array([p.own for p in piv])
            # the driver models are not balanced: the variances of their states span twelve decades, so no pivot of a small state reaches
            # 1e-6 of the largest diagonal entry whatever its sign margin; they are held to the scale-free figure alone
            if not (np.all(own >= MARGIN) and (np.all(margins >= MARGIN) or 'driver' in c)):
                raise CaseRejected('pivot margins %s (over each pivot\'s own diagonal entry %s) below %.0e' % (margins, own, MARGIN))
            check_want(c, cnt, T)
            break
        except CaseRejected as e:
            assert 'driver' not in c, 'driver case %s is rejected: %s' % (name, e)
            if verbose:
                print('%-12s seed %d rejected: %s' % (name, c['seed'] + skipped, e), flush=True)
            skipped += 1
            assert skipped < 100, 'no seed of case %s passes' % name
    lo, _, cnt2, steps2, piv2 = run_case(inp, PREC_LOW, sig)
    mp.prec = PREC + 64
    assert cnt == cnt2 and steps == steps2 and [p.zeros for p in piv2] == list(zeros)
    fields = [f for f in FIELDS if f in hi]
    agree = max(ratio(fx, np.abs(hi[f] - (lo[f] << (PREC - PREC_LOW))).max(), np.abs(hi[f]).max()) for f in fields)
    assert agree < 1e-60, (name, agree)
    err = np.zeros(len(FIELDS))
    for order in ('F', 'C'):
        o, ocnt, osteps = ref_run(inp, sig, order)
        assert list(ocnt) == cnt and list(osteps) == steps, (name, list(ocnt), cnt, list(osteps), steps)
        for j, f in enumerate(FIELDS):
            if f in hi:
                err[j] = max(err[j], rel_err(fx, o[f], hi[f]))
    assert np.all(10 * err < TOL_MEAN), (name, err)
    dead = [i for n in c.get('dead', ()) for i in range(int(inp['block_offsets'][n]), int(inp['block_offsets'][n + 1]))]
    for i in dead:                                                       # a state of zero variance: its draws are its filtered mean, which is zero
        assert not np.any(hi['Xdraw'][:, i, :]) and not np.any(hi['MS'][i])
    out = {k: v for k, v in inp.items() if k != 'Pinf'}
    out.update(counters=np.array(cnt, np.int64), retry_steps=np.array(steps, np.int64), margins=margins, margins_scaled=own, zero_pivots=zeros.astype(np.int64),
               err_oracle=err, agree_256_bits=np.array(agree), prec_bits=np.array(PREC), seeds_skipped=np.array(skipped),
               dead_states=np.array(dead, np.int64), has_sdraw=np.array(sig is not None))
    if sig is not None:
        out['sig'] = np.array(sig, float)
    for f in ('Xdraw', 'MS', 'Sdraw'):
        if f in hi:
            out[f] = fx.f64(hi[f])
    if verbose:
        print('%-12s S %2d T %2d  %4.0f s  seed +%d  counters %s  retry steps %s  margins %s (scaled %s)  zero pivots %s  320 vs 256 bits %.1e  err_oracle %s'
              % (name, inp['A'].shape[0], T, time.time() - t0, skipped, cnt, steps if len(steps) < 4 else '%d..%d' % (steps[0], steps[-1]),
                 ' '.join('%.1e' % v for v in margins), ' '.join('%.1e' % v for v in own), [int(v) for v in zeros], agree, ' '.join('%s %.1e' % (f, e) for f, e in zip(FIELDS, err) if f in hi)), flush=True)
    return {'%s__%s' % (name, k): v for k, v in out.items()}


def build(names, jobs=1):
    if jobs > 1:
        from multiprocessing import Pool
        order = sorted(names, key=lambda n: -sum(CASES[n].get('blocks', [25])) ** 3 * CASES[n]['T'])       # the long ones first
        with Pool(jobs) as pool:
            parts = dict(zip(order, pool.map(build_case, order, chunksize=1)))
        parts = [parts[n] for n in names]
    else:
        parts = [build_case(n) for n in names]
    arrays = {'cases': np.array(names), 'fields': np.array(FIELDS), 'margin_names': np.array(MARGIN_NAMES)}
    for p in parts:
        arrays.update(p)
    return arrays


# ---------------------------------------------------------------------------------------------
# the committed file: A, Q, P0 as their diagonal blocks
def pack_blocks(arrays):
    out = {}
    for k, v in arrays.items():
        name, _, key = k.partition('__')
        if key in ('A', 'Q', 'P0'):
            off = arrays[name + '__block_offsets']
            mask = np.zeros(v.shape, bool)
            for n in range(off.size - 1):
                mask[off[n]:off[n + 1], off[n]:off[n + 1]] = True
            assert not np.any(v[~mask])
            out[k + '_blocks'] = np.concatenate([v[off[n]:off[n + 1], off[n]:off[n + 1]].ravel() for n in range(off.size - 1)])
        else:
            out[k] = v
    return out


def unpack_blocks(g):
    out = {}
    for k in g:
        v = g[k]
        if k.endswith('_blocks'):
            off = g[k.partition('__')[0] + '__block_offsets']; S = int(off[-1]); X = np.zeros((S, S), order='F'); a = 0
            for n in range(off.size - 1):
                b = int(off[n + 1] - off[n]); X[off[n]:off[n + 1], off[n]:off[n + 1]] = v[a:a + b * b].reshape(b, b); a += b * b
            out[k[:-len('_blocks')]] = X
        else:
            out[k] = v
    return out


def load(path=OUT):
    """the fixture as one dict, A, Q, P0 dense again (column-major)"""
    with np.load(path) as g:
        return unpack_blocks({k: g[k] for k in g.files})


def case_of(g, name):
    """the arrays of one case of load()"""
    c = {k[len(name) + 2:]: v for k, v in g.items() if k.startswith(name + '__')}
    c['S'] = c['A'].shape[0]; c['T'] = c['y'].size; c['M'] = c['h_val'].size
    c['err'] = dict(zip(FIELDS, c['err_oracle']))
    return c


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--jobs', type=int, default=1, help='cases in parallel processes')
    ap.add_argument('--only', default='', help='comma-separated case names (with --check or --out elsewhere)')
    ap.add_argument('--check', action='store_true', help='compare with the committed fixture instead of writing it')
    ap.add_argument('--out', default=OUT)
    a = ap.parse_args()
    names = [n for n in a.only.split(',') if n] or list(CASES)
    arrays = build(names, a.jobs)
    if a.check:
        g = load(a.out)
        keys = [k for k in arrays if k != 'cases']
        bad = [k for k in keys if k not in g or not np.array_equal(np.asarray(arrays[k]), g[k], equal_nan=np.asarray(arrays[k]).dtype.kind == 'f')]
        if not a.only:
            bad += [k for k in g if k not in arrays]
        print('fixture matches' if not bad else 'differs in %s' % bad)
        sys.exit(1 if bad else 0)
    assert not a.only or a.out != OUT, 'a partial fixture is not written over the committed one'
    write_npz(a.out, pack_blocks(arrays))
    print('wrote %s (%d bytes)' % (os.path.relpath(a.out, ROOT), os.path.getsize(a.out)))


if __name__ == '__main__':
    main()
