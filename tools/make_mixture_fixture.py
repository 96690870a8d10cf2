"""Multi-precision fixture of the source-separation mixtures (NAGP_FLAG_MIXTURE_RULE): tests/golden/mixture_multiprecision.npz (inputs, gf
runs), with mixture_multiprecision_ihgp.npz (ihgp runs) and mixture_multiprecision_tables.npz (knot tables) beside it.

The machinery is that of tools/make_ep_fixture.py (mom in mpmath floats of PREC + 64 bits, the Kalman algebra in the integer fixed point of
tools/make_smoother_fixture.py at PREC = 320 bits, every run repeated at 256 bits, the knot tables as inputs through interp_rows); what is restated here
are the two runs of oracle/mixture.py as written:

  run_gf_mix    oracle/mixture.py:run_gf: mom at power alpha in the filter too, the refresh (1 - d) site + d / alpha (...) in both passes, R = 1 / ttau
                stored before the clamp, a clamp at every observed filter step, kalman_update_legacy (ONE branch for all sites: the information form
                as soon as any site of the step is 0), RTS by Cholesky without a jitter branch, the smoother's refresh only where v_cav > 0 and not
                clamped, R = 1 / ttau of every site behind it, maxDiffM / maxDiffP over the refreshed steps, nll = -sum lZ per sweep.
  run_ihgp_mix  oracle/mixture.py:run_ihgp: R starts at 0, m is set once before the sweeps (a sweep starts from the smoothed mean of step 0),
                nearest_index on the stored grid, the ttau == 0 branch, the backward pass from PGlist with the last index for R = Inf, the
                smoother's lZ added to nll for 1 < itt < sweeps, R[upd] only, Varft without abs, a missing y through mom as NaN (no isnan guard in
                the filter: NaN sites, clamped to 0, tnu stays NaN), maxDiffP from the smoothed P of step 0 against the previous sweep's.

Inputs are the f64 arrays the product is handed for the stacked model (nagp.api._stack_sources, nagp.ss.discretise: all sub-band blocks of all
sources, then all modulator blocks, block-diagonal Wnmf, no balancing), stored as diagonal blocks.

Margins (MARGIN: those of make_ep_fixture plus cavity_sign): the relative distance of a looked-up R to the mid-point of its cell, |ttau| ahead of a clamp
against the run's largest (every refreshed value the next clamp meets, the negative sites the smoother leaves included), |1 - alpha ttau vm| of every
cavity, |1 + d2lZ v| of every refreshed site, sum w normpdf wherever y is observed, and cavity_sign = min |1 / vm - alpha ttau| / (1 / vm): where the
EP tool rejects a case on a cavity variance that is not positive, this one masks the site as the rule does (the count is stored as `masked`) and
holds the sign to that margin.  A masked MODULATOR site is still a rejection (mom would take the root of its variance), and so is a cubature
point whose variance sn2 / alpha + a^2 . s2 is not positive.  Every margin is asserted per run; the smallest is stored.

A case walks seeds upwards from its base seed, each family on its own (the two are independent runs): `seed`, `seeds_skipped`, `w_lik` are stored per
family.  The walk is capped at 400 seeds; a family that finds none at w_lik = 1e-4 goes on at 1e-2, then to the same two at the signal's own scale (LEVELS
below; said in its stored `recipe`), and is dropped if all fail.  harness.mixture_problem normalises the signal to unit variance, some ten times the scale
of the model it was drawn from: the infinite-horizon filter, whose predictive variances are the steady-state ones from the first step, then sits on the
jitter floor of mom (sum w normpdf < 1e-10) at almost every step, on every seed, and the floor margin cannot hold; its committed runs are on the prior
samples as drawn.  If no committed ihgp run holds a masked site, case m2 walks again at twice that scale until one does (`recipe` says so).

Counts, per run: `clamped` -- entries of ttau that a clamp of the oracle found not positive, over every clamp it executes (ihgp: every step of every
sweep; gf: every observed step of every sweep); `clamped_adf` -- those among them that the filter's own ADF refresh had just written (sweep 1, and
step T - 1 later); `masked` -- sites left out of a smoother refresh by v_cav <= 0.

err_oracle(field): oracle/mixture.py on the same f64 inputs, model column- and row-major, the worse of the two, max-abs over the field's largest entry
(|d| / |nll| entry by entry for nll).  10 x err_oracle < TOL(field) is asserted (TOL: 1e-7 means, PS and maxDiff, 1e-6 sites and R, 1e-8 lZ and nll).

Run:  python tools/make_mixture_fixture.py --jobs 5     (7 minutes on eight cores: m2 190 s and again 150 s for its masked-site walk over 32 seeds, m3 200 s, the
                                                         others 30 - 45 s; the 800 seeds an ihgp family turns away at the unit-variance levels cost 30 - 150 s of that per case)
      python tools/make_mixture_fixture.py --check --jobs 5      (recompute and compare with the committed files, err_oracle left out: 7 minutes)
      python tools/make_mixture_fixture.py --check --only m1 [--sweeps 1]      (some cases / one sweep count, each family's walk started at its committed seed)
      python tools/make_mixture_fixture.py --check --only m1 --sweeps 1 --stored-inputs      (the restatement alone, from the committed inputs: 4 s, the same bytes on any host)
The output is reproducible bit for bit.
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

import make_ep_fixture as ep                                                # noqa: E402
from make_ep_fixture import (MpMom, Sites, CaseRejected, interp_rows, grid_tables, flat_tables, tables_digest, pack_ps, ps_selection,      # noqa: E402,F401
                             dense_H, oracle_mom, pack_blocks, unpack_blocks, to_f64, LIK_NMF, LIK_SQRT, PREC, PREC_LOW,
                             _max0, _isnan, _mpf_rows, _nearest, _lookup_margin)
from nagp import cubature, harness, ihgp_tables, ss as pss                  # noqa: E402

try:
    from mpmath import mp, mpf
    from make_smoother_fixture import Fx, write_npz                         # noqa: E402
except ImportError:                                                         # pragma: no cover
    mp = mpf = Fx = write_npz = None

OUT = os.path.join(ROOT, 'tests', 'golden', 'mixture_multiprecision.npz')
OUT_IHGP, OUT_TABLES = ep.OUT_IHGP, ep.OUT_TABLES
ALPHA, DAMPING = 0.75, 0.2                                                  # source_sep_piano.m:86; scalar damping
SWEEPS = (1, 3)
# the levels of a family's walk: (signal, w_lik).  'unit': harness.mixture_problem's signal, normalised to unit variance; 'prior': the same sum of prior
# samples left at the model's own scale; 'prior*2': twice that (only the walk for a masked site goes there)
LEVELS = (('unit', 1e-4), ('unit', 1e-2), ('prior', 1e-4), ('prior', 1e-2), ('prior*2', 1e-4))
N_LEVELS = 4
MAX_SEEDS = 400
MARGIN = dict(ep.MARGIN, cavity_sign=1e-3)
TOL = dict(ep.TOL, nll=ep.TOL_LOGZ, maxDiffM=ep.TOL_MEAN, maxDiffP=ep.TOL_MEAN)
FIELDS = dict(gf=('MF', 'MS', 'Eft', 'Varft', 'ttau', 'tnu', 'R', 'lZ', 'nll', 'maxDiffM', 'maxDiffP', 'PS'),
              ihgp=('MF', 'MS', 'Eft', 'Varft', 'ttau', 'tnu', 'R', 'nll', 'maxDiffM', 'maxDiffP'))
MASKS = ('ttau', 'tnu', 'R')
K52 = 'matern52'

CASES = {
    'm1': dict(shapes=[(3, 1), (2, 2)], k1=['exp', 'matern32'], k2=[K52, K52], lik=LIK_NMF, shift=0.0, p=7, T=36, seed=21),
    'm1b': dict(shapes=[(3, 1), (2, 2)], k1=['exp', 'matern32'], k2=[K52, K52], lik=LIK_NMF, shift=0.0, p=7, T=36, seed=521),     # m1's shape and mom, another model and signal: the second segment of a batch
    'm2': dict(shapes=[(4, 2), (4, 2), (3, 1)], k1=['exp'] * 3, k2=[K52, 'matern32', K52], lik=LIK_SQRT, shift=1.0, p=7, T=36, seed=21),
    'm3': dict(shapes=[(4, 3)] * 3, k1=['exp'] * 3, k2=[K52] * 3, lik=LIK_SQRT, shift=1.0, p=5, T=24, seed=21),
    'm4': dict(shapes=[(3, 1), (2, 2)], k1=[K52, 'matern32'], k2=[K52, K52], lik=LIK_NMF, shift=0.0, p=7, T=36, seed=21),
}
FAMILIES = ('gf', 'ihgp')


def fields_of(family, itts=None):
    return FIELDS[family]


# ---------------------------------------------------------------------------------------------
# the f64 inputs, as the product forms them
def source_cell(fi):
    """The cell w = {log sn2, {param1_j}, {param2_j}, {W_j}} of a stored family: what the entry points are called with."""
    sd = [int(v) for v in fi['src_D']]; sn = [int(v) for v in fi['src_N']]
    p1s, p2s, Ws = [], [], []; a = b = d0 = n0 = 0
    for D_, N_ in zip(sd, sn):
        p1s.append(fi['param1'][a:a + 3 * D_]); a += 3 * D_
        p2s.append(fi['param2'][b:b + 2 * N_]); b += 2 * N_
        Ws.append(fi['Wnmf'][d0:d0 + D_, n0:n0 + N_]); d0 += D_; n0 += N_
    return [np.array(fi['lik_param'], float), p1s, p2s, Ws]


def stacked(fi, sh, family):
    """(blk, Wnmf, lik_param, A, Q, Pinf) of nagp.api._stack_sources and nagp.ss.discretise for this family."""
    from nagp import api
    k1 = [str(v) for v in sh['kernel1']]; k2 = [str(v) for v in sh['kernel2']]
    blk, W, lik = api._stack_sources(api.SSHandle(), None, source_cell(fi), k1, k2, len(k1))
    A, Q, P = pss.discretise(blk, symmetrize_Q=(family == 'ihgp'))
    return blk, W, lik, np.array(A), np.array(Q), np.array(P)


def shared_inputs(c):
    N = sum(n for _, n in c['shapes'])
    wn, xn = cubature.utp_ws(c['p'], N) if c['lik'] == LIK_SQRT else cubature.sigma_points(c['p'], N)
    return dict(wn=np.array(wn, float).ravel(), xn_unscaled=np.array(xn, float), lik_kind=np.array(c['lik']), link=np.array('softplus'),
                link_shift=np.array(float(c['shift'])), p_cubature=np.array(c['p']), kernel1=np.array(c['k1']), kernel2=np.array(c['k2']),
                ep_fraction=np.array(ALPHA), ep_damping=np.array([DAMPING]), T=np.array(c['T']))


def prior_signal(c, mpb, seed):
    """The sum of harness.mixture_problem's prior samples (one per source, the same generators) before it is normalised to unit variance."""
    y = np.zeros(c['T'])
    for j in range(len(c['shapes'])):
        blk = pss.ss_blocks_nmf(mpb['w'][1][j], mpb['w'][2][j], c['k1'][j], c['k2'][j])
        y = y + harness.sample_prior(blk, mpb['w'][3][j], c['T'], np.random.default_rng(seed + 7919 + j))
    return y


def family_inputs(c, sh, family, seed, w_lik, scale='unit'):
    T = c['T']
    mpb = harness.mixture_problem(c['shapes'], T, seed, c['k1'], c['k2'], w_lik=w_lik)
    y = mpb['y'].copy() if scale == 'unit' else prior_signal(c, mpb, seed) * float(scale.partition('*')[2] or 1)
    y[T // 3] = np.nan
    fi = dict(scale=np.array(scale), src_D=np.array([d for d, _ in c['shapes']]), src_N=np.array([n for _, n in c['shapes']]), param1=np.concatenate(mpb['w'][1]),
              param2=np.concatenate(mpb['w'][2]), lik_param=np.array(mpb['w'][0], float), y=y, seed=np.array(seed), w_lik=np.array(w_lik))
    fi['D'] = np.array(int(fi['src_D'].sum())); fi['N'] = np.array(int(fi['src_N'].sum()))
    import scipy.linalg as sla
    fi['Wnmf'] = sla.block_diag(*mpb['w'][3])
    blk, W, lik, A, Q, P = stacked(fi, sh, family)
    assert np.array_equal(W, fi['Wnmf']) and np.array_equal(lik, fi['lik_param'])
    fi.update(A=A, Q=Q, Pinf=P, h_val=np.array(blk.h_val, float), block_offsets=np.array(blk.offsets, np.int32))
    if family == 'ihgp':
        ro, PPs, PGs, good = ihgp_tables.build_knots(A, Q, blk.offsets, blk.h_val)
        if not all(len(g) == ro.size for g in good):
            raise CaseRejected('a knot of the look-up tables was dropped')
        fi.update(ro=ro, r=np.logspace(-2, 4, 200), tab_src=np.arange(blk.M, dtype=np.int32), PPo=np.concatenate([x.ravel() for x in PPs]),
                  PGo=np.concatenate([x.ravel() for x in PGs]))
        fi['tab_digest'] = np.array(tables_digest(fi))
    return fi


def merged(sh, fi):
    d = dict(sh); d.update(fi)
    return d


# ---------------------------------------------------------------------------------------------
# the sites under the mixtures' rule
def _new_margins():
    return {k: math.inf for k in MARGIN}


class MixSites(Sites):
    """Sites with the refresh of oracle/mixture.py:_refresh, the mask of the smoother's refresh, and margins that end a run as soon as one fails."""

    def __init__(self, M, T, D, margins):
        Sites.__init__(self, M, T, margins, [])
        self.D = D; self.masked = 0; self.clamped_adf = 0; self.fresh = set(); self.adf = set()

    def note(self, key, val):
        val = float(val)
        if val < self.mg[key]:
            self.mg[key] = val
            if not val >= MARGIN[key]:
                raise CaseRejected('margin %s = %.2e below %.0e' % (key, val, MARGIN[key]))

    def denom(self, d2, v):
        z = 1 + d2 * v
        self.note('denom', abs(z))
        return z

    def call(self, mom, mu, s2, alpha, y):
        try:
            res = mom(mu, s2, alpha, y)
        except CaseRejected:
            raise
        except Exception as e:                                          # a cubature point with sn2 / alpha + a^2 . s2 <= 0: the root leaves the reals
            raise CaseRejected('mom: %s' % type(e).__name__)
        if not isinstance(res[0], mpf):
            raise CaseRejected('mom left the reals')
        if y is not None and not self.mg['floor'] >= MARGIN['floor']:
            raise CaseRejected('margin floor = %.2e' % self.mg['floor'])
        return res

    def refresh(self, n, k, mean, var, dl, d2, d, a):
        z = self.denom(d2, var)
        self.ttau[n][k] = (1 - d) * self.ttau[n][k] + d / a * (-d2 / z)
        self.tnu[n][k] = (1 - d) * self.tnu[n][k] + d / a * ((dl - mean * d2) / z)
        self.fresh.add((n, k))

    def filter_update(self, k, fmu, hph, mom, y, alpha, d):
        """mom at power alpha and the refresh of every site -> lZ_k; a missing y (ihgp) leaves NaN sites."""
        a = mpf(alpha)
        lZ, dl, d2 = self.call(mom, fmu, hph, a, y)
        for n in range(self.M):
            if y is None:
                self.ttau[n][k] = mp.nan; self.tnu[n][k] = mp.nan
            else:
                self.refresh(n, k, fmu[n], hph[n], dl[n], d2[n], d, a)
                self.adf.add((n, k))
        return lZ

    def smoother_update(self, k, mm, vm, mom, y, alpha, d):
        """Cavity, mom, refresh where v_cav > 0 -> lZ_k, upd[M]; ttau is left unclamped."""
        a = mpf(alpha); vc, mc, upd = [], [], []
        for n in range(self.M):
            if not vm[n] > 0:
                raise CaseRejected('a smoothed variance is not positive')
            one = 1 - a * self.ttau[n][k] * vm[n]
            self.note('cavity', abs(one)); self.note('cavity_sign', abs(1 / vm[n] - a * self.ttau[n][k]) * vm[n])
            v = 1 / (1 / vm[n] - a * self.ttau[n][k])
            upd.append(bool(v > 0))
            if not upd[-1] and n >= self.D:
                raise CaseRejected('the cavity variance of a modulator site is not positive')
            vc.append(v); mc.append(v * (mm[n] / vm[n] - a * self.tnu[n][k]))
        lZ, dl, d2 = self.call(mom, mc, vc, a, y)
        for n in range(self.M):
            if upd[n]:
                self.refresh(n, k, mc[n], vc[n], dl[n], d2[n], d, a)
            else:
                self.masked += 1
        return lZ, upd

    def clamp(self, k):
        for n in range(self.M):
            t = self.ttau[n][k]
            if (n, k) in self.fresh:
                self.fresh.discard((n, k)); self.pre_clamp.append(t)
            if not t > 0:
                self.clamped += 1
                if (n, k) in self.adf:
                    self.clamped_adf += 1
            self.adf.discard((n, k))
            self.ttau[n][k] = _max0(t)

    def finish(self):
        big = max(abs(v) for v in self.pre_clamp)
        self.note('clamp', min(abs(v) for v in self.pre_clamp) / big)


def _recip(t):
    return mp.nan if _isnan(t) else (mp.inf if t == 0 else 1 / t)


def _masks(st, R):
    nan = {f: np.array([[bool(_isnan(v)) for v in rw] for rw in x]) for f, x in (('ttau', st.ttau), ('tnu', st.tnu), ('R', R))}
    inf = {f: np.array([[bool(mp.isinf(v)) for v in rw] for rw in x]) for f, x in (('ttau', st.ttau), ('tnu', st.tnu), ('R', R))}
    return nan, inf


def _setup(inp, prec):
    mp.prec = prec + 64
    fx = Fx(prec); mg = _new_margins()
    off = [int(o) for o in inp['block_offsets']]; M = len(off) - 1; T = inp['y'].size
    Ab = [fx.of(inp['A'][off[n]:off[n + 1], off[n]:off[n + 1]]) for n in range(M)]
    ys = [None if math.isnan(v) else mpf(float(v)) for v in inp['y']]
    st = MixSites(M, T, int(inp['D']), mg)
    return fx, mg, MpMom(inp, mg), off, M, off[-1], T, Ab, fx.of(inp['h_val']), ys, st, mpf(float(inp['ep_damping'][0])), float(inp['ep_fraction'])


def run_gf_mix(inp, itts, prec):
    """oracle/mixture.py:run_gf at `prec` bits."""
    fx, mg, mom, off, M, S, T, Ab, hv, ys, st, d, alpha = _setup(inp, prec)
    offa = np.array(off[:M]); Qd = fx.of(inp['Q']); hh = np.outer(hv, hv) >> prec
    lZ = [mpf(0)] * T; R = [[mpf(0)] * T for _ in range(M)]
    MS = np.zeros((S, T), dtype=object); PS = [np.zeros((S, S), dtype=object) for _ in range(T)]
    mdM = [mpf(0)] * itts; mdP = [mpf(0)] * itts; nll = [mpf(0)] * itts
    for itt in range(1, itts + 1):
        m = np.zeros(S, dtype=object); P = fx.of(inp['Pinf'])
        hm_prev = [fx.mul(hv, MS[offa, k]) for k in range(T)]; hp_prev = [fx.mul(hh, PS[k][np.ix_(offa, offa)]) for k in range(T)]
        dM = dP = 0
        for k in range(T):
            if k > 0:
                m = np.concatenate([np.dot(Ab[n], m[off[n]:off[n + 1]]) >> prec for n in range(M)])
                P = fx.bd_right_t(fx.bd_left(Ab, off, P), Ab, off) + Qd
            if ys[k] is not None:
                fmu_x = fx.mul(hv, m[offa]); W = fx.mul(P[:, offa], hv[None, :]); hph_x = fx.mul(fx.mul(hv, hv), P[offa, offa])
                fmu = [fx.mpf(v) for v in fmu_x]; hph = [fx.mpf(v) for v in hph_x]
                if itt == 1 or k == T - 1:
                    lZ[k] = st.filter_update(k, fmu, hph, mom, ys[k], alpha, d)
                    for n in range(M):
                        R[n][k] = _recip(st.ttau[n][k])                # before the clamp
                st.clamp(k)
                tt = [st.ttau[n][k] for n in range(M)]; tn = [st.tnu[n][k] for n in range(M)]
                if min(tt) == 0:                                       # kalman_update_legacy: one branch for all the sites of the step
                    v = np.array([fx.from_mpf((tt[n] * fmu[n] - tn[n]) / (tt[n] * hph[n] + 1)) for n in range(M)], dtype=object)
                    g = np.array([fx.from_mpf(tt[n] / (tt[n] * hph[n] + 1)) for n in range(M)], dtype=object)
                    m = m - fx.dot(W, v)
                    P = P - fx.dot(fx.mul(W, g[None, :]), W.T)
                else:
                    den = np.array([fx.from_mpf(hph[n] + 1 / tt[n]) for n in range(M)], dtype=object)
                    K = fx.div(W, den[None, :])
                    v = np.array([fx.from_mpf(tn[n] / tt[n] - fmu[n]) for n in range(M)], dtype=object)
                    m = m + fx.dot(K, v)
                    P = P - fx.dot(fx.mul(K, hv[None, :]), P[offa, :])                          # (K H) P
            MS[:, k] = m; PS[k] = P
        MF = MS.copy()
        for k in range(T - 2, -1, -1):
            PSkp = fx.bd_right_t(fx.bd_left(Ab, off, PS[k]), Ab, off) + Qd
            try:
                G = fx.right_solve_spd(fx.bd_right_t(PS[k], Ab, off), fx.chol(PSkp))
            except ArithmeticError as e:
                raise CaseRejected(str(e))
            Am = np.concatenate([np.dot(Ab[n], MS[off[n]:off[n + 1], k]) >> prec for n in range(M)])
            m = MS[:, k] + fx.dot(G, m - Am)
            P = PS[k] + fx.dot(fx.dot(G, P - PSkp), G.T)
            MS[:, k] = m; PS[k] = P
            if itt < itts and ys[k] is not None:
                hm = fx.mul(hv, m[offa]); hp = fx.mul(hh, P[np.ix_(offa, offa)])
                mm = [fx.mpf(v) for v in hm]; vm = [fx.mpf(v) for v in np.diag(hp)]
                st.smoother_update(k, mm, vm, mom, ys[k], alpha, d)
                for n in range(M):
                    R[n][k] = _recip(st.ttau[n][k])
                dM = max(dM, max(abs(v) for v in hm_prev[k] - hm)); dP = max(dP, max(abs(v) for v in (hp_prev[k] - hp).ravel()))
        mdM[itt - 1] = fx.mpf(dM); mdP[itt - 1] = fx.mpf(dP); nll[itt - 1] = -sum(lZ)
    st.finish()
    Eft = fx.mul(hv[:, None], MS[offa])
    Varft = np.array([[fx.mul(fx.mul(hv[n], hv[n]), PS[k][off[n], off[n]]) for k in range(T)] for n in range(M)], dtype=object)
    out = dict(MF=MF, MS=MS, Eft=Eft, Varft=Varft, PS=np.array(PS, dtype=object), ttau=_mpf_rows(fx, st.ttau), tnu=_mpf_rows(fx, st.tnu), R=_mpf_rows(fx, R),
               lZ=_mpf_rows(fx, [lZ])[0], nll=_mpf_rows(fx, [nll])[0], maxDiffM=_mpf_rows(fx, [mdM])[0], maxDiffP=_mpf_rows(fx, [mdP])[0])
    nan, inf = _masks(st, R)
    return out, fx, mg, nan, inf, dict(clamped=st.clamped, clamped_adf=st.clamped_adf, masked=st.masked)


def run_ihgp_mix(inp, itts, prec, tables=None):
    """oracle/mixture.py:run_ihgp at `prec` bits on the 200-point tables of grid_tables(inp), taken as exact numbers."""
    fx, mg, mom, off, M, S, T, Ab, hv, ys, st, d, alpha = _setup(inp, prec)
    bs = [off[n + 1] - off[n] for n in range(M)]
    r, PPl, PGl = tables if tables is not None else grid_tables(inp)
    r_mp = [mpf(float(v)) for v in r]
    Pinf = [fx.of(inp['Pinf'][off[n]:off[n + 1], off[n]:off[n + 1]]) for n in range(M)]
    cache = {}

    def row(kind, n, ind):
        key = (kind, n, ind)
        if key not in cache:
            b = bs[n]; src = PPl[n][ind] if kind == 'pp' else PGl[n][ind]
            if kind == 'pp':
                cache[key] = fx.of(src.reshape((b, b), order='F'))
            else:
                cache[key] = (fx.of(src[:b * b].reshape((b, b), order='F')), fx.of(src[b * b:].reshape((b, b), order='F')))
        return cache[key]

    def look(Rv):
        before = mg['lookup']
        _lookup_margin(r_mp, Rv, mg)
        if mg['lookup'] < before and not mg['lookup'] >= MARGIN['lookup']:
            raise CaseRejected('margin lookup = %.2e' % mg['lookup'])

    R = [[mpf(0)] * T for _ in range(M)]                               # R starts at 0 (:248)
    m = [np.zeros(b, dtype=object) for b in bs]                        # set once, before the sweeps
    MS = [[np.zeros(b, dtype=object) for _ in range(T)] for b in bs]
    v0_prev = [fx.mul(fx.mul(hv[n], hv[n]), Pinf[n][0, 0]) for n in range(M)]
    mdM = [mpf(0)] * itts; mdP = [mpf(0)] * itts; nll = [mpf(0)] * itts
    for itt in range(1, itts + 1):
        lZ = mpf(0); dM = 0
        hm_prev = [[fx.mul(hv[n], MS[n][k][0]) for k in range(T)] for n in range(M)]
        for k in range(T):
            PP = []
            for n in range(M):
                if k > 0:
                    look(R[n][k - 1])
                    PP.append(row('pp', n, _nearest(r_mp, R[n][k - 1])))
                else:
                    PP.append(Pinf[n])
            Am = [np.dot(Ab[n], m[n]) >> prec for n in range(M)]
            Wc = [fx.mul(PP[n][:, 0], hv[n]) for n in range(M)]
            fmu = [fx.mpf(fx.mul(hv[n], Am[n][0])) for n in range(M)]; hph = [fx.mpf(fx.mul(hv[n], Wc[n][0])) for n in range(M)]
            if itt == 1 or k == T - 1:
                lZ += st.filter_update(k, fmu, hph, mom, ys[k], alpha, d)
                for n in range(M):
                    R[n][k] = _recip(st.ttau[n][k])                    # before the clamp
            st.clamp(k)
            for n in range(M):
                if st.ttau[n][k] == 0:
                    R[n][k] = mp.inf
                    m[n] = Am[n]
                else:
                    ysn = st.tnu[n][k] / st.ttau[n][k]
                    K = fx.div(Wc[n], fx.from_mpf(hph[n] + R[n][k]))
                    AKHA = Ab[n] - fx.mul(np.outer(K, Ab[n][0]) >> prec, hv[n])
                    m[n] = (np.dot(AKHA, m[n]) >> prec) + fx.mul(K, fx.from_mpf(ysn))
                MS[n][k] = m[n]
        MF = [list(rw) for rw in MS]
        Plast = [None] * M
        for k in range(T - 2, -1, -1):
            mm, vm, hm = [], [], []
            for n in range(M):
                look(R[n][k])
                ind = len(r_mp) - 1 if mp.isinf(R[n][k]) else _nearest(r_mp, R[n][k])
                Pn, Gn = row('pg', n, ind)
                Plast[n] = Pn
                m[n] = MS[n][k] + (np.dot(Gn, m[n] - (np.dot(Ab[n], MS[n][k]) >> prec)) >> prec)
                MS[n][k] = m[n]
                hm.append(fx.mul(hv[n], m[n][0]))
                mm.append(fx.mpf(hm[-1])); vm.append(fx.mpf(fx.mul(fx.mul(hv[n], hv[n]), Pn[0, 0])))
            if itt < itts and ys[k] is not None:
                lZk, upd = st.smoother_update(k, mm, vm, mom, ys[k], alpha, d)
                if itt > 1:
                    lZ += lZk
                for n in range(M):
                    if upd[n]:
                        R[n][k] = _recip(st.ttau[n][k])                # R[upd] only, no clamp here
                dM = max(dM, max(abs(hm_prev[n][k] - hm[n]) for n in range(M)))
        v0 = [fx.mul(fx.mul(hv[n], hv[n]), Plast[n][0, 0]) for n in range(M)]
        mdM[itt - 1] = fx.mpf(dM); mdP[itt - 1] = fx.mpf(max(abs(a - b) for a, b in zip(v0_prev, v0))); nll[itt - 1] = -lZ
        v0_prev = v0
    st.finish()
    MFa = np.concatenate([np.array([MF[n][k] for k in range(T)], dtype=object).T for n in range(M)], axis=0)
    MSa = np.concatenate([np.array([MS[n][k] for k in range(T)], dtype=object).T for n in range(M)], axis=0)
    offa = np.array(off[:M])
    Eft = fx.mul(hv[:, None], MSa[offa])
    Varft = np.array([[v] * T for v in v0], dtype=object)              # no abs() here (:510)
    out = dict(MF=MFa, MS=MSa, Eft=Eft, Varft=Varft, ttau=_mpf_rows(fx, st.ttau), tnu=_mpf_rows(fx, st.tnu), R=_mpf_rows(fx, R),
               nll=_mpf_rows(fx, [nll])[0], maxDiffM=_mpf_rows(fx, [mdM])[0], maxDiffP=_mpf_rows(fx, [mdP])[0])
    nan, inf = _masks(st, R)
    return out, fx, mg, nan, inf, dict(clamped=st.clamped, clamped_adf=st.clamped_adf, masked=st.masked)


RUN = dict(gf=run_gf_mix, ihgp=run_ihgp_mix)


# ---------------------------------------------------------------------------------------------
# oracle/mixture.py on the same inputs
class _Disc:
    """Stands in for oracle.ss inside oracle/mixture.py while it runs on the stored model: lti_disc hands back the stored A, Q."""

    def __init__(self, A, Q):
        self.A, self.Q = A, Q

    def lti_disc(self, F, L, Qc, dt):
        return self.A.copy(), self.Q.copy()


def oracle_run(inp, family, itts, mom=None, mixture=None):
    """oracle/mixture.py:run_gf / run_ihgp on the stored A, Q, Pinf, H -> dict of the fixture's fields (PS as a list).  `mixture`: a stand-in for the
    oracle's module (the wrong-oracle variants of the tests)."""
    from oracle import mixture as omx
    mod = mixture or omx
    S = inp['A'].shape[0]
    model = dict(F=inp['A'], L=None, Qc=None, H=dense_H(inp['h_val'], inp['block_offsets'], S), Pinf=inp['Pinf'], Wnmf=inp['Wnmf'], lik_param=inp['lik_param'])
    mom = mom or oracle_mom(inp)
    keep = mod.ssm; mod.ssm = _Disc(inp['A'], inp['Q'])
    try:
        with np.errstate(all='ignore'):
            if family == 'gf':
                o = mod.run_gf(model, inp['y'], mom, float(inp['ep_fraction']), inp['ep_damping'], itts)
                assert o['counters'].get('chol_retries', 0) == 0
                o['PS'] = [o['PS'][k] for k in range(inp['y'].size)]
            else:
                r, PPl, PGl = grid_tables(inp)
                o = mod.run_ihgp(model, inp['y'], mom, float(inp['ep_fraction']), inp['ep_damping'], itts, tables=([int(v) for v in inp['block_offsets']], r, PPl, PGl))
    finally:
        mod.ssm = keep
    return o


def oracle_runs(inp, family, itts):
    outs = []
    for order in ('F', 'C'):
        i2 = dict(inp); i2.update({k: np.array(inp[k], order=order) for k in ('A', 'Q', 'Pinf')})
        outs.append(oracle_run(i2, family, itts))
    return outs


def field_err(got, ref, field):
    """ep.field_err (NaN / Inf patterns must agree; max-abs over the largest entry); nll entry by entry as nlZ; a field that is all zero (maxDiffM of
    a run whose last sweep refreshes nothing) must be zero."""
    ref = np.asarray(ref, float)
    if field in ('maxDiffM', 'maxDiffP') and not np.any(ref):
        return 0.0 if not np.any(np.asarray(got, float)) else math.inf
    return ep.field_err(got, ref, 'nlZ' if field == 'nll' else field)


def bound(err, field):
    """min(max(10 x err_oracle, 1e-12), TOL)."""
    return min(max(10.0 * float(err), 1e-12), TOL[field])


def pack_fields(o, family, steps, S):
    out = {f: np.asarray(o[f]) for f in FIELDS[family] if f != 'PS' and f in o and o[f] is not None}
    if family == 'gf' and o.get('PS') is not None:
        out['PS'] = pack_ps(o['PS'], steps, S)
    return out


def agree(hi, lo, fields):
    worst = 0.0
    for f in fields:
        dd = np.abs(hi[f] - (lo[f] << (PREC - PREC_LOW))).max(); s = np.abs(hi[f]).max()
        if int(s) == 0:
            assert int(dd) == 0
            continue
        worst = max(worst, float(mpf(int(dd)) / mpf(int(s))))
    return worst


def build_run(inp, family, itts, need_masked=False):
    """One (family, sweep count): both precisions, agreement, margins, err_oracle -> dict of stored arrays."""
    S = inp['A'].shape[0]; T = inp['y'].size
    hi, fx, mg, nan, inf, cnt = RUN[family](inp, itts, PREC)
    if need_masked and cnt['masked'] == 0:
        raise CaseRejected('no masked site')
    lo, _, _, nan2, inf2, cnt2 = RUN[family](inp, itts, PREC_LOW)
    mp.prec = PREC + 64
    assert all(np.array_equal(nan[f], nan2[f]) and np.array_equal(inf[f], inf2[f]) for f in MASKS) and cnt == cnt2
    steps, _ = ps_selection(S, T, [T // 3])
    if family == 'gf':
        hi['PS'] = pack_ps(hi['PS'], steps, S); lo['PS'] = pack_ps(lo['PS'], steps, S)
    fields = FIELDS[family]
    ag = agree(hi, lo, fields)
    assert ag < 1e-60, (family, itts, ag)
    ref = to_f64(fx, {f: hi[f] for f in fields}, nan, inf)
    runs = [pack_fields(o, family, steps, S) for o in oracle_runs(inp, family, itts)]
    err = np.zeros(len(fields))
    for j, f in enumerate(fields):
        try:
            err[j] = max(field_err(o[f], ref[f], f) for o in runs)
        except AssertionError as e:
            raise CaseRejected('oracle: %s' % e)
        if not 10 * err[j] < TOL[f]:
            raise CaseRejected('10 x err_oracle(%s) = %.1e reaches the tolerance %.0e' % (f, 10 * err[j], TOL[f]))
    out = dict(ref)
    out.update(err_oracle=err, agree_256_bits=np.array(ag), margins=np.array([mg[k] for k in MARGIN]), prec_bits=np.array(PREC),
               clamped=np.array(cnt['clamped']), clamped_adf=np.array(cnt['clamped_adf']), masked=np.array(cnt['masked']))
    for f in MASKS:
        out['nan_' + f] = nan[f]; out['inf_' + f] = inf[f]
    if family == 'gf':
        out['ps_steps'] = steps
    return out


def stored_case(g, name):
    """(shared, {family: inputs}) of a case as the fixture `g` (load()) holds them."""
    pre = name + '__'; fams = {str(f): {} for f in g[pre + 'families']}; sh = {}
    for k in g:
        if k.startswith(pre):
            parts = k[len(pre):].split('__')
            if parts[0] in fams:
                if len(parts) == 2:
                    fams[parts[0]][parts[1]] = g[k]
            else:
                sh[parts[0]] = g[k]
    return sh, fams


def build_family(name, family, sweeps, sh, start=(0, 0), need_masked=False, stored=None, verbose=True):
    """Walk the seeds of one family -> (inputs, {key: array}) or None (dropped); start = (index into W_LIKS, seeds skipped at that w_lik)."""
    c = CASES[name]; worst = {}
    for wi in range(start[0], len(LEVELS) if need_masked else N_LEVELS):
        scale, w_lik = LEVELS[wi]
        for skipped in range(start[1] if wi == start[0] else 0, MAX_SEEDS):
            seed = c['seed'] + skipped
            try:
                fi = stored if stored is not None else family_inputs(c, sh, family, seed, w_lik, scale)
                inp = merged(sh, fi); out = {}
                for itts in sorted(sweeps, reverse=True):                      # the longer run first: it meets every decision of the shorter one
                    res = build_run(inp, family, itts, need_masked and itts == max(sweeps) and itts > 1)
                    for k, v in res.items():
                        out['i%d__%s' % (itts, k)] = v
            except CaseRejected as e:
                assert stored is None, 'the committed inputs of case %s (%s) are rejected: %s' % (name, family, e)
                if verbose:
                    print('%-3s %-4s %s w_lik %.0e seed %d rejected: %s' % (name, family, scale, w_lik, seed, e), flush=True)
                continue
            if stored is None:
                fi['seeds_skipped'] = np.array(skipped); fi['level'] = np.array(wi)
                fi['recipe'] = np.array('harness.mixture_problem, signal %s, w_lik %.0e%s%s' % (
                    scale, w_lik, '' if wi == 0 else ' (no seed of %d passes at %s)' % (MAX_SEEDS, ', '.join('%s / %.0e' % l for l in LEVELS[:min(wi, N_LEVELS)])),
                    ', the walk for a run with a masked site' if need_masked else ''))
            return fi, out
    return None


def build_case(name, sweeps=SWEEPS, verbose=True, start=None, stored=None, need_masked=()):
    t0 = time.time(); start = start or {}
    if stored is not None:
        sh, sfams = stored_case(stored, name)
    else:
        sh, sfams = shared_inputs(CASES[name]), {}
    out = dict(sh); fams = []
    for family in (FAMILIES if stored is None else sfams):
        got = build_family(name, family, sweeps, sh, start.get(family, (0, 0)), family in need_masked, sfams.get(family), verbose)
        if got is None:
            print('%-3s %-4s DROPPED: no seed passes' % (name, family), flush=True)
            continue
        fams.append(family); fi, runs = got
        for k, v in fi.items():
            out['%s__%s' % (family, k)] = v
        for k, v in runs.items():
            out['%s__%s' % (family, k)] = v
        if verbose:
            for itts in sweeps:
                pre = '%s__i%d__' % (family, itts)
                print('%-3s %-4s sweeps %d  seed %d (w_lik %.0e)  clamped %d (adf %d) masked %d  margins %s  err_oracle %s' % (
                    name, family, itts, int(fi['seed']), float(fi['w_lik']), out[pre + 'clamped'], out[pre + 'clamped_adf'], out[pre + 'masked'],
                    ' '.join('%s %.1e' % (k, v) for k, v in zip(MARGIN, out[pre + 'margins'])),
                    ' '.join('%s %.1e' % (f, e) for f, e in zip(FIELDS[family], out[pre + 'err_oracle']))), flush=True)
    out['families'] = np.array(fams)
    if verbose:
        print('%-3s done in %.0f s' % (name, time.time() - t0), flush=True)
    return {'%s__%s' % (name, k): v for k, v in out.items()}


def _job(args):
    return build_case(*args)


def _has_masked(arrays):
    return any(k.endswith('__masked') and '__ihgp__' in k and int(v) > 0 for k, v in arrays.items())


def build(names, jobs=1, sweeps=SWEEPS, start=None, stored=None, need_masked=None):
    start = start or {}; need_masked = need_masked or {}
    args = [(n, sweeps, True, start.get(n), stored, need_masked.get(n, ())) for n in names]
    if jobs > 1:
        from multiprocessing import Pool
        with Pool(jobs) as pool:
            parts = pool.map(_job, args, chunksize=1)
    else:
        parts = [_job(a) for a in args]
    arrays = {'cases': np.array(names), 'margin_names': np.array(list(MARGIN)), 'fields_gf': np.array(FIELDS['gf']), 'fields_ihgp': np.array(FIELDS['ihgp'])}
    for p in parts:
        arrays.update(p)
    if stored is None and not start and 'm2' in names and max(sweeps) == max(SWEEPS) and not _has_masked(arrays):
        # no committed ihgp run holds a masked site: m2 walks on from its first passing seed until one does
        at = {'gf': (int(arrays['m2__gf__level']), int(arrays['m2__gf__seeds_skipped'])), 'ihgp': (N_LEVELS, 0)}
        for k in [k for k in arrays if k.startswith('m2__')]:
            del arrays[k]
        arrays.update(build_case('m2', sweeps, True, at, None, ('ihgp',)))
    return arrays


def file_of(key):
    if key.endswith('__PPo') or key.endswith('__PGo'):
        return OUT_TABLES
    return OUT_IHGP if '__ihgp__i' in key else ''


def files(path=OUT):
    return [path] + [path[:-4] + e for e in (OUT_IHGP, OUT_TABLES)]


def load(path=OUT):
    g = {}
    for f in files(path):
        g.update(np.load(f))
    return unpack_blocks(g)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--jobs', type=int, default=1, help='cases in parallel processes')
    ap.add_argument('--only', default='', help='comma-separated case names (with --check or --out elsewhere)')
    ap.add_argument('--sweeps', default='', help='comma-separated sweep counts (with --check: a quick partial check)')
    ap.add_argument('--check', action='store_true', help='compare with the committed fixture instead of writing it')
    ap.add_argument('--stored-inputs', action='store_true', help='with --check: restate from the committed inputs instead of building them again')
    ap.add_argument('--out', default=OUT)
    a = ap.parse_args()
    names = [n for n in a.only.split(',') if n] or list(CASES)
    sweeps = tuple(int(s) for s in a.sweeps.split(',') if s) or SWEEPS
    assert a.check or not a.stored_inputs
    start = need = None
    if a.check and (a.sweeps or a.stored_inputs or a.only):      # a partial check starts each family's walk at its committed seed
        g = load(a.out)
        start = {n: {str(f): (int(g['%s__%s__level' % (n, f)]), int(g['%s__%s__seeds_skipped' % (n, f)])) for f in g[n + '__families']} for n in names}
        need = {n: tuple(str(f) for f in g[n + '__families'] if int(g['%s__%s__level' % (n, f)]) >= N_LEVELS) for n in names}
    arrays = build(names, a.jobs, sweeps, start, load(a.out) if a.stored_inputs else None, need)
    if a.check:
        g = load(a.out)
        keys = [k for k in arrays if k not in ('cases',) and not k.endswith('err_oracle')]
        bad = [k for k in keys if k not in g or not np.array_equal(np.asarray(arrays[k]), g[k], equal_nan=np.asarray(arrays[k]).dtype.kind == 'f')]
        if not a.only and not a.sweeps:
            bad += [k for k in g if k not in arrays]
        print('fixture matches' if not bad else 'differs in %s' % bad)
        sys.exit(1 if bad else 0)
    assert (not a.only and not a.sweeps) or a.out != OUT, 'a partial fixture is not written over the committed one'
    packed = pack_blocks(arrays)
    for ext in ('', OUT_IHGP, OUT_TABLES):
        write_npz(a.out[:-4] + ext if ext else a.out, {k: v for k, v in packed.items() if file_of(k) == ext})
    for path in files(a.out):
        print('wrote %s (%d bytes)' % (os.path.relpath(path, ROOT), os.path.getsize(path)))


if __name__ == '__main__':
    main()
