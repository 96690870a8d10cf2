"""GPU (-m gpu): nagp_ep_sample / nagp.gf_ep_sample -- joint posterior draws of a full-covariance EP run -- against the NumPy
restatement of tests/epsample_ref.py (pinned to the oracle without a GPU in tests/test_epsample_host.py) at the project's
TOL_MEAN = 1e-7, relative to the largest magnitude of each array; against the product's own run (out['MS'], out['PS']); and the
bit-for-bit properties of a draw (prefix of a longer call, any device batch).  The generator is counter-based and restated on the
host, so every comparison is deterministic.  The sites come from the oracle's run_predict on the very matrices the library gets."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nagp
from nagp import harness, Mom, SSHandle, ss as pss
from nagp.api import _Problem
from oracle import gf_ep as ogf, lik as olik
import epsample_ref as ref

pytestmark = pytest.mark.gpu
TOL_MEAN = 1e-7
SEED = 5
M_ZERO = 3


def rel(a, b):
    a = np.asarray(a, float); b = np.asarray(b, float)
    assert a.shape == b.shape, (a.shape, b.shape)
    assert not np.any(np.isnan(a)) and not np.any(np.isnan(b))
    return float(np.max(np.abs(a - b)) / (np.max(np.abs(b)) + 1e-300)) if a.size else 0.0


@pytest.fixture(scope='module', autouse=True)
def _lib(nagp_lib):
    assert nagp_lib.nagp_device_count() >= 1
    return nagp_lib


_CACHE = {}


def case(D, N, T, itts, gap=None, kernel1='matern32', kernel2='matern52', seed=42, n_ref=0, pk1=False, zero_sites=False):
    """problem, sites of the oracle's run on the library's matrices, and (computed once) the restatement's draws.  pk1: the run and the
    draws predict at the first step too.  zero_sites: some precisions of the run are set to zero afterwards -- one site among non-zero
    ones, one whole step, one site with tnu = 0 as well -- any valid sites define a law, and these take the per-site ttau == 0 branch."""
    key = (D, N, T, itts, gap, kernel1, kernel2, seed, pk1, zero_sites)
    if key not in _CACHE:
        pr = harness.nmf_problem(D, N, T, seed, kernel1=kernel1, kernel2=kernel2)
        blk = pss.ss_blocks_nmf(pr['param1'], pr['param2'], kernel1, kernel2)
        prob = _Problem(blk, pr['W'], np.log(pr['w_lik']))
        md = dict(A=prob.A, Q=prob.Q, Pinf=prob.Pinf, offsets=blk.offsets, h_val=blk.h_val)
        y = pr['y'].copy()
        if gap:
            y[gap[0]:gap[1]] = np.nan
        model = dict(A=prob.A, Q=prob.Q, H=ref.dense_H(md), Pinf=prob.Pinf, Wnmf=pr['W'], lik_param=np.log(pr['w_lik']))
        res = ogf.run_predict(model, y, olik.Mom(olik.LIK_POWER_NMF, p=5), 0.5, 0.5 * np.ones(itts), itts, predict_at_k1=pk1)
        if zero_sites:
            res = dict(res, ttau=res['ttau'].copy(), tnu=res['tnu'].copy())
            res['ttau'][1, 5] = 0.0; res['ttau'][:, 40] = 0.0; res['ttau'][M_ZERO, 50] = 0.0; res['tnu'][M_ZERO, 50] = 0.0
        _CACHE[key] = dict(prob=prob, md=md, y=y, res=res, W=pr['W'], D=D, N=N, pk1=pk1, ref={})
    c = _CACHE[key]
    if n_ref and n_ref not in c['ref']:
        c['ref'][n_ref] = ref.sample(c['md'], c['res']['ttau'], c['res']['tnu'], c['y'], c['pk1'], n_ref, SEED, sig=(c['W'], 0, 0, 0.0))
    return c


def gpu(c, n, seed=SEED, signal=dict(amp='linear', link='softplus'), **kw):
    return nagp.ep_sample(c['prob'], c['res']['ttau'], c['res']['tnu'], c['y'], n, seed, int(c.get('pk1', False)), True, signal, return_counters=True, **kw)


def check_parity(name, c, n):
    F, X, Sd, MS, cnt = gpu(c, n)
    Xr, Fr, Sr, MSr, cntr, _ = c['ref'][n]
    figs = dict(Xdraw=rel(X, Xr), Fdraw=rel(F, Fr), Sdraw=rel(Sd, Sr), MS=rel(MS, MSr))
    print('%s n_draws=%d: ' % (name, n) + '  '.join('%s %.2e' % kv for kv in figs.items()) + '  counters %s' % cnt)
    assert max(figs.values()) < TOL_MEAN, figs
    assert not cnt.any() and not cntr.any()
    assert rel(F, np.einsum('ms,nst->nmt', ref.dense_H(c['md']), X)) < 1e-13
    return F, X, Sd, MS


@pytest.mark.parametrize('T', [1, 2, 3, 65])
def test_parity_small_model_short_series(T):
    """S = 18 (D/N = 3/2); T = 1: the last step only, 2 and 3: one and two backward steps, 65: a gap and one step past 64"""
    c = case(3, 2, T, 2, (20, 35) if T > 40 else None, n_ref=5)
    check_parity('S=18 T=%d' % T, c, 5)


def test_parity_with_zero_precision_sites():
    """the per-site ttau == 0 branch of the update beside non-zero sites, at a whole step, and with tnu = 0"""
    check_parity('S=18 T=65 zero sites', case(3, 2, 65, 2, (20, 35), n_ref=5, zero_sites=True), 5)


def synthetic_blocks(sizes, T, seed, p0_scale=1.0, pk1=False):
    """a model with the given block sizes (not one of the drivers'): A = 0.9 x an orthogonal matrix per block, Pinf = c I per block,
    Q = Pinf - A Pinf A' = 0.19 c I, h_val in 0.5 .. 2; sites and tnu drawn, two precisions zero; a gap and a NaN at each end.
    p0_scale: the first state's covariance is that multiple of Pinf (not stationary: a prediction at the first step then matters)"""
    from nagp import _lib as L
    from types import SimpleNamespace
    rng = np.random.default_rng(seed)
    S = int(sum(sizes)); M = len(sizes); off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    A = np.zeros((S, S)); P = np.zeros((S, S))
    for n, b in enumerate(sizes):
        o = off[n]; q, _ = np.linalg.qr(rng.standard_normal((b, b)))
        A[o:o + b, o:o + b] = 0.9 * q; P[o:o + b, o:o + b] = rng.uniform(0.5, 2.0) * np.eye(b)
    Q = P - A @ P @ A.T; Q = np.tril(Q) + np.tril(Q, -1).T
    hv = rng.uniform(0.5, 2.0, M)
    Af, Qf, Pf = L.f64(A), L.f64(Q), L.f64(p0_scale * P)
    blk = SimpleNamespace(S=S, M=M, D=M - 1, N=1, offsets=off, h_val=hv)
    model = L.Model(S=S, M=M, D=M - 1, N=1, block_offsets=off.ctypes.data_as(L.c_ip), A=L.dptr(Af), Q=L.dptr(Qf), Pinf=L.dptr(Pf), h_val=L.dptr(hv),
                    Wnmf=None, lik_param=0.0)
    W = L.f64(rng.uniform(0.1, 1.0, (M - 1, 1)))
    prob = SimpleNamespace(blk=blk, model=model, W=W, keep=(Af, Qf, Pf, hv, off))
    ttau = rng.uniform(0.5, 50.0, (M, T)); ttau[0, 3] = 0.0; ttau[M - 1, 7] = 0.0; tnu = rng.standard_normal((M, T))
    y = np.zeros(T); y[0] = y[T - 1] = np.nan; y[T // 3:T // 2] = np.nan
    md = dict(A=Af, Q=Qf, Pinf=Pf, offsets=off, h_val=hv)
    return dict(prob=prob, md=md, y=y, res=dict(ttau=ttau, tnu=tnu), W=W, pk1=pk1, ref={})


def test_parity_every_block_size_from_one_to_eight_states():
    """S = 36 in blocks of 1, 8, 5, 7, 2, 3, 4, 6 states: every specialisation of the filter's block passes, mixed in one model"""
    c = synthetic_blocks([1, 8, 5, 7, 2, 3, 4, 6], 40, 11)
    c['ref'][4] = ref.sample(c['md'], c['res']['ttau'], c['res']['tnu'], c['y'], False, 4, SEED, sig=(c['W'], 0, 0, 0.0))
    check_parity('S=36 blocks 1..8', c, 4)


def test_parity_with_a_prediction_at_the_first_step():
    """predict_at_k1 = 1 (gf_ep_modulator's predict mode).  The drivers' Pinf is stationary, so there the option changes nothing; here the
    first covariance is 2 Pinf and it does"""
    c = synthetic_blocks([4, 4, 3, 2], 30, 12, p0_scale=2.0, pk1=True)
    args = (c['md'], c['res']['ttau'], c['res']['tnu'], c['y'])
    c['ref'][4] = ref.sample(*args, True, 4, SEED, sig=(c['W'], 0, 0, 0.0))
    F, X, Sd, MS = check_parity('S=13 predict_at_k1', c, 4)
    assert rel(MS, ref.sample(*args, False, 1, SEED)[3]) > 1e-3                      # not the same law as without the option


def test_two_device_batches_under_a_budget_of_one_mib(monkeypatch):
    """S = 18, T = 65 under NAGP_EPS_BUDGET_MB = 1: 50 draws run as 48 + 2 and give the bits of the unbatched call"""
    c = case(3, 2, 65, 2, (20, 35))
    whole = gpu(c, 50)
    monkeypatch.setenv('NAGP_EPS_BUDGET_MB', '1')
    parts = gpu(c, 50)
    assert all(np.array_equal(a, b) for a, b in zip(whole, parts))
    with pytest.raises(nagp.NagpError, match=r'\(-4\).*budget'):
        gpu(case(8, 3, 400, 2, (100, 180), kernel1='exp'), 2)                         # 4 MiB of per-step storage: refused under 1 MiB


def test_parity_exp_sub_bands_worst_conditioned():
    """S = 25: exp sub-bands (two-state blocks), D/N/T = 8/3/400, gap 100..179"""
    check_parity('S=25 exp', case(8, 3, 400, 2, (100, 180), kernel1='exp', n_ref=5), 5)


def test_parity_speech_model_draw_counts_prefix_and_batches(monkeypatch):
    """S = 73 (D/N = 16/3), T = 150, gap 50..79: across the 64-lane and 16-row paddings.  n_draws = 1, 5, 17 (one draw past a block of
    16); draws 0..4 of 17 are the 5-draw call bit for bit; a forced small device batch gives the same bits."""
    c = case(16, 3, 150, 2, (50, 80), n_ref=17)
    c['ref'][5] = tuple(a[:5] if i < 3 else a for i, a in enumerate(c['ref'][17][:5])) + (None,)
    c['ref'][1] = tuple(a[:1] if i < 3 else a for i, a in enumerate(c['ref'][17][:5])) + (None,)
    r17 = check_parity('S=73', c, 17)
    r5 = check_parity('S=73', c, 5)
    r1 = check_parity('S=73', c, 1)
    for a17, a5, a1 in zip(r17[:3], r5[:3], r1[:3]):
        assert np.array_equal(a17[:5], a5) and np.array_equal(a17[:1], a1)
    assert np.array_equal(r17[3], r5[3]) and np.array_equal(r17[3], r1[3])
    monkeypatch.setenv('NAGP_EPS_BUDGET_MB', '14')            # 12.4 MiB of per-step storage; a draw takes 0.1 MiB: batches of fewer than 16
    rb = gpu(c, 17)
    for a, b in zip(r17, rb[:4]):
        assert np.array_equal(a, b)


def test_parity_matern52_sub_bands_six_state_blocks():
    check_parity('S=24 matern52 sub-bands', case(3, 2, 65, 2, (20, 35), kernel1='matern52', n_ref=5), 5)


def test_ceiling_of_S_and_one_above():
    """S = 80 (D/N = 17/4) is served; S = 81 (D/N = 18/3) is refused before any device call"""
    check_parity('S=80', case(17, 4, 40, 1, (10, 20), n_ref=3), 3)
    c = case(18, 3, 6, 1)
    with pytest.raises(nagp.NagpError, match=r'\(-2\).*S <= 80'):
        gpu(c, 2)


def test_caller_supplied_normals_and_the_signal_options():
    """z in place of the generator; Sdraw = sum_d a_d z_d on Fdraw for both amplitude kinds and both links"""
    c = case(3, 2, 65, 2, (20, 35))
    S = c['md']['A'].shape[0]
    z = np.random.default_rng(3).standard_normal((4, 65, S))
    Xr, Fr, _, MSr, _, _ = ref.sample(c['md'], c['res']['ttau'], c['res']['tnu'], c['y'], False, 4, 0, z=z)
    F, X, _, MS, cnt = gpu(c, 4, signal=None, z=z)
    assert max(rel(X, Xr), rel(F, Fr), rel(MS, MSr)) < TOL_MEAN and not cnt.any()
    for amp in ('linear', 'sqrt'):
        for link, shift in (('softplus', 0.0), ('softplus', 1.5), ('exp', 0.0)):
            F, _, Sd, _, _ = gpu(c, 4, signal=dict(amp=amp, link=link, link_shift=shift), z=z)
            want = ref.signal(F, 3, c['W'], int(amp == 'sqrt'), int(link == 'exp'), shift)
            d = rel(Sd, want)
            print('Sdraw %s %s shift %.1f: %.2e' % (amp, link, shift, d))
            assert d < TOL_MEAN


@pytest.mark.parametrize('D,N,T', [(3, 2, 60), (16, 3, 150)])
def test_draws_from_the_products_own_run_reproduce_its_smoothed_means(D, N, T):
    """nagp.gf_ep_modulator_nmf with two sweeps, then nagp.gf_ep_sample on its out: MS within TOL_MEAN of out['MS']"""
    pr = harness.nmf_problem(D, N, T, 42)
    y = pr['y'].copy(); y[T // 3:T // 3 + T // 5] = np.nan
    t = np.arange(1, T + 1.0)
    mom = Mom('likModulatorNMFPower', p_cubature=5)
    out = nagp.gf_ep_modulator_nmf(pr['w'], t, y, SSHandle(), mom, t, 'matern32', 'matern52', 1, D, N, 0.5, 0.5 * np.ones(2), 2, nargout=6)[5]
    F, X, Sd, MS, cnt = nagp.gf_ep_sample(pr['w'], t, y, SSHandle(), 'matern32', 'matern52', 1, D, N, out, 3, seed=1, states=True, signal=mom, return_counters=True)
    d = rel(MS, out['MS'])
    print('D/N/T = %d/%d/%d: MS of the chain against out.MS %.2e' % (D, N, T, d))
    assert d < TOL_MEAN and not cnt.any()
    assert F.shape == (3, D + N, T) and X.shape == (3, MS.shape[0], T) and Sd.shape == (3, T)


def test_plan_sample_draws_from_every_problem_of_an_executed_plan():
    """Plan.sample: per problem what nagp.ep_sample gives on the plan's sites; plans that are not predict-mode EP plans refuse"""
    from nagp import _lib as L
    D, N, T = 3, 2, 40
    probs, ys = [], []
    for q in range(2):
        pr = harness.nmf_problem(D, N, T, 40 + q)
        probs.append((pss.ss_blocks_nmf(pr['param1'], pr['param2'], 'matern32', 'matern52'), pr['W'], np.log(pr['w_lik'])))
        y = pr['y'].copy(); y[10 + q:20] = np.nan; ys.append(y)
    mom = Mom('likModulatorNMFPower', p_cubature=5)
    plan = nagp.Plan(L.KIND_GF_EP, probs, T, mom=mom, ep_fraction=0.5, ep_damping=0.5 * np.ones(2), ep_itts=2)
    with pytest.raises(nagp.NagpError, match='upload and execute'):
        plan.sample(2)
    plan.upload(ys)
    with pytest.raises(nagp.NagpError, match='upload and execute'):                   # uploaded, not run: the plan holds no sites of these data
        plan.sample(2)
    plan.execute()
    outs = plan.download()
    draws = plan.sample(3, seed=2, states=True, signal=mom)
    assert len(draws) == 2
    for q, (F, X, Sd, MS) in enumerate(draws):
        d = rel(MS, outs[q].MS)
        print('plan problem %d: MS of the chain against the plan\'s MS %.2e' % (q, d))
        assert d < TOL_MEAN and F.shape == (3, D + N, T) and X.shape == (3, MS.shape[0], T) and Sd.shape == (3, T)
        one = nagp.ep_sample(plan.probs[q], outs[q].ttau, outs[q].tnu, ys[q], 3, 2, 0, True, mom)
        assert all(np.array_equal(a, b) for a, b in zip((F, X, Sd, MS), one))
    plan.close()
    nl = nagp.Plan(L.KIND_GF_EP, probs, T, mom=mom, ep_fraction=0.5, ep_damping=0.5 * np.ones(2), ep_itts=2, mode=L.MODE_NLML)
    with pytest.raises(nagp.NagpError, match=r'\(-2\)'):
        nl.sample(2)
    nl.close()
    mx = nagp.Plan(L.KIND_GF_EP, probs, T, mom=mom, ep_fraction=0.5, ep_damping=0.1 * np.ones(2), ep_itts=2, flags=L.FLAG_MIXTURE_RULE)
    mx.upload(ys); mx.execute()
    with pytest.raises(nagp.NagpError, match=r'\(-2\).*FLAG_MIXTURE_RULE.*mixture drivers'):
        mx.sample(2)
    mx.close()
    plan2 = nagp.Plan(L.KIND_GF_EP, probs, T, mom=mom, ep_fraction=0.5, ep_damping=0.5 * np.ones(2), ep_itts=2)
    plan2.upload(ys); plan2.execute(); plan2.upload(ys)
    with pytest.raises(nagp.NagpError, match='upload and execute'):                   # a new upload: the sites belong to the run before it
        plan2.sample(2)
    plan2.close()


def test_draws_from_a_gf_ep_modulator_run():
    """the plain driver: one modulator per sub-band, balanced, predicts at the first step; Sdraw with Wnmf = I"""
    T = 80
    cfg = harness.cfg1(T, 5)
    y = cfg['y'].copy(); y[30:45] = np.nan
    t = np.arange(1, T + 1.0)
    mom = Mom('likModulatorPower', p_cubature=5); ss = SSHandle('ss_modulators')
    out = nagp.gf_ep_modulator(cfg['w'], t, y, ss, mom, t, cfg['kernel1'], cfg['kernel2'], 1, 0.5, 0.3 * np.ones(2), 2, nargout=6)[5]
    F, X, Sd, MS, cnt = nagp.gf_ep_sample(cfg['w'], t, y, ss, cfg['kernel1'], cfg['kernel2'], 1, None, None, out, 3, seed=1, states=True, signal=mom,
                                          return_counters=True)
    D = cfg['D']; d = rel(MS, out['MS'])
    print('gf_ep_modulator, D = %d, T = %d: MS of the chain against out.MS %.2e' % (D, T, d))
    assert d < TOL_MEAN and not cnt.any() and F.shape == (3, 2 * D, T)
    assert rel(Sd, ref.signal(F, D, np.eye(D), 0, 0, 0.0)) < TOL_MEAN


def test_draws_from_a_gf_ep_modulator_nmf_constraints_run():
    """the constraints driver: sigmoid-constrained parameters split into tuned and fixed, balanced"""
    D, N, T = 4, 2, 80
    pr = harness.nmf_problem(D, N, T, 3, 'constraints')
    cons = harness.CONSTRAINTS_DEMO(D); tune = harness.TUNE_DEMO
    w, wf = harness.constrained_vectors(pr, cons, tune)
    y = pr['y'].copy(); y[30:45] = np.nan
    t = np.arange(1, T + 1.0)
    mom = Mom('likModulatorNMFPower', p_cubature=5)
    out = nagp.gf_ep_modulator_nmf_constraints(w, t, y, SSHandle(), mom, t, 'matern32', 'matern52', 1, D, N, 0.5, 0.5 * np.ones(2), 2, cons, wf, tune, nargout=6)[5]
    F, X, Sd, MS, cnt = nagp.gf_ep_sample(w, t, y, SSHandle(), 'matern32', 'matern52', 1, D, N, out, 3, seed=1, states=True, signal=mom, constraints=cons,
                                          w_fixed=wf, tune_hypers=tune, return_counters=True)
    d = rel(MS, out['MS'])
    print('gf_ep_modulator_nmf_constraints, D/N/T = %d/%d/%d: MS of the chain against out.MS %.2e' % (D, N, T, d))
    assert d < TOL_MEAN and not cnt.any() and F.shape == (3, D + N, T) and Sd.shape == (3, T)
    assert rel(Sd, ref.signal(F, D, pr['W'], 0, 0, 0.0)) < 1e-6                      # W through the sigmoid and back: 1e-9 relative


def test_unit_vector_extraction_reproduces_the_products_smoothed_covariances():
    """T = 8, S = 18: z = 0 and the 144 unit vectors give x = m + L z; the diagonal blocks of L L' are out['PS'] within TOL_MEAN"""
    D, N, T = 3, 2, 8
    pr = harness.nmf_problem(D, N, T, 42)
    t = np.arange(1, T + 1.0)
    mom = Mom('likModulatorNMFPower', p_cubature=5)
    out = nagp.gf_ep_modulator_nmf(pr['w'], t, pr['y'], SSHandle(), mom, t, 'matern32', 'matern52', 1, D, N, 0.5, 0.5 * np.ones(2), 2, nargout=6)[5]
    S = out['MS'].shape[0]
    z = np.zeros((S * T + 1, T, S))
    for k in range(T):
        for j in range(S):
            z[1 + k * S + j, k, j] = 1.0
    F, X, _, MS = nagp.gf_ep_sample(pr['w'], t, pr['y'], SSHandle(), 'matern32', 'matern52', 1, D, N, out, S * T + 1, states=True, z=z)
    Lmap = (X[1:] - X[0][None]).transpose(2, 1, 0).reshape(T * S, T * S)
    C = (Lmap @ Lmap.T).reshape(T, S, T, S)
    PS = np.stack([C[k, :, k, :] for k in range(T)], axis=2)
    d = rel(PS, out['PS']); dm = rel(X[0], out['MS'])
    print('unit vectors: PS %.2e  mean %.2e' % (d, dm))
    assert d < TOL_MEAN and dm < TOL_MEAN and np.array_equal(X[0], MS)
