"""nagp_reconstruct_sources without a GPU: the NumPy restatement the GPU tests compare with (tests/recon_sources_ref.py) pinned against
oracle/recon.py, against itself and against Monte-Carlo estimates, and the argument checks of the entry point (all of them run before
any device call)."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nagp
from nagp import _lib as L
from nagp.cubature import gauher, sigma_points
from oracle import recon as orc
import recon_sources_ref as ref


def rel(a, b):
    a = np.asarray(a, float); b = np.asarray(b, float)
    assert a.shape == b.shape, (a.shape, b.shape)
    assert np.array_equal(np.isnan(a), np.isnan(b))
    return float(np.nanmax(np.abs(a - b)) / (np.nanmax(np.abs(b)) + 1e-300)) if a.size else 0.0


softplus = lambda g: np.log(1.0 + np.exp(g))


def marginals(D, N, T, seed):
    """Eft ~ N(0,1), sub-band variances in [0.05, 0.6], modulator variances in [0.05, 1]"""
    rng = np.random.default_rng(seed)
    Eft = rng.normal(0, 1, (D + N, T))
    Varft = np.concatenate([rng.uniform(0.05, 0.6, (D, T)), rng.uniform(0.05, 1.0, (N, T))])
    return Eft, Varft


def uneven_W(rng):
    """D = 6, N = 4: sources of 2 / 1 / 3 sub-bands over 1 / 1 / 2 components"""
    Ws = [rng.uniform(0.1, 0.6, s) for s in ((2, 1), (1, 1), (3, 2))]
    W, off = nagp.recon.stack_sources(Ws)
    return W, off


def test_linear_one_source_restatement_is_the_oracle():
    D, N, T = 5, 3, 40
    Eft, Varft = marginals(D, N, T, 1); W = np.random.default_rng(2).uniform(0, 0.5, (D, N))
    a = ref.sampling(Eft, Varft, W, [0, D], softplus, 'linear', 50, 11); b = orc.sampling(Eft, Varft, W, softplus, 50, 11)
    for k in ('Esig', 'Vsig', 'Eft_mod', 'Varft_mod'):
        assert rel(a[k], b[k]) < 1e-13, k
    assert rel(a['Esrc'][0], a['Esig']) < 1e-13 and rel(a['Vsrc'][0], a['Vsig']) < 1e-13
    gx, gw = gauher(32)
    for exp_link, lk in ((False, softplus), (True, np.exp)):
        a = ref.population(Eft, 0.3 * Varft, W, [0, D], lk, 'linear', gx, gw, exp_link=exp_link)
        b = orc.moments(Eft, 0.3 * Varft, W, lk, gx, gw, exp_link=exp_link)
        for k in ('Esig', 'Vsig', 'Eft_mod', 'Varft_mod'):
            assert rel(a[k], b[k]) < 1e-13, (k, exp_link)
        assert rel(a['Esrc'][0], a['Esig']) < 1e-13 and rel(a['Vsrc'][0], a['Vsig']) < 1e-13
        assert rel(a['Eenv'], W @ b['Eft_mod']) < 1e-13


@pytest.mark.parametrize('kind', ['linear', 'sqrt'])
def test_sources_add_up_to_the_signal_draw_by_draw(kind):
    W, off = uneven_W(np.random.default_rng(3)); D, N = W.shape
    assert off == [0, 2, 3, 6] and (D, N) == (6, 4)
    Eft, Varft = marginals(D, N, 30, 4)
    lm, envs, sig, sigj = ref.sampled_signals(Eft, Varft, W, off, softplus, kind, 20, 5)
    assert sigj.shape == (3, 30, 20) and envs.shape == (6, 30, 20)
    assert np.max(np.abs(sigj.sum(axis=0) - sig)) < 1e-13 * np.max(np.abs(sig))
    r = ref.sampling(Eft, Varft, W, off, softplus, kind, 20, 5)
    assert rel(r['Esrc'].sum(axis=0), r['Esig']) < 1e-13
    # a source sees its own components only: the second source is sub-band 2 times the amplitude of component 1
    x = W[2, 1] * lm[1]
    assert rel(envs[2], np.sqrt(x) if kind == 'sqrt' else x) < 1e-13


@pytest.mark.parametrize('p', [5, 7])
def test_sqrt_population_values_are_what_the_draws_estimate(p):
    """Means within 0.03 and variances within 0.1 of 40 000-draw estimates, relative to each array's largest entry (the bounds of
    test_posterior_reconstruction_of_signal_and_amplitudes)."""
    W, off = uneven_W(np.random.default_rng(3)); D, N = W.shape
    Eft, Varft = marginals(D, N, 12, 6)
    gx, gw = gauher(32); wn, xn = sigma_points(p, N)
    pop = ref.population(Eft, Varft, W, off, softplus, 'sqrt', gx, gw, wn=wn, xn=xn)
    big = ref.sampling(Eft, Varft, W, off, softplus, 'sqrt', 40000, 7)
    for k in ('Esig', 'Esrc', 'Eenv', 'Eft_mod'):
        assert rel(pop[k], big[k]) < 0.03, k
    for k in ('Vsig', 'Vsrc', 'Varft_mod'):
        assert rel(pop[k], big[k]) < 0.1, k


def test_stack_sources_and_equal_blocks():
    W, off = nagp.recon.stack_sources([np.ones((2, 1)), 2 * np.ones((3, 2))])
    assert off == [0, 2, 5] and W.shape == (5, 3)
    assert np.array_equal(W, np.array([[1, 0, 0], [1, 0, 0], [0, 2, 2], [0, 2, 2], [0, 2, 2.0]]))
    with pytest.raises(ValueError):
        nagp.reconstruct_sources(np.zeros((7, 3)), np.ones((7, 3)), np.ones((5, 2)), sources=2)      # 5 sub-bands in 2 equal blocks


# ---------------------------------------------------------------------------------------------
# argument checks of the C entry point: each returns NAGP_EINVAL before the first device call
def _raw(D=3, N=2, T=4, Eft=True, Varft=True, W=True, opts=True, out=True, outputs=('Esig',), offsets=None, rule1=True, ruleN=True, **kw):
    nagp.build()
    E = np.zeros((D + N, max(T, 1)), order='F'); V = np.ones((D + N, max(T, 1)), order='F'); Wm = np.ones((max(D, 1), max(N, 1)), order='F')
    gx, gw = gauher(8); wn, xn = sigma_points(5, max(N, 1)); xn = np.asfortranarray(xn)
    o = L.ReconOpts(amp_kind=L.AMP_SQRT, link_kind=L.LINK_SOFTPLUS, n_sources=1)
    if rule1:
        o.n_gh = gx.size; o.gh_x = L.dptr(gx); o.gh_w = L.dptr(gw)
    if ruleN:
        o.n_pts = wn.size; o.wn = L.dptr(wn); o.xn_unscaled = L.dptr(xn)
    offs = None
    if offsets is not None:
        offs = np.ascontiguousarray(offsets, dtype=np.int32); o.source_offsets = offs.ctypes.data_as(L.c_ip)
    for k, v in kw.items():
        setattr(o, k, v)
    bufs = {k: np.zeros((D + N + 8) * max(T, 1)) for k in outputs}
    ro = L.ReconOut(**{k: L.dptr(a) for k, a in bufs.items()})
    st = L.lib().nagp_reconstruct_sources(D, N, T, L.dptr(E) if Eft else L.c_dp(), L.dptr(V) if Varft else L.c_dp(), L.dptr(Wm) if W else L.c_dp(),
                                          ctypes.byref(o) if opts else None, ctypes.byref(ro) if out else None)
    return st


BAD = [dict(Eft=False), dict(Varft=False), dict(W=False), dict(opts=False), dict(out=False),
       dict(D=0), dict(N=0), dict(N=10), dict(D=56, N=9), dict(T=0),
       dict(amp_kind=2), dict(amp_kind=-1), dict(link_kind=2),
       dict(n_samples=1), dict(n_samples=-3),
       dict(n_sources=0), dict(n_sources=9, D=12, offsets=list(range(9)) + [12]),
       dict(n_sources=2), dict(n_sources=2, offsets=[1, 2, 3]), dict(n_sources=2, offsets=[0, 2, 2]), dict(n_sources=2, offsets=[0, 3, 3]),
       dict(n_sources=2, offsets=[0, 0, 3]), dict(n_sources=3, offsets=[0, 2, 1, 3]), dict(n_sources=1, offsets=[0, 2]),
       dict(rule1=False), dict(n_gh=0), dict(n_gh=257), dict(ruleN=False), dict(n_pts=0),
       dict(rule1=False, amp_kind=0), dict(outputs=())]


@pytest.mark.parametrize('case', BAD, ids=lambda c: ','.join('%s=%s' % kv for kv in c.items()).replace(' ', ''))
def test_entry_point_refuses_bad_arguments_before_any_device_call(case):
    st = _raw(**case)
    assert st == -1, st                                     # NAGP_EINVAL
    with pytest.raises(nagp.NagpError, match='invalid argument'):
        L.check(st)


def test_rules_are_needed_only_where_they_are_used():
    """The exp link needs no 1-D rule, the linear kind and the sampling form no N-dimensional one: such calls pass the argument checks
    (without a GPU they then stop at the device, with one they run)."""
    for kw in (dict(rule1=False, link_kind=L.LINK_EXP), dict(ruleN=False, amp_kind=L.AMP_LINEAR), dict(rule1=False, ruleN=False, n_samples=2)):
        assert _raw(**kw) != -1, kw


def test_python_mirror_passes_the_refusals_on():
    E = np.zeros((5, 3)); V = np.ones((5, 3)); W = np.ones((3, 2))
    for kw in (dict(n_samples=1), dict(sources=[0, 2, 2, 3]), dict(sources=[0, 1, 2]), dict(sources=[1, 3]), dict(amplitude=7), dict(link=5)):
        with pytest.raises(nagp.NagpError, match='invalid argument'):
            nagp.reconstruct_sources(E, V, W, **kw)
    with pytest.raises(ValueError):
        nagp.reconstruct_sources(np.zeros((4, 3)), np.ones((4, 3)), W)
