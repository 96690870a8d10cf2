"""nagp_ep_sample (joint posterior draws of a full-covariance EP run) against a 96-digit restatement, and its retry branches.

tests/golden/epsample_multiprecision.npz (tools/make_epsample_fixture.py) holds, per case, the f64 inputs the library is handed (the
diagonal blocks of A, Q, P0; h_val, the sites, y, three draws' worth of normals z) and Xdraw, MS (two cases: Sdraw) computed from those
exact doubles in 320-bit fixed point and rounded to f64 once; the counters [jitter retries, clamped pivots], the steps that retried, the
margin of every pivot decision, and err_oracle: the error of tests/epsample_ref.py against that run, per field (max-abs difference over
the field's largest entry).  The cases cover every instantiation NTL = ceil(S / 16) = 1 .. 5 (4 had never been launched), the sizes that
are whole tiles, both sides of the filter's switch to 512 threads at S = 32 | 33, the drivers' conditioning, and the three branches of
eps_factor_kernel no other test takes: the jitter retry on a recomputed PSkp, a clamped pivot of chol(C_k) / chol(PF_{T-1}), and the
"not positive definite even with the jitter" exit.

BOUND(field, case) = min(max(10 x err_oracle, 1e-12), 1e-7): the factor 10 stands for another summation order (16 x 16 x 4 MFMA tiles
over up to 80 columns) of the same rounding-times-conditioning error the f64 restatement shows -- the reasoning of
tests/test_smoother_fixture.py; the generator asserts 10 x err_oracle < 1e-7, so the cap never passes a test.  Nothing is tuned on a
device.  err_oracle is 1e-16 .. 1e-14 on every case, so every bound is 1e-12.

CPU: the fixture holds what it claims; its inputs are what the recipe, nagp.ss and the oracle build; the restatement meets it (the first
run of ref.chol_retry and of the clamp branch of ref.chol_clamped); six wrong restatements miss it; the generator reproduces it.
GPU (-m gpu): every case through nagp.ep_sample on the stored normals; the retry cases in device batches; NAGP_ENOTPD; each output alone;
draw counts around the block of 16.  The measured errors are printed beside err_oracle (profiles/r21_ep_sample_fixture.txt).
"""
import ctypes
import functools
import importlib.util
import math
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import epsample_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, 'tests', 'golden', 'epsample_multiprecision.npz')
TOL_MEAN = 1e-7
MARGIN = 1e-6
FIELDS = ('Xdraw', 'Fdraw', 'MS', 'Sdraw')
B52 = [8, 8, 8, 8, 8, 1, 6, 5]
# name: S, T, blocks (None: a driver model), counters (None: 0 < retries < T - 1), dead states
TABLE = {
    's16': (16, 24, [4, 4, 4, 4], (0, 0), 0), 's32': (32, 24, [8] * 4, (0, 0), 0), 's33': (33, 24, [8, 8, 8, 8, 1], (0, 0), 0),
    's48': (48, 24, [8] * 6, (0, 0), 0), 's52_pk1': (52, 24, B52, (0, 0), 0), 's64': (64, 24, [8] * 8, (0, 0), 0), 's80': (80, 24, [8] * 10, (0, 0), 0),
    'drv_s18': (18, 24, None, (0, 0), 0), 'drv_exp_s25': (25, 24, None, (0, 0), 0),
    'retry_some': (13, 24, [4, 4, 3, 2], None, 0), 'retry_all': (13, 24, [4, 2, 3, 4], (23, 48), 2), 'retry_all_T1': (13, 1, [4, 2, 3, 4], (0, 2), 2),
    'retry_all_T2': (13, 2, [4, 2, 3, 4], (1, 4), 2), 'retry_s52': (52, 24, B52, (23, 24), 1),
}
CASES = tuple(TABLE)
DRIVERS = {'drv_s18': (3, 2, 'matern32'), 'drv_exp_s25': (8, 3, 'exp')}
RETRY = ('retry_some', 'retry_all', 'retry_all_T1', 'retry_all_T2', 'retry_s52')
SDRAW = {'s16': (0, 0, 1.5), 's33': (1, 1, 0.0)}            # (amplitude kind, link kind, shift): linear / softplus 1.5, sqrt / exp
ENOTPD = -6


@functools.lru_cache(maxsize=None)
def _tool():
    spec = importlib.util.spec_from_file_location('make_epsample_fixture', os.path.join(ROOT, 'tools', 'make_epsample_fixture.py'))
    mod = importlib.util.module_from_spec(spec); spec.loader.exec_module(mod)
    return mod


@functools.lru_cache(maxsize=None)
def _fixture():
    return _tool().load(FIXTURE)


@functools.lru_cache(maxsize=None)
def _case(name):
    """the arrays of a case (read-only), with Fdraw = H Xdraw formed once"""
    c = _tool().case_of(_fixture(), name)
    off = c['block_offsets'][:-1]
    c['Fdraw'] = c['h_val'][None, :, None] * c['Xdraw'][:, off, :]
    c['sig'] = tuple(c['sig']) if bool(c['has_sdraw']) else None
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def _fields(c):
    return [f for f in FIELDS if f in c]


def _bound(c, f):
    return min(max(10.0 * float(c['err'][f]), 1e-12), TOL_MEAN)


def _err(x, want):
    """the suite's metric: max-abs difference over the largest entry of the reference (0 / 0 = 0: the means of a series without observations)"""
    x = np.asarray(x, float)
    assert x.shape == want.shape, (x.shape, want.shape)
    assert np.all(np.isfinite(x))
    return float(np.abs(x - want).max() / (np.abs(want).max() + 1e-300))


def _ref_run(c, mod=ref, pk1=None):
    o, cnt, steps = _tool().ref_run(dict(c, predict_at_k1=c['predict_at_k1'] if pk1 is None else pk1), c['sig'], ref=mod)
    return o, [int(v) for v in cnt], [int(v) for v in steps]


# ---------------------------------------------------------------------------------------------
# CPU
def test_fixture_holds_the_cases_it_claims():
    g = _fixture()
    assert tuple(g['cases']) == CASES and tuple(g['fields']) == FIELDS
    assert tuple(g['margin_names']) == ('first_attempt', 'second_attempt', 'clamped_factor')
    for name, (S, T, blocks, counters, dead) in TABLE.items():
        c = _case(name)
        assert (c['S'], c['T']) == (S, T) and T <= 24, name
        if blocks is not None:
            assert list(np.diff(c['block_offsets'])) == blocks, name
        assert c['z'].shape == c['Xdraw'].shape[:1] + (T, S) and c['Xdraw'].shape == (3, S, T) and c['MS'].shape == (S, T)
        assert c['ttau'].shape == c['tnu'].shape == (c['M'], T) and int(c['D']) + int(c['N']) == c['M']
        assert np.all(c['ttau'] >= 0) and np.all(np.isfinite(c['ttau'])) and np.all(np.isfinite(c['tnu']))
        assert (name in SDRAW) == ('Sdraw' in c)
        if name in SDRAW:
            assert c['Sdraw'].shape == (3, T) and c['sig'] == SDRAW[name]
        r, cl = (int(v) for v in c['counters'])
        if counters is None:
            assert 0 < r < T - 1 and cl > 0, (name, r, cl)
        else:
            assert (r, cl) == counters, (name, r, cl)
        if dead:                                              # a state of zero variance: a retry at every step, its pivots clamped at every step
            assert (r, cl) == (T - 1, dead * T) and c['dead_states'].size == dead
            assert list(c['zero_pivots']) == [T - 1, 0, dead * T]          # the first attempt ends at the first of them
            assert not c['Xdraw'][:, c['dead_states'], :].any() and not c['MS'][c['dead_states']].any()
        else:
            assert not c['zero_pivots'].any() and c['dead_states'].size == 0
        assert c['retry_steps'].size == r and (r == 0 or (c['retry_steps'][0] == 0 and np.all(np.diff(c['retry_steps']) == 1)))
        assert np.all(c['margins_scaled'] >= MARGIN), (name, c['margins_scaled'])
        if name not in DRIVERS:                               # (not balanced: variances of 1e1 .. 1e-11 side by side; see the generator)
            assert np.all(c['margins'] >= MARGIN), (name, c['margins'])
        assert np.isinf(c['margins'][1]) == (r == 0)
        assert float(c['agree_256_bits']) < 1e-60 and int(c['prec_bits']) == 320
        assert np.all(10 * c['err_oracle'] < TOL_MEAN)
    sizes = [TABLE[n][0] for n in CASES]
    assert {math.ceil(s / 16) for s in sizes} == {1, 2, 3, 4, 5} and {16, 32, 48, 64, 80} <= set(sizes) and {32, 33} <= set(sizes)
    assert bool(_case('s52_pk1')['predict_at_k1']) and not any(bool(_case(n)['predict_at_k1']) for n in CASES if n != 's52_pk1')
    assert os.path.getsize(FIXTURE) < 1 << 20


def _recipe(sizes, T, seed, rho, dead=(), p0_scale=1.0, p0_set=()):
    """the synthetic model of tests/test_epsample_gpu.py:synthetic_blocks with rho a parameter, restated"""
    rng = np.random.default_rng(seed)
    S = int(sum(sizes)); M = len(sizes); off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    A = np.zeros((S, S)); P = np.zeros((S, S))
    for n, b in enumerate(sizes):
        o = off[n]; q, _ = np.linalg.qr(rng.standard_normal((b, b)))
        A[o:o + b, o:o + b] = rho * q; P[o:o + b, o:o + b] = rng.uniform(0.5, 2.0) * np.eye(b)
    for n in dead:
        P[off[n]:off[n + 1], off[n]:off[n + 1]] = 0.0
    Q = P - A @ P @ A.T; Q = np.tril(Q) + np.tril(Q, -1).T
    hv = rng.uniform(0.5, 2.0, M); W = rng.uniform(0.1, 1.0, (M - 1, 1))
    ttau = rng.uniform(0.5, 50.0, (M, T)); tnu = rng.standard_normal((M, T))
    if T > 3:
        ttau[0, 3] = 0.0
    if T > 7:
        ttau[M - 1, 7] = 0.0
    y = np.zeros(T); y[0] = y[T - 1] = np.nan; y[T // 3:T // 2] = np.nan
    P0 = p0_scale * P
    for i, v in p0_set:
        P0[i, i] = v
    return dict(A=A, Q=Q, P0=P0, h_val=hv, block_offsets=off, Wnmf=W, ttau=ttau, tnu=tnu, y=y)


RECIPES = {'s52_pk1': dict(p0_scale=2.0), 'retry_some': dict(rho=0.999, p0_set=[(3, -0.005)]), 'retry_all': dict(dead=[1]), 'retry_all_T1': dict(dead=[1]),
           'retry_all_T2': dict(dead=[1]), 'retry_s52': dict(dead=[5])}


@pytest.mark.parametrize('name', [n for n in CASES if n not in DRIVERS])
def test_synthetic_inputs_are_what_the_recipe_builds(name):
    """bit for bit (seed 11 plus the stored number of skipped seeds); the normals z are those of the seed + 7919"""
    c = _case(name); S, T, blocks, _, _ = TABLE[name]
    kw = dict(RECIPES.get(name, {})); rho = kw.pop('rho', 0.9)
    seed = 11 + int(c['seeds_skipped'])
    assert int(c['seed']) == seed and float(c['rho']) == rho
    want = _recipe(blocks, T, seed, rho, **kw)
    for k, v in want.items():
        assert np.array_equal(c[k], v, equal_nan=True), k
    assert np.array_equal(c['z'], np.random.default_rng(seed + 7919).standard_normal((3, T, S)))
    assert int(c['D']) == len(blocks) - 1 and int(c['N']) == 1
    assert np.sum(c['ttau'] == 0) == (2 if T > 7 else 0) and np.isnan(c['y'][0]) and np.isnan(c['y'][-1]) and np.all(np.isnan(c['y'][T // 3:T // 2]))


@pytest.mark.parametrize('name', sorted(DRIVERS))
def test_driver_inputs_are_what_nagp_ss_and_the_oracle_build(name):
    """the block layout, h_val, Pinf, Wnmf and y bit for bit (no expm in them), A and Q at rtol 1e-13 of the block's largest entry; the stored
    sites within 1e-9 of a fresh run of oracle.gf_ep.run_predict (two sweeps) on the stored matrices"""
    from nagp import harness, ss as pss
    from oracle import gf_ep as ogf, lik as olik
    c = _case(name); D, N, k1 = DRIVERS[name]; T = c['T']
    pr = harness.nmf_problem(D, N, T, 42, kernel1=k1, kernel2='matern52')
    blk = pss.ss_blocks_nmf(pr['param1'], pr['param2'], k1, 'matern52')
    A, Q, P = pss.discretise(blk)
    y = pr['y'].copy(); y[T // 3:T // 2] = np.nan
    assert np.array_equal(blk.offsets, c['block_offsets']) and np.array_equal(blk.h_val, c['h_val']) and np.array_equal(P, c['P0'])
    assert np.array_equal(pr['W'], c['Wnmf']) and np.array_equal(y, c['y'], equal_nan=True) and (int(c['D']), int(c['N'])) == (D, N)
    assert np.array_equal(c['z'], np.random.default_rng(42 + 7919).standard_normal((3, T, c['S'])))
    for n in range(blk.M):
        o, e = blk.offsets[n], blk.offsets[n + 1]
        for X, key in ((A, 'A'), (Q, 'Q')):
            want = c[key][o:e, o:e]
            assert np.abs(X[o:e, o:e] - want).max() <= 1e-13 * np.abs(want).max(), (key, n)
    model = dict(A=c['A'], Q=c['Q'], H=ref.dense_H(dict(A=c['A'], offsets=c['block_offsets'], h_val=c['h_val'])), Pinf=c['P0'], Wnmf=c['Wnmf'],
                 lik_param=np.log(pr['w_lik']))
    with np.errstate(all='ignore'):
        res = ogf.run_predict(model, c['y'], olik.Mom(olik.LIK_POWER_NMF, p=5), 0.5, 0.5 * np.ones(2), 2, predict_at_k1=False)
    assert _err(res['ttau'], c['ttau']) < 1e-9 and _err(res['tnu'], c['tnu']) < 1e-9


@pytest.mark.parametrize('name', CASES)
def test_restatement_meets_the_fixture_within_the_bound(name, capsys):
    """tests/epsample_ref.py on the stored inputs: every field within BOUND, the counters and the steps that retried as stored; on the
    retry cases this is the first run of ref.chol_retry's second attempt and of the clamp branch of ref.chol_clamped"""
    c = _case(name)
    o, cnt, steps = _ref_run(c)
    err = {f: _err(o[f], c[f]) for f in _fields(c)}
    with capsys.disabled():
        print('\n%-12s restatement  ' % name + '  '.join('%s %.1e (%.1e)' % (f, e, c['err'][f]) for f, e in err.items()) + '  counters %s' % cnt)
    assert cnt == [int(v) for v in c['counters']] and steps == [int(v) for v in c['retry_steps']]
    for f, e in err.items():
        assert e <= _bound(c, f), (f, e, _bound(c, f))
    dead = c['dead_states']
    assert not o['Xdraw'][:, dead, :].any() and not o['MS'][dead].any()


# the wrong restatements: each a copy of the module with one function replaced
def _mutant(**repl):
    spec = importlib.util.spec_from_file_location('epsample_ref_mutant', os.path.join(ROOT, 'tests', 'epsample_ref.py'))
    mod = importlib.util.module_from_spec(spec); spec.loader.exec_module(mod)
    for k, v in repl.items():
        setattr(mod, k, v(mod) if callable(v) else v)
    return mod


def _retry_every_entry(mod):
    def chol_retry(P):
        Ls = np.tril(P); Ls = Ls + np.tril(Ls, -1).T
        Lc, bad = mod.chol_clamped(Ls)
        if bad == 0:
            return Lc, 0, True
        Lc, bad = mod.chol_clamped(Ls + mod.JITTER)                   # on every entry, not on the diagonal
        return Lc, 1, bad == 0
    return chol_retry


def _retry_half_factored(mod):
    def chol_retry(P):
        n = P.shape[0]; V = np.tril(P).astype(float); retried = 0; ok = True
        for j in range(n):
            if not V[j, j] > 0.0 and not retried:                     # the second attempt goes on from here instead of from PSkp:
                V[np.arange(j, n), np.arange(j, n)] += mod.JITTER     # the columns before j keep the factor of the matrix without the jitter
                retried = 1
            if not V[j, j] > 0.0:
                V[j:, j] = 0.0; ok = False
                continue
            r = math.sqrt(V[j, j]); V[j, j] = r; V[j + 1:, j] /= r
            v = V[j + 1:, j]; V[j + 1:, j + 1:] -= np.tril(np.outer(v, v))
        return V, retried, ok
    return chol_retry


def _clamp_diagonal_only(mod):
    def chol_clamped(C):
        n = C.shape[0]; Lc = np.tril(C).astype(float); clamped = 0
        for j in range(n):
            d = Lc[j, j]
            if not d > 0.0:
                Lc[j, j] = 0.0; clamped += 1                          # the rest of the column stays
                continue
            r = math.sqrt(d); Lc[j, j] = r; Lc[j + 1:, j] /= r
            v = Lc[j + 1:, j]; Lc[j + 1:, j + 1:] -= np.tril(np.outer(v, v))
        return Lc, clamped
    return chol_clamped


def _downdate_with_the_jittered_pskp(mod):
    def backward_factors(model, PF, retry_steps=None):
        A, Q = model['A'], model['Q']; T, S, _ = PF.shape
        G = np.zeros((T, S, S)); Lc = np.zeros((T, S, S)); cnt = np.zeros(2, np.int64)
        for k in range(T - 1):
            L, r, _ = mod.chol_retry(A @ PF[k] @ A.T + Q); cnt[0] += r
            if r and retry_steps is not None:
                retry_steps.append(k)
            G[k] = np.linalg.solve(L.T, np.linalg.solve(L, (PF[k] @ A.T).T)).T
            Lc[k], c = mod.chol_clamped(PF[k] - G[k] @ (L @ L.T) @ G[k].T); cnt[1] += c       # not the Joseph form with the true Q
        Lc[T - 1], c = mod.chol_clamped(PF[T - 1]); cnt[1] += c
        return G, Lc, cnt
    return backward_factors


# name: (replacement, pk1 override, the case that must catch it, whether it only concerns the retry / the clamp: then s16 must not see it)
MUTANTS = {
    'jitter_doubled': (dict(JITTER=2 * 0.005), None, 'retry_all', True),
    'jitter_on_every_entry': (dict(chol_retry=_retry_every_entry), None, 'retry_s52', True),
    'second_attempt_on_the_half_factored_matrix': (dict(chol_retry=_retry_half_factored), None, 'retry_some', True),
    'clamped_pivot_zeroes_the_diagonal_only': (dict(chol_clamped=_clamp_diagonal_only), None, 'retry_some', True),
    'downdate_with_the_jittered_pskp': (dict(backward_factors=_downdate_with_the_jittered_pskp), None, 'retry_all', False),
    'predict_at_k1_ignored': (dict(), False, 's52_pk1', False),
}


@pytest.mark.parametrize('mutant', sorted(MUTANTS))
def test_the_bounds_bite(mutant, capsys):
    """a deliberately wrong restatement exceeds BOUND on the case named for it; one that only concerns the retry or the clamp stays inside
    BOUND on s16 -- the retry cases are what catches it"""
    repl, pk1, name, retry_only = MUTANTS[mutant]
    mod = _mutant(**repl)
    c = _case(name)
    try:
        o, cnt, _ = _ref_run(c, mod, pk1)
        worst = {f: _err(o[f], c[f]) / _bound(c, f) for f in _fields(c)}
    except (np.linalg.LinAlgError, AssertionError) as e:                # a factor with a zero column, non-finite draws: caught as well
        worst = {'(%s)' % type(e).__name__: math.inf}
    with capsys.disabled():
        print('\n%-44s on %-10s error / BOUND  ' % (mutant, name) + '  '.join('%s %.1e' % kv for kv in worst.items()))
    assert max(worst.values()) > 1.0, worst
    if retry_only:
        s = _case('s16')
        o, cnt, _ = _ref_run(s, mod)
        assert cnt == [0, 0] and all(_err(o[f], s[f]) <= _bound(s, f) for f in _fields(s))


def test_generator_reproduces_the_committed_bytes_of_the_two_smallest_cases():
    pytest.importorskip('mpmath')
    tool = _tool()
    with np.load(FIXTURE) as g:
        stored = {k: g[k] for k in g.files}
    for name in ('retry_all_T1', 's16'):
        built = tool.pack_blocks(tool.build_case(name, verbose=False))
        assert sorted(built) == sorted(k for k in stored if k.startswith(name + '__'))
        for k, v in built.items():
            v = np.asarray(v)
            assert v.dtype == stored[k].dtype and v.shape == stored[k].shape and v.tobytes() == stored[k].tobytes(), k


# ---------------------------------------------------------------------------------------------
# GPU
gpu = pytest.mark.gpu


@pytest.fixture(scope='module')
def _lib(nagp_lib):
    assert nagp_lib.nagp_device_count() >= 1
    return nagp_lib


def _problem(c, P0=None):
    """the L.Model of a case from its stored blocks, as tests/test_epsample_gpu.py:synthetic_blocks builds one"""
    from nagp import _lib as L
    S, M, D, N = c['S'], c['M'], int(c['D']), int(c['N'])
    off = np.ascontiguousarray(c['block_offsets'], dtype=np.int32)
    Af, Qf, Pf, hv = L.f64(c['A']), L.f64(c['Q']), L.f64(c['P0'] if P0 is None else P0), L.f64(np.array(c['h_val']))
    blk = SimpleNamespace(S=S, M=M, D=D, N=N, offsets=off, h_val=hv)
    model = L.Model(S=S, M=M, D=D, N=N, block_offsets=off.ctypes.data_as(L.c_ip), A=L.dptr(Af), Q=L.dptr(Qf), Pinf=L.dptr(Pf), h_val=L.dptr(hv),
                    Wnmf=None, lik_param=0.0)
    return SimpleNamespace(blk=blk, model=model, W=L.f64(np.array(c['Wnmf'])), keep=(Af, Qf, Pf, hv, off))


def _signal(c):
    if c['sig'] is None:
        return None
    amp, link, shift = c['sig']
    return dict(amp='sqrt' if amp else 'linear', link='exp' if link else 'softplus', link_shift=float(shift))


def _sample(c, z=None, n=None, seed=0, prob=None, **kw):
    """nagp.ep_sample on a case -> dict(Fdraw, Xdraw, Sdraw, MS, counters); z: the stored normals unless given (None with n: the generator)"""
    import nagp
    if n is None:
        z = c['z'] if z is None else z; n = z.shape[0]
    kw.setdefault('states', True); kw.setdefault('signal', _signal(c))
    F, X, Sd, MS, cnt = nagp.ep_sample(prob or _problem(c), c['ttau'], c['tnu'], c['y'], n, seed, int(bool(c['predict_at_k1'])), z=z, return_counters=True, **kw)
    return dict(Fdraw=F, Xdraw=X, Sdraw=Sd, MS=MS, counters=[int(v) for v in cnt])


def _raw(c, want, n=3, P0=None):
    """nagp_ep_sample through ctypes with exactly the outputs named in `want` ('X', 'F', 'S', 'M') -> (status, dict of the arrays, counters)"""
    from nagp import _lib as L
    prob = _problem(c, P0); S, M, T = c['S'], c['M'], c['T']
    tt, tn, y, z = L.f64(c['ttau']), L.f64(c['tnu']), L.f64(c['y'], 'C'), L.f64(c['z'][:n], 'C')
    out = dict(X=np.zeros((n, T, S)), F=np.zeros((n, T, M)), S=np.zeros((n, T)), M=np.zeros((S, T), order='F'))
    sg = None
    if 'S' in want:
        amp, link, shift = c['sig']
        sg = L.EpSampleSig(Wnmf=L.dptr(prob.W), amp_kind=int(amp), link_kind=int(link), link_shift=float(shift))
    cnt = np.full(2, -1, dtype=np.int64)
    st = L.lib().nagp_ep_sample(ctypes.byref(prob.model), L.dptr(tt), L.dptr(tn), L.dptr(y), T, int(bool(c['predict_at_k1'])), n, 0, L.dptr(z),
                                ctypes.byref(sg) if sg is not None else None, *(L.dptr(out[k] if k in want else None) for k in 'XFSM'),
                                cnt.ctypes.data_as(L.c_lp), 0)
    res = {k: (out[k].transpose(0, 2, 1) if k in 'XF' else out[k]) for k in want}
    return st, res, cnt


@gpu
@pytest.mark.parametrize('name', CASES)
def test_kernels_meet_the_multiprecision_fixture(_lib, name, capsys):
    """every case on its stored normals: Xdraw, Fdraw (against H Xdraw of the fixture), MS and Sdraw within BOUND, the counters as stored;
    the draws of a state of zero variance are its filtered mean, zero, exactly"""
    c = _case(name)
    o = _sample(c)
    err = {f: _err(o[f], c[f]) for f in _fields(c)}
    with capsys.disabled():
        print('\n%-12s S %2d NTL %d  ' % (name, c['S'], (c['S'] + 15) // 16) + '  '.join('%s %.1e (%.1e)' % (f, e, c['err'][f]) for f, e in err.items())
              + '  counters %s      [measured (err_oracle)]' % o['counters'])
    assert o['counters'] == [int(v) for v in c['counters']]
    for f, e in err.items():
        assert e <= _bound(c, f), (f, e, _bound(c, f))
    dead = c['dead_states']
    assert not o['Xdraw'][:, dead, :].any() and not o['MS'][dead].any() and not o['Fdraw'][:, [n for n in range(c['M']) if c['block_offsets'][n] in dead], :].any()


def _batch_of(c, budget_mb):
    """draws of one device batch under NAGP_EPS_BUDGET_MB = budget_mb for a call with z, Xdraw and Fdraw (eps_fixed_bytes, eps_draw_bytes and
    batch_plan of csrc/nagp_api_layout.hpp, restated)"""
    S, M, T = c['S'], c['M'], c['T']; nb2 = int(np.sum(np.diff(c['block_offsets']) ** 2))
    fixed = 8 * (T * (2 * S * S + 2 * S + 2 * M + 1) + 3 * S * S + 2 * nb2 + M + 8) + 4 * (2 * M + 2 + S) + 4096
    per_draw = 8 * T * (2 * S + M)
    nb = ((budget_mb << 20) - fixed) // per_draw
    return nb - nb % 16 if nb > 16 else nb


@gpu
@pytest.mark.parametrize('name', RETRY)
def test_retry_cases_in_device_batches_give_the_bits_of_one_batch(_lib, name, monkeypatch, capsys):
    """NAGP_EPS_BUDGET_MB takes whole MiB, under which three draws of these sizes never split: the stored normals are repeated to one batch
    and three draws more.  Bit for bit the unbatched call; the counters unchanged (the factorisation runs once whatever the batches); the
    first three draws still within BOUND of the fixture."""
    c = _case(name)
    mb = 2 if c['S'] > 32 else 1
    nb = _batch_of(c, mb); n = nb + 3
    assert 0 < nb < n <= 32768
    z = np.tile(c['z'], (n // 3 + 1, 1, 1))[:n]
    whole = _sample(c, z=z)
    monkeypatch.setenv('NAGP_EPS_BUDGET_MB', str(mb))
    parts = _sample(c, z=z)
    with capsys.disabled():
        print('\n%-12s %d draws as %d + 3 under %d MiB: counters %s' % (name, n, nb, mb, parts['counters']))
    assert parts['counters'] == whole['counters'] == [int(v) for v in c['counters']]
    for f in ('Xdraw', 'Fdraw', 'MS'):
        assert np.array_equal(whole[f], parts[f]), f
    for j in range(nb, n):                                              # the second batch: the same normals as a draw of the first, the same bits
        assert np.array_equal(parts['Xdraw'][j], parts['Xdraw'][j % 3])
    for f in ('Xdraw', 'Fdraw'):
        assert _err(parts[f][:3], c[f]) <= _bound(c, f)
    assert _err(parts['MS'], c['MS']) <= _bound(c, 'MS')


@gpu
def test_not_positive_definite_even_with_the_jitter_is_reported(_lib):
    """retry_some's model with P0[3, 3] = -0.05: the smallest eigenvalue of PSkp is -4.7e-2 .. -3.0e-2 over the first steps, ten times beyond
    the jitter.  nagp.ep_sample raises, the C entry point returns NAGP_ENOTPD, and a valid call afterwards returns the bits it returned before."""
    import nagp
    s16 = _case('s16'); before = _sample(s16)
    c = _case('retry_some')
    P0 = np.array(c['P0']); i, v = _tool().NOTPD_P0; P0[i, i] = v
    with pytest.raises(np.linalg.LinAlgError):
        _ref_run(dict(c, P0=P0))
    with pytest.raises(nagp.NagpError, match=r'\(-6\).*not positive definite'):
        _sample(c, prob=_problem(c, P0))
    st, _, cnt = _raw(c, 'XFM', P0=P0)
    assert st == ENOTPD and b'not positive definite' in _lib.nagp_last_error()
    after = _sample(s16)
    assert after['counters'] == before['counters'] == [0, 0]
    for f in ('Xdraw', 'Fdraw', 'Sdraw', 'MS'):
        assert np.array_equal(before[f], after[f]), f


@gpu
def test_each_output_alone_is_the_matching_part_of_the_full_call(_lib):
    """s33 (the 512-thread filter, 15 padded rows): MS alone is the call without a draw, a grid of one mean-chain workgroup"""
    c = _case('s33')
    st, full, cnt = _raw(c, 'XFSM')
    assert st == 0 and list(cnt) == [0, 0]
    for f, k in (('Xdraw', 'X'), ('Fdraw', 'F'), ('Sdraw', 'S'), ('MS', 'M')):
        assert _err(full[k], c[f]) <= _bound(c, f), f
    for k in 'MXFS':
        st, one, cnt = _raw(c, k)
        assert st == 0 and list(cnt) == [0, 0] and list(one) == [k]
        assert np.array_equal(one[k], full[k]), k
    o = _sample(c, states=False, fdraw=False, signal=None)               # the wrapper's MS-only call
    assert o['Xdraw'] is None and o['Fdraw'] is None and o['Sdraw'] is None and np.array_equal(o['MS'], full['M'])


@gpu
def test_draw_counts_around_the_block_of_sixteen(_lib):
    """s16 with the generator, n = 16, 32, 33: draws 0 .. 15 of each are the 16-draw call bit for bit, MS is the same array in all three"""
    c = _case('s16'); prob = _problem(c)
    r = {n: _sample(c, n=n, seed=5, prob=prob) for n in (16, 32, 33)}
    for n in (16, 32, 33):
        assert r[n]['Xdraw'].shape == (n, 16, c['T']) and r[n]['counters'] == [0, 0]
        for f in ('Xdraw', 'Fdraw', 'Sdraw'):
            assert np.array_equal(r[n][f][:16], r[16][f]), (n, f)
        assert np.array_equal(r[n]['MS'], r[16]['MS'])
        assert _err(r[n]['MS'], c['MS']) <= _bound(c, 'MS')
    assert np.array_equal(r[33]['Xdraw'][:32], r[32]['Xdraw']) and not np.array_equal(r[33]['Xdraw'][32], r[33]['Xdraw'][0])
