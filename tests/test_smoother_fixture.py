"""The EKF filter and the RTS smoother against a 96-digit restatement of one global iteration of gf_giekf_modulator_nmf.

tests/golden/ekf_rts_multiprecision.npz (tools/make_smoother_fixture.py) holds, per case, the f64 inputs the product is handed
(A, Q, Pinf, h_val, block_offsets, Wnmf, lik_param, y), the filtered and smoothed means MF, MS, the outputs Eft, Varft and the smoothed
covariance PS at four steps, computed in 320-bit fixed point from those exact doubles and rounded to f64 once, and err_oracle: the error
of the f64 oracle (oracle/giekf.py:run_predict) against that run, per field (max-abs error over the largest entry of the field).

CPU: the inputs are still what nagp.ss builds; the fixture reproduces at another precision and satisfies the output equations; the two
oracles stay at err_oracle; the badly conditioned cases are harder for the oracle than the baseline.

GPU (-m gpu): every case through Plan(KIND_GIEKF) under the default gain form, NAGP_GAIN_FORM=solve, NAGP_GAIN_FORM=inv and
NAGP_NO_GAIN_MFMA=1, pipelined and serial, with and without the smoothed covariances (which changes the span-pass kernels), chunks
shorter than the sequence; every field against the FIXTURE within BOUND(field, case) = max(10 x err_oracle, 1e-12) <= TOL_MEAN = 1e-7
(the factor 10: another summation order -- 16x16 MFMA tiles over up to 160 columns -- of the same rounding-times-conditioning error the
oracle shows), no jitter retry, no failed factorisation.  Measured errors are printed beside err_oracle (DESIGN.md section 2 has the tables).
"""
import importlib.util
import os

import numpy as np
import pytest

from nagp import ss as pss
from oracle import giekf as oek

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, 'tests', 'golden', 'ekf_rts_multiprecision.npz')
TOL_MEAN = 1e-7
FIELDS = ('MF', 'MS', 'Eft', 'Varft', 'PS')
CASES = ('a_l1', 'a_l3', 'b_l1', 'b_l3', 'c', 'd_bal', 'd_unbal', 'e', 'f')
BASELINE = {1: 'a_l1', 3: 'a_l3'}                       # the balanced baseline with the same l_iter
HARD = ('b_l1', 'b_l3', 'c', 'd_unbal')                 # unbalanced long length-scales: must be harder for the f64 oracle than the baseline
VARIANTS = {'default': {}, 'solve': {'NAGP_GAIN_FORM': 'solve'}, 'inv': {'NAGP_GAIN_FORM': 'inv'}, 'valu': {'NAGP_NO_GAIN_MFMA': '1'}}
SCHEDULES = {'pipelined': {}, 'serial': {'NAGP_NO_PIPELINE': '1'}}


def _fixture():
    return np.load(FIXTURE)


def _case(g, name):
    keys = [k[len(name) + 2:] for k in g.files if k.startswith(name + '__')]
    c = {k: g['%s__%s' % (name, k)] for k in keys}
    c['D'], c['N'], c['l_iter'] = int(c['D']), int(c['N']), int(c['l_iter'])
    c['S'] = c['A'].shape[0]; c['T'] = c['y'].size
    c['err'] = dict(zip(FIELDS, c['err_oracle']))
    return c


def _bound(c, f):
    """max(10 x err_oracle, 1e-12); err_oracle <= 1e-8 is asserted below, so the bound never reaches TOL_MEAN."""
    return min(max(10.0 * float(c['err'][f]), 1e-12), TOL_MEAN)


def _ps_cols(S, j):
    """the columns of PS stored at the j-th stored step (tools/make_smoother_fixture.py:ps_selection)"""
    stride = 1 if S <= 40 else (4 if S <= 100 else 8)
    return np.arange(j * stride // 4, S, stride)


def _pack_ps(PS_at, c):
    """PS_at(k) -> S x S array; the stored steps and columns side by side, as the fixture holds them"""
    return np.concatenate([np.asarray(PS_at(int(k)))[:, _ps_cols(c['S'], j)] for j, k in enumerate(c['ps_steps'])], axis=1)


def _err(x, ref):
    x = np.asarray(x, float)
    assert x.shape == ref.shape, (x.shape, ref.shape)
    assert np.all(np.isfinite(x))
    return float(np.abs(x - ref).max() / np.abs(ref).max())


def _tool():
    spec = importlib.util.spec_from_file_location('make_smoother_fixture', os.path.join(ROOT, 'tools', 'make_smoother_fixture.py'))
    mod = importlib.util.module_from_spec(spec); spec.loader.exec_module(mod)
    return mod


def _blocks(c):
    blk = pss.ss_blocks_nmf(c['param1'], c['param2'], str(c['kernel1']), str(c['kernel2']))
    return pss.balance_blocks(blk) if bool(c['balanced']) else blk


def _oracle_model(c):
    H = np.zeros((c['h_val'].size, c['S'])); H[np.arange(c['h_val'].size), c['block_offsets'][:-1]] = c['h_val']
    return dict(A=c['A'], Q=c['Q'], H=H, Pinf=c['Pinf'], Wnmf=c['Wnmf'], lik_param=c['lik_param'])


# ---------------------------------------------------------------------------------------------
# CPU
def test_fixture_holds_the_cases_it_claims():
    g = _fixture()
    assert tuple(g['cases']) == CASES and tuple(g['fields']) == FIELDS
    shapes = {}
    for name in CASES:
        c = _case(g, name)
        assert c['T'] <= 32 and int(c['prec_bits']) >= 200 and float(c['agree_256_bits']) < 1e-60      # 60 digits or more
        assert int(c['chol_retries_oracle']) == 0
        nan = np.where(np.isnan(c['y']))[0]
        assert nan.size >= 1 and 0 < nan[0] < c['T'] - 1 and list(c['ps_steps']) == [0, nan[0] - 1, nan[0] + 1, c['T'] - 1]
        assert np.all(c['err_oracle'] <= 1e-8), (name, c['err_oracle'])            # 10 x err_oracle stays below TOL_MEAN
        for f in ('MF', 'MS'):
            assert c[f].shape == (c['S'], c['T'])
        assert c['Eft'].shape == c['Varft'].shape == (c['D'] + c['N'], c['T'])
        shapes[name] = (c['D'], c['N'], c['S'], bool(c['balanced']), c['l_iter'])
    assert shapes['a_l1'] == (3, 2, 18, True, 1) and shapes['a_l3'] == (3, 2, 18, True, 3)
    assert shapes['b_l1'] == (3, 2, 18, False, 1) and shapes['b_l3'] == (3, 2, 18, False, 3)
    assert shapes['c'][:4] == (16, 3, 73, False) and shapes['d_bal'][:4] == (32, 6, 146, True) and shapes['d_unbal'][:4] == (32, 6, 146, False)
    assert shapes['e'][:4] == (5, 2, 36, False) and str(_case(g, 'e')['kernel1']) == 'matern52'
    assert np.isnan(_case(g, 'b_l1')['y'][-1]) and np.isnan(_case(g, 'b_l3')['y'][-1])       # a missing LAST observation
    b = _case(g, 'b_l1'); assert sorted(b['param2'][2:]) == [1500.0, 20000.0]
    cc = _case(g, 'c'); assert cc['param1'][16:32].min() == 3.0 and abs(float(np.exp(cc['lik_param'][0])) - 1e-6) < 1e-20
    f = _case(g, 'f'); o = f['block_offsets']
    worst = max(np.abs(np.linalg.inv(f['A'][o[n]:o[n + 1], o[n]:o[n + 1]])).sum(axis=1).max() for n in range(5))
    assert 4.0 < worst <= 8.0                    # the largest amplification the guard of the explicit-inverse gain lets through
    assert os.path.getsize(FIXTURE) < 600 * 1024


@pytest.mark.parametrize('name', CASES)
def test_fixture_inputs_are_what_nagp_ss_builds(name):
    """Pinf, h_val and the block layout bit for bit (no expm in them); A and Q within one ulp of the block's largest entry (expm)."""
    c = _case(_fixture(), name)
    blk = _blocks(c)
    A, Q, P = pss.discretise(blk)
    assert np.array_equal(blk.offsets, c['block_offsets']) and np.array_equal(blk.h_val, c['h_val']) and np.array_equal(P, c['Pinf'])
    for n in range(blk.M):
        o, e = blk.offsets[n], blk.offsets[n + 1]
        for X, name_ in ((A, 'A'), (Q, 'Q')):
            ref = c[name_][o:e, o:e]
            assert np.abs(X[o:e, o:e] - ref).max() <= 2.0 ** -52 * np.abs(ref).max(), (name_, n)
    off = np.zeros((c['S'], c['S']), bool)
    for n in range(blk.M):
        off[blk.offsets[n]:blk.offsets[n + 1], blk.offsets[n]:blk.offsets[n + 1]] = True
    assert not np.any(c['A'][~off]) and not np.any(c['Q'][~off]) and not np.any(c['Pinf'][~off])


@pytest.mark.parametrize('name', CASES)
def test_fixture_satisfies_its_output_equations(name):
    """In f64, to rounding: the last smoothed mean is the last filtered one, Eft = H MS, Varft = diag(H PS H') at the stored steps,
    PS is symmetric where it is stored in full, and a missing observation leaves the predicted mean: MF_k = A MF_{k-1}."""
    c = _case(_fixture(), name)
    off = c['block_offsets'][:-1]; hv = c['h_val']; S = c['S']
    assert np.array_equal(c['MS'][:, -1], c['MF'][:, -1])
    assert np.abs(c['Eft'] - hv[:, None] * c['MS'][off]).max() <= 4 * 2.0 ** -53 * np.abs(c['Eft']).max()
    pos = 0; seen = 0
    for j, k in enumerate(c['ps_steps']):
        cols = _ps_cols(S, j); blkps = c['PS'][:, pos:pos + cols.size]; pos += cols.size
        for n, o in enumerate(off):
            if o in cols:
                v = hv[n] ** 2 * blkps[o, list(cols).index(o)]
                assert abs(v - c['Varft'][n, k]) <= 4 * 2.0 ** -53 * abs(v); seen += 1
        if cols.size == S:
            assert np.abs(blkps - blkps.T).max() <= 2.0 ** -52 * np.abs(blkps).max()
        assert np.all(np.diag(blkps[cols]) > 0)
    assert pos == c['PS'].shape[1] and seen >= 1
    for k in np.where(np.isnan(c['y']))[0]:
        pred = c['A'] @ c['MF'][:, k - 1]
        assert np.abs(pred - c['MF'][:, k]).max() <= 8 * 2.0 ** -53 * np.abs(c['MF'][:, k]).max()


@pytest.mark.parametrize('name', ['a_l1', 'b_l3', 'e', 'f'])
def test_fixture_is_reproduced_at_another_precision(name):
    """The tool's step function at 192 bits instead of 320 (the small cases: a few seconds) rounds to the stored doubles, to one ulp of
    each field's largest entry -- the fixture is a property of the equations, not of the working precision."""
    pytest.importorskip('mpmath')
    tool = _tool(); c = _case(_fixture(), name)
    assert tool.CASES[name]['l_iter'] == c['l_iter']
    run, fx = tool.run_case(c, c['D'], c['N'], c['l_iter'], 192)
    run['PS'] = tool.pack_ps(run['PS'], c['ps_steps'], c['S'])
    for f in FIELDS:
        assert _err(fx.f64(run[f]), c[f]) <= 2.0 ** -52, f


def test_the_restated_measurement_model_has_the_jacobian_it_claims():
    """h and dh of the tool for both links (softplus with a shift, exp) against central differences in 96-digit arithmetic."""
    mpm = pytest.importorskip('mpmath')
    tool = _tool(); c = _case(_fixture(), 'a_l1')
    mpm.mp.prec = 384
    fx = tool.Fx(320); off = np.array([int(o) for o in c['block_offsets']]); D, N = c['D'], c['N']
    hv = fx.of(c['h_val']); W = fx.of(c['Wnmf']); x = fx.of(c['MS'][:, 3])
    for link, shift in (('softplus', 0.0), ('softplus', 1.5), ('exp', 0.0)):
        lk, dlk = tool.link_funs(fx, link, shift)
        mu, J = tool.meas(fx, x, hv, off, W, D, N, lk, dlk)
        z = c['h_val'][:D] * c['MS'][off[:D], 3]; gg = c['h_val'][D:] * c['MS'][off[D:D + N], 3]
        lg = np.exp(gg) if link == 'exp' else np.log1p(np.exp(gg - shift))
        assert abs(float(fx.mpf(mu)) - z @ c['Wnmf'] @ lg) <= 1e-13 * np.abs(z).max() * np.abs(c['Wnmf'] @ lg).max() * D
        h = 1 << 200                                                 # 2^-120
        for i in range(c['S']):
            xp = x.copy(); xp[i] += h; xm = x.copy(); xm[i] -= h
            fd = ((tool.meas(fx, xp, hv, off, W, D, N, lk, dlk)[0] - tool.meas(fx, xm, hv, off, W, D, N, lk, dlk)[0]) << 320) // (2 * h)
            assert abs(float(fx.mpf(fd - J[i]))) < 1e-30, (link, i)


@pytest.mark.parametrize('name', CASES)
def test_oracles_meet_the_fixture_at_the_stored_error(name, capsys):
    """oracle/giekf.py (all fields) and the compiled oracle/cpu (Eft, Varft; plain and structured form) against the fixture: within the
    bound the kernels are held to, which is built from the error stored when the fixture was made -- an oracle that drifts fails here."""
    from oracle import cpu as ocpu
    c = _case(_fixture(), name)
    model = _oracle_model(c)
    with np.errstate(all='ignore'):
        o = oek.run_predict(model, c['y'], c['D'], c['N'], 1, c['l_iter'])
    assert o['counters'].get('chol_retries', 0) == 0
    got = dict(MF=o['MF'], MS=o['MS'], Eft=o['Eft'], Varft=o['Varft'], PS=_pack_ps(lambda k: o['PS'][k], c))
    err = {f: _err(got[f], c[f]) for f in FIELDS}
    lines = ['%-8s oracle/giekf.py  ' % name + '  '.join('%s %.1e (%.1e)' % (f, err[f], c['err'][f]) for f in FIELDS)]
    cerr = {}
    for structured in (False, True):
        r = ocpu.giekf_predict(model, c['y'], c['D'], c['N'], 1, c['l_iter'], structured=structured)
        assert r['status'] == 0 and r['counters'] == dict(chol_retries=0, not_pd=0)
        cerr[structured] = {f: _err(r[f], c[f]) for f in ('Eft', 'Varft')}
        lines.append('%-8s oracle/cpu %-10s ' % (name, 'structured' if structured else 'plain') + '  '.join('%s %.1e' % (f, e) for f, e in cerr[structured].items()))
    with capsys.disabled():
        print('\n' + '\n'.join(lines) + '      [measured (err_oracle stored)]')
    for f in FIELDS:
        assert err[f] <= _bound(c, f), (f, err[f], c['err'][f])
    for structured in (False, True):
        for f in ('Eft', 'Varft'):
            assert cerr[structured][f] <= _bound(c, f), (structured, f)


def test_unbalanced_long_length_scales_are_harder_for_the_f64_oracle_than_the_baseline(capsys):
    """err_oracle of b, c and the unbalanced d exceeds that of the balanced baseline with the same l_iter in at least one field:
    otherwise the cases do not stress what they claim to and have to be drawn again."""
    g = _fixture()
    with capsys.disabled():
        print('\nerr_oracle      ' + ''.join('%-10s' % f for f in FIELDS))
        for name in CASES:
            print('%-16s' % name + ''.join('%-10.1e' % e for e in _case(g, name)['err_oracle']))
    for name in HARD:
        c = _case(g, name); a = _case(g, BASELINE[c['l_iter']])
        assert np.any(c['err_oracle'] > a['err_oracle']), name


# ---------------------------------------------------------------------------------------------
# GPU
@pytest.fixture(scope='module')
def _lib(nagp_lib):
    assert nagp_lib.nagp_device_count() >= 1
    return nagp_lib


def _gpu_run(c, env, want_ps):
    from nagp import _lib as L
    from nagp.plan import Plan
    blk = _blocks(c); blk.h_val = np.array(c['h_val'])
    T = c['T']; chunk = 5 if T <= 12 else (10 if T <= 24 else 12)          # spans end inside the sequence
    os.environ.update(env)
    try:
        plan = Plan(L.KIND_GIEKF, [(blk, c['Wnmf'], c['lik_param'], dict(A=c['A'], Q=c['Q'], Pinf=c['Pinf']))], T, ep_itts=1,
                    l_iter=c['l_iter'], flags=L.FLAG_WANT_PS if want_ps else 0, chunk=chunk)
        plan.upload([c['y']]); plan.execute(); o = plan.download(want_PS=want_ps, want_MF=True)[0]; plan.close()
    finally:
        for k in env:
            os.environ.pop(k, None)
    return o


@pytest.mark.gpu
@pytest.mark.parametrize('variant', list(VARIANTS))
@pytest.mark.parametrize('name', CASES)
def test_kernels_meet_the_multiprecision_fixture(_lib, name, variant, capsys):
    """Every output field of the plan against the fixture, within max(10 x err_oracle, 1e-12), for each gain form / gain kernel, both
    schedules, with and without smoothed covariances; no jitter retry and no failed factorisation (the fixture has neither branch)."""
    from nagp import _lib as L                                             # noqa: F401
    c = _case(_fixture(), name)
    lines, bad = [], []
    for sched, senv in SCHEDULES.items():
        for want_ps in (False, True):
            o = _gpu_run(c, dict(VARIANTS[variant], **senv), want_ps)
            assert o.counters[0] == 0 and o.counters[3] == 0, (sched, want_ps, o.counters)      # NAGP_CNT_CHOL_RETRY, NAGP_CNT_NOTPD
            got = dict(MF=o.MF, MS=o.MS, Eft=o.Eft, Varft=o.Varft)
            if want_ps:
                got['PS'] = _pack_ps(lambda k: o.PS[:, :, k], c)
            err = {f: _err(got[f], c[f]) for f in got}
            lines.append('%-8s %-7s %-9s PS %d  ' % (name, variant, sched, want_ps)
                         + '  '.join('%s %.1e (%.1e)' % (f, err[f], c['err'][f]) for f in err))
            bad += [(sched, want_ps, f, err[f], _bound(c, f)) for f in err if not err[f] <= _bound(c, f)]
    with capsys.disabled():
        print('\n' + '\n'.join(lines) + '      [measured (err_oracle)]')
    assert not bad, bad
