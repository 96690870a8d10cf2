"""The cubature moments `mom`, the ADF sweep and the Power-EP sweeps of the gf and ihgp families against a multi-precision restatement.

tests/golden/ep_multiprecision.npz (with the ihgp runs in ep_multiprecision_ihgp.npz and the knot tables in ep_multiprecision_tables.npz beside
it; tools/make_ep_fixture.py) holds, per case,
the f64 inputs the product is handed (A, Q, Pinf, h_val, block_offsets, Wnmf, lik_param, y, wn, xn_unscaled, ep_fraction, ep_damping; for
ihgp the product's own knot-level look-up tables), and per family and sweep count the outputs MF, MS, Eft, Varft, ttau, tnu, R (ihgp), lZ
and PS at four steps (gf), nlZ, computed from those exact doubles in 320-bit arithmetic (mpmath floats for mom, integer fixed point for
the Kalman algebra), repeated at 256 bits, and rounded to f64 once.  Every discontinuity of the algorithm (table look-up, clamp, cavity sign,
site denominator, jitter floor) is decided with a stored margin, so no case, step or site is excused here.  err_oracle is the error of
oracle/*.py and oracle/cpu against that run.

BOUND(field, case, family) = min(max(10 x err_oracle, 1e-12), TOL) with TOL the suite's 1e-7 (means), 1e-6 (sites), 1e-8 (log Z); the
generator asserts 10 x err_oracle < TOL, so the cap never passes a test.  The factor 10 stands for another summation order of the same
rounding-times-conditioning error; the ihgp look-up adds none (both sides interpolate the stored knots with the same elementwise
expression, tool.interp_rows).  Nothing here is tuned on a device.

CPU: the fixture holds what it claims; its inputs are what nagp.ss / nagp.ihgp_tables build; the oracles stay at err_oracle; the
generator reproduces the committed bytes; five deliberately wrong oracles (see test_the_bounds_bite) exceed the bounds on case a.

GPU (-m gpu): every case, family, sweep count and field through Plan on every launch path the sweeps have, with the plan's NAGP_STAMPS
lines asserted; a batch of two segments; nagp_mom_eval on the stored triples; NaN / Inf patterns and the clamped-site counter.
"""
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest

from nagp import ihgp_tables, ss as pss

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    if 'make_ep_fixture' in sys.modules:
        return sys.modules['make_ep_fixture']
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    spec = importlib.util.spec_from_file_location('make_ep_fixture', os.path.join(ROOT, 'tools', 'make_ep_fixture.py'))
    mod = importlib.util.module_from_spec(spec); sys.modules['make_ep_fixture'] = mod; spec.loader.exec_module(mod)
    return mod


tool = _tool()
CASES = ('a', 'a2', 'b', 'c', 'd', 'e', 'f', 'g', 'p')
SHAPES = dict(a=(8, 3, 40), a2=(8, 3, 40), b=(8, 3, 40), c=(8, 7, 24), d=(32, 6, 20), e=(8, 3, 40), f=(5, 2, 40), g=(4, 8, 24), p=(3, 3, 40))
MOM_CASES = ('a', 'c', 'e', 'g', 'p')
_G = {}


def _fixture():
    if not _G:
        _G.update(tool.load())
    return _G


def _case(name):
    """(inp, fams): the case's shared inputs and, per family, its model (and knot tables)."""
    g = _fixture(); pre = name + '__'
    fams = {f: {} for f in g[pre + 'families']}
    inp = {}
    for k in g:
        if not k.startswith(pre):
            continue
        parts = k[len(pre):].split('__')
        if parts[0] in fams:
            if len(parts) == 2:
                fams[parts[0]][parts[1]] = g[k]
        else:
            inp[parts[0]] = g[k]
    return inp, fams


def _run(name, family, itts):
    """The stored outputs of one run with err (field -> err_oracle) and the margins by name."""
    g = _fixture(); pre = '%s__%s__i%d__' % (name, family, itts)
    c = {k[len(pre):]: g[k] for k in g if k.startswith(pre)}
    c['err'] = dict(zip(tool.fields_of(family, itts), c['err_oracle']))
    c['mg'] = dict(zip(tool.MARGIN, c['margins']))
    return c


def _runs(name):
    return [(f, i) for f in _case(name)[1] for i in tool.SWEEPS]


# ---------------------------------------------------------------------------------------------
# CPU
def test_fixture_holds_the_cases_it_claims():
    g = _fixture()
    assert tuple(g['cases']) == CASES and tuple(g['margin_names']) == tuple(tool.MARGIN)
    for name in CASES:
        inp, fams = _case(name)
        D, N, T = SHAPES[name]
        assert (int(inp['D']), int(inp['N']), inp['y'].size) == (D, N, T) and T <= 40
        assert list(np.where(np.isnan(inp['y']))[0]) == [T // 3]                      # one interior missing sample
        assert float(inp['ep_fraction']) == 0.5 and list(inp['ep_damping']) == [0.5, 0.4, 0.3]
        assert int(inp['seeds_skipped']) >= 0 and int(inp['seed']) == tool.CASES[name]['seed'] + int(inp['seeds_skipped'])
        assert tuple(fams) == (('gf',) if name == 'p' else ('gf', 'ihgp'))
        for family, itts in _runs(name):
            c = _run(name, family, itts)
            assert int(c['prec_bits']) >= 320 and float(c['agree_256_bits']) < 1e-60
            for k, lim in tool.MARGIN.items():
                assert c['mg'][k] >= lim, (name, family, itts, k, c['mg'][k])
            for f in tool.fields_of(family, itts):
                assert 10 * c['err'][f] < tool.TOL[f], (name, family, itts, f)       # the cap of the bound is never what passes a test
            M = fams[family]['h_val'].size; S = fams[family]['A'].shape[0]
            assert c['Eft'].shape == c['Varft'].shape == c['ttau'].shape == c['tnu'].shape == (M, T) and c['nlZ'].shape == (itts,)
            assert c['MF'].shape == c['MS'].shape == (S, T)
            if family == 'gf':
                assert list(c['ps_steps']) == [0, T // 3 - 1, T // 3 + 1, T - 1] and c['lZ'].shape == (T,)
            else:
                assert c['R'].shape == (M, T) and np.all(np.isinf(c['R'][:, T // 3])) and np.all(np.isnan(c['tnu'][:, T // 3]))
                assert np.all(c['Varft'] == c['Varft'][:, :1])                        # constant in time
    a, b, c_, d, e, f, p = (_case(n) for n in 'abcdefp')
    assert str(a[0]['link']) == 'softplus' and int(a[0]['p_cubature']) == 7 and a[1]['gf']['A'].shape[0] == 41 and not bool(a[1]['gf']['balanced'])
    assert str(b[0]['link']) == 'exp' and str(b[0]['recipe']) == 'constraints' and bool(b[1]['gf']['balanced']) and bool(b[0]['constraints_variant'])
    assert int(c_[0]['p_cubature']) == 5 and c_[0]['wn'].size == 99
    assert d[1]['gf']['A'].shape[0] == 82 and d[0]['wn'].size == 305 and bool(d[0]['constraints_variant'])     # S = 82: four registers of sub-bands per lane
    assert int(e[0]['lik_kind']) == tool.LIK_SQRT and float(e[0]['link_shift']) == 1.0
    assert str(f[0]['kernel1']) == 'matern52' and int(np.diff(f[1]['ihgp']['block_offsets']).max()) == 6      # split blocks (gf), block stride 8 (ihgp)
    assert int(p[0]['lik_kind']) == tool.LIK_POWER and p[1]['gf']['h_val'].size == 6 and int(p[0]['p_cubature']) == 9 and bool(p[0]['predict_at_k1'])
    for name in MOM_CASES:
        inp, _ = _case(name)
        n = inp['mom_y'].size
        assert 24 <= n <= 48 and inp['mom_mu'].shape == inp['mom_s2'].shape == inp['mom_dlZ'].shape == inp['mom_d2lZ'].shape
        assert float(inp['mom_agree_256_bits']) < 1e-60 and all(10 * e_ < tool.MOM_TOL[f_] for f_, e_ in zip(tool.MOM_FIELDS, inp['mom_err_oracle']))
        assert np.sum(inp['mom_alpha'] == 1.0) == 6 and np.sum(inp['mom_alpha'] == 0.5) > 6      # six filter-side arguments of the run; six cavity-side ones and the stress inputs that keep the floor margin
    a2 = _case('a2')      # a's shape and mom (one plan can hold both), another model and another signal
    assert all(np.array_equal(a[0][k], a2[0][k]) for k in ('wn', 'xn_unscaled', 'lik_kind', 'link', 'link_shift', 'D', 'N')) and a[0]['y'].size == a2[0]['y'].size
    assert not np.array_equal(a[0]['param1'], a2[0]['param1']) and not np.array_equal(a[0]['y'], a2[0]['y'])
    for path in tool.files():
        assert os.path.getsize(path) < 1024 * 1024


@pytest.mark.parametrize('name', CASES)
def test_fixture_inputs_are_what_nagp_builds(name):
    """The generator's own construction of the inputs today against the stored ones: block layout, h_val, Pinf, W, the sigma points bit for
    bit (no expm in them); A, Q at rtol 1e-13 of the block's largest entry; y and the knot tables (expm and DARE solves behind them) at
    1e-9; and the interpolated 200-point tables bit for bit (their SHA-256 was stored when the fixture was made)."""
    inp, fams = _case(name)
    new, nfams = tool.case_inputs(tool.CASES[name], int(inp['seed']))
    for k in ('param1', 'param2', 'lik_param', 'wn', 'xn_unscaled') + (('Wnmf',) if 'Wnmf' in inp else ()):
        assert np.array_equal(new[k], inp[k]), k
    obs = ~np.isnan(inp['y'])
    assert np.array_equal(np.isnan(new['y']), ~obs) and np.abs(new['y'][obs] - inp['y'][obs]).max() <= 1e-9 * np.abs(inp['y'][obs]).max()
    for family, fam in fams.items():
        nf = nfams[family]; off = fam['block_offsets']
        assert np.array_equal(nf['block_offsets'], off) and np.array_equal(nf['h_val'], fam['h_val']) and np.array_equal(nf['Pinf'], fam['Pinf'])
        mask = np.zeros(fam['A'].shape, bool)
        for n in range(off.size - 1):
            o, e = off[n], off[n + 1]; mask[o:e, o:e] = True
            for X in ('A', 'Q'):
                assert np.abs(nf[X][o:e, o:e] - fam[X][o:e, o:e]).max() <= 1e-13 * np.abs(fam[X][o:e, o:e]).max(), (X, n)
        assert not np.any(fam['A'][~mask]) and not np.any(fam['Q'][~mask]) and not np.any(fam['Pinf'][~mask])
        if family == 'ihgp':
            assert np.array_equal(nf['tab_src'], fam['tab_src']) and np.allclose(nf['ro'], fam['ro'], rtol=1e-15) and np.allclose(np.logspace(-2, 4, 200), fam['r'], rtol=1e-15)
            for k in ('PPo', 'PGo'):
                assert np.abs(nf[k] - fam[k]).max() <= 1e-9 * np.abs(fam[k]).max(), k
            assert tool.tables_digest(fam) == str(fam['tab_digest'])


def test_table_expression_is_the_reference_interpolation():
    """tool.interp_rows against the dense interpolation matrix of the oracle (apxGrid's neqinterp) and the product's np.interp rows:
    the same numbers to a few ulp, and the knots themselves exactly."""
    from oracle import ihgp as oih
    _, fams = _case('f'); fam = fams['ihgp']
    nk = fam['ro'].size; tab = fam['PPo'][:nk * 36].reshape(nk, 36)
    got = tool.interp_rows(fam['ro'], tab, fam['r'])
    scale = np.abs(tab).max(axis=0)
    assert np.abs(got - oih.neqinterp_matrix(fam['ro'], fam['r']) @ tab).max() <= 8 * 2.0 ** -52 * scale.max()
    assert np.abs(got - ihgp_tables._interp_rows(fam['ro'], tab, fam['r'])).max() <= 8 * 2.0 ** -52 * scale.max()
    assert np.array_equal(tool.interp_rows(fam['ro'], tab, fam['ro']), tab)


def _oracle_fields(name, family, itts, mom=None):
    inp, fams = _case(name); fam = fams[family]
    S = fam['A'].shape[0]; T = inp['y'].size
    o = tool.oracle_run(inp, fam, family, itts, mom=mom)
    if family == 'gf':
        o['PS'] = [o['PS'][k] for k in range(T)]
    return tool.pack_fields(o, family, tool.ps_selection(S, T, [T // 3])[0], S)


@pytest.mark.parametrize('name', CASES)
def test_oracles_meet_the_fixture_at_the_stored_error(name, capsys):
    """oracle/gf_ep.py, oracle/ihgp.py (model column- and row-major) and the compiled oracle/cpu (both forms, each build of tool.CPU_BUILDS) against the
    fixture, the worst of them within BOUND(field) = min(max(10 x err_oracle, 1e-12), TOL): the bound the device is held to.  The oracles of the host
    that runs this are the same kind of f64 evaluation in another summation order (another BLAS, another -march=native build), which is what the
    factor 10 allows for; a factor 2 between two hosts' figures would compare two sampled maxima of rounding noise (the figure of a field like
    ttau or R = 1 / ttau rests on the smallest site of the case), not the oracle with the fixture.  An oracle that drifts fails here, and so does a
    fixture that no longer matches the equations.  The measurement is printed beside the stored err_oracle."""
    inp, fams = _case(name); lines = []
    for family, itts in _runs(name):
        c = _run(name, family, itts); fam = fams[family]
        S = fam['A'].shape[0]; T = inp['y'].size; steps = tool.ps_selection(S, T, [T // 3])[0]
        runs = [tool.pack_fields(r, family, steps, S) for r in tool.oracle_numpy_runs(inp, fam, family, itts) + tool.oracle_cpu_runs(inp, fam, family, itts)]
        for f in tool.fields_of(family, itts):
            err = max(tool.field_err(r[f], c[f], f) for r in runs if f in r)
            lines.append('%s %-4s sweeps %d %-5s %.1e (%.1e)' % (name, family, itts, f, err, c['err'][f]))
            assert err <= tool.bound(c['err'][f], f), (family, itts, f, err, c['err'][f])
    with capsys.disabled():
        print('\n' + '\n'.join(lines) + '      [measured (err_oracle stored)]')


@pytest.mark.parametrize('name', MOM_CASES)
def test_oracle_mom_meets_the_stored_triples(name):
    from oracle import cpu as ocpu, lik as olik
    inp, _ = _case(name)
    om = tool.oracle_mom(inp)
    link = olik.exp_link() if str(inp['link']) == 'exp' else olik.softplus_link(float(inp['link_shift']))
    cm = olik.Mom(int(inp['lik_kind']), link=link, p=int(inp['p_cubature']), wn=inp['wn'], xn_unscaled=inp['xn_unscaled'])
    err = np.zeros(3)
    for j in range(inp['mom_y'].size):
        mu, s2, y, a = inp['mom_mu'][:, j], inp['mom_s2'][:, j], inp['mom_y'][j], inp['mom_alpha'][j]
        for r in (om(inp['lik_param'], mu, s2, inp.get('Wnmf'), a, [y], 0), ocpu.mom(cm, inp['lik_param'], y, mu, s2, inp.get('Wnmf'), a)):
            err = np.maximum(err, tool.mom_errs(r, inp, j))
    assert np.all(err <= np.maximum(2 * inp['mom_err_oracle'], 1e-13)), (err, inp['mom_err_oracle'])


def test_generator_reproduces_the_committed_bytes():
    """--check on the quick part of case a (one sweep, both families, both precisions) from the committed inputs: the committed outputs, margins,
    agreement and counts come out bit for bit on any host (the inputs themselves are compared by test_fixture_inputs_are_what_nagp_builds, at the
    ulp expm and BLAS move them by; err_oracle by test_oracles_meet_the_fixture_at_the_stored_error)."""
    pytest.importorskip('mpmath')
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'make_ep_fixture.py'), '--check', '--only', 'a', '--sweeps', '1', '--stored-inputs'],
                       capture_output=True, text=True)
    assert r.returncode == 0 and 'fixture matches' in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


def _exceeds(name, family, itts, got):
    """The fields of `got` that exceed their bound against the fixture."""
    c = _run(name, family, itts); bad = []
    for f in tool.fields_of(family, itts):
        try:
            e = tool.field_err(got[f], c[f], f)
        except AssertionError:                       # another NaN / Inf pattern
            e = np.inf
        if not e <= tool.bound(c['err'][f], f):
            bad.append((f, e))
    return bad


def test_the_bounds_bite(monkeypatch):
    """The f64 oracle made wrong in one place at a time, on case a with three sweeps: each variant exceeds the bound of at least one stored
    field -- what shows that a kernel wrong in the same way would fail the GPU tests below.
      1  one cubature weight x (1 + 1e-6)                          2  -dlZ^2 dropped from the modulators' d2lZ
      3  sn2 / alpha replaced by sn2                               4  the look-up shifted by one grid index at one step (ihgp)
    The unmodified oracle passes the same check.  A fifth variant, R taken after the clamp instead of before it, cannot bite anything: wherever
    the clamp acts (ttau <= 0 or NaN) both orders end with R = Inf, because the block update overwrites R there (ihgp_ep_modulator_nmf.m:269-290;
    oracle/ihgp.py sets R = Inf where ttau == 0).  It is an equivalent mutant, and the test shows that by bit-equality of every field; a fifth
    biting variant takes its place: 5  R not set to Inf at a clamped site (the statement that makes the ordering immaterial)."""
    from oracle import ihgp as oih, gf_ep as ogf
    inp, _ = _case('a'); D = int(inp['D'])
    for family in ('gf', 'ihgp'):
        assert not _exceeds('a', family, 3, _oracle_fields('a', family, 3))
    wn = inp['wn'].copy(); wn[3] *= 1 + 1e-6

    def drop(kw):
        def post(res):
            lZ, dl, d2 = res; d2 = d2.copy(); d2[D:] += dl[D:] ** 2
            return lZ, dl, d2
        return post

    def sn2(kw):
        kw['sn2'] = kw['sn2'] * kw['ep_fraction']
    variants = {'weight': tool.oracle_mom(inp, wn=wn), 'dlZ2': tool.oracle_mom(inp, mutate=drop), 'sn2': tool.oracle_mom(inp, mutate=sn2)}
    for vname, mom in variants.items():
        for family in ('gf', 'ihgp'):
            bad = _exceeds('a', family, 3, _oracle_fields('a', family, 3, mom=mom))
            assert bad, (vname, family)
    calls = [0]; nearest = oih.nearest_index

    def shifted(r, Rv):
        calls[0] += 1
        i = nearest(r, Rv)
        return min(i + 1, r.size - 1) if calls[0] == 100 and np.isfinite(Rv) else i
    monkeypatch.setattr(oih, 'nearest_index', shifted)
    bad = _exceeds('a', 'ihgp', 3, _oracle_fields('a', 'ihgp', 3))
    monkeypatch.setattr(oih, 'nearest_index', nearest)
    assert bad and calls[0] > 100, 'look-up'
    # R after the clamp: site_update_filter hands back the clamped ttau, so R = 1 / ttau is taken behind the clamp
    ref = _oracle_fields('a', 'ihgp', 3)
    upd = ogf.site_update_filter

    def clamped_first(*a):
        tt, tn = upd(*a)
        return ogf.matlab_max0(tt), tn
    monkeypatch.setattr(oih, 'site_update_filter', clamped_first)
    got = _oracle_fields('a', 'ihgp', 3)
    monkeypatch.setattr(oih, 'site_update_filter', upd)
    assert all(np.array_equal(got[f], ref[f], equal_nan=True) for f in ref)
    # ... so what that ordering protects is pinned by the statement that makes it immaterial: R = Inf at a clamped site (:287) left out
    import inspect
    src = inspect.getsource(oih.run_predict)
    assert src.count('R[n, k] = np.inf') == 1
    ns = dict(vars(oih)); exec(src.replace('R[n, k] = np.inf', 'pass'), ns)
    monkeypatch.setattr(oih, 'run_predict', ns['run_predict'])
    bad = _exceeds('a', 'ihgp', 3, _oracle_fields('a', 'ihgp', 3))
    monkeypatch.undo()
    assert bad, 'R = Inf at clamped sites'


# ---------------------------------------------------------------------------------------------
# GPU
@pytest.fixture(scope='module')
def _lib(nagp_lib):
    assert nagp_lib.nagp_device_count() >= 1
    return nagp_lib


def _mom(inp):
    from nagp import Mom
    lik = {tool.LIK_POWER: 'likModulatorPower', tool.LIK_NMF: 'likModulatorNMFPower', tool.LIK_SQRT: 'likModulatorPreCalcwn'}[int(inp['lik_kind'])]
    return Mom(lik, link=str(inp['link']), link_shift=float(inp['link_shift']), p_cubature=int(inp['p_cubature']), wn=inp['wn'], xn_unscaled=inp['xn_unscaled'])


def _problem(inp, fam):
    blk = pss.ss_blocks_nmf(inp['param1'], inp['param2'], str(inp['kernel1']), str(inp['kernel2']))
    if bool(fam['balanced']):
        blk = pss.balance_blocks(blk)
    assert np.array_equal(blk.offsets, fam['block_offsets'])
    blk.h_val = np.array(fam['h_val'])
    return (blk, inp.get('Wnmf'), inp['lik_param'], dict(A=fam['A'], Q=fam['Q'], Pinf=fam['Pinf']))


def _plan_run(names, family, itts, env, capfd, chunk=0, want_ps=True):
    """The cases `names` (one plan, one problem each) under the developer switches `env` -> (outputs per case, the plan's NAGP_STAMPS lines)."""
    from nagp import _lib as L
    from nagp.plan import Plan
    cases = [_case(n) for n in names]; inp0 = cases[0][0]
    kind = L.KIND_GF_EP if family == 'gf' else L.KIND_IHGP
    want_ps = want_ps and family == 'gf'
    flags = (L.FLAG_WANT_PS if want_ps else 0) if family == 'gf' else (L.FLAG_IHGP_CONSTRAINTS if bool(inp0['constraints_variant']) else 0)
    tabs = [tool.flat_tables(fams['ihgp']) for _, fams in cases] if family == 'ihgp' else []
    build = ihgp_tables.build_tables
    served = []

    def fixture_tables(A_, Q_, offsets, h_val, *a, **kw):
        q = len(served); served.append(q)
        assert np.array_equal(A_, cases[q][1]['ihgp']['A']) and np.array_equal(Q_, cases[q][1]['ihgp']['Q'])
        return tabs[q]
    env = dict(env, NAGP_STAMPS='1')
    os.environ.update(env); ihgp_tables.build_tables = fixture_tables
    try:
        capfd.readouterr()
        plan = Plan(kind, [_problem(inp, fams[family]) for inp, fams in cases], inp0['y'].size, mom=_mom(inp0), ep_fraction=float(inp0['ep_fraction']),
                    ep_damping=inp0['ep_damping'][:itts], ep_itts=itts, predict_at_k1=int(bool(inp0['predict_at_k1'])), flags=flags, chunk=chunk)
        plan.upload([inp['y'] for inp, _ in cases]); plan.execute()
        outs = plan.download(want_PS=want_ps, want_MF=True); plan.close()
        stamps = capfd.readouterr().err
    finally:
        ihgp_tables.build_tables = build
        for k in env:
            os.environ.pop(k, None)
    assert family != 'ihgp' or len(served) == len(names)
    return outs, stamps


def _device_fields(o, family, name):
    inp, fams = _case(name); S = fams[family]['A'].shape[0]; T = inp['y'].size
    d = dict(MF=o.MF, MS=o.MS, Eft=o.Eft, Varft=o.Varft, ttau=o.ttau, tnu=o.tnu, R=o.R, lZ=o.lZ, nlZ=o.nlZ)
    if family == 'gf' and o.PS is not None:
        d['PS'] = [o.PS[:, :, k] for k in range(T)]
    return tool.pack_fields(d, family, tool.ps_selection(S, T, [T // 3])[0], S)


def _check(name, family, itts, o, label, lines):
    """Every stored field of the run against its bound; the NaN / Inf patterns (inside field_err) and the clamped-site counter."""
    c = _run(name, family, itts); got = _device_fields(o, family, name); bad = []
    for f in tool.fields_of(family, itts):
        if f not in got:                           # PS of a plan that does not store the smoothed covariances
            continue
        try:
            e = tool.field_err(got[f], c[f], f)
        except AssertionError as ex:
            e = np.inf; bad.append((label, name, family, itts, f, str(ex)))
        lines.append('%-22s %s %-4s sweeps %d %-5s %.1e (err_oracle %.1e, bound %.1e)' % (label, name, family, itts, f, e, c['err'][f], tool.bound(c['err'][f], f)))
        if not e <= tool.bound(c['err'][f], f):
            bad.append((label, name, family, itts, f, e, tool.bound(c['err'][f], f)))
    lines.append('%-22s %s %-4s sweeps %d clamped %d (fixture %d), chol retries %d, not PD %d' % (label, name, family, itts, o.counters[1], int(c['clamped']), o.counters[0], o.counters[3]))
    if int(o.counters[1]) != int(c['clamped']) or o.counters[0] != 0 or o.counters[3] != 0:
        bad.append((label, name, family, itts, 'counters', list(o.counters), int(c['clamped'])))
    return bad


# variant -> (developer switches, the words the plan's NAGP_STAMPS lines must hold for the cases the variant runs on, those cases); the lines name the
# form of every stage the plan chose: ADF kernel, table / direct stage 1b, block stride, sequential kernels, split blocks, likelihood, site refresh, MFMA passes
_ROLE8, _SP, _NOSP = 'role-specialised waves 1', 'sparse-point form: 1', 'sparse-point form: 0'
_DIRECT, _TAB, _SEQ0, _SEQ1 = 'table form of stage 1b 0', 'table form of stage 1b 1', 'sequential kernels in every sweep 0', 'sequential kernels in every sweep 1'
_ROLE = ('a', 'a2', 'b', 'c', 'd')                 # the cases the role layout serves
IHGP_VARIANTS = {
    'default': ({}, None, CASES[:-1]),                                                      # what each case is there for: see _default_words
    'tables': ({'NAGP_IH_TABLES': '1'}, [_ROLE8, _TAB], _ROLE),                             # ihgp_adf8b_kernel, table form of stage 1b
    'no-roles': ({'NAGP_IH_ROLES': '0'}, [_SP, 'role-specialised waves 0'], _ROLE),         # ihgp_adf_kernel
    'general': ({'NAGP_NO_SPARSE': '1'}, [_NOSP, 'role-specialised waves 0', 'staged form: 0', _SEQ0], CASES[:-1]),      # ihgp_filter_kernel, affine scans behind it
    'ring-4': ({'NAGP_IH_KB': '4'}, [_ROLE8, 'ring 4 steps'], ('a',)),
    'ring-8': ({'NAGP_IH_KB': '8'}, [_ROLE8, 'ring 8 steps'], ('a',)),
    'sequential': ({'NAGP_IH_SEQ': '1', 'NAGP_NO_SPARSE': '1'}, [_NOSP, 'staged form: 0', _SEQ1], ('a', 'e', 'f')),      # the sequential kernels for every sweep
}
_A8, _SPGF = 'role-specialised waves: 1', 'sparse-point ADF 1'
_REF_SP, _REF_SQ, _REF_GEN = 'site refresh: sparse-point form 1', 'staged square-root form 1', 'site refresh: sparse-point form 0, staged square-root form 0'
_SP_OF = dict(a=48, c=64, d=160)                   # Sp = 16 ceil(4 M / 16) of the MFMA span passes
GF_VARIANTS = {
    'default': ({}, None, CASES),
    'no-roles': ({'NAGP_NO_GF_ROLES': '1'}, [_SPGF, 'role-specialised waves: 0'], _ROLE),                     # sparse-point 256-thread form
    'general': ({'NAGP_NO_SPARSE': '1'}, ['sparse-point ADF 0', 'role-specialised waves: 0', _REF_GEN], CASES),      # general form (ADF and refresh)
    'generic-refresh': ({'NAGP_NO_SPARSE_EP': '1'}, [_REF_GEN], ('a', 'c', 'd', 'e')),                        # generic site refresh behind the default ADF sweep
    'mfma-passes': ({}, None, ('a', 'c', 'd')),                                                               # no PS asked for: the span passes run on MFMA
    'no-mfma': ({'NAGP_NO_MFMA': '1'}, ['MFMA span passes at Sp 0'], ('a', 'c', 'd')),                        # ... and on the VALU kernels
    'chunks': ({}, ['chunk 7,', 'pipelined 1'], ('a', 'd', 'f')),                                             # spans of 7 steps: shorter than T, pipelined smoother
    'serial': ({'NAGP_NO_PIPELINE': '1'}, ['chunk 7,', 'pipelined 0'], ('a', 'd', 'f')),                      # the same spans, serial schedule
}
CHUNK = {'chunks': 7, 'serial': 7}       # (the default plan of T <= 40 has one span: NAGP_CHUNKS never goes below 2048 steps, so the span length is the plan's argument)
NO_PS = ('mfma-passes', 'no-mfma')       # with PS stored the column-owner form (Sp >= 80: case d) runs the VALU span passes whatever the switch says; the
                                         # four-wave form (a: Sp 48, c: Sp 64) stays on MFMA.  These two variants do not ask for PS, so both forms are switched


def _default_words(name, family, variant='default'):
    """What the default plan of a case must say it launches."""
    if family == 'ihgp':
        return {'e': ['staged form: 1', 'block stride 4', _SEQ0], 'f': [_NOSP, 'staged form: 0', 'block stride 8', _SEQ0],
                'g': ['role-specialised waves 0', 'block stride 4', _SEQ0]}.get(name, [_ROLE8, _DIRECT, 'block stride 4', _SEQ0])
    if variant == 'mfma-passes':
        return ['MFMA span passes at Sp %d' % _SP_OF[name]]
    return {'e': ['sparse-point ADF 0', _REF_SQ, 'likelihood 2'], 'f': ['sparse-point ADF 0', 'role-specialised waves: 0', 'split blocks 1'],
            'g': ['role-specialised waves: 0', 'split blocks 0'], 'p': ['likelihood 0', 'split blocks 0']}.get(name, [_A8, _SPGF, _REF_SP, 'split blocks 0', 'likelihood 1'])


def _variant(family, variant, capfd):
    env, words, names = (IHGP_VARIANTS if family == 'ihgp' else GF_VARIANTS)[variant]
    lines, bad = [], []
    for name in names:
        for itts in tool.SWEEPS:
            outs, stamps = _plan_run([name], family, itts, env, capfd, chunk=CHUNK.get(variant, 0), want_ps=variant not in NO_PS)
            for w in (words if words is not None else _default_words(name, family, variant)):
                assert w in stamps, (variant, name, w, stamps)
            bad += _check(name, family, itts, outs[0], variant, lines)
    with capfd.disabled():
        print('\n' + '\n'.join(lines))
    assert not bad, bad


@pytest.mark.gpu
@pytest.mark.parametrize('variant', list(IHGP_VARIANTS))
def test_ihgp_sweeps_meet_the_multiprecision_fixture(_lib, variant, capfd):
    """KIND_IHGP on the fixture's tables: ihgp_adf8_kernel with direct moments (default; case e the staged square-root sweep, case f the general
    kernel at block stride 8, case g -- eight components -- outside the role layout), its table form, ihgp_adf_kernel, ihgp_filter_kernel, ring
    depths 4 and 8, the sequential kernels; one and three sweeps; every field within BOUND."""
    _variant('ihgp', variant, capfd)


@pytest.mark.gpu
@pytest.mark.parametrize('variant', list(GF_VARIANTS))
def test_gf_sweeps_meet_the_multiprecision_fixture(_lib, variant, capfd):
    """KIND_GF_EP: gf_adf8 (default; case f with split blocks, case p the plain likelihood with M = 2 D), the sparse-point 256-thread form, the
    general form, the generic site refresh, the span passes on MFMA and without it (plans that do not store PS), spans shorter than T with the pipelined and the serial smoother; one and three sweeps; every field within BOUND."""
    _variant('gf', variant, capfd)


@pytest.mark.gpu
@pytest.mark.parametrize('family', ['gf', 'ihgp'])
def test_a_batch_of_two_segments_meets_the_fixture(_lib, family, capfd):
    """Two DIFFERENT segments in one batched plan, in both orders.  A plan holds problems of one shape and one `mom` (rule, link, likelihood), so
    the segments are case a and case a2 -- a's shape and mom, another model, other tables, another signal (a with c, as first asked for, cannot be
    one plan).  Every field of each segment within ITS case's BOUND: a segment that read the other's model, tables, y, sites or ring would be off by
    orders of magnitude.  Each segment is also bit-equal to its plan of one segment."""
    lines, bad = [], []
    for itts in tool.SWEEPS:
        one = {n: _plan_run([n], family, itts, {}, capfd)[0][0] for n in ('a', 'a2')}
        for order in (['a', 'a2'], ['a2', 'a']):
            outs, _ = _plan_run(order, family, itts, {}, capfd)
            for q, n in enumerate(order):
                bad += _check(n, family, itts, outs[q], 'batch %s[%d]' % ('+'.join(order), q), lines)
                assert np.array_equal(outs[q].Eft, one[n].Eft) and np.array_equal(outs[q].ttau, one[n].ttau) and np.array_equal(outs[q].nlZ, one[n].nlZ), (order, q)
    with capfd.disabled():
        print('\n' + '\n'.join(lines))
    assert not bad, bad


@pytest.mark.gpu
@pytest.mark.parametrize('name', MOM_CASES)
def test_mom_eval_meets_the_stored_triples(_lib, name, capsys):
    """nagp_mom_eval (one launch for all triples of one alpha) against the multi-precision lZ, dlZ, d2lZ: within min(max(10 x err_oracle,
    1e-12), 1e-9 / 1e-8 / 1e-8), errors of dlZ and d2lZ over the vector's largest entry -- in place of the `rounding noise on the vector's
    scale` rule of tests/test_gpu_parity.py:test_mom_callback_itself_against_oracle, which stays as it is."""
    inp, _ = _case(name); mom = _mom(inp); err = np.zeros(3)
    for alpha in (1.0, 0.5):
        sel = np.where(inp['mom_alpha'] == alpha)[0]
        args = (inp['Wnmf'],) if 'Wnmf' in inp else ()
        lZ, dl, d2 = mom(inp['lik_param'], inp['mom_mu'][:, sel], inp['mom_s2'][:, sel], *args, alpha, [inp['mom_y'][sel]], 0)
        for i, j in enumerate(sel):
            err = np.maximum(err, tool.mom_errs((lZ[i], dl[:, i], d2[:, i]), inp, j))
    bounds = np.array([min(max(10 * e, 1e-12), tool.MOM_TOL[f]) for f, e in zip(tool.MOM_FIELDS, inp['mom_err_oracle'])])
    with capsys.disabled():
        print('\nmom %s: ' % name + '  '.join('%s %.1e (err_oracle %.1e, bound %.1e)' % (f, e, eo, b) for f, e, eo, b in zip(tool.MOM_FIELDS, err, inp['mom_err_oracle'], bounds)))
    assert np.all(err <= bounds), (err, bounds)
