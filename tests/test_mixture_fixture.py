"""The source-separation mixtures (NAGP_FLAG_MIXTURE_RULE: gf_ep_mods_nmf_mixture, ihgp_ep_mods_nmf_mixture) against a multi-precision restatement.

tests/golden/mixture_multiprecision.npz (with the ihgp runs in mixture_multiprecision_ihgp.npz and the knot tables in mixture_multiprecision_tables.npz
beside it; tools/make_mixture_fixture.py) holds, per case and family, the f64 inputs the product is handed for the stacked model (A, Q, Pinf as their
diagonal blocks, h_val, block_offsets, the block-diagonal Wnmf, lik_param, y; for ihgp the product's own knot-level look-up tables) and, per sweep
count, the outputs of oracle/mixture.py's two runs restated in 320-bit arithmetic from those exact doubles, repeated at 256 bits, rounded to f64 once:
MF, MS, Eft, Varft, ttau, tnu, R, nll, maxDiffM, maxDiffP, and for gf lZ and PS at four steps.  Every discontinuity of the rule (table look-up, clamp,
cavity, the sign of the cavity variance, site denominator, jitter floor) is decided with a stored margin, so no case, step or site is excused here.

BOUND(field) = min(max(10 x err_oracle, 1e-12), TOL), TOL 1e-7 (means, PS, maxDiff), 1e-6 (sites, R), 1e-8 (lZ, nll); err_oracle is the error of
oracle/mixture.py against the run, and the generator asserts 10 x err_oracle < TOL, so the cap never passes a test.  Nothing here is tuned on a device.

What the library reports and how it is read here:
  nll     the library's nlZ record is taken behind a sweep's refresh (nlZ[0]: sweep 1's filter; nlZ[i], i >= 1: behind the refresh of sweep i), the
          oracle's nll at the end of a sweep.  Under the mixtures' rule the smoother's refresh adds nothing to the sum before sweep 2, so
          nll[0] = nlZ[0], nll[i] = nlZ[i + 1], and the last entry is -sum lZ (gf) / -lZ[T - 1] (ihgp) of the downloaded lZ.
  clamped the library's counter: ihgp -- every entry the clamp of a filter pass finds not positive (the fixture's `clamped`); gf -- the sites its ADF
          step leaves not positive (`clamped_adf`): the negative sites the smoother's refresh leaves are clamped by the next fixed-site pass without
          being counted.  They are pinned by ttau, tnu, R and everything behind them.

CPU: the fixture holds what it claims; its inputs are what nagp.api._stack_sources and nagp.ss.discretise build; oracle/mixture.py stays within BOUND;
the generator reproduces the committed bytes; seven deliberately wrong oracles exceed the bounds (test_the_bounds_bite).
GPU (-m gpu): every case, family, sweep count and field through Plan(..., flags=FLAG_MIXTURE_RULE) on every launch path a mixture plan can take, the
plan's NAGP_STAMPS words asserted; a batch of two segments; the Python entry points.
"""
import importlib.util
import inspect
import os
import re
import subprocess
import sys
import types

import numpy as np
import pytest

from nagp import ihgp_tables, ss as pss

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROFILE = os.path.join(ROOT, 'profiles', 'r20_mixture_parity.txt')


def _tool():
    if 'make_mixture_fixture' in sys.modules:
        return sys.modules['make_mixture_fixture']
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    spec = importlib.util.spec_from_file_location('make_mixture_fixture', os.path.join(ROOT, 'tools', 'make_mixture_fixture.py'))
    mod = importlib.util.module_from_spec(spec); sys.modules['make_mixture_fixture'] = mod; spec.loader.exec_module(mod)
    return mod


tool = _tool()
CASES = ('m1', 'm1b', 'm2', 'm3', 'm4')
SHAPES = dict(m1=([(3, 1), (2, 2)], 36), m1b=([(3, 1), (2, 2)], 36), m2=([(4, 2), (4, 2), (3, 1)], 36), m3=([(4, 3)] * 3, 24), m4=([(3, 1), (2, 2)], 36))
MASKED_RUN = ('m2', 'ihgp', 3)                     # the committed run with a site that v_cav <= 0 masks out of a smoother refresh
_G = {}


def _fixture():
    if not _G:
        _G.update(tool.load())
    return _G


def _case(name):
    """(shared, {family: inputs merged with the shared ones})."""
    sh, fams = tool.stored_case(_fixture(), name)
    return sh, {f: tool.merged(sh, fi) for f, fi in fams.items()}


def _run(name, family, itts):
    g = _fixture(); pre = '%s__%s__i%d__' % (name, family, itts)
    c = {k[len(pre):]: g[k] for k in g if k.startswith(pre)}
    c['err'] = dict(zip(tool.FIELDS[family], c['err_oracle']))
    c['mg'] = dict(zip(tool.MARGIN, c['margins']))
    return c


def _runs(name):
    return [(f, i) for f in _case(name)[1] for i in tool.SWEEPS]


# ---------------------------------------------------------------------------------------------
# CPU
def test_fixture_holds_the_cases_it_claims():
    g = _fixture()
    assert tuple(g['cases']) == CASES and tuple(g['margin_names']) == tuple(tool.MARGIN) == ('lookup', 'clamp', 'cavity', 'denom', 'floor', 'cavity_sign')
    assert tool.MARGIN == dict(lookup=1e-6, clamp=1e-8, cavity=1e-3, denom=1e-2, floor=1e-6, cavity_sign=1e-3)
    masked = {}; clamped = {}
    for name in CASES:
        sh, fams = _case(name); shapes, T = SHAPES[name]
        assert tuple(fams) == ('gf', 'ihgp'), 'a dropped family must be taken out of this list and named in DESIGN.md'
        assert float(sh['ep_fraction']) == 0.75 and list(sh['ep_damping']) == [0.2] and int(sh['T']) == T <= 40
        assert [str(k) for k in sh['kernel1']] == tool.CASES[name]['k1'] and [str(k) for k in sh['kernel2']] == tool.CASES[name]['k2']
        for family, inp in fams.items():
            assert [(int(d), int(n)) for d, n in zip(inp['src_D'], inp['src_N'])] == shapes and inp['y'].size == T
            assert list(np.where(np.isnan(inp['y']))[0]) == [T // 3]                      # one interior missing sample
            lvl = int(inp['level']); scale, w_lik = tool.LEVELS[lvl]
            assert str(inp['scale']) == scale and float(inp['w_lik']) == w_lik and np.array_equal(inp['lik_param'], [np.log(w_lik)])
            assert 0 <= int(inp['seeds_skipped']) < tool.MAX_SEEDS and int(inp['seed']) == tool.CASES[name]['seed'] + int(inp['seeds_skipped'])
            assert ('signal %s, w_lik %.0e' % (scale, w_lik)) in str(inp['recipe']) and (lvl == 0) == ('no seed of' not in str(inp['recipe']))
            assert (lvl >= tool.N_LEVELS) == ('masked site' in str(inp['recipe'])) == ((name, family) == MASKED_RUN[:2])
            # the stacking order: all sub-band blocks of all sources, then all modulator blocks; Wnmf block diagonal
            bs = [2 * pss.KERNEL_ORDER[k] for (d, _), k in zip(shapes, tool.CASES[name]['k1']) for _ in range(d)]
            bs += [pss.KERNEL_ORDER[k] for (_, n), k in zip(shapes, tool.CASES[name]['k2']) for _ in range(n)]
            assert list(np.diff(inp['block_offsets'])) == bs and inp['h_val'].size == len(bs)
            D, N = int(inp['D']), int(inp['N']); mask = np.zeros((D, N), bool); d0 = n0 = 0
            for d, n in shapes:
                mask[d0:d0 + d, n0:n0 + n] = True; d0 += d; n0 += n
            assert inp['Wnmf'].shape == (D, N) and not np.any(inp['Wnmf'][~mask]) and np.all(inp['Wnmf'][mask] > 0)
            for itts in tool.SWEEPS:
                c = _run(name, family, itts)
                assert int(c['prec_bits']) >= 320 and float(c['agree_256_bits']) < 1e-60
                for k, lim in tool.MARGIN.items():
                    assert c['mg'][k] >= lim, (name, family, itts, k, c['mg'][k])
                for f in tool.FIELDS[family]:
                    assert 10 * c['err'][f] < tool.TOL[f], (name, family, itts, f)       # the cap of the bound is never what passes a test
                M = inp['h_val'].size; S = inp['A'].shape[0]
                assert c['Eft'].shape == c['Varft'].shape == c['ttau'].shape == c['tnu'].shape == c['R'].shape == (M, T) and c['MF'].shape == c['MS'].shape == (S, T)
                assert c['nll'].shape == c['maxDiffM'].shape == c['maxDiffP'].shape == (itts,)
                for f in tool.MASKS:
                    assert np.array_equal(c['nan_' + f], np.isnan(c[f])) and np.array_equal(c['inf_' + f], np.isinf(c[f]))
                assert 0 <= int(c['clamped_adf']) <= int(c['clamped']) and (itts > 1 or int(c['masked']) == 0)
                masked[(name, family, itts)] = int(c['masked']); clamped[(name, family, itts)] = int(c['clamped'])
                if family == 'gf':
                    assert list(c['ps_steps']) == [0, T // 3 - 1, T // 3 + 1, T - 1] and c['lZ'].shape == (T,)
                    assert not np.any(np.isnan(c['tnu'])) and np.all(c['ttau'][:, T // 3] == 0) and np.all(c['R'][:, T // 3] == 0)      # the guarded missing step
                    assert np.all(c['ttau'] >= 0) and (itts == 1) == (not np.any(c['maxDiffM']))
                else:
                    assert np.all(np.isinf(c['R'][:, T // 3])) and np.all(np.isnan(c['tnu'][:, T // 3])) and np.all(c['ttau'][:, T // 3] == 0)      # no isnan guard
                    assert np.all(c['Varft'] == c['Varft'][:, :1])                        # constant in time
    assert masked[MASKED_RUN] > 0                                                          # the v_cav <= 0 mask is no dead branch of the fixture
    assert any(v > 0 for (n, f, i), v in clamped.items() if f == 'gf') and any(v > 0 for (n, f, i), v in clamped.items() if f == 'ihgp')
    assert any(int(_run(n, f, 3)['clamped']) > int(_run(n, f, 3)['clamped_adf']) for n in CASES for f in ('gf', 'ihgp'))      # a site negative between smoother and filter
    m1, m1b, m2, m3, m4 = (_case(n) for n in CASES)
    assert all(np.array_equal(m1[0][k], m1b[0][k]) for k in ('wn', 'xn_unscaled', 'lik_kind', 'link', 'link_shift', 'kernel1', 'kernel2'))
    assert not np.array_equal(m1[1]['gf']['param1'], m1b[1]['gf']['param1']) and not np.array_equal(m1[1]['gf']['y'], m1b[1]['gf']['y'])
    assert int(m1[0]['lik_kind']) == tool.LIK_NMF and int(m1[0]['p_cubature']) == 7 and float(m1[0]['link_shift']) == 0.0
    assert int(m2[0]['lik_kind']) == tool.LIK_SQRT and float(m2[0]['link_shift']) == 1.0 and int(m2[0]['p_cubature']) == 7 and m2[1]['gf']['h_val'].size == 16
    assert int(m3[0]['lik_kind']) == tool.LIK_SQRT and int(m3[0]['p_cubature']) == 5 and m3[0]['xn_unscaled'].shape[0] == 9 and m3[1]['gf']['h_val'].size == 21
    assert int(np.diff(m4[1]['ihgp']['block_offsets']).max()) == 6                         # split blocks (gf), block stride 8 (ihgp)
    for path in tool.files():
        assert os.path.getsize(path) < 1024 * 1024


@pytest.mark.parametrize('name', CASES)
def test_fixture_inputs_are_what_nagp_builds(name):
    """nagp.harness.mixture_problem -> nagp.api._stack_sources -> nagp.ss.discretise today against the stored inputs: parameters, Wnmf, Pinf, h_val and the
    offsets bit for bit; A and Q within one ulp of the block's largest entry (expm); y and the knot tables (Cholesky factors, DARE solves) at 1e-9; the
    interpolated 200-point tables bit for bit (their SHA-256 was stored when the fixture was made)."""
    sh, fams = _case(name)
    new_sh = tool.shared_inputs(tool.CASES[name])
    for k in ('wn', 'xn_unscaled'):
        assert np.array_equal(new_sh[k], sh[k]), k
    for family, inp in fams.items():
        nf = tool.family_inputs(tool.CASES[name], sh, family, int(inp['seed']), float(inp['w_lik']), str(inp['scale']))
        for k in ('param1', 'param2', 'lik_param', 'Wnmf', 'Pinf', 'h_val', 'block_offsets', 'src_D', 'src_N'):
            assert np.array_equal(nf[k], inp[k]), (family, k)
        c = tool.CASES[name]      # the `prior` signals are harness.mixture_problem's own prior samples, before it normalises their sum
        mpb = tool.harness.mixture_problem(c['shapes'], c['T'], int(inp['seed']), c['k1'], c['k2'], w_lik=float(inp['w_lik'])); raw = tool.prior_signal(c, mpb, int(inp['seed']))
        assert np.array_equal(mpb['y'], raw / np.sqrt(np.var(raw)))
        obs = ~np.isnan(inp['y'])
        assert np.array_equal(np.isnan(nf['y']), ~obs) and np.abs(nf['y'][obs] - inp['y'][obs]).max() <= 1e-9 * np.abs(inp['y'][obs]).max()
        off = inp['block_offsets']; mask = np.zeros(inp['A'].shape, bool)
        for n in range(off.size - 1):
            o, e = off[n], off[n + 1]; mask[o:e, o:e] = True
            for X in ('A', 'Q'):
                assert np.abs(nf[X][o:e, o:e] - inp[X][o:e, o:e]).max() <= np.spacing(np.abs(inp[X][o:e, o:e]).max()), (family, X, n)
        assert not np.any(inp['A'][~mask]) and not np.any(inp['Q'][~mask]) and not np.any(inp['Pinf'][~mask])
        if family == 'ihgp':
            assert np.array_equal(inp['Q'], inp['Q'].T)
            assert np.array_equal(nf['tab_src'], inp['tab_src']) and np.allclose(nf['ro'], inp['ro'], rtol=1e-15) and np.allclose(np.logspace(-2, 4, 200), inp['r'], rtol=1e-15)
            for k in ('PPo', 'PGo'):
                assert np.abs(nf[k] - inp[k]).max() <= 1e-9 * np.abs(inp[k]).max(), k
            assert tool.tables_digest(inp) == str(inp['tab_digest'])


def _oracle_fields(name, family, itts, mom=None, mixture=None):
    inp = _case(name)[1][family]
    S = inp['A'].shape[0]; T = inp['y'].size
    o = tool.oracle_run(inp, family, itts, mom=mom, mixture=mixture)
    return tool.pack_fields(o, family, tool.ps_selection(S, T, [T // 3])[0], S)


@pytest.mark.parametrize('name', CASES)
def test_oracle_meets_the_fixture_at_the_stored_error(name, capsys):
    """oracle/mixture.py (model column- and row-major) against the fixture, the worse within BOUND(field): the bound the device is held to."""
    lines = []
    for family, itts in _runs(name):
        c = _run(name, family, itts); inp = _case(name)[1][family]
        S = inp['A'].shape[0]; T = inp['y'].size; steps = tool.ps_selection(S, T, [T // 3])[0]
        runs = [tool.pack_fields(o, family, steps, S) for o in tool.oracle_runs(inp, family, itts)]
        for f in tool.FIELDS[family]:
            err = max(tool.field_err(r[f], c[f], f) for r in runs)
            lines.append('%s %-4s sweeps %d %-8s %.1e (%.1e)' % (name, family, itts, f, err, c['err'][f]))
            assert err <= tool.bound(c['err'][f], f), (family, itts, f, err, c['err'][f])
    with capsys.disabled():
        print('\n' + '\n'.join(lines) + '      [measured (err_oracle stored)]')


def test_generator_reproduces_the_committed_bytes():
    """--check on the quick part of case m1 (one sweep, both families, both precisions) from the committed inputs: outputs, masks, margins, agreement
    and counts come out bit for bit on any host."""
    pytest.importorskip('mpmath')
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'make_mixture_fixture.py'), '--check', '--only', 'm1', '--sweeps', '1', '--stored-inputs'],
                       capture_output=True, text=True)
    assert r.returncode == 0 and 'fixture matches' in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


def _exceeds(name, family, itts, got):
    """The fields of `got` that exceed their bound against the fixture."""
    c = _run(name, family, itts); bad = []
    for f in tool.FIELDS[family]:
        try:
            e = tool.field_err(got[f], c[f], f)
        except AssertionError:                       # another NaN / Inf pattern
            e = np.inf
        if not e <= tool.bound(c['err'][f], f):
            bad.append((f, e))
    return bad


def _mutant(edits):
    """oracle/mixture.py with `edits` [(old, new, occurrences)] applied to its source: a stand-in module for tool.oracle_run."""
    from oracle import mixture as omx
    src = inspect.getsource(omx)
    for old, new, cnt in edits:
        assert src.count(old) == cnt, (old, src.count(old))
        src = src.replace(old, new)
    mod = types.ModuleType('oracle.mixture_mutant'); mod.__package__ = 'oracle'
    exec(compile(src, '<mixture mutant>', 'exec'), mod.__dict__)
    return mod


REFRESH_S = 'ttau[:, k], tnu[:, k] = _refresh(ttau[:, k], tnu[:, k], m_cav, v_cav, dlZ_, d2lZ_, d, a, upd)\n'
MUTANTS = {
    1: ('d instead of d / alpha in _refresh', [('d / a * (', 'd * (', 2)], ('m1', 3)),
    2: ('mom at power 1 in the filter', [('lZ[k], dlZ, d2lZ = mom6(lik_param, fmu, HPH, Wnmf, yall, k)', 'lZ[k], dlZ, d2lZ = mom(lik_param, fmu, HPH, Wnmf, 1.0, yall, k)', 1),
                                         ('lZ_k, dlZ, d2lZ = mom6(lik_param, fmu, HPH, Wnmf, yall, k)', 'lZ_k, dlZ, d2lZ = mom(lik_param, fmu, HPH, Wnmf, 1.0, yall, k)', 1)], ('m1', 3)),
    3: ("a clamp after the smoother's refresh", [(REFRESH_S, REFRESH_S.rstrip('\n') + '; ttau[:, k] = matlab_max0(ttau[:, k])\n', 2)], ('m1', 3)),
    4: ('R taken after the clamp', [('R[:, k] = 1.0 / ttau[:, k]\n                ttau[:, k] = matlab_max0(ttau[:, k])',
                                     'R[:, k] = 1.0 / matlab_max0(ttau[:, k])\n                ttau[:, k] = matlab_max0(ttau[:, k])', 1),
                                    ('R[:, k] = 1.0 / ttau[:, k]\n            ttau[:, k] = matlab_max0(ttau[:, k])',
                                     'R[:, k] = 1.0 / matlab_max0(ttau[:, k])\n            ttau[:, k] = matlab_max0(ttau[:, k])', 1)], ('m1', 1)),
    5: ('every site refreshed regardless of v_cav > 0', [('upd = v_cav > 0', 'upd = np.ones(v_cav.shape, bool)', 2)], MASKED_RUN[::2]),
    6: ("(ihgp) the smoother's lZ left out of nll", [('if itt > 1:\n                    lZ = lZ + lZ_k', 'if False:\n                    lZ = lZ + lZ_k', 1)], ('m1', 3)),
    7: ('(ihgp) R started at exp(lik) instead of 0', [('R = np.zeros((M, T)); ys =', 'R = np.exp(float(np.ravel(lik_param)[0])) * np.ones((M, T)); ys =', 1)], ('m1', 3)),
    8: ('(ihgp) m set to zero at the start of every sweep instead of once', [('        lZ = 0.0; maxDiffM = 0.0\n', '        lZ = 0.0; maxDiffM = 0.0; m = np.zeros(S)\n', 1)], ('m1', 3)),
}
# 4 runs on m1 with ONE sweep: with three, every R the gf filter writes at k < T - 1 is overwritten by the smoother's refresh of the sweep before the last
# (R = 1 / ttau of every site, :282), and on ihgp the block update sets R = Inf wherever the clamp acts, whichever came first
EQUIVALENT = {7: 8}       # R's start value is never read: every entry is written by the first filter pass before the look-up of the next step, the gain
                          # of its own step and the backward pass read it -> bit-equal in every field; what takes its place is the other statement about how
                          # a sweep starts (m, P set once before the sweeps: a sweep's filter starts from the smoothed mean of step 0)


def test_the_bounds_bite():
    """oracle/mixture.py made wrong in one place at a time (MUTANTS; on m1 with three sweeps, variant 4 with one, variant 5 on the run with a masked site): each variant exceeds the
    bound of at least one field in at least one family, or is bit-equal in every field of both families and replaced (EQUIVALENT).  The unmodified oracle and
    the unmodified source through the same machinery pass."""
    for family in ('gf', 'ihgp'):
        assert not _exceeds('m1', family, 3, _oracle_fields('m1', family, 3))
        assert not _exceeds('m1', family, 3, _oracle_fields('m1', family, 3, mixture=_mutant([])))
    assert not _exceeds(*MASKED_RUN, _oracle_fields(*MASKED_RUN))
    for num, (what, edits, (name, itts)) in MUTANTS.items():
        mod = _mutant(edits); bad = {}; same = True
        for family in (('ihgp',) if '(ihgp)' in what or num == 5 else ('gf', 'ihgp')):
            got = _oracle_fields(name, family, itts, mixture=mod); ref = _oracle_fields(name, family, itts)
            same = same and all(np.array_equal(got[f], ref[f], equal_nan=True) for f in ref)
            bad[family] = _exceeds(name, family, itts, got)
        if num in EQUIVALENT:
            assert same and not any(bad.values()), (num, what, bad)
        else:
            assert any(bad.values()), (num, what)
    assert set(EQUIVALENT.values()) <= set(MUTANTS) - set(EQUIVALENT)


# ---------------------------------------------------------------------------------------------
# GPU
@pytest.fixture(scope='module')
def _lib(nagp_lib):
    assert nagp_lib.nagp_device_count() >= 1
    return nagp_lib


_LINES = {}                                        # test id -> measured lines (the whole module's go to PROFILE)


@pytest.fixture(scope='module', autouse=True)
def _profile():
    yield
    if len(_LINES) == N_GPU_TESTS:                 # a run of the whole module
        try:
            with open(PROFILE, 'w') as fh:
                fh.write('# tests/test_mixture_fixture.py -m gpu on an MI355X: per run and field, the device error against tests/golden/mixture_multiprecision*.npz\n'
                         '# (err_oracle, bound); "plan:" lines are what the plan says it launches\n')
                for key in sorted(_LINES):
                    fh.write('\n'.join(_LINES[key]) + '\n')
        except OSError:                            # a read-only checkout
            pass


def _mom(sh):
    from nagp import Mom
    lik = {tool.LIK_NMF: 'likModulatorNMFPower', tool.LIK_SQRT: 'likModulatorPreCalcwn'}[int(sh['lik_kind'])]
    return Mom(lik, link=str(sh['link']), link_shift=float(sh['link_shift']), p_cubature=int(sh['p_cubature']), wn=sh['wn'], xn_unscaled=sh['xn_unscaled'])


def _problem(inp, family):
    blk, W, lik, A, Q, P = tool.stacked(inp, inp, family)
    assert np.array_equal(blk.offsets, inp['block_offsets']) and np.array_equal(blk.h_val, inp['h_val']) and np.array_equal(W, inp['Wnmf'])
    return (blk, W, lik, dict(A=inp['A'], Q=inp['Q'], Pinf=inp['Pinf']))


class _Tables:
    """ihgp_tables.build_tables replaced by the fixture's 200-point tables, served in the order the plan asks for them (test_ep_fixture._plan_run)."""

    def __init__(self, inps):
        self.inps, self.tabs, self.served, self.build = inps, [tool.flat_tables(i) for i in inps], [], ihgp_tables.build_tables

    def __call__(self, A_, Q_, offsets, h_val, *a, **kw):
        q = len(self.served); self.served.append(q)
        assert np.array_equal(A_, self.inps[q]['A']) and np.array_equal(Q_, self.inps[q]['Q'])
        return self.tabs[q]

    def __enter__(self):
        ihgp_tables.build_tables = self
        return self

    def __exit__(self, *a):
        ihgp_tables.build_tables = self.build


def _plan_run(names, family, itts, env, capfd, chunk=0, want_ps=True):
    """The cases `names` (one plan, one problem each) under the developer switches `env` -> (outputs per case, the plan's NAGP_STAMPS lines)."""
    from nagp import _lib as L
    from nagp.plan import Plan
    inps = [_case(n)[1][family] for n in names]; sh = inps[0]
    kind = L.KIND_GF_EP if family == 'gf' else L.KIND_IHGP
    want_ps = want_ps and family == 'gf'
    flags = L.FLAG_MIXTURE_RULE | (L.FLAG_WANT_PS if want_ps else 0)
    env = dict(env, NAGP_STAMPS='1')
    os.environ.update(env)
    try:
        with _Tables(inps if family == 'ihgp' else []) as tabs:
            capfd.readouterr()
            plan = Plan(kind, [_problem(inp, family) for inp in inps], sh['y'].size, mom=_mom(sh), ep_fraction=float(sh['ep_fraction']),
                        ep_damping=np.full(itts, float(sh['ep_damping'][0])), ep_itts=itts, flags=flags, chunk=chunk)
            plan.upload([inp['y'] for inp in inps]); plan.execute()
            outs = plan.download(want_PS=want_ps, want_MF=True); plan.close()
            stamps = capfd.readouterr().err
    finally:
        for k in env:
            os.environ.pop(k, None)
    assert family != 'ihgp' or len(tabs.served) == len(names)
    return outs, stamps


def _nll(o, family, itts):
    """The oracle's nll per sweep from the library's records (module docstring)."""
    if itts == 1:
        return np.array([o.nlZ[0]])
    last = -np.sum(o.lZ) if family == 'gf' else -o.lZ[-1]
    return np.array([o.nlZ[0]] + [o.nlZ[i + 1] for i in range(1, itts - 1)] + [last])


def _device_fields(o, family, name, itts):
    inp = _case(name)[1][family]; S = inp['A'].shape[0]; T = inp['y'].size
    d = dict(MF=o.MF, MS=o.MS, Eft=o.Eft, Varft=o.Varft, ttau=o.ttau, tnu=o.tnu, R=o.R, lZ=o.lZ, nll=_nll(o, family, itts), maxDiffM=o.maxDiffM, maxDiffP=o.maxDiffP)
    if family == 'gf' and o.PS is not None:
        d['PS'] = [o.PS[:, :, k] for k in range(T)]
    return tool.pack_fields(d, family, tool.ps_selection(S, T, [T // 3])[0], S)


def _check(name, family, itts, o, label, lines):
    """Every stored field of the run against its bound; the NaN / Inf patterns (inside field_err) and the counters."""
    c = _run(name, family, itts); got = _device_fields(o, family, name, itts); bad = []; cells = []
    for f in tool.FIELDS[family]:
        if f not in got:                           # PS of a plan that does not store the smoothed covariances
            continue
        try:
            e = tool.field_err(got[f], c[f], f)
        except AssertionError as ex:
            e = np.inf; bad.append((label, name, family, itts, f, str(ex)))
        cells.append('%s %.1e (%.1e, %.1e)' % (f, e, c['err'][f], tool.bound(c['err'][f], f)))
        if not e <= tool.bound(c['err'][f], f):
            bad.append((label, name, family, itts, f, e, tool.bound(c['err'][f], f)))
    want = int(c['clamped'] if family == 'ihgp' else c['clamped_adf'])
    lines.append('%-24s %-3s %-4s sweeps %d  %s  clamped %d (fixture %d), chol retries %d, not PD %d' % (label, name, family, itts, '  '.join(cells), o.counters[1], want, o.counters[0], o.counters[3]))
    if int(o.counters[1]) != want or o.counters[0] != 0 or o.counters[3] != 0:
        bad.append((label, name, family, itts, 'counters', list(o.counters), want))
    return bad


def _facts(stamps, family):
    """The words of the plan's NAGP_STAMPS lines that name the launch path, in one short string."""
    def g(pat):
        m = re.search(pat, stamps)
        return m.group(1) if m else '-'
    if family == 'ihgp':
        return 'src %s stride %s staged %s sparse %s roles %s tables %s seq %s ring %s' % (
            g(r'block-structured mom (\d)'), g(r'block stride (\d)'), g(r'staged form: (\d)'), g(r'sparse-point form: (\d)'), g(r'role-specialised waves (\d)'),
            g(r'table form of stage 1b (\d)'), g(r'sequential kernels in every sweep (\d)'), g(r'sparse-point form: \d \(LDS \d+ B, ring (\d+) steps'))
    return 'adf-sparse %s split %s lik %s mfma-sp %s roles %s refresh-sparse %s refresh-staged %s chunk %s pipelined %s' % (
        g(r'sparse-point ADF (\d)'), g(r'split blocks (\d)'), g(r'likelihood (\d)'), g(r'MFMA span passes at Sp (\d+)'), g(r'role-specialised waves: (\d)'),
        g(r'site refresh: sparse-point form (\d)'), g(r'staged square-root form (\d)'), g(r'smoother: chunk (\d+),'), g(r'pipelined (\d)'))


# variant -> (developer switches, chunk, PS asked for).  Every variant runs on every case; _expected_facts says what the plan's NAGP_STAMPS lines must name
# as launched, so a switch that does not reach a case is seen (and listed in DESIGN.md section 2) instead of passing for a second run of the default path.
IHGP_VARIANTS = {
    'default': ({}, 0, True),
    'tables': ({'NAGP_IH_TABLES': '1'}, 0, True),
    'no-roles': ({'NAGP_IH_ROLES': '0'}, 0, True),
    'general': ({'NAGP_NO_SPARSE': '1'}, 0, True),
    'no-src': ({'NAGP_NO_SRC': '1'}, 0, True),
    'sequential': ({'NAGP_IH_SEQ': '1', 'NAGP_NO_SPARSE': '1'}, 0, True),
    'ring-4': ({'NAGP_IH_KB': '4'}, 0, True),
    # a plan of several sources takes the block-structured cubature (mom_src) in the general kernel, so the switches of the role layout reach it only beside NAGP_NO_SRC
    'no-src+tables': ({'NAGP_NO_SRC': '1', 'NAGP_IH_TABLES': '1'}, 0, True),
    'no-src+no-roles': ({'NAGP_NO_SRC': '1', 'NAGP_IH_ROLES': '0'}, 0, True),
    'no-src+general': ({'NAGP_NO_SRC': '1', 'NAGP_NO_SPARSE': '1'}, 0, True),
    'no-src+sequential': ({'NAGP_NO_SRC': '1', 'NAGP_IH_SEQ': '1', 'NAGP_NO_SPARSE': '1'}, 0, True),
    'no-src+ring-4': ({'NAGP_NO_SRC': '1', 'NAGP_IH_KB': '4'}, 0, True),
}
GF_VARIANTS = {
    'default': ({}, 0, True),
    'no-roles': ({'NAGP_NO_GF_ROLES': '1'}, 0, True),
    'general': ({'NAGP_NO_SPARSE': '1'}, 0, True),
    'generic-refresh': ({'NAGP_NO_SPARSE_EP': '1'}, 0, True),
    'no-src': ({'NAGP_NO_SRC': '1'}, 0, True),
    'no-ps': ({}, 0, False),
    'no-ps+no-mfma': ({'NAGP_NO_MFMA': '1'}, 0, False),
    'chunks': ({}, 7, True),
    'serial': ({'NAGP_NO_PIPELINE': '1'}, 7, True),
    # the sparse-point and the staged site refresh do not take a block-structured Wnmf either: the switch of the refresh reaches a mixture plan only beside NAGP_NO_SRC
    'no-src+generic-refresh': ({'NAGP_NO_SRC': '1', 'NAGP_NO_SPARSE_EP': '1'}, 0, True),
    'no-src+no-roles': ({'NAGP_NO_SRC': '1', 'NAGP_NO_GF_ROLES': '1'}, 0, True),
    'no-src+general': ({'NAGP_NO_SRC': '1', 'NAGP_NO_SPARSE': '1'}, 0, True),
}
_NMF = ('m1', 'm1b')                               # plain NMF likelihood, three components, blocks of at most four states: the cases the sparse-point / role forms serve
_SP_GF = dict(m1=32, m1b=32, m2=64, m3=96, m4=48)  # Sp = 16 ceil(4 M / 16)... of the MFMA span passes (M = 8, 16, 21 sites; m4: 8 sites + 3 tail rows)


def _expected_facts(family, name, env, chunk):
    """What a mixture plan launches, by case and switches (the plan's own rules, nagp_api_plan.hpp, restated for these five shapes):
    ihgp -- several sources and blocks of <= 4 states: the general kernel with the block-structured cubature (mom_src), which no switch of the sparse-point /
            role / staged forms reaches; m4 (a six-state block: stride 8, no mom_src): the general kernel, and the sequential kernels under NAGP_IH_SEQ;
            beside NAGP_NO_SRC: m1, m1b the role layout (its table form, its ring, the flat sparse-point form), m2 the staged square-root sweep, m3 (nine
            components) the general kernel;
    gf   -- m1, m1b: the role-specialised sparse-point ADF sweep; m2, m3 (square-root amplitudes) and m4 (split blocks) the general one; the site refresh is
            the generic one unless NAGP_NO_SRC lets the sparse-point (m1, m1b) or the staged (m2) form in."""
    on = lambda k: k in env
    if family == 'ihgp':
        src = int(name != 'm4' and not on('NAGP_NO_SRC'))
        sparse = int(not src and name in _NMF and not on('NAGP_NO_SPARSE')); staged = int(not src and name == 'm2' and not on('NAGP_NO_SPARSE'))
        roles = int(sparse and env.get('NAGP_IH_ROLES') != '0'); tables = int(roles and on('NAGP_IH_TABLES'))
        seq = int(on('NAGP_IH_SEQ') and not src and not sparse and not staged)
        return 'src %d stride %d staged %d sparse %d roles %d tables %d seq %d ring %d' % (src, 8 if name == 'm4' else 4, staged, sparse, roles, tables, seq,
                                                                                          int(env['NAGP_IH_KB']) if roles and on('NAGP_IH_KB') else 16)
    sparse = int(name in _NMF and not on('NAGP_NO_SPARSE')); roles = int(sparse and not on('NAGP_NO_GF_ROLES'))
    ref_ok = on('NAGP_NO_SRC') and not on('NAGP_NO_SPARSE_EP') and not on('NAGP_NO_SPARSE')
    T = SHAPES[name][1]
    return 'adf-sparse %d split %d lik %d mfma-sp %d roles %d refresh-sparse %d refresh-staged %d chunk %d pipelined %d' % (
        sparse, int(name == 'm4'), 2 if name in ('m2', 'm3') else 1, 0 if on('NAGP_NO_MFMA') else _SP_GF[name], roles, int(ref_ok and name in _NMF),
        int(ref_ok and name == 'm2'), chunk or T, int(bool(chunk) and not on('NAGP_NO_PIPELINE')))


N_GPU_TESTS = len(IHGP_VARIANTS) + len(GF_VARIANTS) + 2 + 2


def _variant(family, variant, capfd):
    env, chunk, want_ps = (IHGP_VARIANTS if family == 'ihgp' else GF_VARIANTS)[variant]
    lines, bad = [], []
    for name in CASES:
        for itts in tool.SWEEPS:
            outs, stamps = _plan_run([name], family, itts, env, capfd, chunk=chunk, want_ps=want_ps)
            facts = _facts(stamps, family)
            lines.append('%-24s %-3s %-4s sweeps %d plan: %s' % (variant, name, family, itts, facts))
            assert facts == _expected_facts(family, name, env, chunk), (variant, name, facts, _expected_facts(family, name, env, chunk), stamps)
            bad += _check(name, family, itts, outs[0], variant, lines)
    _LINES['%s %s' % (family, variant)] = lines
    with capfd.disabled():
        print('\n' + '\n'.join(lines))
    assert not bad, bad


@pytest.mark.gpu
@pytest.mark.parametrize('variant', list(IHGP_VARIANTS))
def test_ihgp_mixture_meets_the_multiprecision_fixture(_lib, variant, capfd):
    """KIND_IHGP with NAGP_FLAG_MIXTURE_RULE on the fixture's tables, every case at one and three sweeps, every field within BOUND, on each launch path."""
    _variant('ihgp', variant, capfd)


@pytest.mark.gpu
@pytest.mark.parametrize('variant', list(GF_VARIANTS))
def test_gf_mixture_meets_the_multiprecision_fixture(_lib, variant, capfd):
    """KIND_GF_EP with NAGP_FLAG_MIXTURE_RULE, every case at one and three sweeps, every field within BOUND, on each launch path."""
    _variant('gf', variant, capfd)


@pytest.mark.gpu
@pytest.mark.parametrize('family', ['gf', 'ihgp'])
def test_a_batch_of_two_segments_meets_the_fixture(_lib, family, capfd):
    """m1 and m1b (one shape and one mom, another model, other tables, another signal) in one batched plan, in both orders: every field of each segment
    within ITS case's BOUND, and each segment bit-equal to its plan of one segment."""
    lines, bad = [], []
    for itts in tool.SWEEPS:
        one = {n: _plan_run([n], family, itts, {}, capfd)[0][0] for n in ('m1', 'm1b')}
        for order in (['m1', 'm1b'], ['m1b', 'm1']):
            outs, _ = _plan_run(order, family, itts, {}, capfd)
            for q, n in enumerate(order):
                bad += _check(n, family, itts, outs[q], 'batch %s[%d]' % ('+'.join(order), q), lines)
                for f in ('Eft', 'Varft', 'MS', 'ttau', 'tnu', 'R', 'nlZ', 'maxDiffM'):
                    assert np.array_equal(getattr(outs[q], f), getattr(one[n], f), equal_nan=True), (order, q, f)
    _LINES['batch %s' % family] = lines
    with capfd.disabled():
        print('\n' + '\n'.join(lines))
    assert not bad, bad


@pytest.mark.gpu
@pytest.mark.parametrize('family', ['gf', 'ihgp'])
def test_python_entry_points_meet_the_fixture(_lib, family, capfd):
    """nagp.gf_ep_mods_nmf_mixture / nagp.ihgp_ep_mods_nmf_mixture on m1's recipe (the cell w, the stored signal): bit-equal to the Plan run of the same inputs
    where the A and Q the entry point builds agree bitwise with the stored ones, within BOUND otherwise."""
    import nagp
    from nagp.api import SSHandle
    sh, fams = _case('m1'); inp = fams[family]; T = inp['y'].size; t = np.arange(1, T + 1.0)
    k1 = [str(k) for k in sh['kernel1']]; k2 = [str(k) for k in sh['kernel2']]
    A, Q = tool.stacked(inp, inp, family)[3:5]
    same = np.array_equal(A, inp['A']) and np.array_equal(Q, inp['Q'])
    fn = nagp.gf_ep_mods_nmf_mixture if family == 'gf' else nagp.ihgp_ep_mods_nmf_mixture
    lines, bad = [], []
    for itts in tool.SWEEPS:
        with _Tables([dict(inp, A=A, Q=Q)] if family == 'ihgp' else []):
            r = fn(tool.source_cell(inp), t, inp['y'], SSHandle(), _mom(sh), t, k1, k2, len(k1), float(sh['ep_fraction']), float(sh['ep_damping'][0]), itts, nargout=6)
        ref = _plan_run(['m1'], family, itts, {}, capfd)[0][0]
        c = _run('m1', family, itts)
        got = dict(Eft=r[0], Varft=r[1], ttau=r[5]['ttau'], tnu=r[5]['tnu'], R=r[5]['R'], MS=r[5]['MS'], maxDiffM=r[5]['maxDiffM'], maxDiffP=r[5]['maxDiffP']); cells = []
        for f, v in got.items():
            e = tool.field_err(v, c[f], f)
            cells.append('%s %.1e (%.1e, %.1e)' % (f, e, c['err'][f], tool.bound(c['err'][f], f)))
            if same:
                assert np.array_equal(v, getattr(ref, f), equal_nan=True), (family, itts, f)
            if not e <= tool.bound(c['err'][f], f):
                bad.append((family, itts, f, e))
        lines.append('%-24s %-3s %-4s sweeps %d  %s%s' % ('entry point', 'm1', family, itts, '  '.join(cells), '  [A and Q as stored: bit-equal to the plan]' if same else ''))
    _LINES['entry %s' % family] = lines
    with capfd.disabled():
        print('\n' + '\n'.join(lines))
    assert not bad, bad
