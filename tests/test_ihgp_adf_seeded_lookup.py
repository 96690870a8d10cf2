"""The seeded look-up of the three-barrier schedule of ihgp_adf8_kernel (direct form, at most six components).  The window of the
table look-up is seeded from ttau beside the division R = 1 / ttau (csrc/nagp_lookup.hpp: lookup_mid_ttau); behind R only the branch
beyond the grid, the pick among three and the selects are left.  The arithmetic of a step is unchanged; the table form
(NAGP_IH_TABLES=1) keeps the look-up from R and is the cross-check inside the same build.  (A second change, the modulators' chain
replicated on the lanes of the link chain, was measured slower and is not in the kernel; the cases chosen for it -- modulator counts
1, 2, 5, 6 -- stay as cases of the look-up on wave 1.)

Cases through the oracle: the five of tests/test_ihgp_adf_straight_head.py (chosen there for R = Inf, R < 1e-2 and the branch beyond the
grid), and for wave 1's lanes N = 1 (D = 40, among the five), N = 2 and N = 5 at D = 8 (CD nd = 2 nd and 5 nd lanes: no multiple of
anything convenient), N = 6 at D = 32 with two sweeps (the second sweep's launch continues from the filtered mean and R of step T - 2).
Every case asserts (NAGP_STAMPS=1) that the plan chose the role kernel and is compared with the NumPy oracle and with the table form at
the tolerances tests/test_gpu_parity.py applies to these sweeps, or bit for bit with another run.

The role kernel runs the forward pass of a later sweep as the fixed-site recursion plus ONE continued launch (k_start = T - 1); there is
no uninterrupted launch of that sweep to compare with.  The continued launch is therefore pinned from both sides: its prologue takes
the look-up from R (lookup_mid), every step inside a launch from ttau, and tests/test_ihgp_lookup_seeded_host.py shows the two agree for
every ttau; here the two-sweep results are bit-equal at ring depths 4 / 8 / 16 (the continued step sits in another slot at each), and
the continued step leaves R = 1 / ttau exactly as every step of an uninterrupted one-sweep launch (k_start = 0) does."""
import numpy as np
import pytest

import nagp
from nagp import harness, Mom, Plan, SSHandle, _lib as L
from oracle import ihgp as oih, lik as olik

from test_ihgp_direct_moments import TOL_MEAN, TOL_LOGZ, rel, relz
from test_ihgp_adf_streamed_ring import FIELDS, _segments, _run_plan
from test_ihgp_adf_straight_head import CASES as HEAD_CASES, _oracle as _head_oracle, _run as _head_run

pytestmark = pytest.mark.gpu

P_OF_N = {1: 9, 2: 9, 5: 7, 6: 7}      # a cubature rule the role layout serves in that dimension

_ORACLE = {}


def _compare(tag, res, ref):
    figs = {}
    for name, a, b in (('direct vs oracle', res['direct'], ref), ('tables vs oracle', res['tables'], ref), ('direct vs tables', res['direct'], res['tables'])):
        figs[name] = (rel(a[0], b[0]), rel(a[1], b[1]), relz(a[5]['nlZ'], b[5]['nlZ']))
        print('%s %s: Eft %.2e Varft %.2e nlZ %.2e' % ((tag, name) + figs[name]))
    for name, (fe, fv, fz) in figs.items():
        assert fe < TOL_MEAN and fv < TOL_MEAN and fz < TOL_LOGZ, (tag, name, fe, fv, fz)


@pytest.mark.parametrize('case', HEAD_CASES, ids=lambda c: 'D%d-N%d-T%d-y%g-sweeps%d' % (c[0], c[1], c[2], c[4], c[5]))
def test_seeded_lookup_against_the_oracle_and_the_table_form(case, nagp_lib, monkeypatch, capfd):
    D, N, T, seed, scale, itts = case
    ref = _head_oracle(*case[:5], itts)
    assert np.all(np.isfinite(ref[0])) and np.all(np.isfinite(ref[1])) and np.all(np.isfinite(ref[5]['nlZ']))
    res = {form: _head_run(D, N, T, seed, scale, itts, form, monkeypatch, capfd) for form in ('direct', 'tables')}
    _compare('D=%d N=%d T=%d y x %g sweeps=%d' % (D, N, T, scale, itts), res, ref)


def _run(D, N, T, seed, itts, form, monkeypatch, capfd):
    pr = harness.nmf_problem(D, N, T, seed, 'constraints'); t = np.arange(1, T + 1.0)
    d = np.array([0.5, 0.4])[:itts]
    monkeypatch.setenv('NAGP_STAMPS', '1')
    monkeypatch.delenv('NAGP_IH_TABLES', raising=False)
    if form == 'tables': monkeypatch.setenv('NAGP_IH_TABLES', '1')
    capfd.readouterr()
    res = nagp.ihgp_ep_modulator_nmf(pr['w'], t, pr['y'], SSHandle(), Mom('likModulatorNMFPower', p_cubature=P_OF_N[N]), t,
                                     'matern32', 'matern52', 1, D, N, 0.5, d, itts, nargout=6)
    assert 'role-specialised waves 1' in capfd.readouterr().err, (form, 'the plan did not choose ihgp_adf8_kernel')
    monkeypatch.delenv('NAGP_IH_TABLES', raising=False); monkeypatch.delenv('NAGP_STAMPS', raising=False)
    if (D, N, T, seed, itts) not in _ORACLE:
        _ORACLE[(D, N, T, seed, itts)] = oih.ihgp_ep_modulator_nmf(pr['w'], t, pr['y'], None, olik.Mom(olik.LIK_POWER_NMF, p=P_OF_N[N]), t,
                                                                   'matern32', 'matern52', 1, D, N, 0.5, d, itts)
    return res


MODULATOR_COUNTS = [(8, 2, 120, 7301, 1), (8, 5, 120, 7302, 1), (32, 6, 120, 7002, 2)]


@pytest.mark.parametrize('case', MODULATOR_COUNTS, ids=lambda c: 'D%d-N%d-T%d-sweeps%d' % (c[0], c[1], c[2], c[4]))
def test_modulator_counts_against_the_oracle_and_the_table_form(case, nagp_lib, monkeypatch, capfd):
    D, N, T, seed, itts = case
    res = {form: _run(D, N, T, seed, itts, form, monkeypatch, capfd) for form in ('direct', 'tables')}
    ref = _ORACLE[(D, N, T, seed, itts)]
    assert np.all(np.isfinite(ref[0])) and np.all(np.isfinite(ref[1])) and np.all(np.isfinite(ref[5]['nlZ']))
    _compare('D=%d N=%d T=%d sweeps=%d' % (D, N, T, itts), res, ref)


def _depths(probs, ys, T, monkeypatch, capfd):
    monkeypatch.setenv('NAGP_STAMPS', '1')
    monkeypatch.delenv('NAGP_IH_TABLES', raising=False)
    outs = {}
    for kb in (4, 8, 16):
        monkeypatch.setenv('NAGP_IH_KB', str(kb))
        out, depth = _run_plan(probs, ys, T, 7, capfd)
        assert depth == kb, (kb, depth)
        outs[kb] = out[0]
    monkeypatch.delenv('NAGP_IH_KB', raising=False)
    return outs


def test_seeded_lookup_gives_the_same_bits_at_every_ring_depth(nagp_lib, monkeypatch, capfd):
    """D = 32, N = 6, T = 203, two sweeps, NAGP_IH_KB = 4, 8, 16: the site update reads ttau / tnu of a slot that it writes later in the
    same step, behind the window's reads -- a slot not yet filled, or already overwritten, shows at one depth and not at another."""
    D, N, T = 32, 6, 203
    probs, ys = _segments(D, N, T, 7400, 1)
    outs = _depths(probs, ys, T, monkeypatch, capfd)
    assert np.all(np.isfinite(outs[16].Eft)) and np.all(np.isfinite(outs[16].nlZ))
    for kb in (4, 8):
        for f in FIELDS:
            assert np.array_equal(getattr(outs[kb], f), getattr(outs[16], f), equal_nan=True), (kb, f)


def test_seeded_lookup_in_a_batch_equals_the_segments_one_at_a_time(nagp_lib, monkeypatch, capfd):
    """A plan of three segments (three workgroups of one launch) gives, bit for bit, what three plans of one segment give."""
    D, N, T = 32, 6, 50
    probs, ys = _segments(D, N, T, 7500, 3)
    monkeypatch.setenv('NAGP_STAMPS', '1')
    monkeypatch.delenv('NAGP_IH_TABLES', raising=False)
    batch, _ = _run_plan(probs, ys, T, 7, capfd)
    for q in range(3):
        one = _run_plan(probs[q:q + 1], ys[q:q + 1], T, 7, capfd)[0][0]
        for f in FIELDS:
            assert np.array_equal(getattr(batch[q], f), getattr(one, f), equal_nan=True), (q, f)
        assert np.all(np.isfinite(one.Eft)) and np.all(np.isfinite(one.nlZ))
    assert not np.array_equal(batch[0].Eft, batch[1].Eft)      # the segments are different problems


def _plan_run(probs, ys, T, itts, capfd, expect_role=True):
    capfd.readouterr()
    plan = Plan(L.KIND_IHGP, probs, T, mom=Mom('likModulatorNMFPower', p_cubature=7), ep_fraction=0.5, ep_damping=np.array([0.5, 0.4])[:itts], ep_itts=itts)
    err = capfd.readouterr().err
    if expect_role: assert 'role-specialised waves 1' in err, 'the plan did not choose ihgp_adf8_kernel'
    plan.upload(ys); plan.execute(); out = plan.download()[0]; plan.close()
    return out, err


def test_continued_launch_of_the_second_sweep_at_a_ring_slot_of_its_own(nagp_lib, monkeypatch, capfd):
    """D = 32, N = 6, T = 37, two sweeps: the second sweep's launch has k_start = 36 -- slot 4 of a ring of 16 and of 8, slot 0 of a ring of
    4 -- and takes its first look-up from R of step 35 in memory (the prologue's head), the path the loop no longer takes.  Bit-equal at
    the three depths.
    This stands where a comparison of a continued sweep with an uninterrupted one was asked for: the role kernel has no uninterrupted
    launch of a later sweep (later sweeps launch only k = T - 1), so there is nothing to compare bit for bit.  The continued launch runs
    the prologue's head and one site update whose seeded index is never consumed -- it does not exercise the seeded look-up; the check of
    R against 1 / ttau below only pins the division the seed runs beside.  The prologue path is covered at tolerance by the two-sweep
    N = 6 case against the table form."""
    D, N, T = 32, 6, 37
    probs, ys = _segments(D, N, T, 7600, 1)
    outs = _depths(probs, ys, T, monkeypatch, capfd)
    assert np.all(np.isfinite(outs[16].Eft)) and np.all(np.isfinite(outs[16].nlZ))
    for kb in (4, 8):
        for f in FIELDS:
            assert np.array_equal(getattr(outs[kb], f), getattr(outs[16], f), equal_nan=True), (kb, f)
    # one sweep, uninterrupted (k_start = 0): its R of every step is 1 / ttau of the same step, the division of the site update, and the
    # continued launch of the two-sweep plan leaves R and ttau of its own step in the same relation
    monkeypatch.setenv('NAGP_STAMPS', '1')
    one, _ = _plan_run(probs, ys, T, 1, capfd)
    monkeypatch.delenv('NAGP_STAMPS', raising=False)
    for o in (one, outs[16]):
        with np.errstate(divide='ignore'):
            assert np.array_equal(o.R[:, T - 1], 1.0 / o.ttau[:, T - 1])
    with np.errstate(divide='ignore'):
        assert np.array_equal(one.R, 1.0 / one.ttau)


def test_stamped_and_plain_instantiation_give_the_same_bits(nagp_lib, monkeypatch, capfd):
    """D = 32, N = 6, T = 120 (seed 7700), two sweeps: with NAGP_STAMPS the plan takes ihgp_adf8_kernel<6, false, true>, without it
    <6, false, false> -- the kernel bench.py and every caller outside the tests run.  Every output is bit-equal."""
    D, N, T = 32, 6, 120
    probs, ys = _segments(D, N, T, 7700, 1)
    monkeypatch.delenv('NAGP_IH_TABLES', raising=False); monkeypatch.delenv('NAGP_IH_KB', raising=False)
    monkeypatch.setenv('NAGP_STAMPS', '1')
    stamped, _ = _plan_run(probs, ys, T, 2, capfd)
    monkeypatch.delenv('NAGP_STAMPS', raising=False)
    plain, err = _plan_run(probs, ys, T, 2, capfd, expect_role=False)
    assert '[nagp' not in err      # no diagnostics: the plain instantiation
    assert np.all(np.isfinite(plain.Eft)) and np.all(np.isfinite(plain.nlZ))
    for f in FIELDS:
        assert np.array_equal(getattr(stamped, f), getattr(plain, f), equal_nan=True), f
    assert np.array_equal(stamped.counters, plain.counters)


def test_clamped_site_counter_equals_the_table_forms(nagp_lib, monkeypatch, capfd):
    """D = 8, N = 3, T = 300 (seed 7001), y x 30, one sweep -- the case of tests/test_ihgp_adf_straight_head.py in which nearly every
    site is clamped (R = Inf at 3 289 of 3 300 site-steps of the oracle), modulators among them.  The counter of clamped sites of the
    direct form equals the table form's.  It also equals the number of
    zeros among the ttau the sweep returns (a clamped site stores ttau = 0)."""
    D, N, T = 8, 3, 300
    probs, ys = _segments(D, N, T, 7001, 1)
    ys = [y * 30.0 for y in ys]
    got = {}
    for form in ('direct', 'tables'):
        monkeypatch.setenv('NAGP_STAMPS', '1')
        monkeypatch.delenv('NAGP_IH_TABLES', raising=False)
        if form == 'tables': monkeypatch.setenv('NAGP_IH_TABLES', '1')
        capfd.readouterr()
        plan = Plan(L.KIND_IHGP, probs, T, mom=Mom('likModulatorNMFPower', p_cubature=9), ep_fraction=0.5, ep_damping=np.array([0.5]), ep_itts=1)
        assert 'role-specialised waves 1' in capfd.readouterr().err
        plan.upload(ys); plan.execute(); got[form] = plan.download()[0]; plan.close()
    monkeypatch.delenv('NAGP_IH_TABLES', raising=False); monkeypatch.delenv('NAGP_STAMPS', raising=False)
    cd, ct = int(got['direct'].counters[1]), int(got['tables'].counters[1])
    nmod = int(np.sum(got['direct'].ttau[D:, :] == 0.0))
    print('clamped sites: direct %d, tables %d; zeros of ttau %d (modulators %d)' % (cd, ct, int(np.sum(got['direct'].ttau == 0.0)), nmod))
    assert cd == ct and cd > 1000 and nmod > 0
    assert cd == int(np.sum(got['direct'].ttau == 0.0))
