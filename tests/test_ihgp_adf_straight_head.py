"""The serial tail and head of the three-barrier schedule of ihgp_adf8_kernel (direct form, at most six components): the straight-line
table look-up (csrc/nagp_lookup.hpp; one branch, for finite R beyond the grid), H PP H' selected from three entries read beside the grid
words, the outputs' sums in one batch of LDS reads, ttau / tnu / the W row read ahead of B5, the gain of a clamped site by a select, and the
stamps as instantiations of their own (NAGP_STAMPS).  The arithmetic of a step is unchanged; the table form (NAGP_IH_TABLES=1, ihgp_adf8b_kernel) keeps the
earlier code and is the cross-check inside the same build.

The cases through the oracle are chosen for what the look-up meets (counted on the oracle's R, site-steps of D + N sites x T steps):

  D, N, T, seed       y scale  sweeps   R = Inf   R < 1e-2   finite R > 1e4   of
  8, 3, 300, 7001     x 1      1              8        584                0   3 300
  8, 3, 300, 7001     x 30     1          3 289          2                0   3 300
  8, 3, 300, 7001     x 30     2          2 238         43                0   3 300
  32, 6, 120, 7002    x 1      1             71          0                0   4 560
  40, 1, 120, 7003    x 1      1              5          0                1   4 920      (the branch beyond the grid, once)

Every case runs through the public interface, asserts (NAGP_STAMPS=1) that the plan chose the role kernel, and is compared with the NumPy
oracle and with the table form at the tolerances tests/test_gpu_parity.py applies to these sweeps, or bit for bit with another run."""
import numpy as np
import pytest

import nagp
from nagp import harness, Mom, Plan, SSHandle, _lib as L
from oracle import ihgp as oih, lik as olik

from test_ihgp_direct_moments import P_OF_CD, TOL_MEAN, TOL_LOGZ, rel, relz
from test_ihgp_adf_streamed_ring import FIELDS, _segments, _run_plan

pytestmark = pytest.mark.gpu

_ORACLE = {}


def _problem(D, N, T, seed, scale):
    pr = harness.nmf_problem(D, N, T, seed, 'constraints')
    return pr, pr['y'] * scale, np.arange(1, T + 1.0)


def _oracle(D, N, T, seed, scale, itts):
    """The NumPy oracle of a case, computed once."""
    key = (D, N, T, seed, scale, itts)
    if key not in _ORACLE:
        pr, y, t = _problem(D, N, T, seed, scale)
        d = np.array([0.5, 0.4])[:itts]
        _ORACLE[key] = oih.ihgp_ep_modulator_nmf(pr['w'], t, y, None, olik.Mom(olik.LIK_POWER_NMF, p=P_OF_CD[N]), t, 'matern32', 'matern52',
                                                 1, D, N, 0.5, d, itts)
    return _ORACLE[key]


def _run(D, N, T, seed, scale, itts, form, monkeypatch, capfd):
    pr, y, t = _problem(D, N, T, seed, scale)
    d = np.array([0.5, 0.4])[:itts]
    monkeypatch.setenv('NAGP_STAMPS', '1')
    monkeypatch.delenv('NAGP_IH_TABLES', raising=False)
    if form == 'tables': monkeypatch.setenv('NAGP_IH_TABLES', '1')
    capfd.readouterr()
    res = nagp.ihgp_ep_modulator_nmf(pr['w'], t, y, SSHandle(), Mom('likModulatorNMFPower', p_cubature=P_OF_CD[N]), t,
                                     'matern32', 'matern52', 1, D, N, 0.5, d, itts, nargout=6)
    assert 'role-specialised waves 1' in capfd.readouterr().err, (form, 'the plan did not choose ihgp_adf8_kernel')
    monkeypatch.delenv('NAGP_IH_TABLES', raising=False); monkeypatch.delenv('NAGP_STAMPS', raising=False)
    return res


CASES = [(8, 3, 300, 7001, 1.0, 1), (8, 3, 300, 7001, 30.0, 1), (8, 3, 300, 7001, 30.0, 2), (32, 6, 120, 7002, 1.0, 1), (40, 1, 120, 7003, 1.0, 1)]


@pytest.mark.parametrize('case', CASES, ids=lambda c: 'D%d-N%d-T%d-y%g-sweeps%d' % (c[0], c[1], c[2], c[4], c[5]))
def test_straight_head_against_the_oracle_and_the_table_form(case, nagp_lib, monkeypatch, capfd):
    D, N, T, seed, scale, itts = case
    ref = _oracle(*case[:5], itts)
    assert np.all(np.isfinite(ref[0])) and np.all(np.isfinite(ref[1])) and np.all(np.isfinite(ref[5]['nlZ']))
    res = {form: _run(D, N, T, seed, scale, itts, form, monkeypatch, capfd) for form in ('direct', 'tables')}
    figs = {}
    for name, a, b in (('direct vs oracle', res['direct'], ref), ('tables vs oracle', res['tables'], ref), ('direct vs tables', res['direct'], res['tables'])):
        figs[name] = (rel(a[0], b[0]), rel(a[1], b[1]), relz(a[5]['nlZ'], b[5]['nlZ']))
        print('D=%d N=%d T=%d y x %g sweeps=%d %s: Eft %.2e Varft %.2e nlZ %.2e' % ((D, N, T, scale, itts, name) + figs[name]))
    for name, (fe, fv, fz) in figs.items():
        assert fe < TOL_MEAN and fv < TOL_MEAN and fz < TOL_LOGZ, (name, fe, fv, fz)


def test_straight_head_gives_the_same_bits_at_every_ring_depth(nagp_lib, monkeypatch, capfd):
    """D = 32, N = 6, T = 203, two sweeps, NAGP_IH_KB = 4, 8, 16: ttau and tnu are now read ahead of B5 -- a slot not yet filled, or already
    overwritten, at that point shows at one depth and not at another."""
    D, N, T = 32, 6, 203
    probs, ys = _segments(D, N, T, 7100, 1)
    monkeypatch.setenv('NAGP_STAMPS', '1')
    monkeypatch.delenv('NAGP_IH_TABLES', raising=False)
    outs = {}
    for kb in (4, 8, 16):
        monkeypatch.setenv('NAGP_IH_KB', str(kb))
        out, depth = _run_plan(probs, ys, T, 7, capfd)
        assert depth == kb, (kb, depth)
        outs[kb] = out[0]
    monkeypatch.delenv('NAGP_IH_KB', raising=False)
    assert np.all(np.isfinite(outs[16].Eft)) and np.all(np.isfinite(outs[16].nlZ))
    for kb in (4, 8):
        for f in FIELDS:
            assert np.array_equal(getattr(outs[kb], f), getattr(outs[16], f), equal_nan=True), (kb, f)


def test_straight_head_in_a_batch_equals_the_segments_one_at_a_time(nagp_lib, monkeypatch, capfd):
    """A plan of three segments (three workgroups of one launch) gives, bit for bit, what three plans of one segment give."""
    D, N, T = 32, 6, 50
    probs, ys = _segments(D, N, T, 7200, 3)
    monkeypatch.setenv('NAGP_STAMPS', '1')
    monkeypatch.delenv('NAGP_IH_TABLES', raising=False)
    batch, _ = _run_plan(probs, ys, T, 7, capfd)
    for q in range(3):
        one = _run_plan(probs[q:q + 1], ys[q:q + 1], T, 7, capfd)[0][0]
        for f in FIELDS:
            assert np.array_equal(getattr(batch[q], f), getattr(one, f), equal_nan=True), (q, f)
        assert np.all(np.isfinite(one.Eft)) and np.all(np.isfinite(one.nlZ))
    assert not np.array_equal(batch[0].Eft, batch[1].Eft)      # the segments are different problems


def test_stamped_and_plain_instantiation_give_the_same_bits(nagp_lib, monkeypatch, capfd):
    """D = 32, N = 6, T = 120 (seed 7002): with NAGP_STAMPS the plan takes ihgp_adf8_kernel<6, false, true>, without it <6, false, false> --
    the kernel bench.py and every caller outside the tests run.  Every output is bit-equal."""
    D, N, T = 32, 6, 120
    probs, ys = _segments(D, N, T, 7002, 1)
    monkeypatch.delenv('NAGP_IH_TABLES', raising=False); monkeypatch.delenv('NAGP_IH_KB', raising=False)
    monkeypatch.setenv('NAGP_STAMPS', '1')
    stamped = _run_plan(probs, ys, T, 7, capfd)[0][0]
    monkeypatch.delenv('NAGP_STAMPS', raising=False)
    capfd.readouterr()
    plan = Plan(L.KIND_IHGP, probs, T, mom=Mom('likModulatorNMFPower', p_cubature=7), ep_fraction=0.5, ep_damping=np.array([0.5, 0.4]), ep_itts=2)
    assert '[nagp' not in capfd.readouterr().err      # no diagnostics: the plain instantiation
    plan.upload(ys); plan.execute(); plain = plan.download()[0]; plan.close()
    assert np.all(np.isfinite(plain.Eft)) and np.all(np.isfinite(plain.nlZ))
    for f in FIELDS:
        assert np.array_equal(getattr(stamped, f), getattr(plain, f), equal_nan=True), f
