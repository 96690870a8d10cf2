"""The three-barrier schedule of the role-specialised IHGP ADF sweep (ihgp_adf8_kernel, direct form, at most six components):
Q / 2Q / v of a step on serial wave 0 (msr_qv_serial: pairs of lanes, 2 (N (N + 1) / 2 + N) lanes of the wave), the link tables on
wave 1, both straight behind the head of the step and without barrier B1; the link-table words of the reduction read ahead of B5
(msr_reduce_tab / msr_reduce_bins).  The table form (NAGP_IH_TABLES=1) and seven components keep the schedule with B1 (ihgp_adf8b_kernel): the table form
is the cross-check inside the same build.

Every case runs through the public interface, asserts (NAGP_STAMPS=1) that the plan chose the role kernel, and is compared with the
NumPy oracle and with the table form at the tolerances tests/test_gpu_parity.py applies to these sweeps."""
import numpy as np
import pytest

import nagp
from nagp import harness, Mom, Plan, SSHandle, _lib as L
from nagp import ss as pss
from oracle import ihgp as oih, lik as olik

from test_gpu_parity import TOL_MEAN, TOL_LOGZ, rel, relz
from test_ihgp_direct_moments import _both_forms

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('D', [8, 32, 40])
@pytest.mark.parametrize('N', [1, 3, 6])
def test_three_barrier_schedule_against_the_oracle_and_the_table_form(N, D, nagp_lib, monkeypatch, capfd):
    """D in {8, 32, 40}: 4, 8 and 16 terms per partial sum (msp_qterms), with operands beyond the sub-bands at 8 and 40 (discarded) and
    none at 32; N = 1 uses 4 lanes of wave 0, N = 3 uses 18, N = 6 uses 54.  T = 496, one ADF sweep."""
    _both_forms(D, N, 496, 1, 7200 + 10 * D + N, monkeypatch, capfd)


def test_seven_components_keep_the_schedule_with_b1(nagp_lib, monkeypatch, capfd):
    """N = 7: the 70 lanes the pairs would need do not fit wave 0; Q / 2Q / v stay on the workers behind B1."""
    _both_forms(8, 7, 496, 1, 7301, monkeypatch, capfd)


@pytest.mark.parametrize('T', [503, 17])
def test_three_barrier_schedule_at_ring_boundaries(T, nagp_lib, monkeypatch, capfd):
    """T = 503: a partial last I/O ring.  T = 17: with the ring of 16 steps the second ring holds one step -- the Q / 2Q / v and link
    tables that step uses were formed ahead of the flush of the first ring."""
    _both_forms(32, 6, T, 1, 7400 + T, monkeypatch, capfd)


def test_three_barrier_schedule_with_a_launch_for_the_last_step_only(nagp_lib, monkeypatch, capfd):
    """Two EP sweeps: the second sweep's filter pass launches the kernel with k_start = T - 1: the prologue's head, Q / 2Q / v and link
    tables, one trip of the loop, no head behind it."""
    _both_forms(8, 3, 500, 2, 7501, monkeypatch, capfd)


@pytest.mark.parametrize('T,itts', [(503, 1), (500, 2)])
def test_seven_components_with_a_partial_last_ring_and_a_launch_for_the_last_step_only(T, itts, nagp_lib, monkeypatch, capfd):
    """ihgp_adf8b_kernel<7, false> and <7, true> (the block ring): T = 503, a partial last ring; two EP sweeps, the second sweep's filter
    pass launches the kernel with k_start = T - 1.  (A last ring of one step at N = 7: tests/test_ihgp_adf_streamed_ring.py, T = 33.)"""
    _both_forms(8, 7, T, itts, 7700 + T, monkeypatch, capfd)


@pytest.mark.parametrize('T,itts', [(17, 1), (503, 1), (500, 2)])
def test_four_wave_kernel_at_ring_boundaries_and_with_a_launch_for_the_last_step_only(T, itts, nagp_lib, monkeypatch, capfd):
    """ihgp_adf_kernel (NAGP_IH_ROLES=0; the head, the site update and the block ring it shares with ihgp_adf8b_kernel and
    ihgp_adf8sq_kernel), D = 8, N = 3: a second ring of one step, a partial last ring, the launch with k_start = T - 1, against the NumPy
    oracle at the tolerances tests/test_gpu_parity.py applies to these sweeps."""
    D, N, p = 8, 3, 9
    pr = harness.nmf_problem(D, N, T, 7800 + T, 'constraints'); t = np.arange(1, T + 1.0)
    d = np.array([0.5, 0.4])[:itts]
    monkeypatch.setenv('NAGP_STAMPS', '1'); monkeypatch.setenv('NAGP_IH_ROLES', '0')
    capfd.readouterr()
    r = nagp.ihgp_ep_modulator_nmf(pr['w'], t, pr['y'], SSHandle(), Mom('likModulatorNMFPower', p_cubature=p), t, 'matern32', 'matern52', 1, D, N, 0.5, d, itts,
                                   nargout=6)
    err = capfd.readouterr().err
    assert 'ihgp ADF sweep in the sparse-point form: 1' in err and 'role-specialised waves 0' in err, 'the plan did not choose ihgp_adf_kernel'
    monkeypatch.delenv('NAGP_STAMPS', raising=False); monkeypatch.delenv('NAGP_IH_ROLES', raising=False)
    ref = oih.ihgp_ep_modulator_nmf(pr['w'], t, pr['y'], None, olik.Mom(olik.LIK_POWER_NMF, p=p), t, 'matern32', 'matern52', 1, D, N, 0.5, d, itts)
    fe, fv, fz = rel(r[0], ref[0]), rel(r[1], ref[1]), relz(r[5]['nlZ'], ref[5]['nlZ'])
    print('four-wave kernel D=%d N=%d T=%d sweeps=%d vs oracle: Eft %.2e Varft %.2e nlZ %.2e' % (D, N, T, itts, fe, fv, fz))
    assert fe < TOL_MEAN and fv < TOL_MEAN and fz < TOL_LOGZ, (fe, fv, fz)


def test_three_barrier_schedule_in_a_batch_equals_the_segments_one_at_a_time(nagp_lib, monkeypatch, capfd):
    """A plan of three segments (three workgroups of one launch) gives, bit for bit, what three plans of one segment give."""
    D, N, T = 32, 6, 200
    probs, ys = [], []
    for q in range(3):
        pr = harness.nmf_problem(D, N, T, 7600 + q, 'constraints')
        blk = pss.balance_blocks(pss.ss_blocks_nmf(pr['param1'], pr['param2'], 'matern32', 'matern52'))
        probs.append((blk, pr['W'], np.log(pr['w_lik']))); ys.append(pr['y'])
    kw = dict(mom=Mom('likModulatorNMFPower', p_cubature=7), ep_fraction=0.5, ep_damping=np.array([0.5, 0.4]), ep_itts=2)
    monkeypatch.setenv('NAGP_STAMPS', '1')
    monkeypatch.delenv('NAGP_IH_TABLES', raising=False)

    def run(pp, yy):
        capfd.readouterr()
        plan = Plan(L.KIND_IHGP, pp, T, **kw)
        assert 'role-specialised waves 1' in capfd.readouterr().err, 'the plan did not choose ihgp_adf8_kernel'
        plan.upload(yy); plan.execute(); out = plan.download(); plan.close()
        return out

    batch = run(probs, ys)
    for q in range(3):
        one = run(probs[q:q + 1], ys[q:q + 1])[0]
        for f in ('Eft', 'Varft', 'ttau', 'tnu', 'R', 'lZ', 'nlZ', 'MS'):
            a, b = getattr(batch[q], f), getattr(one, f)
            assert np.array_equal(a, b, equal_nan=True), (q, f)
        assert np.all(np.isfinite(one.Eft)) and np.all(np.isfinite(one.nlZ))
    assert not np.array_equal(batch[0].Eft, batch[1].Eft)      # the segments are different problems
