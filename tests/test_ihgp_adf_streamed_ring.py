"""The streamed I/O ring of the three-barrier schedule of ihgp_adf8_kernel (direct form, at most six components): the ring of kb = 16 / 8 /
4 steps is circular, slot k mod kb serves step k.  In the window between B5 of step k and B2 of step k + 1 four worker waves write the
inputs of step k + 1 into their slot (loaded one window earlier), load the inputs of step k + 2 and flush the outputs of step k - 1; the
first step is filled ahead of the loop, the last one flushed behind it.  The table form (NAGP_IH_TABLES=1) and seven components keep the
block ring (ihgp_adf8b_kernel: fill, kb steps, flush): the table form is the cross-check inside the same build.

Every case runs through the public interface, asserts (NAGP_STAMPS=1) that the plan chose the role kernel, and is compared with the
NumPy oracle and with the table form at the tolerances tests/test_gpu_parity.py applies to these sweeps, or bit for bit with another
run of the same kernel."""
import re

import numpy as np
import pytest

from nagp import harness, Mom, Plan, _lib as L
from nagp import ss as pss

from test_ihgp_direct_moments import _both_forms

pytestmark = pytest.mark.gpu

FIELDS = ('Eft', 'Varft', 'ttau', 'tnu', 'R', 'lZ', 'nlZ', 'MS')


@pytest.mark.parametrize('DN', [(8, 3), (32, 6)])
@pytest.mark.parametrize('T', [1, 2, 3, 5, 15, 16, 17, 33, 503])
def test_streamed_ring_at_lengths_around_the_ring(T, DN, nagp_lib, monkeypatch, capfd):
    """One ADF sweep.  T = 1: the step filled ahead of the loop is the one flushed behind it, no window does anything.  T = 2, 3: shorter
    than or equal to the look-ahead plus the flush lag (fill k + 1, load k + 2, flush k - 1).  T = 5: one lap of the shortest ring and a
    step.  T = 15, 16, 17: one slot short of a lap of 16, exactly a lap, one beyond (the first slot written a second time).  T = 33, 503:
    several laps with a partial last one."""
    D, N = DN
    _both_forms(D, N, T, 1, 8100 + 10 * D + N + 1000 * (T % 7), monkeypatch, capfd)


def _segments(D, N, T, seed, n):
    probs, ys = [], []
    for q in range(n):
        pr = harness.nmf_problem(D, N, T, seed + q, 'constraints')
        blk = pss.balance_blocks(pss.ss_blocks_nmf(pr['param1'], pr['param2'], 'matern32', 'matern52'))
        probs.append((blk, pr['W'], np.log(pr['w_lik']))); ys.append(pr['y'])
    return probs, ys


def _run_plan(probs, ys, T, p, capfd):
    """One plan of the role kernel: its outputs and the ring depth its plan line states."""
    capfd.readouterr()
    plan = Plan(L.KIND_IHGP, probs, T, mom=Mom('likModulatorNMFPower', p_cubature=p), ep_fraction=0.5, ep_damping=np.array([0.5, 0.4]), ep_itts=2)
    err = capfd.readouterr().err
    assert 'role-specialised waves 1' in err, 'the plan did not choose ihgp_adf8_kernel'
    m = re.search(r'sparse-point form: 1 \(LDS \d+ B, ring (\d+) steps', err)
    assert m, err
    plan.upload(ys); plan.execute(); out = plan.download(); plan.close()
    return out, int(m.group(1))


def test_streamed_ring_gives_the_same_bits_at_every_depth(nagp_lib, monkeypatch, capfd):
    """D = 32, N = 6, T = 203, two sweeps, NAGP_IH_KB = 4, 8, 16: a slot written before its last reader is through, or flushed after its
    next writer, shows at one depth and not at another (203 = 50 laps of 4 + 3 = 25 laps of 8 + 3 = 12 laps of 16 + 11)."""
    D, N, T = 32, 6, 203
    probs, ys = _segments(D, N, T, 8300, 1)
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


def test_streamed_ring_in_a_plan_that_shortens_the_ring_by_itself(nagp_lib, monkeypatch, capfd):
    """D = 40, N = 1: 41 sites, the workspace of the role layout leaves no room for 16 steps.  T = 100."""
    D, N, T = 40, 1, 100
    _both_forms(D, N, T, 1, 8401, monkeypatch, capfd)
    probs, ys = _segments(D, N, T, 8401, 1)
    monkeypatch.setenv('NAGP_STAMPS', '1')
    monkeypatch.delenv('NAGP_IH_KB', raising=False)
    _, depth = _run_plan(probs, ys, T, 9, capfd)
    print('D=%d N=%d: the plan chose a ring of %d steps' % (D, N, depth))
    assert depth in (4, 8, 16)


def test_streamed_ring_with_a_launch_for_the_last_step_in_the_middle_of_a_lap(nagp_lib, monkeypatch, capfd):
    """Two EP sweeps at T = 37: the second sweep's filter pass launches the kernel with k_start = T - 1 = 36, slot 4 of a ring of 16 (4 of
    8, 0 of 4): filled ahead of the loop, flushed behind it, nothing before it is flushed again."""
    _both_forms(8, 3, 37, 2, 8501, monkeypatch, capfd)


def test_streamed_ring_in_a_batch_equals_the_segments_one_at_a_time(nagp_lib, monkeypatch, capfd):
    """A plan of three segments (three workgroups of one launch) gives, bit for bit, what three plans of one segment give."""
    D, N, T = 32, 6, 50
    probs, ys = _segments(D, N, T, 8600, 3)
    monkeypatch.setenv('NAGP_STAMPS', '1')
    monkeypatch.delenv('NAGP_IH_TABLES', raising=False)
    batch, _ = _run_plan(probs, ys, T, 7, capfd)
    for q in range(3):
        one = _run_plan(probs[q:q + 1], ys[q:q + 1], T, 7, capfd)[0][0]
        for f in FIELDS:
            assert np.array_equal(getattr(batch[q], f), getattr(one, f), equal_nan=True), (q, f)
        assert np.all(np.isfinite(one.Eft)) and np.all(np.isfinite(one.nlZ))
    assert not np.array_equal(batch[0].Eft, batch[1].Eft)      # the segments are different problems


def test_seven_components_keep_the_block_ring(nagp_lib, monkeypatch, capfd):
    """N = 7, T = 33: two whole rings of 16 steps and one of a single step, filled and flushed by the whole workgroup."""
    _both_forms(8, 7, 33, 1, 8701, monkeypatch, capfd)
