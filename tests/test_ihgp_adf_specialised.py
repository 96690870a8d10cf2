"""The serial chains of the three-barrier schedule of ihgp_adf8_kernel with what a plan fixes taken out of the step: K and PAD of
Q / 2Q / v on wave 0 are constants of the instantiation the plan picks by its D (csrc/nagp_qform.hpp), wave 1's loop exists once per
link kind and holds the link's shift in a register, and exp / log are written out (csrc/nagp_explog.hpp).  The arithmetic of a step is
unchanged, so everything here is bit for bit:

  D, N      K, PAD        form the plan names
  16, 3     4, no         K4
  12, 1     4, padded     run-time
  32, 6     8, no         K8
  20, 3     8, padded     run-time
  40, 6     16, padded    K16-pad

The developer switch NAGP_IH_QFORM=0 makes every plan take the run-time form (the six paths behind a branch nest, as before): the
cross-check inside the same build.  T = 120 throughout, two sweeps unless said otherwise: the second sweep's filter pass is the continued
launch (k_start = T - 1), so every comparison below covers the prologue of a continued launch as well.  The role kernel has no
uninterrupted launch of a later sweep to compare a continued one with (later sweeps launch only k = T - 1); as in
tests/test_ihgp_adf_seeded_lookup.py the continued launch is pinned from both sides instead: bit-equal between the forms, the ring
depths (its step sits in another slot at each) and the stamped and plain instantiations, and R = 1 / ttau at its step as at every step
of an uninterrupted one-sweep launch."""
import re

import numpy as np
import pytest

import nagp
from nagp import Mom, Plan, SSHandle, harness, _lib as L

from test_ihgp_direct_moments import P_OF_CD, TOL_MEAN, TOL_LOGZ, rel, relz
from test_ihgp_adf_streamed_ring import FIELDS, _segments
from test_ihgp_adf_straight_head import _oracle

pytestmark = pytest.mark.gpu

T = 120
SHAPES = [(16, 3, 'K4'), (12, 1, 'run-time'), (32, 6, 'K8'), (20, 3, 'run-time'), (40, 6, 'K16-pad')]
LINKS = [('softplus', 0.0), ('softplus', 1.0), ('exp', 0.0)]
_SWITCHES = ('NAGP_STAMPS', 'NAGP_IH_TABLES', 'NAGP_IH_KB', 'NAGP_IH_QFORM')


def _plan(probs, ys, N, monkeypatch, capfd, link=('softplus', 0.0), itts=2, qform=True, stamps=True, kb=None):
    """One plan of the role kernel.  Returns its outputs, the Q/v form and the ring depth its plan line names (None without NAGP_STAMPS)."""
    for s in _SWITCHES:
        monkeypatch.delenv(s, raising=False)
    if stamps: monkeypatch.setenv('NAGP_STAMPS', '1')
    if not qform: monkeypatch.setenv('NAGP_IH_QFORM', '0')
    if kb: monkeypatch.setenv('NAGP_IH_KB', str(kb))
    capfd.readouterr()
    mom = Mom('likModulatorNMFPower', link=link[0], link_shift=link[1], p_cubature=P_OF_CD[N])
    plan = Plan(L.KIND_IHGP, probs, T, mom=mom, ep_fraction=0.5, ep_damping=np.array([0.5, 0.4])[:itts], ep_itts=itts)
    err = capfd.readouterr().err
    form = depth = None
    if stamps:
        assert 'role-specialised waves 1' in err and 'table form of stage 1b 0' in err, 'the plan did not choose the three-barrier ihgp_adf8_kernel'
        m = re.search(r'sparse-point form: 1 \(LDS \d+ B, ring (\d+) steps.*Q/v form ([\w-]+),', err)
        assert m, err
        depth, form = int(m.group(1)), m.group(2)
    else:
        assert '[nagp' not in err      # no diagnostics: the plain instantiation
    plan.upload(ys); plan.execute(); out = plan.download(); plan.close()
    for s in _SWITCHES:
        monkeypatch.delenv(s, raising=False)
    return out, form, depth


def _same_bits(a, b, what):
    for f in FIELDS:
        assert np.array_equal(getattr(a, f), getattr(b, f), equal_nan=True), (what, f)
    assert np.array_equal(a.counters, b.counters), what


@pytest.mark.parametrize('link', LINKS, ids=lambda l: '%s-shift%g' % l)
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'D%d-N%d' % s[:2])
def test_fixed_form_equals_the_run_time_form(shape, link, nagp_lib, monkeypatch, capfd):
    """The instantiation the plan picks against the run-time form under NAGP_IH_QFORM=0: every output array bit-equal, both link kinds,
    the softplus with shift 0 and 1."""
    D, N, name = shape
    probs, ys = _segments(D, N, T, 9100 + 10 * D + N, 1)
    picked, form, _ = _plan(probs, ys, N, monkeypatch, capfd, link=link)
    assert form == name, (form, name)
    fallback, form0, _ = _plan(probs, ys, N, monkeypatch, capfd, link=link, qform=False)
    assert form0 == 'run-time', form0
    print('D=%d N=%d %s shift %g: form %s; finite Eft %d of %d, clamped sites %d' % (D, N, link[0], link[1], form, int(np.sum(np.isfinite(picked[0].Eft))),
                                                                                  picked[0].Eft.size, int(picked[0].counters[1])))
    assert np.all(np.isfinite(picked[0].Eft)) and np.all(np.isfinite(picked[0].nlZ))
    _same_bits(picked[0], fallback[0], (D, N, link))
    if link != LINKS[0]:      # the link's kind and shift reach the kernel: another link, another result
        base, _, _ = _plan(probs, ys, N, monkeypatch, capfd, link=LINKS[0])
        assert not np.array_equal(base[0].Eft, picked[0].Eft)


@pytest.mark.parametrize('shape', [SHAPES[0], SHAPES[2]], ids=lambda s: 'D%d-N%d' % s[:2])
def test_fixed_forms_give_the_same_bits_at_every_ring_depth(shape, nagp_lib, monkeypatch, capfd):
    """NAGP_IH_KB = 4, 8, 16, two sweeps: the continued launch's step T - 1 = 119 sits in slot 3, 7, 7."""
    D, N, name = shape
    probs, ys = _segments(D, N, T, 9300 + D, 1)
    outs = {}
    for kb in (4, 8, 16):
        out, form, depth = _plan(probs, ys, N, monkeypatch, capfd, kb=kb)
        assert depth == kb and form == name, (kb, depth, form)
        outs[kb] = out[0]
    assert np.all(np.isfinite(outs[16].Eft)) and np.all(np.isfinite(outs[16].nlZ))
    for kb in (4, 8):
        _same_bits(outs[kb], outs[16], kb)


def test_continued_launch_of_the_second_sweep(nagp_lib, monkeypatch, capfd):
    """D = 32, N = 6, softplus with shift 1, two sweeps: the launch with k_start = T - 1 runs the prologue's Q / 2Q / v and link tables (the
    same functions as the loop's) and one site update.  Bit-equal between the picked and the run-time form; R = 1 / ttau at its step as
    at every step of the uninterrupted launch of a one-sweep plan."""
    D, N = 32, 6
    link = ('softplus', 1.0)
    probs, ys = _segments(D, N, T, 9400, 1)
    two, form, _ = _plan(probs, ys, N, monkeypatch, capfd, link=link)
    two0, _, _ = _plan(probs, ys, N, monkeypatch, capfd, link=link, qform=False)
    one, _, _ = _plan(probs, ys, N, monkeypatch, capfd, link=link, itts=1)
    assert form == 'K8'
    _same_bits(two[0], two0[0], 'two sweeps')
    with np.errstate(divide='ignore'):
        assert np.array_equal(one[0].R, 1.0 / one[0].ttau)
        assert np.array_equal(two[0].R[:, T - 1], 1.0 / two[0].ttau[:, T - 1])
    assert np.all(np.isfinite(two[0].Eft)) and np.all(np.isfinite(two[0].nlZ))
    assert not np.array_equal(one[0].Eft, two[0].Eft)


def test_fixed_form_in_a_batch_equals_the_segments_one_at_a_time(nagp_lib, monkeypatch, capfd):
    """A plan of three segments (three workgroups of one launch) gives, bit for bit, what three plans of one segment give."""
    D, N = 32, 6
    probs, ys = _segments(D, N, T, 9500, 3)
    batch, form, _ = _plan(probs, ys, N, monkeypatch, capfd)
    assert form == 'K8'
    for q in range(3):
        one = _plan(probs[q:q + 1], ys[q:q + 1], N, monkeypatch, capfd)[0][0]
        _same_bits(batch[q], one, q)
        assert np.all(np.isfinite(one.Eft)) and np.all(np.isfinite(one.nlZ))
    assert not np.array_equal(batch[0].Eft, batch[1].Eft)      # the segments are different problems


@pytest.mark.parametrize('shape', [SHAPES[0], SHAPES[2], SHAPES[4], SHAPES[3]], ids=lambda s: 'D%d-N%d' % s[:2])
def test_stamped_and_plain_instantiation_give_the_same_bits(shape, nagp_lib, monkeypatch, capfd):
    """With NAGP_STAMPS the plan takes ihgp_adf8_kernel<N, false, true, form>, without it <N, false, false, form> -- the kernel bench.py
    and every caller outside the tests run.  One shape per form."""
    D, N, name = shape
    probs, ys = _segments(D, N, T, 9600 + D, 1)
    stamped, form, _ = _plan(probs, ys, N, monkeypatch, capfd)
    assert form == name
    plain, _, _ = _plan(probs, ys, N, monkeypatch, capfd, stamps=False)
    assert np.all(np.isfinite(plain[0].Eft)) and np.all(np.isfinite(plain[0].nlZ))
    _same_bits(stamped[0], plain[0], shape)


def test_fixed_form_against_the_oracle(nagp_lib, monkeypatch, capfd):
    """D = 32, N = 6, T = 120 (seed 7002), one sweep through the public interface: the case of tests/test_ihgp_adf_straight_head.py, whose
    oracle run is shared, at its tolerances."""
    D, N, seed = 32, 6, 7002
    ref = _oracle(D, N, T, seed, 1.0, 1)
    pr = harness.nmf_problem(D, N, T, seed, 'constraints'); t = np.arange(1, T + 1.0)
    for s in _SWITCHES:
        monkeypatch.delenv(s, raising=False)
    monkeypatch.setenv('NAGP_STAMPS', '1')
    capfd.readouterr()
    res = nagp.ihgp_ep_modulator_nmf(pr['w'], t, pr['y'], SSHandle(), Mom('likModulatorNMFPower', p_cubature=P_OF_CD[N]), t,
                                     'matern32', 'matern52', 1, D, N, 0.5, np.array([0.5]), 1, nargout=6)
    err = capfd.readouterr().err
    monkeypatch.delenv('NAGP_STAMPS', raising=False)
    assert 'role-specialised waves 1' in err and 'Q/v form K8,' in err, err
    fe, fv, fz = rel(res[0], ref[0]), rel(res[1], ref[1]), relz(res[5]['nlZ'], ref[5]['nlZ'])
    print('D=%d N=%d T=%d K8 vs oracle: Eft %.2e Varft %.2e nlZ %.2e' % (D, N, T, fe, fv, fz))
    assert fe < TOL_MEAN and fv < TOL_MEAN and fz < TOL_LOGZ, (fe, fv, fz)
