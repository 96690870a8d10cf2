"""The leaner serial tails of the three-barrier schedule of ihgp_adf8_kernel: wave 1's softplus link as softplus_short
(csrc/nagp_explog.hpp: max(x, 0) + log1p(exp(-|x|)), never 1 + exp(x) as a rounded argument) and wave 0's second-moment contraction
w'Rw from the lane's static products P_q = W_dj W_dj' (doubled off the diagonal; msp_wproducts / msp_outputs_b, csrc/nagp_momsp.hpp), one
FMA per entry of R.  Both change roundings, so this schedule is no longer bit-equal to link_eval / msp_outputs of the other schedules;
what holds it is the oracle at the tolerances of tests/test_gpu_parity.py here and the multi-precision fixture (tests/test_ep_fixture.py).
Everything that is the SAME arithmetic stays bit for bit: ring depths, the form of Q / 2Q / v, stamped and plain instantiations, a batch
against its segments, and R = 1 / ttau.

  D, N      form of Q / 2Q / v     cubature
  16, 3     K4                     ut9
  32, 6     K8 (bench.py's cfg3)   ut7
  40, 4     K16-pad                ut9
  12, 2     run-time               ut9

T = 400.  Two sweeps: the second sweep's filter pass is the continued launch (k_start = T - 1).  The role kernel has no uninterrupted
launch of a later sweep to compare a continued one with (later sweeps launch only k = T - 1), so, as in
tests/test_ihgp_adf_specialised.py, the continued launch is pinned from both sides: bit-equal between the forms, the ring depths and
the stamped and plain instantiations, within tolerance of the oracle's second sweep, and R = 1 / ttau at its step.

The clamped-site case is case a of the multi-precision fixture (tests/golden/ep_multiprecision.npz; 8 sub-bands, 3 components, 40 steps,
run-time form): every stored field within the fixture's bound and the oracle's count of clamped sites reproduced.  The same check fails
when the product table is built wrong -- off-diagonal entries not doubled, bit 64 of the developer switch NAGP_STAMP_WORKER, read ahead
of the loop -- which shows that the check sees the table."""
import re

import numpy as np
import pytest

import nagp
from nagp import Mom, Plan, SSHandle, harness, _lib as L
from oracle import ihgp as oih, lik as olik

from test_gpu_parity import TOL_MEAN, TOL_LOGZ, rel, relz
from test_ihgp_adf_streamed_ring import FIELDS, _segments
import test_ep_fixture as epf

pytestmark = pytest.mark.gpu

T = 400
P_OF_N = {2: 9, 3: 9, 4: 9, 6: 7}
SHAPES = [(16, 3, 'K4'), (32, 6, 'K8'), (40, 4, 'K16-pad'), (12, 2, 'run-time')]
SEEDS = {(16, 3): 11163, (32, 6): 11326, (40, 4): 11404, (12, 2): 11123}      # 11000 + 10 D + N; (12, 2): + 1, see the oracle test
SITE_MAX = 1e8      # tools/fuzz_conditioning.py
LINKS = [('softplus', 0.0), ('exp', 0.0)]
_SWITCHES = ('NAGP_STAMPS', 'NAGP_IH_TABLES', 'NAGP_IH_KB', 'NAGP_IH_QFORM', 'NAGP_STAMP_WORKER')
_ids = dict(ids=lambda s: 'D%d-N%d' % s[:2])


def _clear(monkeypatch):
    for s in _SWITCHES:
        monkeypatch.delenv(s, raising=False)


def _public(D, N, seed, link, itts, monkeypatch, capfd, tables=False):
    """One call through the public interface; the plan's lines (NAGP_STAMPS) name the kernel and the form it chose."""
    pr = harness.nmf_problem(D, N, T, seed, 'constraints'); t = np.arange(1, T + 1.0)
    _clear(monkeypatch)
    monkeypatch.setenv('NAGP_STAMPS', '1')
    if tables: monkeypatch.setenv('NAGP_IH_TABLES', '1')
    capfd.readouterr()
    res = nagp.ihgp_ep_modulator_nmf(pr['w'], t, pr['y'], SSHandle(), Mom('likModulatorNMFPower', link=link[0], link_shift=link[1], p_cubature=P_OF_N[N]), t,
                                     'matern32', 'matern52', 1, D, N, 0.5, np.array([0.5, 0.4])[:itts], itts, nargout=6)
    err = capfd.readouterr().err
    _clear(monkeypatch)
    assert 'role-specialised waves 1' in err and 'table form of stage 1b %d' % int(tables) in err, err
    m = re.search(r'Q/v form ([\w-]+),', err)
    return res, (m.group(1) if m else None)


def _oracle(D, N, seed, link, itts):
    pr = harness.nmf_problem(D, N, T, seed, 'constraints'); t = np.arange(1, T + 1.0)
    lk = olik.softplus_link(link[1]) if link[0] == 'softplus' else olik.exp_link()
    return oih.ihgp_ep_modulator_nmf(pr['w'], t, pr['y'], None, olik.Mom(olik.LIK_POWER_NMF, link=lk, p=P_OF_N[N]), t, 'matern32', 'matern52',
                                     1, D, N, 0.5, np.array([0.5, 0.4])[:itts], itts)


@pytest.mark.parametrize('itts', [1, 2], ids=lambda i: 'sweeps%d' % i)
@pytest.mark.parametrize('link', LINKS, ids=lambda l: l[0])
@pytest.mark.parametrize('shape', SHAPES, **_ids)
def test_lean_tail_against_the_oracle_and_the_table_form(shape, link, itts, nagp_lib, monkeypatch, capfd):
    """The picked form against the NumPy oracle and against the table form of the same build (which keeps link_eval's softplus and
    msp_outputs' contraction), at the tolerances tests/test_gpu_parity.py applies to these sweeps.  The table form against the oracle is
    printed beside them.

    Every problem here is one on which the reference algorithm itself is determined: no site parameter of the ORACLE lies beyond SITE_MAX
    = 1e8, the project's criterion (tools/fuzz_conditioning.py, tools/full_length_parity.py) for a site update -d2 / (1 + d2 v) whose
    denominator is O(1e-9 .. 1e-15), so that its size and sign are rounding noise in the reference.  The test asserts that on the oracle
    before it compares anything.  It is why D = 12 / N = 2 takes seed 11123 and not 11122 = 11000 + 10 D + N like the others: with seed
    11122, exp link, two sweeps, the oracle's own site refresh of the second sweep produces |ttau| = 2.9e14 and |tnu| = 1.6e14 (step 199,
    second modulator; its neighbours are below 30).  Two correct evaluations of the first sweep that differ by 1e-13 then land on
    opposite signs of that site -- the direct form gives ttau = 0 (clamped), the table form +1.5e14 -- and their Eft differ by 0.14, in
    the commit before this change exactly as in this one.  The largest oracle site of the sixteen cases used: 1.1e4."""
    D, N, name = shape
    seed = SEEDS[(D, N)]
    ref = _oracle(D, N, seed, link, itts)
    assert np.all(np.isfinite(ref[0])) and np.all(np.isfinite(ref[1])) and np.all(np.isfinite(ref[5]['nlZ']))
    for f in ('ttau', 'tnu'):      # the reference is determined on this problem (see above)
        s = np.asarray(ref[5][f], float)
        assert np.max(np.abs(s[np.isfinite(s)])) < SITE_MAX, (f, float(np.max(np.abs(s[np.isfinite(s)]))))
    new, form = _public(D, N, seed, link, itts, monkeypatch, capfd)
    tab, _ = _public(D, N, seed, link, itts, monkeypatch, capfd, tables=True)
    assert form == name, (form, name)
    figs = {}
    for what, a, b in (('lean tail vs oracle', new, ref), ('tables vs oracle', tab, ref), ('lean tail vs tables', new, tab)):
        figs[what] = (rel(a[0], b[0]), rel(a[1], b[1]), relz(a[5]['nlZ'], b[5]['nlZ']))
        print('D=%d N=%d %s sweeps=%d %s: Eft %.2e Varft %.2e nlZ %.2e' % ((D, N, link[0], itts, what) + figs[what]))
    for what in ('lean tail vs oracle', 'lean tail vs tables'):
        fe, fv, fz = figs[what]
        assert fe < TOL_MEAN and fv < TOL_MEAN and fz < TOL_LOGZ, (what, fe, fv, fz)


def _plan(probs, ys, N, monkeypatch, capfd, link=LINKS[0], itts=2, qform=True, stamps=True, kb=None, worker=None):
    """One plan of the role kernel: its outputs, the Q/v form and the ring depth its plan line names (None without NAGP_STAMPS)."""
    _clear(monkeypatch)
    if stamps: monkeypatch.setenv('NAGP_STAMPS', '1')
    if not qform: monkeypatch.setenv('NAGP_IH_QFORM', '0')
    if kb: monkeypatch.setenv('NAGP_IH_KB', str(kb))
    if worker is not None: monkeypatch.setenv('NAGP_STAMP_WORKER', str(worker))
    capfd.readouterr()
    mom = Mom('likModulatorNMFPower', link=link[0], link_shift=link[1], p_cubature=P_OF_N[N])
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
    _clear(monkeypatch)
    return out, form, depth


def _same_bits(a, b, what):
    for f in FIELDS:
        assert np.array_equal(getattr(a, f), getattr(b, f), equal_nan=True), (what, f)
    assert np.array_equal(a.counters, b.counters), what


@pytest.mark.parametrize('link', LINKS + [('softplus', 1.0)], ids=lambda l: '%s-shift%g' % l)
@pytest.mark.parametrize('shape', SHAPES, **_ids)
def test_picked_form_equals_the_run_time_form_and_R_is_the_exact_reciprocal(shape, link, nagp_lib, monkeypatch, capfd):
    """Two sweeps: the instantiation the plan picks against the run-time form under NAGP_IH_QFORM=0, every output bit-equal (both run the
    same tails).  R = 1 / ttau exactly at every step of a one-sweep plan and at the continued launch's step of the two-sweep plan."""
    D, N, name = shape
    probs, ys = _segments(D, N, T, 11300 + 10 * D + N, 1)
    picked, form, _ = _plan(probs, ys, N, monkeypatch, capfd, link=link)
    assert form == name, (form, name)
    fallback, form0, _ = _plan(probs, ys, N, monkeypatch, capfd, link=link, qform=False)
    assert form0 == 'run-time', form0
    assert np.all(np.isfinite(picked[0].Eft)) and np.all(np.isfinite(picked[0].nlZ))
    _same_bits(picked[0], fallback[0], (D, N, link))
    one, _, _ = _plan(probs, ys, N, monkeypatch, capfd, link=link, itts=1)
    with np.errstate(divide='ignore'):
        assert np.array_equal(one[0].R, 1.0 / one[0].ttau)
        assert np.array_equal(picked[0].R[:, T - 1], 1.0 / picked[0].ttau[:, T - 1])
    assert not np.array_equal(one[0].Eft, picked[0].Eft)


@pytest.mark.parametrize('shape', SHAPES[:2], **_ids)
def test_lean_tail_gives_the_same_bits_at_every_ring_depth(shape, nagp_lib, monkeypatch, capfd):
    """NAGP_IH_KB = 4, 8, 16, two sweeps: the continued launch's step T - 1 = 399 sits in slot 3, 7, 15."""
    D, N, name = shape
    probs, ys = _segments(D, N, T, 11500 + D, 1)
    outs = {}
    for kb in (4, 8, 16):
        out, form, depth = _plan(probs, ys, N, monkeypatch, capfd, kb=kb)
        assert depth == kb and form == name, (kb, depth, form)
        outs[kb] = out[0]
    assert np.all(np.isfinite(outs[16].Eft)) and np.all(np.isfinite(outs[16].nlZ))
    for kb in (4, 8):
        _same_bits(outs[kb], outs[16], kb)


@pytest.mark.parametrize('shape', SHAPES, **_ids)
def test_stamped_and_plain_instantiation_give_the_same_bits(shape, nagp_lib, monkeypatch, capfd):
    """With NAGP_STAMPS the plan takes ihgp_adf8_kernel<N, false, true, form>, without it <N, false, false, form> -- the kernel bench.py
    and every caller outside the tests run.  Two sweeps, one shape per form."""
    D, N, name = shape
    probs, ys = _segments(D, N, T, 11600 + D, 1)
    stamped, form, _ = _plan(probs, ys, N, monkeypatch, capfd)
    assert form == name
    plain, _, _ = _plan(probs, ys, N, monkeypatch, capfd, stamps=False)
    assert np.all(np.isfinite(plain[0].Eft)) and np.all(np.isfinite(plain[0].nlZ))
    _same_bits(stamped[0], plain[0], shape)


def test_a_batch_of_three_equals_the_segments_one_at_a_time(nagp_lib, monkeypatch, capfd):
    """A plan of three segments (three workgroups of one launch) gives, bit for bit, what three plans of one segment give."""
    D, N = 32, 6
    probs, ys = _segments(D, N, T, 11700, 3)
    batch, form, _ = _plan(probs, ys, N, monkeypatch, capfd)
    assert form == 'K8'
    for q in range(3):
        one = _plan(probs[q:q + 1], ys[q:q + 1], N, monkeypatch, capfd)[0][0]
        _same_bits(batch[q], one, q)
        assert np.all(np.isfinite(one.Eft)) and np.all(np.isfinite(one.nlZ))
    assert not np.array_equal(batch[0].Eft, batch[1].Eft)      # the segments are different problems


def test_clamped_sites_of_the_fixture_and_a_wrong_product_table(nagp_lib, capfd):
    """Case a of the multi-precision fixture, one and three sweeps: every stored field within the fixture's bound, the oracle's count of
    clamped sites (which is not zero) reproduced.  With the off-diagonal products not doubled the same check fails."""
    lines = []
    for itts in epf.tool.SWEEPS:
        outs, stamps = epf._plan_run(['a'], 'ihgp', itts, {}, capfd)
        assert 'role-specialised waves 1' in stamps and 'table form of stage 1b 0' in stamps, stamps
        assert int(epf._run('a', 'ihgp', itts)['clamped']) > 0
        bad = epf._check('a', 'ihgp', itts, outs[0], 'lean tail', lines)
        wrong, _ = epf._plan_run(['a'], 'ihgp', itts, {'NAGP_STAMP_WORKER': '64'}, capfd)
        bad_wrong = epf._check('a', 'ihgp', itts, wrong[0], 'products not doubled', lines)
        with capfd.disabled():
            print('\n' + '\n'.join(lines))
        assert not bad, bad
        assert bad_wrong, 'the fixture does not see a product table whose off-diagonal entries are not doubled'
