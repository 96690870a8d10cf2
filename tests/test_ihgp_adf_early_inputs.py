"""The prediction of the three-barrier ihgp_adf8_kernel formed in the serial waves' idle window: with m_k = A m_{k-1} + wc g the operands
P1 = A (A m_{k-1}), P2 = A wc, pa = h P1[0], pb = h P2[0] are known ahead of barrier B5, and behind the gain fmu of step k + 1 is the single
fma(pb, g, pa); A m_k = fma(P2, g, P1) and the mean for the ring follow off the chain (csrc/nagp_ihgp.hpp, lambda step).  A (Am + wc g) and
A Am + (A wc) g round differently, so the sweep is not bit-equal to the commit before; what holds it is the NumPy oracle at the tolerances of
tests/test_gpu_parity.py and, on its case a, the multi-precision fixture at the bound of tests/test_ep_fixture.py.  Nothing that takes a
decision moves: ttau's clamp, the table index, R's non-finite pattern and the counter of clamped sites must equal the oracle's exactly, and
R = 1 / ttau exactly wherever the launch wrote it.

One plan per fresh child process, as tests/test_ihgp_adf_ttau_chain.py; the oracle of every problem runs beside them in a process of its
own, started once for the module.  Shapes: the smallest that reach each path of the changed step.

  D = 32, N = 6, T = 503                 K8, bench.py's cfg3 shape, outputs on both halves of wave 0
  D = 16, N = 3, T = 17                  K4
  D = 31, N = 6, T = 257                 the run-time form of Q / 2Q / v
  D = 40, N = 1, T = 203                 K16-pad, more sub-bands than half a wave
  D = 32, N = 6, T = 1 and T = 2         no step k + 1 / one: the prologue's head alone forms A m, the loop's window its first operands
  D = 32, N = 6, T = 500, two sweeps     the continued launch (k_start = T - 1 > 0): the prologue's head from the stored mean and R.  That
                                         launch runs ONE step with no head behind it -- the only continued launch a plan makes -- so the
                                         operands its window forms from a k_start > 0 prologue are never consumed, here or by any caller
  D = 8, N = 3, T = 40, seed 9313        the clamp rule: 223 of 440 sites have ttau = 0 -> gain 0, fmu of the next step is pa itself
  D = 16, N = 3, T = 65, exp link        wave 1's other copy of the loop
  D = 16, N = 3, T = 65, ring 4, 8, 16   every depth of the I/O ring (the mean for the ring is formed behind the fmu store)
  D = 31 / 40 / 32 again, no NAGP_STAMPS the plain instantiations, the kernels every caller outside the tests runs (the stamped <6, true, K16-pad>
                                         and <6, true, run-time> spill registers since this change, the plain ones do not)
The counts of clamped sites are the oracle's, found on the CPU; the test requires them of the oracle again before it compares anything.
The first six problems of the list in this docstring and the fixture case are those of tests/test_ihgp_adf_ttau_chain.py, whose helpers
and fixture test this module imports: the same launches, asked again because the step behind them changed."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from test_ihgp_adf_ttau_chain import P_OF_CD, DAMPING, SITE_MAX, _setup_path, _rel_finite
from test_ihgp_adf_ttau_chain import test_clamped_sites_of_the_multiprecision_fixture      # noqa: F401  (case a of the fixture, 1 and 3 sweeps: collected here as well)

# D, N, T, sweeps, seed, link | ring depth (0: the plan's; -1: the plan's, and no NAGP_STAMPS: the plain instantiation), form of Q / 2Q / v,
# clamped sites of the oracle (None: not asserted to be non-zero)
CASES = [((32, 6, 1, 1, 9401, 'softplus'), 0, 'K8', None), ((32, 6, 2, 1, 9402, 'softplus'), 0, 'K8', None),
         ((16, 3, 17, 1, 9203, 'softplus'), 0, 'K4', None), ((8, 3, 40, 1, 9313, 'softplus'), 0, 'run-time', 223),
         ((16, 3, 65, 1, 9403, 'exp'), 0, 'K4', None),
         ((16, 3, 65, 1, 9404, 'softplus'), 4, 'K4', None), ((16, 3, 65, 1, 9404, 'softplus'), 8, 'K4', None),
         ((16, 3, 65, 1, 9404, 'softplus'), 16, 'K4', None),
         ((40, 1, 203, 1, 9204, 'softplus'), 0, 'K16-pad', None), ((31, 6, 257, 1, 9202, 'softplus'), 0, 'run-time', 286),
         ((40, 1, 203, 1, 9204, 'softplus'), -1, 'K16-pad', None), ((31, 6, 257, 1, 9202, 'softplus'), -1, 'run-time', 286),
         ((32, 6, 503, 1, 9201, 'softplus'), 0, 'K8', 226), ((32, 6, 503, 1, 9201, 'softplus'), -1, 'K8', 226),
         ((32, 6, 500, 2, 9205, 'softplus'), 0, 'K8', None)]      # (the long oracles last)
PROBLEMS = sorted({c[0] for c in CASES})
_ids = ['D%d-N%d-T%d-sweeps%d-%s-%s-%s' % (c[0][:4] + (c[0][5], c[2], 'plain' if c[1] < 0 else 'ring%d' % c[1])) for c in CASES]


def _child_gpu(D, N, T, itts, seed, link, kb, out):
    _setup_path()
    os.environ['NAGP_DEVELOPER'] = '1'
    for v in ('NAGP_STAMPS', 'NAGP_IH_TABLES', 'NAGP_IH_KB', 'NAGP_IH_PLACE', 'NAGP_IH_QFORM', 'NAGP_STAMP_WORKER'): os.environ.pop(v, None)
    if kb >= 0: os.environ['NAGP_STAMPS'] = '1'
    if kb > 0: os.environ['NAGP_IH_KB'] = str(kb)
    import nagp
    from nagp import harness, Mom, Plan, _lib as L
    from nagp import ss as pss
    nagp.lib()
    pr = harness.nmf_problem(D, N, T, seed, 'constraints')
    blk = pss.balance_blocks(pss.ss_blocks_nmf(pr['param1'], pr['param2'], 'matern32', 'matern52'))
    plan = Plan(L.KIND_IHGP, [(blk, pr['W'], np.log(pr['w_lik']))], T, mom=Mom('likModulatorNMFPower', link=link, link_shift=0.0, p_cubature=P_OF_CD[N]),
                ep_fraction=0.5, ep_damping=np.array(DAMPING[:itts]), ep_itts=itts)
    plan.upload([pr['y']]); plan.execute(); o = plan.download()[0]; plan.close()
    np.savez(out, counters=np.asarray(o.counters), **{f: np.asarray(getattr(o, f)) for f in ('Eft', 'Varft', 'ttau', 'tnu', 'R', 'lZ', 'nlZ')})


def _child_oracle(D, N, T, itts, seed, link, out):
    _setup_path()
    from nagp import harness
    from oracle import ihgp as oih, lik as olik
    count = [0]
    max0 = oih.matlab_max0

    def counting_max0(x):
        count[0] += int(np.sum(~(np.asarray(x) > 0)))
        return max0(x)
    oih.matlab_max0 = counting_max0
    pr = harness.nmf_problem(D, N, T, seed, 'constraints'); t = np.arange(1, T + 1.0)
    lk = olik.softplus_link(0.0) if link == 'softplus' else olik.exp_link()
    ref = oih.ihgp_ep_modulator_nmf(pr['w'], t, pr['y'], None, olik.Mom(olik.LIK_POWER_NMF, link=lk, p=P_OF_CD[N]), t, 'matern32', 'matern52', 1, D, N, 0.5,
                                    np.array(DAMPING[:itts]), itts)
    r = ref[5]
    np.savez(out, Eft=ref[0], Varft=ref[1], ttau=r['ttau'], tnu=r['tnu'], R=r['R'], nlZ=r['nlZ'], clamped=np.array(count[0]))


@pytest.fixture(scope='module')
def oracles(tmp_path_factory):
    """problem -> the oracle's process and its output file; all started here, each collected by the first test that needs it"""
    d = tmp_path_factory.mktemp('early_inputs_oracle')
    env = dict(os.environ, OMP_NUM_THREADS='2', OPENBLAS_NUM_THREADS='2', MKL_NUM_THREADS='2')
    procs = {}
    for p in PROBLEMS:
        out = str(d / ('ref_%d_%d_%d_%d_%d_%s.npz' % p))
        procs[p] = [subprocess.Popen([sys.executable, os.path.abspath(__file__), 'oracle'] + [str(v) for v in p] + [out], env=env,
                                     stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True), out, None]
    yield procs
    for e in procs.values():
        if e[0].poll() is None: e[0].kill()
        if e[2] is None: e[0].communicate()


@pytest.mark.gpu
@pytest.mark.parametrize('case', CASES, ids=_ids)
def test_sweep_with_the_prediction_from_the_idle_window_meets_the_oracle(case, oracles, nagp_lib, tmp_path):
    from test_gpu_parity import TOL_MEAN, TOL_SITE, TOL_LOGZ, relz
    prob, kb, want_form, want_clamped = case
    D, N, T, itts, seed, link = prob
    out = str(tmp_path / 'gpu.npz')
    r = subprocess.run([sys.executable, os.path.abspath(__file__), 'gpu'] + [str(v) for v in prob] + [str(kb), out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    if kb < 0:
        assert '[nagp' not in r.stderr, r.stderr      # no diagnostics: the plain instantiation of the plan the stamped case beside this one names
        depth, form = 0, want_form + ' (plain)'
    else:
        # the plan chose the three-barrier kernel, the form of Q / 2Q / v and the ring depth the case is about
        assert 'role-specialised waves 1' in r.stderr and 'table form of stage 1b 0' in r.stderr and 'look-up thresholds proved 1' in r.stderr, r.stderr
        m = re.search(r'sparse-point form: 1 \(LDS \d+ B, ring (\d+) steps.*Q/v form ([\w-]+),', r.stderr)
        assert m, r.stderr
        depth, form = int(m.group(1)), m.group(2)
        assert form == want_form and (not kb or depth == kb), (form, depth)
    e = oracles[prob]
    if e[2] is None:
        e[2], _ = e[0].communicate(timeout=300)
    assert e[0].returncode == 0, e[2]
    z, ref = np.load(out), np.load(e[1])
    clamped = int(ref['clamped'])
    assert np.all(np.isfinite(ref['Eft'])) and np.all(np.isfinite(ref['Varft'])) and np.all(np.isfinite(ref['nlZ']))
    for f in ('ttau', 'tnu'):          # the reference is determined on this problem
        assert np.max(np.abs(ref[f][np.isfinite(ref[f])])) < SITE_MAX
    if want_clamped is not None:
        assert clamped == want_clamped > 0 and int(np.sum(np.isinf(ref['R']))) == want_clamped
    figs = {f: _rel_finite(z[f], ref[f]) for f in ('Eft', 'Varft', 'ttau', 'tnu', 'R')}
    figs['nlZ'] = relz(z['nlZ'].reshape(-1), ref['nlZ'].reshape(-1))
    # lZ of the steps: the oracle keeps their sum only, -nlZ of the first sweep (later sweeps rewrite lZ of the refreshed steps)
    figs['lZ'] = relz(-np.sum(z['lZ']), ref['nlZ'].reshape(-1)[0]) if itts == 1 else 0.0
    print('D=%d N=%d T=%d sweeps=%d %s form %s ring %d: ' % (D, N, T, itts, link, form, depth) + ' '.join('%s %.2e' % kv for kv in figs.items()) +
          ' | clamped %d (oracle %d), R non-finite %d' % (int(z['counters'][1]), clamped, int(np.sum(~np.isfinite(z['R'])))))
    for f in ('Eft', 'Varft'): assert figs[f] < TOL_MEAN, (f, figs)
    for f in ('ttau', 'tnu', 'R'): assert figs[f] < TOL_SITE, (f, figs)
    for f in ('nlZ', 'lZ'): assert figs[f] < TOL_LOGZ, (f, figs)
    assert np.array_equal(z['ttau'] == 0.0, ref['ttau'] == 0.0)
    assert int(z['counters'][1]) == clamped, (int(z['counters'][1]), clamped)
    with np.errstate(divide='ignore'):      # R stays the exact division wherever this launch wrote it
        if itts == 1: assert np.array_equal(z['R'], 1.0 / z['ttau'])
        else: assert np.array_equal(z['R'][:, T - 1], 1.0 / z['ttau'][:, T - 1])


if __name__ == '__main__':
    a = sys.argv
    if a[1] == 'gpu': _child_gpu(int(a[2]), int(a[3]), int(a[4]), int(a[5]), int(a[6]), a[7], int(a[8]), a[9])
    else: _child_oracle(int(a[2]), int(a[3]), int(a[4]), int(a[5]), int(a[6]), a[7], a[8])
