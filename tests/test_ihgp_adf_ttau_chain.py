"""The site update of the three-barrier ihgp_adf8_kernel with R = 1 / ttau off its chains: the table index of step k + 1 from ttau through
the threshold table of the grid (csrc/nagp_lookup.hpp: lookup_thresholds, lookup_mid_bits; exact by construction,
tests/test_ihgp_lookup_thresholds_host.py) and the gain as (tnu - fmu ttau) / (1 + HPH ttau), selected to 0 by ttau <= t_inf where the
parent asked R < Inf.  R stays the exact division and is an output only.  The gain rounds differently from the parent's
(tnu R - fmu) / (HPH + R), so what holds the sweep is the NumPy oracle at the tolerances of tests/test_gpu_parity.py and, on its case a,
the multi-precision fixture at the bound of tests/test_ep_fixture.py; the index, and with it R's non-finite pattern and the counter of
clamped sites, must equal the oracle's exactly.

One plan per fresh child process, as tests/test_ihgp_adf_placement.py; the oracle of every case runs beside them in processes of its
own, started once for the module.  The oracle's counter: every site that ttau = max(ttau, 0) finds not positive (oracle.ihgp.matlab_max0,
counted as tools/make_ep_fixture.py counts), in every sweep.

  D = 32, N = 6, T = 503                 K8, bench.py's cfg3 shape; 226 clamped sites
  D = 31, N = 6, T = 257                 the padded form of Q / 2Q / v, an idle lane beside the last sub-band; 286 clamped sites
  D = 16, N = 3, T = 17                  K4, ut9 in three dimensions
  D = 40, N = 1, T = 203                 more sub-bands than half a wave
  D = 32, N = 6, T = 500, two sweeps     the launch for k = T - 1 of a later sweep: the continued launch (k_start = T - 1 > 0)
  D = 8, N = 3, T = 40, seed 9313        the clamp rule: 223 of 440 sites have ttau = 0 -> R = Inf, gain 0, table index 0
The counts are the oracle's, found on the CPU; the test requires them of the oracle again before it compares anything.

No check with a wrong table here: shifting the thresholds by one entry would take a switch in the product's plan that nothing else needs."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P_OF_CD = {1: 9, 3: 9, 6: 7}      # a rule the role layout serves in that dimension (tests/test_gpu_bin_sums.py)
DAMPING = [0.5, 0.4]
SITE_MAX = 1e8                    # tools/fuzz_conditioning.py: the reference is determined on the problem (tests/test_ihgp_adf_lean_tail.py)
# D, N, T, sweeps, seed, clamped sites of the oracle (None: not asserted to be non-zero)
CASES = [(32, 6, 503, 1, 9201, 226), (31, 6, 257, 1, 9202, 286), (16, 3, 17, 1, 9203, None), (40, 1, 203, 1, 9204, None),
         (32, 6, 500, 2, 9205, None), (8, 3, 40, 1, 9313, 223)]
_ids = ['D%d-N%d-T%d-sweeps%d' % c[:4] for c in CASES]


def _setup_path():
    sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'nonstationary-audio-gp_amd'))


def _child_gpu(D, N, T, itts, seed, out):
    _setup_path()
    os.environ['NAGP_DEVELOPER'] = '1'; os.environ['NAGP_STAMPS'] = '1'
    for v in ('NAGP_IH_TABLES', 'NAGP_IH_KB', 'NAGP_IH_PLACE', 'NAGP_IH_QFORM', 'NAGP_STAMP_WORKER'): os.environ.pop(v, None)
    import nagp
    from nagp import harness, Mom, Plan, _lib as L
    from nagp import ss as pss
    nagp.lib()
    pr = harness.nmf_problem(D, N, T, seed, 'constraints')
    blk = pss.balance_blocks(pss.ss_blocks_nmf(pr['param1'], pr['param2'], 'matern32', 'matern52'))
    plan = Plan(L.KIND_IHGP, [(blk, pr['W'], np.log(pr['w_lik']))], T, mom=Mom('likModulatorNMFPower', p_cubature=P_OF_CD[N]), ep_fraction=0.5,
                ep_damping=np.array(DAMPING[:itts]), ep_itts=itts)
    plan.upload([pr['y']]); plan.execute(); o = plan.download()[0]; plan.close()
    np.savez(out, counters=np.asarray(o.counters), **{f: np.asarray(getattr(o, f)) for f in ('Eft', 'Varft', 'ttau', 'tnu', 'R', 'lZ', 'nlZ')})


def _child_oracle(D, N, T, itts, seed, out):
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
    ref = oih.ihgp_ep_modulator_nmf(pr['w'], t, pr['y'], None, olik.Mom(olik.LIK_POWER_NMF, p=P_OF_CD[N]), t, 'matern32', 'matern52', 1, D, N, 0.5,
                                    np.array(DAMPING[:itts]), itts)
    r = ref[5]
    np.savez(out, Eft=ref[0], Varft=ref[1], ttau=r['ttau'], tnu=r['tnu'], R=r['R'], nlZ=r['nlZ'], clamped=np.array(count[0]))


@pytest.fixture(scope='module')
def oracles(tmp_path_factory):
    """case -> the oracle's process and its output file; all started here, each collected by the test that needs it"""
    d = tmp_path_factory.mktemp('ttau_chain_oracle')
    env = dict(os.environ, OMP_NUM_THREADS='2', OPENBLAS_NUM_THREADS='2', MKL_NUM_THREADS='2')
    procs = {}
    for c in CASES:
        out = str(d / ('ref_%d_%d_%d_%d.npz' % c[:4]))
        procs[c] = (subprocess.Popen([sys.executable, os.path.abspath(__file__), 'oracle'] + [str(v) for v in c[:5]] + [out], env=env,
                                     stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True), out)
    yield procs
    for p, _ in procs.values():
        if p.poll() is None: p.kill()
        p.communicate()


def _rel_finite(a, b):
    """max |a - b| / max |b| over the finite entries; the non-finite patterns must be the same, value for value"""
    a = np.asarray(a, float); b = np.asarray(b, float)
    assert a.shape == b.shape, (a.shape, b.shape)
    fa, fb = np.isfinite(a), np.isfinite(b)
    assert np.array_equal(fa, fb) and np.array_equal(a[~fa], b[~fb], equal_nan=True)
    return float(np.max(np.abs(a[fa] - b[fb])) / (np.max(np.abs(b[fb])) + 1e-300)) if fa.any() else 0.0


@pytest.mark.gpu
@pytest.mark.parametrize('case', CASES, ids=_ids)
def test_sweep_with_the_lookup_and_the_gain_from_ttau_meets_the_oracle(case, oracles, nagp_lib, tmp_path):
    from test_gpu_parity import TOL_MEAN, TOL_SITE, TOL_LOGZ, relz
    D, N, T, itts, seed, want_clamped = case
    out = str(tmp_path / 'gpu.npz')
    r = subprocess.run([sys.executable, os.path.abspath(__file__), 'gpu'] + [str(v) for v in case[:5]] + [out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    # the plan chose the three-barrier kernel and its grid gave a proved threshold table
    assert 'role-specialised waves 1' in r.stderr and 'table form of stage 1b 0' in r.stderr and 'look-up thresholds proved 1' in r.stderr, r.stderr
    form = re.search(r'Q/v form ([\w-]+),', r.stderr).group(1)
    proc, ref_path = oracles[case]
    log, _ = proc.communicate(timeout=300)
    assert proc.returncode == 0, log
    z, ref = np.load(out), np.load(ref_path)
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
    print('D=%d N=%d T=%d sweeps=%d form %s: ' % (D, N, T, itts, form) + ' '.join('%s %.2e' % kv for kv in figs.items()) +
          ' | clamped %d (oracle %d), R non-finite %d' % (int(z['counters'][1]), clamped, int(np.sum(~np.isfinite(z['R'])))))
    for f in ('Eft', 'Varft'): assert figs[f] < TOL_MEAN, (f, figs)
    for f in ('ttau', 'tnu', 'R'): assert figs[f] < TOL_SITE, (f, figs)
    for f in ('nlZ', 'lZ'): assert figs[f] < TOL_LOGZ, (f, figs)
    assert np.array_equal(z['ttau'] == 0.0, ref['ttau'] == 0.0)
    assert int(z['counters'][1]) == clamped, (int(z['counters'][1]), clamped)
    with np.errstate(divide='ignore'):      # R stays the exact division wherever this launch wrote it
        if itts == 1: assert np.array_equal(z['R'], 1.0 / z['ttau'])
        else: assert np.array_equal(z['R'][:, T - 1], 1.0 / z['ttau'][:, T - 1])


@pytest.mark.gpu
def test_clamped_sites_of_the_multiprecision_fixture(nagp_lib, capfd):
    """Case a of tests/golden/ep_multiprecision.npz (8 sub-bands, 3 components, 40 steps), every sweep count it stores: each field within
    min(max(10 x the oracle's own error, 1e-12), TOL) and the fixture's count of clamped sites, which is not zero, reproduced."""
    import test_ep_fixture as epf
    lines = []
    for itts in epf.tool.SWEEPS:
        outs, stamps = epf._plan_run(['a'], 'ihgp', itts, {}, capfd)
        assert 'role-specialised waves 1' in stamps and 'table form of stage 1b 0' in stamps and 'look-up thresholds proved 1' in stamps, stamps
        assert int(epf._run('a', 'ihgp', itts)['clamped']) > 0
        bad = epf._check('a', 'ihgp', itts, outs[0], 'ttau chain', lines)
        with capfd.disabled():
            print('\n' + '\n'.join(lines))
        assert not bad, bad


if __name__ == '__main__':
    a = sys.argv
    (_child_gpu if a[1] == 'gpu' else _child_oracle)(int(a[2]), int(a[3]), int(a[4]), int(a[5]), int(a[6]), a[7])
