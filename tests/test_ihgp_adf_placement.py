"""The weights of the cubature points placed inside c0 / c1 / c2 (csrc/nagp_msr_desc.hpp: msr_place_weights) in the three-barrier
ihgp_adf8_kernel: worker lane p stores the three weights of point p at pos[k][p] and the bin sums read them from there, through the placed
copy of the lists.  With NAGP_IH_PLACE=0 the plan hands the kernel the second copy of the lists and identity positions, the addresses it
used before there was a placement.  A lane adds the same numbers in the same order either way, so every output must keep its bits.

Each case creates, in a fresh child process, one plan with the placement and one with NAGP_IH_PLACE=0 on the same problem
(harness.nmf_problem(..., 'constraints')), asserts from the plan lines (NAGP_STAMPS=1) that both chose the role kernel and which lists each
read, and compares Eft, Varft, ttau, tnu, R, lZ, nlZ, MS and the counter of clamped sites with np.array_equal(..., equal_nan=True).

  D = 32, N = 6, T = 503, one sweep     the headline rule (ut7, 305 points, most weights moved), a partial last lap of the I/O ring
  D = 32, N = 6, T = 500, two sweeps    the second sweep's launch for the last step alone (k_start = T - 1)
  D = 16, N = 3, T = 17                 ut9 in three dimensions (77 points, two worker waves); also against the NumPy oracle at the
                                        tolerances of tests/test_gpu_parity.py
  D = 40, N = 1, T = 203                the K16-pad form of Q / 2Q / v, a ring of 8 steps, five points"""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ('Eft', 'Varft', 'ttau', 'tnu', 'R', 'lZ', 'nlZ', 'MS')
P_OF_CD = {1: 9, 3: 9, 6: 7}      # a rule the role layout serves in that dimension (tests/test_gpu_bin_sums.py)
DAMPING = [0.5, 0.4]


def _child(D, N, T, itts, seed, public, out):
    """Runs in the child: the pair of plans, then (public) one call of the public interface with the placement, for the oracle's comparison."""
    sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'nonstationary-audio-gp_amd'))
    os.environ['NAGP_DEVELOPER'] = '1'; os.environ['NAGP_STAMPS'] = '1'
    for v in ('NAGP_IH_TABLES', 'NAGP_IH_KB', 'NAGP_IH_PLACE'): os.environ.pop(v, None)
    import nagp
    from nagp import harness, Mom, Plan, SSHandle, _lib as L
    from nagp import ss as pss
    nagp.lib()
    pr = harness.nmf_problem(D, N, T, seed, 'constraints')
    blk = pss.balance_blocks(pss.ss_blocks_nmf(pr['param1'], pr['param2'], 'matern32', 'matern52'))
    probs = [(blk, pr['W'], np.log(pr['w_lik']))]
    mom = Mom('likModulatorNMFPower', p_cubature=P_OF_CD[N])
    res = {}
    for place in (1, 0):
        if place: os.environ.pop('NAGP_IH_PLACE', None)
        else: os.environ['NAGP_IH_PLACE'] = '0'
        sys.stderr.write('=== plan with NAGP_IH_PLACE %s\n' % ('unset' if place else '0')); sys.stderr.flush()
        plan = Plan(L.KIND_IHGP, probs, T, mom=mom, ep_fraction=0.5, ep_damping=np.array(DAMPING[:itts]), ep_itts=itts)
        plan.upload([pr['y']]); plan.execute(); o = plan.download()[0]; plan.close()
        for f in FIELDS: res['%s_%d' % (f, place)] = np.asarray(getattr(o, f))
        res['counters_%d' % place] = np.asarray(o.counters)
    os.environ.pop('NAGP_IH_PLACE', None)
    if public:
        t = np.arange(1, T + 1.0)
        r = nagp.ihgp_ep_modulator_nmf(pr['w'], t, pr['y'], SSHandle(), mom, t, 'matern32', 'matern52', 1, D, N, 0.5, np.array(DAMPING[:itts]), itts, nargout=6)
        res['pub_Eft'] = np.asarray(r[0]); res['pub_Varft'] = np.asarray(r[1]); res['pub_nlZ'] = np.asarray(r[5]['nlZ'])
    np.savez(out, **res)


CASES = [(32, 6, 503, 1, 9101, False), (32, 6, 500, 2, 9102, False), (16, 3, 17, 1, 9103, True), (40, 1, 203, 1, 9104, False)]


@pytest.mark.gpu
@pytest.mark.parametrize('D,N,T,itts,seed,oracle', CASES)
def test_placed_weights_give_the_bits_of_identity_positions(D, N, T, itts, seed, oracle, nagp_lib, tmp_path):
    out = str(tmp_path / 'pair.npz')
    r = subprocess.run([sys.executable, os.path.abspath(__file__), str(D), str(N), str(T), str(itts), str(seed), str(int(oracle)), out],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    # the plan lines: both plans chose the role kernel; the first read the placed copy, the second the second copy at identity positions
    parts = r.stderr.split('=== plan with NAGP_IH_PLACE ')
    assert len(parts) == 3 and parts[1].startswith('unset') and parts[2].startswith('0'), r.stderr
    cyc = []
    for part, placed in ((parts[1], 1), (parts[2], 0)):
        assert 'role-specialised waves 1' in part, part
        m = re.search(r'weights placed (\d) \(LDS cycles of member reads \+ weight stores (\d+) \+ (\d+), second copy (\d+) \+ (\d+)\)', part)
        assert m and int(m.group(1)) == placed, part
        cyc.append([int(m.group(i)) for i in range(2, 6)])
    print('D=%d N=%d T=%d sweeps=%d: LDS cycles of reads + stores, placed %d + %d, identity %d + %d' % (D, N, T, itts, cyc[0][0], cyc[0][1], cyc[0][2], cyc[0][3]))
    assert cyc[1][:2] == cyc[1][2:] == cyc[0][2:] and sum(cyc[0][:2]) <= sum(cyc[0][2:])
    if N == 6: assert sum(cyc[0][:2]) <= 0.75 * sum(cyc[0][2:]), cyc      # the headline rule: the two plans do read different addresses
    z = np.load(out)
    assert np.all(np.isfinite(z['Eft_1'])) and np.all(np.isfinite(z['nlZ_1']))
    for f in FIELDS + ('counters',):
        assert np.array_equal(z[f + '_1'], z[f + '_0'], equal_nan=True), f
    if oracle:
        from nagp import harness
        from oracle import ihgp as oih, lik as olik
        from test_gpu_parity import TOL_MEAN, TOL_LOGZ, rel, relz
        pr = harness.nmf_problem(D, N, T, seed, 'constraints'); t = np.arange(1, T + 1.0)
        ref = oih.ihgp_ep_modulator_nmf(pr['w'], t, pr['y'], None, olik.Mom(olik.LIK_POWER_NMF, p=P_OF_CD[N]), t, 'matern32', 'matern52', 1, D, N, 0.5,
                                        np.array(DAMPING[:itts]), itts)
        fe, fv, fz = rel(z['pub_Eft'], ref[0]), rel(z['pub_Varft'], ref[1]), relz(z['pub_nlZ'], ref[5]['nlZ'])
        print('against the oracle: Eft %.2e Varft %.2e nlZ %.2e' % (fe, fv, fz))
        assert fe < TOL_MEAN and fv < TOL_MEAN and fz < TOL_LOGZ, (fe, fv, fz)


if __name__ == '__main__':
    _child(int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5]), bool(int(sys.argv[6])), sys.argv[7])
