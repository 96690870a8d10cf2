"""GPU (-m gpu): the cubature sums of the role-specialised ADF sweeps (nagp_momsp.hpp, msr_sums: bin sums over static member
lists) against the NumPy oracle, one ADF sweep each, for the rules the role layout serves: ut7 in six dimensions (305 points, the
headline rule), ut9 in three and in four dimensions (points with four non-centre coordinates), ut5 in seven dimensions."""
import numpy as np
import pytest

import nagp
from nagp import harness, Mom, SSHandle
from oracle import gf_ep as ogf, ihgp as oih, lik as olik

pytestmark = pytest.mark.gpu
TOL_MEAN, TOL_SITE, TOL_LOGZ = 1e-7, 1e-6, 1e-8

RULES = [(7, 6), (9, 3), (9, 4), (5, 7)]      # (p_cubature, N)


def rel(a, b):
    a = np.asarray(a, float); b = np.asarray(b, float)
    assert a.shape == b.shape, (a.shape, b.shape)
    assert np.array_equal(np.isnan(a), np.isnan(b))
    return float(np.nanmax(np.abs(a - b)) / (np.nanmax(np.abs(b)) + 1e-300)) if a.size else 0.0


def relz(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b)) / np.abs(np.asarray(b))))


@pytest.fixture(scope='module', autouse=True)
def _lib(nagp_lib):
    assert nagp_lib.nagp_device_count() >= 1
    return nagp_lib


@pytest.mark.parametrize('p,N', RULES)
def test_ihgp_adf_sweep_bin_sums_against_the_oracle(p, N):
    D, T = 8, 120
    pr = harness.nmf_problem(D, N, T, 310 + 10 * p + N); t = np.arange(1, T + 1.0)
    d = 0.5 * np.ones(1)
    r = nagp.ihgp_ep_modulator_nmf(pr['w'], t, pr['y'], SSHandle(), Mom('likModulatorNMFPower', p_cubature=p), t, 'matern32', 'matern52',
                                   1, D, N, 0.5, d, 1, nargout=6)
    o = oih.ihgp_ep_modulator_nmf(pr['w'], t, pr['y'], None, olik.Mom(olik.LIK_POWER_NMF, p=p), t, 'matern32', 'matern52', 1, D, N, 0.5, d, 1)
    assert rel(r[0], o[0]) < TOL_MEAN and rel(r[1], o[1]) < TOL_MEAN
    assert rel(r[5]['ttau'], o[5]['ttau']) < TOL_SITE and rel(r[5]['tnu'], o[5]['tnu']) < TOL_SITE
    assert relz(r[5]['nlZ'], o[5]['nlZ']) < TOL_LOGZ


@pytest.mark.parametrize('p,N', RULES)
def test_gf_adf_sweep_bin_sums_against_the_oracle(p, N):
    D, T = 6, 100
    pr = harness.nmf_problem(D, N, T, 410 + 10 * p + N); t = np.arange(1, T + 1.0)
    d = 0.5 * np.ones(1)
    Eft, Varft, _, _, _, out = nagp.gf_ep_modulator_nmf(pr['w'], t, pr['y'], SSHandle(), Mom('likModulatorNMFPower', p_cubature=p), t,
                                                        'matern32', 'matern52', 1, D, N, 0.5, d, 1, nargout=6)
    o = ogf.gf_ep_modulator_nmf(pr['w'], t, pr['y'], None, olik.Mom(olik.LIK_POWER_NMF, p=p), t, 'matern32', 'matern52', 1, D, N, 0.5, d, 1)
    assert rel(Eft, o[0]) < TOL_MEAN and rel(Varft, o[1]) < TOL_MEAN
    assert rel(out['ttau'], o[5]['ttau']) < TOL_SITE and rel(out['tnu'], o[5]['tnu']) < TOL_SITE
    assert relz(out['nlZ'], o[5]['nlZ']) < TOL_LOGZ
