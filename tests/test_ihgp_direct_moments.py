"""Stage 1b of the role-specialised IHGP ADF sweep (nagp_momsp.hpp) in its two forms:

  direct (the product)             sum_d a_d mu_d = v . lk_p,   sum_d a_d^2 s2_d = lk_p' Q lk_p      (msr_stage1b_direct;
                                   ihgp_adf8_kernel, at seven components ihgp_adf8b_kernel<7, false>)
  tables (NAGP_IH_TABLES=1)        the same two numbers as centre + deviations: s0 + sum ve, q0 + sum t1 + cross terms (msp_stage1b;
                                   ihgp_adf8b_kernel<CD, true>)

with Q = W' diag(s2) W, v = W' mu and lk_p the link values at the coordinates of sigma point p (likModulatorNMFPower.m:44-47).

CPU part: the two formulas and the reference's literal one in NumPy on the sigma points of ut7 in six dimensions.
GPU part (-m gpu): the kernel in both forms against the NumPy oracle and against each other, at the tolerances tests/test_gpu_parity.py
applies to these sweeps."""
import numpy as np
import pytest

import nagp
from nagp import cubature, harness, Mom, SSHandle
from oracle import ihgp as oih, lik as olik

from test_gpu_parity import TOL_MEAN, TOL_LOGZ, rel, relz


def test_direct_and_table_form_of_the_per_point_moments_are_the_same_quantity():
    """CD = 6, D = 32, the 305 points of ut7: seeded random W >= 0, s2 > 0, mu, link values > 0.  The literal form
    (a = W lk_p; a.mu, a^2.s2), the direct form and the table form agree to 1e-13 relative at every point.  The link values are
    drawn within a factor of two of the centre's, so the table form's cancellation (deviations of both signs) amplifies rounding
    by at most 16; each form is a few dozen operations of 1.1e-16.  (mu has both signs, so the first sum can be arbitrarily close to
    zero: its differences are taken relative to sum_d a_d |mu_d|, the size of its terms; the second sum has positive terms only.)"""
    CD, D = 6, 32
    rng = np.random.default_rng(20260)
    _, xn = cubature.utp_ws(7, CD)
    xd = np.unique(xn)                                                  # distinct coordinate values; the centre's is 0
    code = np.searchsorted(xd, xn)                                      # (CD, n_pts)
    c0 = int(np.searchsorted(xd, 0.0))
    assert xd[c0] == 0.0 and xn.shape == (CD, 305) and np.max(np.sum(code != c0, axis=0)) <= 4
    for _ in range(20):
        W = rng.uniform(0.0, 1.0, (D, CD)); s2 = rng.uniform(0.01, 2.0, D); mu = rng.normal(0.0, 1.0, D)
        l0 = rng.uniform(0.5, 2.0, CD)
        link = l0[:, None] * rng.uniform(0.5, 2.0, (CD, xd.size)); link[:, c0] = l0      # link table [j][c]
        lk = link[np.arange(CD)[:, None], code]                        # (CD, n_pts)
        # literal
        a = W @ lk
        sam_ref, sa2_ref = mu @ a, s2 @ (a * a)
        # direct
        Q = W.T @ (s2[:, None] * W); v = W.T @ mu
        sam_dir = v @ lk
        sa2_dir = np.einsum('jp,jk,kp->p', lk, Q, lk)
        # tables: e, t1 = e (Q_jj e + 2 (Q l0)_j), ve = v_j e, q0, s0 and the cross terms of the non-centre coordinates
        e = link - l0[:, None]
        t1 = e * (np.diag(Q)[:, None] * e + 2.0 * (Q @ l0)[:, None]); ve = v[:, None] * e
        q0, s0 = l0 @ Q @ l0, v @ l0
        sam_tab = np.empty(xn.shape[1]); sa2_tab = np.empty(xn.shape[1])
        for p in range(xn.shape[1]):
            nz = [j for j in range(CD) if code[j, p] != c0]
            sam_tab[p] = s0 + sum(ve[j, code[j, p]] for j in nz)
            cr = sum(2.0 * Q[j, j2] * e[j, code[j, p]] * e[j2, code[j2, p]] for i, j in enumerate(nz) for j2 in nz[i + 1:])
            sa2_tab[p] = q0 + sum(t1[j, code[j, p]] for j in nz) + cr
        scale_m = np.abs(mu) @ a                                        # sum_d a_d |mu_d|: the size of the terms of the first sum
        for got in (sam_dir, sam_tab):
            assert np.max(np.abs(got - sam_ref) / scale_m) < 1e-13
        for got in (sa2_dir, sa2_tab):
            assert np.max(np.abs(got - sa2_ref) / sa2_ref) < 1e-13
        assert np.max(np.abs(sa2_dir - sa2_tab) / sa2_ref) < 1e-13 and np.max(np.abs(sam_dir - sam_tab) / scale_m) < 1e-13


P_OF_CD = {1: 9, 3: 9, 6: 7, 7: 5}      # a rule the role layout serves in that dimension (tests/test_gpu_bin_sums.py)


def _both_forms(D, N, T, itts, seed, monkeypatch, capfd):
    """One call per form through the public interface; NAGP_STAMPS makes the plan say which kernel it chose."""
    p = P_OF_CD[N]
    pr = harness.nmf_problem(D, N, T, seed, 'constraints'); t = np.arange(1, T + 1.0)
    d = np.array([0.5, 0.4])[:itts]
    res = {}
    monkeypatch.setenv('NAGP_STAMPS', '1')
    for form in ('direct', 'tables'):
        monkeypatch.delenv('NAGP_IH_TABLES', raising=False)
        if form == 'tables': monkeypatch.setenv('NAGP_IH_TABLES', '1')
        capfd.readouterr()
        res[form] = nagp.ihgp_ep_modulator_nmf(pr['w'], t, pr['y'], SSHandle(), Mom('likModulatorNMFPower', p_cubature=p), t,
                                               'matern32', 'matern52', 1, D, N, 0.5, d, itts, nargout=6)
        assert 'role-specialised waves 1' in capfd.readouterr().err, (form, 'the plan did not choose ihgp_adf8_kernel')
    monkeypatch.delenv('NAGP_IH_TABLES', raising=False); monkeypatch.delenv('NAGP_STAMPS', raising=False)
    ref = oih.ihgp_ep_modulator_nmf(pr['w'], t, pr['y'], None, olik.Mom(olik.LIK_POWER_NMF, p=p), t, 'matern32', 'matern52', 1, D, N, 0.5, d, itts)
    figs = {}
    for name, a, b in (('direct vs oracle', res['direct'], ref), ('tables vs oracle', res['tables'], ref), ('direct vs tables', res['direct'], res['tables'])):
        figs[name] = (rel(a[0], b[0]), rel(a[1], b[1]), relz(a[5]['nlZ'], b[5]['nlZ']))
        print('D=%d N=%d T=%d sweeps=%d %s: Eft %.2e Varft %.2e nlZ %.2e' % ((D, N, T, itts, name) + figs[name]))
    for name, (fe, fv, fz) in figs.items():
        assert fe < TOL_MEAN and fv < TOL_MEAN and fz < TOL_LOGZ, (name, fe, fv, fz)


@pytest.mark.gpu
@pytest.mark.parametrize('D', [8, 32])
@pytest.mark.parametrize('N', [1, 3, 6, 7])
def test_role_kernel_direct_and_table_form_against_the_oracle(N, D, nagp_lib, monkeypatch, capfd):
    """CD in {1, 3, 6, 7} x D in {8, 32}, T = 496 (a whole number of I/O rings of 16, 8 or 4 steps), one ADF sweep."""
    _both_forms(D, N, 496, 1, 5200 + 10 * D + N, monkeypatch, capfd)


@pytest.mark.gpu
def test_role_kernel_both_forms_with_a_partial_last_ring(nagp_lib, monkeypatch, capfd):
    """T = 503: the last I/O ring of the sweep holds 7 (ring of 16 or 8) or 3 (ring of 4) steps."""
    _both_forms(32, 6, 503, 1, 5601, monkeypatch, capfd)


@pytest.mark.gpu
def test_role_kernel_both_forms_with_a_second_launch_continuing_the_sweep(nagp_lib, monkeypatch, capfd):
    """Two EP sweeps: the second sweep's filter pass launches the kernel for the last step only (k_start = T - 1 > 0), continuing from
    the filtered mean and R of step T - 2."""
    _both_forms(8, 3, 500, 2, 5602, monkeypatch, capfd)
