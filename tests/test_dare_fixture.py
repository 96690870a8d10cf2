"""CPU: the infinite-horizon look-up tables of 6- and 8-state sub-band blocks against a 60-digit solution of the same equations.

tests/golden/dare_sixeight_states.npz (tools/make_dare_fixture.py) holds, per block, the f64 (A, Q, h) the product forms and, at the
32 knots ro = logspace(-2, 4, 32), the predictive DARE solution PP, the smoother gain G and the smoothed covariance PS2 solved in
mpmath at 60 digits and rounded to f64.  Both table builders -- the host's batched doubling (nagp/ihgp_tables.py) and the oracle's
SciPy solvers (oracle/ihgp.py) -- are held to it block by block, on the 200-row tables, against the knot rows pushed through the
same interpolation (oracle.ihgp.neqinterp_matrix); error = max-abs difference over max-abs of the fixture, for PP, G and PS2 apart.

Measured on the fixture's 19 blocks (the worst block of each size):

                         plain QQ = P - G PP G', SciPy's PP as it comes      QQ as a PSD sum, PP after Newton steps
                         PP        G         PS2                                PP        G         PS2
  host, 6 states         1.0e-12   3.5e-12   3.1e-6                             5.7e-14   5.2e-12   4.6e-13
  host, 8 states         6.6e-11   1.6e-10   2.1e-3                             1.1e-13   1.9e-10   2.2e-11
  SciPy, 6 states        4.4e-9    2.3e-10   4.3e-7      (oracle, refined)      8.3e-14   5.3e-12   5.6e-13
  SciPy, 8 states        3.0e-6    2.5e-6    1.3e-4      (oracle, refined)      1.2e-13   2.5e-10   2.2e-11
  3-state modulators     host <= 3.1e-13 in every table, SciPy's (unchanged for blocks of up to 4 states) <= 9.6e-11

The host's doubling was the closer solver for PP and G at every block and SciPy's QZ solver the worse one (3e-6 on 8-state
blocks), but both lost PS2: the smoother's QQ = P - G PP G' is 1e-12 .. 1e-7 of P on these blocks, and the subtraction in f64
turned a 1e-11 error of PP into 2e-3 of PS2 (even the exact PP and G, rounded to f64, give 1.5e-6 through that formula).  Both
builders now form QQ as a sum of positive semi-definite terms equal to it in exact arithmetic and refine PP by Newton steps (the
oracle for blocks of more than 4 states only); the remaining 2e-10 of G is the f64 solve with A P A' + Q, conditioned 1e12.
"""
import importlib.util
import os

import numpy as np
import pytest
import scipy.linalg as sla

from nagp import harness, ihgp_tables, ss as pss
from oracle import ihgp as oih, ss as oss, gf_ep as ogf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, 'tests', 'golden', 'dare_sixeight_states.npz')
TOL_TABLE = 1e-9            # max-abs error over max-abs of the fixture, PP / G / PS2 of every block
NAMES = ('PP', 'G', 'PS2')


def _fixture():
    return np.load(FIXTURE)


def _problem(g, q):
    """Problem q of the fixture: its blocks' ids, the block-diagonal A, Q, H, the block starts and the fixture's 200-row tables
    (the knot rows through the interpolation of ihgp_ep_modulator_nmf.m:131) per block."""
    ids = np.where(g['block_problem'] == q)[0]
    sizes = [int(g['block_size'][i]) for i in ids]
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    hv = np.array([float(g['h_%d' % i]) for i in ids])
    A = sla.block_diag(*[g['A_%d' % i] for i in ids]); Q = sla.block_diag(*[g['Q_%d' % i] for i in ids])
    H = np.zeros((len(ids), off[-1])); H[np.arange(len(ids)), off[:-1]] = hv
    U = oih.neqinterp_matrix(g['ro'], np.logspace(-2, 4, 200))
    tabs = [{k: U @ g['%s_%d' % (k, i)] for k in NAMES} for i in ids]
    return ids, sizes, off, hv, A, Q, H, tabs


def _host_tables(A, Q, off, hv, sizes):
    r, PP, ppo, PG, pgo = ihgp_tables.build_tables(A, Q, off, hv)
    out = []
    for n, b in enumerate(sizes):
        pg = PG[pgo[n]:pgo[n] + 400 * b * b].reshape(200, -1)
        out.append({'PP': PP[ppo[n]:ppo[n] + 200 * b * b].reshape(200, -1), 'G': pg[:, b * b:], 'PS2': pg[:, :b * b]})
    return out


def _oracle_tables(A, Q, H, off, sizes):
    r, PPl, PPo, rol = oih.forward_tables(A, Q, H, off)
    PGl = oih.smoother_tables(A, Q, H, off, r, PPo, rol)
    return [{'PP': PPl[n], 'G': PGl[n][:, b * b:], 'PS2': PGl[n][:, :b * b]} for n, b in enumerate(sizes)]


def _err(x, ref):
    assert x.shape == ref.shape, (x.shape, ref.shape)          # no knot dropped
    return float(np.abs(x - ref).max() / np.abs(ref).max())


def _tool():
    spec = importlib.util.spec_from_file_location('make_dare_fixture', os.path.join(ROOT, 'tools', 'make_dare_fixture.py'))
    mod = importlib.util.module_from_spec(spec); spec.loader.exec_module(mod)
    return mod


def test_fixture_inputs_are_the_products_model():
    """A, Q, h of every block are what the product's entry points form for the stored recipe (balance, lti_disc, Q = (Q + Q')/2),
    and the fixture covers what it claims: 6- and 8-state sub-band blocks, the 3-state modulators beside them, both ends of the
    length-scale range of CONSTRAINTS_DEMO."""
    g = _fixture(); tool = _tool()
    assert list(g['problem_recipe']) == [p[0] for p in tool.PROBLEMS] and list(g['problem_kernel1']) == [p[1] for p in tool.PROBLEMS]
    assert np.array_equal(g['ro'], np.logspace(-2, 4, 32)) and int(g['dps']) >= 50
    for q, (recipe, k1) in enumerate(tool.PROBLEMS):
        blk, A, Q = tool.product_blocks(recipe, k1)
        ids = np.where(g['block_problem'] == q)[0]
        assert [int(g['block_size'][i]) for i in ids] == list(blk.sizes)
        for n, i in enumerate(ids):
            o, e = blk.offsets[n], blk.offsets[n + 1]
            assert np.allclose(g['A_%d' % i], A[o:e, o:e], rtol=1e-13, atol=0) and np.allclose(g['Q_%d' % i], Q[o:e, o:e], rtol=1e-12, atol=0)
            assert float(g['h_%d' % i]) == blk.h_val[n]
    assert sorted(set(int(b) for b in g['block_size'])) == [3, 6, 8]
    assert sorted(g['edge_params'][:, 1]) == sorted(harness.CONSTRAINTS_DEMO(3)[1])


def test_fixture_solves_its_equations():
    """At every knot, in f64: the DARE residual and G (A P A' + Q) = P A' vanish to rounding of the fixture's size, PS2 is symmetric
    positive semi-definite."""
    g = _fixture()
    for i in range(g['block_size'].size):
        b = int(g['block_size'][i]); A = g['A_%d' % i]; Q = g['Q_%d' % i]; hv = float(g['h_%d' % i])
        for j, r in enumerate(g['ro']):
            PP, G, PS2 = (g['%s_%d' % (k, i)][j].reshape(b, b, order='F') for k in NAMES)
            S = hv * hv * PP[0, 0] + r; K = PP[:, 0] * hv / S
            res = A @ (PP - S * np.outer(K, K)) @ A.T + Q - PP
            assert np.abs(res).max() < 1e-13 * np.abs(PP).max(), (i, j)
            P = PP - r * np.outer(K, K)
            assert np.abs(G @ (A @ P @ A.T + Q) - P @ A.T).max() < 1e-13 * np.abs(P).max(), (i, j)
            assert np.allclose(PS2, PS2.T, rtol=0, atol=1e-15 * np.abs(PS2).max()) and np.linalg.eigvalsh(PS2).min() > -1e-12 * np.abs(PS2).max()


@pytest.mark.parametrize('q', range(5))
def test_host_and_oracle_tables_meet_the_multiprecision_fixture(q, capsys):
    """Both builders' 200-row tables against the fixture's (see the module docstring for the figures); prints the per-block table."""
    g = _fixture()
    ids, sizes, off, hv, A, Q, H, ref = _problem(g, q)
    host = _host_tables(A, Q, off, hv, sizes)
    orc = _oracle_tables(A, Q, H, off, sizes)
    rows = []
    for n, i in enumerate(ids):
        eh = [_err(host[n][k], ref[n][k]) for k in NAMES]; eo = [_err(orc[n][k], ref[n][k]) for k in NAMES]
        rows.append((i, sizes[n], eh, eo))
    with capsys.disabled():
        print('\n%s %s:  block  states |  host PP / G / PS2          |  oracle PP / G / PS2' % (g['problem_recipe'][q], g['problem_kernel1'][q]))
        for i, b, eh, eo in rows:
            print('   %2d  %d |  %.1e %.1e %.1e  |  %.1e %.1e %.1e' % ((i, b) + tuple(eh) + tuple(eo)))
    for i, b, eh, eo in rows:
        assert max(eh) < TOL_TABLE, ('host', i, b, eh)
        assert max(eo) < TOL_TABLE, ('oracle', i, b, eo)


@pytest.mark.parametrize('k1', ['matern52', 'matern72'])
def test_ihgp_tables_of_six_and_eight_state_blocks_meet_the_multiprecision_fixture(k1):
    """Sub-band blocks of six and eight states (steady-state covariances conditioned ~1e8 / ~1e12), the tables as the product builds
    them from the problem's hyper-parameters: the host's and the oracle's against the fixture at 1e-9 each, and the host's PP solving
    the predictive DARE to 1e-11 of its size at the two grid points that are knots of the solver (the rest is interpolated)."""
    g = _fixture()
    q = [n for n in range(g['problem_recipe'].size) if (g['problem_recipe'][n], g['problem_kernel1'][n]) == ('demo_nmf', k1)][0]
    ids, sizes, off, hv, A0, Q0, H0, ref = _problem(g, q)
    pr = harness.nmf_problem(3, 2, 5, int(g['seed']), kernel1=k1)
    lik, p1, p2, W = oss.unpack_log(pr['w'], 1, 3, 2)
    model = ogf.assemble(lik, p1, p2, W, k1, 'matern52', True, True)
    ilist, r, PPl, PGl = oih.build_tables(model)
    blk = pss.balance_blocks(pss.ss_blocks_nmf(p1, p2, k1, 'matern52'))
    A, Q, P = pss.discretise(blk, symmetrize_Q=True)
    r2, PP, ppo, PG, pgo = ihgp_tables.build_tables(A, Q, blk.offsets, blk.h_val)
    b0 = {'matern52': 6, 'matern72': 8}[k1]
    assert np.allclose(r, r2) and list(blk.sizes) == [b0] * 3 + [3, 3] and list(ilist) == list(blk.offsets)
    for n in range(5):
        b = blk.sizes[n]; o = blk.offsets[n]
        pp = PP[ppo[n]:ppo[n] + 200 * b * b].reshape(200, -1); pg = PG[pgo[n]:pgo[n] + 400 * b * b].reshape(200, -1)
        for tab in ({'PP': pp, 'G': pg[:, b * b:], 'PS2': pg[:, :b * b]}, {'PP': PPl[n], 'G': PGl[n][:, b * b:], 'PS2': PGl[n][:, :b * b]}):
            assert all(_err(tab[k], ref[n][k]) < TOL_TABLE for k in NAMES), (n, [_err(tab[k], ref[n][k]) for k in NAMES])
        Ab = A[o:o + b, o:o + b]; Qb = Q[o:o + b, o:o + b]; h = np.zeros((1, b)); h[0, 0] = blk.h_val[n]
        for gi in (0, 199):     # residual of the predictive DARE  P = A (P - P h' (h P h' + r)^-1 h P) A' + Q
            Pm = pp[gi].reshape(b, b, order='F')
            K = Pm @ h.T / (h @ Pm @ h.T + r2[gi])
            res = Ab @ (Pm - K @ h @ Pm) @ Ab.T + Qb - Pm
            assert np.abs(res).max() < 1e-11 * np.abs(Pm).max(), (n, gi)
