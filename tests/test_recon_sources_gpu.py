"""nagp_reconstruct_sources on the GPU against the NumPy restatement of the experiment scripts' post-processing
(tests/recon_sources_ref.py; experiments/source_sep_piano.m:165-244, noise_reduction_speech.m:142): sampling form to 1e-10, population
form to 1e-12 (the tolerances and the rel() of test_posterior_reconstruction_of_signal_and_amplitudes)."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nagp
from nagp import Mom, SSHandle, harness, _lib as L
from nagp.cubature import gauher, sigma_points
import recon_sources_ref as ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ('Esig', 'Vsig', 'Esrc', 'Vsrc', 'Eenv', 'Eft_mod', 'Varft_mod')
TOL_SAMPLING, TOL_POPULATION = 1e-10, 1e-12
GRID_CAP = 65536            # blocks of the sampling launch (csrc/nagp_api_entry.hpp): longer series take a second round of the grid


def rel(a, b):
    a = np.asarray(a, float); b = np.asarray(b, float)
    assert a.shape == b.shape, (a.shape, b.shape)
    assert np.array_equal(np.isnan(a), np.isnan(b))
    return float(np.nanmax(np.abs(a - b)) / (np.nanmax(np.abs(b)) + 1e-300)) if a.size else 0.0


@pytest.fixture(scope='module', autouse=True)
def _lib(nagp_lib):
    assert nagp_lib.nagp_device_count() >= 1
    return nagp_lib


def link_of(link):
    return (lambda g: np.log(1.0 + np.exp(g))) if link == 'softplus' else np.exp


def tame(Eft, Varft, D, link):
    """usable marginals: positive variances; exp link: keep exp(g) tame as the existing reconstruction test does"""
    Eft = np.array(Eft); Varft = np.maximum(np.abs(Varft), 1e-12)
    if link == 'exp':
        Eft[D:] *= 0.2; Varft[D:] = np.minimum(Varft[D:], 0.5)
    return Eft, Varft


@pytest.fixture(scope='module')
def mixture_run():
    """marginals of a source-separation mixture: three sources of two sub-bands with 1 / 1 / 2 components, T = 200"""
    shapes = [(2, 1), (2, 1), (2, 2)]; k1 = ['matern32'] * 3; k2 = ['matern52'] * 3; T = 200
    # (observation noise 0.1: with the harness default of 1e-4 the mixtures' EP rule diverges on this instance -- in the oracle as well,
    # |Eft| ~ 1e15 after two sweeps -- and the marginals are no input for a reconstruction)
    mp = harness.mixture_problem(shapes, T, 21, k1, k2, w_lik=0.1); t = np.arange(1, T + 1.0)
    r = nagp.gf_ep_mods_nmf_mixture(mp['w'], t, mp['y'], SSHandle(), Mom('likModulatorNMFPower', p_cubature=7), t, k1, k2, 3, 0.75, 0.2, 2, nargout=6)
    W, off = nagp.recon.stack_sources(mp['w'][3])
    assert off == [0, 2, 4, 6] and W.shape == (6, 4) and r[0].shape == (10, T)
    assert np.all(np.isfinite(r[0])) and np.all(np.isfinite(r[1])) and np.max(np.abs(r[0])) < 100.0
    return dict(Eft=r[0], Varft=r[1], W=W, off=off, Ws=mp['w'][3])


@pytest.fixture(scope='module')
def precalcwn_run():
    """marginals of a likModulatorPreCalcwn run (the sqrt-amplitude likelihood), one source, D = 6, N = 3"""
    D, N, T = 6, 3, 200
    pr = harness.nmf_problem(D, N, T, 55, sqrt_amp=True); t = np.arange(1, T + 1.0)
    wn, xn = sigma_points(5, N)
    Eft, Varft = nagp.gf_ep_modulator_nmf(pr['w'], t, pr['y'], SSHandle(), Mom('likModulatorPreCalcwn', wn=wn, xn_unscaled=xn), t,
                                          'matern32', 'matern52', 1, D, N, 0.5, 0.5 * np.ones(2), 2)
    return dict(Eft=Eft, Varft=Varft, W=pr['W'], off=[0, D])


def check_all(Eft, Varft, W, off, link, amp, s=None, seed=2019, rules=(5,), what=''):
    lk = link_of(link); D, N = W.shape
    if s:
        got = nagp.reconstruct_sources(Eft, Varft, W, amplitude=amp, sources=off, link=link, n_samples=s, seed=seed)
        exp = ref.sampling(Eft, Varft, W, off, lk, amp, s, seed)
        for k in KEYS:
            e = rel(got[k], exp[k]); print('%s sampling s=%d %s %s %s: %.2e' % (what, s, link, amp, k, e))
            assert e < TOL_SAMPLING, (k, e)
    gx, gw = gauher(32)
    for p in rules:
        wn, xn = sigma_points(p, N)
        got = nagp.reconstruct_sources(Eft, Varft, W, amplitude=amp, sources=off, link=link, p_cubature=p)
        exp = ref.population(Eft, Varft, W, off, lk, amp, gx, gw, exp_link=(link == 'exp'), wn=wn, xn=xn)
        for k in KEYS:
            e = rel(got[k], exp[k]); print('%s population p=%d %s %s %s: %.2e' % (what, p, link, amp, k, e))
            assert e < TOL_POPULATION, (k, p, e)


@pytest.mark.parametrize('amp', ['sqrt', 'linear'])
@pytest.mark.parametrize('link', ['softplus', 'exp'])
@pytest.mark.parametrize('run', ['mixture', 'precalcwn'])
def test_parity_with_the_restatement_on_marginals_of_real_runs(run, link, amp, mixture_run, precalcwn_run):
    """every output, sampling form with s = 250 and population form with ut5 and a 4-point Gauss-Hermite grid (mvhermgauss)"""
    g = mixture_run if run == 'mixture' else precalcwn_run
    D = g['W'].shape[0]
    Eft, Varft = tame(g['Eft'], g['Varft'], D, link)
    check_all(Eft, Varft, g['W'], g['off'], link, amp, s=250, rules=(5, 4), what=run)


def test_a_list_of_source_matrices_and_equal_blocks_name_the_same_sources(mixture_run):
    g = mixture_run; Eft, Varft = tame(g['Eft'], g['Varft'], 6, 'softplus')
    a = nagp.reconstruct_sources(Eft, Varft, g['W'], sources=g['off'], n_samples=6, seed=3)
    b = nagp.reconstruct_sources(Eft, Varft, g['Ws'], n_samples=6, seed=3)
    c = nagp.reconstruct_sources(Eft, Varft, g['W'], sources=3, n_samples=6, seed=3)
    for k in KEYS:
        assert np.array_equal(a[k], b[k]) and np.array_equal(a[k], c[k]), k


@pytest.mark.parametrize('link', ['softplus', 'exp'])
def test_linear_one_source_mode_is_nagp_reconstruct(link, precalcwn_run):
    g = precalcwn_run; D = 6
    Eft, Varft = tame(g['Eft'], g['Varft'], D, link)
    for s in (250, 0):
        old = nagp.reconstruct_signal(Eft, Varft, g['W'], link=link, n_samples=s, seed=2019)
        new = nagp.reconstruct_sources(Eft, Varft, g['W'], amplitude='linear', link=link, n_samples=s, seed=2019)
        for k in ('Esig', 'Vsig', 'Eft_mod', 'Varft_mod'):
            e = rel(new[k], old[k]); print('s=%d %s %s: %.2e' % (s, link, k, e))
            assert e < 1e-12, (k, s, e)
        assert np.array_equal(new['Esrc'][0], new['Esig']) and np.array_equal(new['Vsrc'][0], new['Vsig'])


def synthetic(D, N, T, seed):
    rng = np.random.default_rng(seed)
    Eft = rng.normal(0, 1, (D + N, T))
    Varft = np.concatenate([rng.uniform(0.05, 0.6, (D, T)), rng.uniform(0.05, 1.0, (N, T))])
    return Eft, Varft


@pytest.mark.parametrize('s', [2, 6, 250, 258])
def test_sample_counts_tail_of_a_block_partial_trip_second_trip(s):
    Eft, Varft = synthetic(3, 2, 5, s); W = np.random.default_rng(9).uniform(0.1, 0.5, (3, 2))
    check_all(Eft, Varft, W, [0, 1, 3], 'softplus', 'sqrt', s=s, rules=(), what='edge')


@pytest.mark.parametrize('amp', ['sqrt', 'linear'])
def test_a_single_time_step(amp):
    Eft, Varft = synthetic(3, 2, 1, 17); W = np.random.default_rng(9).uniform(0.1, 0.5, (3, 2))
    check_all(Eft, Varft, W, [0, 2, 3], 'softplus', amp, s=6, rules=(5,), what='T=1')


def test_series_one_step_longer_than_the_grid():
    T = GRID_CAP + 1
    Eft, Varft = synthetic(2, 1, T, 23); W = np.array([[0.4], [0.3]])
    check_all(Eft, Varft, W, [0, 1, 2], 'softplus', 'sqrt', s=6, rules=(5,), what='T=cap+1')


def test_paper_size_48_subbands_9_modulators_3_sources():
    D, N, T = 48, 9, 8
    Eft, Varft = synthetic(D, N, T, 31); rng = np.random.default_rng(32)
    W, off = nagp.recon.stack_sources([rng.uniform(0.05, 0.3, (16, 3)) for _ in range(3)])
    assert off == [0, 16, 32, 48]
    check_all(Eft, Varft, W, off, 'softplus', 'sqrt', s=100, rules=(5,), what='57')
    check_all(Eft, Varft, W, off, 'softplus', 'linear', s=100, rules=(5,), what='57')


@pytest.mark.parametrize('s', [0, 20])
@pytest.mark.parametrize('amp', ['sqrt', 'linear'])
def test_outputs_are_independent(amp, s):
    Eft, Varft = synthetic(5, 3, 7, 41); W = np.random.default_rng(42).uniform(0.1, 0.5, (5, 3)); off = [0, 2, 5]
    full = nagp.reconstruct_sources(Eft, Varft, W, amplitude=amp, sources=off, n_samples=s, seed=5)
    for sub in (('Eenv',), ('Vsrc',), ('Esig', 'Varft_mod'), ('Vsig', 'Esrc', 'Eft_mod'), KEYS[1:]):
        part = nagp.reconstruct_sources(Eft, Varft, W, amplitude=amp, sources=off, n_samples=s, seed=5, outputs=sub)
        assert set(part) == set(sub)
        for k in sub:
            assert np.array_equal(part[k], full[k]), (k, sub)


@pytest.mark.parametrize('s', [0, 20])
def test_negative_weight_under_sqrt_is_nan_in_its_subband_its_source_and_the_total(s):
    Eft, Varft = synthetic(5, 3, 7, 43); W = np.random.default_rng(44).uniform(0.1, 0.5, (5, 3)); off = [0, 2, 3, 5]
    good = nagp.reconstruct_sources(Eft, Varft, W, sources=off, n_samples=s, seed=5)
    assert all(np.all(np.isfinite(good[k])) for k in KEYS)
    Wb = W.copy(); Wb[:, :] = W; Wb[3, :] = [-5.0, 0.0, 0.0]           # sub-band 3 (source 2): W_d . link(g) < 0 whatever g
    bad = nagp.reconstruct_sources(Eft, Varft, Wb, sources=off, n_samples=s, seed=5)
    assert np.all(np.isnan(bad['Eenv'][3])) and np.all(np.isnan(bad['Esrc'][2])) and np.all(np.isnan(bad['Vsrc'][2]))
    assert np.all(np.isnan(bad['Esig'])) and np.all(np.isnan(bad['Vsig']))
    keep = [0, 1, 2, 4]
    assert np.array_equal(bad['Eenv'][keep], good['Eenv'][keep])
    assert np.array_equal(bad['Esrc'][:2], good['Esrc'][:2]) and np.array_equal(bad['Vsrc'][:2], good['Vsrc'][:2])
    assert np.array_equal(bad['Eft_mod'], good['Eft_mod']) and np.array_equal(bad['Varft_mod'], good['Varft_mod'])
    lin = nagp.reconstruct_sources(Eft, Varft, Wb, amplitude='linear', sources=off, n_samples=s, seed=5)      # the linear kind has no such rule
    assert all(np.all(np.isfinite(lin[k])) for k in KEYS)


@pytest.mark.parametrize('s', [0, 50])
def test_mex_gateway_reconstruct_sources(s, mixture_run, tmp_path):
    """matlab/nagp_mex.c against the mock MEX API: 'reconstruct_sources' with the struct nagp_reconstruct_sources.m builds, on dumped
    marginals; sizes right, values those of the Python call to 1e-12 (tests/c/mex_recon_driver.c)."""
    g = mixture_run; D, N = g['W'].shape
    Eft, Varft = tame(g['Eft'], g['Varft'], D, 'softplus')
    res = nagp.reconstruct_sources(Eft, Varft, g['W'], sources=g['off'], n_samples=s, seed=77)
    gx, gw = gauher(32); wn, xn = sigma_points(5, N)
    arrs = dict(D=[D], N=[N], amp_kind=[1], link_kind=[0], link_shift=[0.0], n_samples=[s], seed=[77], Eft=Eft, Varft=Varft, Wnmf=g['W'],
                gh_x=gx, gh_w=gw, wn=wn, xn_unscaled=xn, **res)
    with open(tmp_path / 'meta.txt', 'w') as fh:
        for k, a in arrs.items():
            a = np.asfortranarray(np.asarray(a, dtype=np.float64)); a.ravel(order='F').tofile(str(tmp_path / (k + '.bin'))); fh.write('%s %d\n' % (k, a.size))
        np.asarray(g['off'], dtype=np.int32).tofile(str(tmp_path / 'source_offsets.bin')); fh.write('source_offsets %d\n' % len(g['off']))
    c = os.path.join(ROOT, 'tests', 'c'); pkg = os.path.join(ROOT, 'nonstationary-audio-gp_amd'); exe = str(tmp_path / 'mex_recon_driver')
    cmd = ['gcc', '-Wall', '-Werror', '-O1', '-std=c99', '-I', os.path.join(ROOT, 'include'), '-I', c, '-o', exe, os.path.join(c, 'mex_recon_driver.c'),
           os.path.join(c, 'mex_mock.c'), os.path.join(ROOT, 'matlab', 'nagp_mex.c'), '-L', pkg, '-lnagp', '-lm', '-Wl,-rpath,' + pkg,
           '-Wl,-rpath,/opt/rocm/lib', '-Wl,-rpath-link,/opt/rocm/lib']
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
