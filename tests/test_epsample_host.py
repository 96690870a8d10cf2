"""nagp_ep_sample (joint posterior draws of a full-covariance EP run) without a GPU: the export and its binding, every refusal of the
entry point (all decided on the host before any device call), and the NumPy restatement the GPU tests compare with
(tests/epsample_ref.py) pinned to the oracle's run_predict -- the filtered and smoothed moments at 1e-12, and the exact law: with
the caller's normals set to zero and to the unit vectors the restatement returns the affine map x = m + L z, and L L' must be the
joint covariance of the oracle's smoother (PS_k on the diagonal, G_k PS_{k+1} beside it, products of gains further out)."""
import ctypes
import glob
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nagp
from nagp import _lib as L, harness, Mom, SSHandle
from oracle import gf_ep as ogf, lik as olik, ss as oss
import epsample_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EUNSUPPORTED, ENOMEM = -1, -2, -4


def test_entry_point_is_exported_and_bound():
    path = nagp.build()
    out = subprocess.run(['nm', '-D', '--defined-only', path], capture_output=True, text=True).stdout
    syms = set(re.findall(r' T (nagp_[a-z0-9_]+)', out))
    assert {'nagp_ep_sample', 'nagp_ep_sample_timings'} <= syms
    assert {'nagp_ep_sample', 'nagp_ep_sample_timings'} <= set(L.EXPORTS)
    fn = L.lib().nagp_ep_sample
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 16
    assert callable(nagp.gf_ep_sample) and callable(nagp.Plan.sample)


# ---- refusals through ctypes (the plain C caller below walks the same list on exactly-sized heap blocks)
def _call(S=4, M=2, T=6, n=3, off=None, null=(), outs=('X', 'F', 'M'), sig=None, tt=2.0, tn=0.1, D=1, N=1, model_null=()):
    Sa = max(S, 1); Ma = max(M, 1)
    off = np.asarray([0, 2, 4] if off is None else off, np.int32)
    A = L.f64(0.9 * np.eye(Sa)); Q = L.f64(0.19 * np.eye(Sa)); P = L.f64(np.eye(Sa)); hv = np.ones(Ma)
    keep = dict(A=A, Q=Q, Pinf=P, h_val=hv)
    md = L.Model(S=S, M=M, D=D, N=N, block_offsets=None if 'off' in model_null else off.ctypes.data_as(L.c_ip),
                 **{k: L.dptr(None if k in model_null else v) for k, v in keep.items()}, Wnmf=None, lik_param=0.0)
    Tn = 6
    arrs = dict(ttau=np.full((Ma, Tn), tt, order='F'), tnu=np.full((Ma, Tn), tn, order='F'), y=np.zeros(Tn))
    p = {k: L.dptr(None if k in null else v) for k, v in arrs.items()}
    na = max(n, 1)
    X = np.zeros((na, Tn, Sa)); F = np.zeros((na, Tn, Ma)); Sd = np.zeros((na, Tn)); MS = np.zeros((Sa, Tn), order='F')
    sg = None
    if sig is not None:
        W = L.f64(np.full((max(D, 1), max(N, 1)), 0.3)); keep['W'] = W
        sg = L.EpSampleSig(Wnmf=L.dptr(None if sig.get('null') else W), amp_kind=sig.get('amp', 0), link_kind=sig.get('link', 0), link_shift=sig.get('shift', 0.0))
    return L.lib().nagp_ep_sample(None if 'model' in null else ctypes.byref(md), p['ttau'], p['tnu'], p['y'], T, 0, n, 7, None,
                                  ctypes.byref(sg) if sg is not None else None, L.dptr(X if 'X' in outs else None), L.dptr(F if 'F' in outs else None),
                                  L.dptr(Sd if 'S' in outs else None), L.dptr(MS if 'M' in outs else None), None, 0)


@pytest.mark.parametrize('kw', [dict(null=('model',)), dict(null=('ttau',)), dict(null=('tnu',)), dict(null=('y',)), dict(model_null=('off',)),
                                dict(model_null=('A',)), dict(model_null=('Q',)), dict(model_null=('Pinf',)), dict(model_null=('h_val',))])
def test_null_inputs_are_refused_on_the_host(kw):
    assert _call(**kw) == EINVAL
    assert b'null' in L.lib().nagp_last_error()


@pytest.mark.parametrize('kw', [dict(T=0), dict(T=-1), dict(n=0), dict(n=-2), dict(S=0), dict(M=0), dict(off=[0, 0, 4]), dict(off=[0, 2, 3]), dict(off=[1, 2, 4]),
                                dict(tt=-1.0), dict(tt=float('nan')), dict(tt=float('inf')), dict(tn=float('nan')), dict(tn=float('-inf')),
                                dict(outs=()), dict(outs=('X', 'S')), dict(outs=('S',), sig=dict(null=True)), dict(outs=('S',), sig=dict(amp=2)),
                                dict(outs=('S',), sig=dict(link=5)), dict(outs=('S',), sig=dict(shift=float('nan'))), dict(outs=('S',), sig=dict(), D=2, N=1)])
def test_bad_sizes_sites_outputs_and_signal_options_are_refused_on_the_host(kw):
    assert _call(**kw) == EINVAL


def test_shapes_beyond_the_kernels_and_the_budget_are_refused_on_the_host(monkeypatch):
    assert _call(S=9, M=1, off=[0, 9]) == EUNSUPPORTED and b'states' in L.lib().nagp_last_error()          # a block of nine states
    assert _call(S=81, M=81, off=list(range(82))) == EUNSUPPORTED and b'S <= 80' in L.lib().nagp_last_error()   # one above the ceiling (nothing is read)
    assert _call(T=1 << 29) == ENOMEM and b'budget' in L.lib().nagp_last_error()                           # 8 T 2 S^2 = 128 GiB > 48 GiB
    monkeypatch.setenv('NAGP_EPS_BUDGET_MB', '1')
    assert _call(T=5000) == ENOMEM and b'checkpoint' in L.lib().nagp_last_error()
    ms = np.ones(3)
    assert L.lib().nagp_ep_sample_timings(L.dptr(ms)) == 0 and not ms.any()                                # a refused call reports no time
    assert L.lib().nagp_ep_sample_timings(None) == EINVAL


def test_argument_checks_in_plain_c():
    """tests/c/abi_ep_sample_errors.c: a stand-alone C program on exactly-sized heap blocks against libnagp_asan.so (the host code of the C
    ABI built with AddressSanitizer), on the CPU only: every invalid call returns its status and ASan reports nothing."""
    lib = nagp.build(asan=True)
    clang = '/opt/rocm/lib/llvm/bin/clang'
    rt = glob.glob('/opt/rocm/lib/llvm/lib/clang/*/lib/linux') + glob.glob('/opt/rocm/lib/llvm/lib/clang/*/lib/x86_64-unknown-linux-gnu')
    with tempfile.TemporaryDirectory() as td:
        exe = os.path.join(td, 'abi_ep_sample_errors')
        r = subprocess.run([clang, '-fsanitize=address', '-shared-libsan', '-g', '-O1', '-std=c99', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'include'),
                            '-o', exe, os.path.join(ROOT, 'tests', 'c', 'abi_ep_sample_errors.c'), lib, '-lm', '-Wl,-rpath,/opt/rocm/lib',
                            '-Wl,-rpath-link,/opt/rocm/lib'] + ['-Wl,-rpath,' + d for d in rt], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        env = dict(os.environ, ASAN_OPTIONS='detect_leaks=0:abort_on_error=0:exitcode=66', LD_LIBRARY_PATH=':'.join(rt + [os.environ.get('LD_LIBRARY_PATH', '')]))
        r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
        assert r.returncode == 0 and 'all error paths returned their status' in r.stdout, r.stdout + r.stderr
        assert 'AddressSanitizer' not in r.stderr, r.stderr


def test_device_block_and_budget_rule_on_the_host_under_the_sanitizers(tmp_path):
    """tests/c/eps_layout_check.cpp: eps_block against its hand-chained offsets for every combination of the optional parts, and the
    budget rule of include/nagp.h against the block it must cover (a stand-alone program, host code only)"""
    exe = str(tmp_path / 'eps_layout_check')
    r = subprocess.run(['c++', '-std=c++17', '-O1', '-g', '-Wall', '-Werror', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined', '-I',
                        os.path.join(ROOT, 'nonstationary-audio-gp_amd', 'csrc'), '-o', exe, os.path.join(ROOT, 'tests', 'c', 'eps_layout_check.cpp')],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60, env=dict(os.environ, ASAN_OPTIONS='detect_leaks=1:exitcode=66'))
    assert r.returncode == 0 and 'the block and the budget rule of nagp_ep_sample are as written out' in r.stdout, r.stdout + r.stderr
    assert 'Sanitizer' not in r.stderr and 'runtime error' not in r.stderr, r.stderr


def test_python_wrappers_check_their_arguments_and_fail_loudly_without_a_gpu(nagp_lib):
    D, N, T = 3, 2, 12
    pr = harness.nmf_problem(D, N, T, 1)
    t = np.arange(1, T + 1.0)
    out = dict(ttau=np.ones((D + N, T)), tnu=np.zeros((D + N, T)))
    args = (pr['w'], t, pr['y'], SSHandle(), 'matern32', 'matern52', 1, D, N)
    with pytest.raises(ValueError, match='ttau and tnu'):
        nagp.gf_ep_sample(*args, dict(ttau=np.ones((D + N, T + 1)), tnu=np.zeros((D + N, T + 1))), 2)
    with pytest.raises(ValueError, match='n_draws x T x S'):
        nagp.gf_ep_sample(*args, out, 2, z=np.zeros((2, T, 3)))
    with pytest.raises(ValueError, match='amp must be'):
        nagp.gf_ep_sample(*args, out, 2, signal=dict(amp='cubic'))
    with pytest.raises(nagp.NagpError, match=r'\(-1\)'):
        nagp.gf_ep_sample(*args, out, 0)
    with pytest.raises(nagp.NagpError, match=r'\(-1\).*ttau'):
        nagp.gf_ep_sample(*args, dict(ttau=-np.ones((D + N, T)), tnu=np.zeros((D + N, T))), 2)
    if nagp_lib.nagp_device_count() < 1:               # the library's own view: torch may miss a device that libnagp opened first in this process
        with pytest.raises(nagp.NagpError):
            nagp.gf_ep_sample(*args, out, 2, signal=Mom('likModulatorNMFPower', p_cubature=5))


# ---- the restatement against the oracle
def run_case(D, N, T, itts, gaps=(), kernel1='matern32', kernel2='matern52', seed=42, p=5, all_missing=False):
    pr = harness.nmf_problem(D, N, T, seed, kernel1=kernel1, kernel2=kernel2)
    lik, p1, p2, W = oss.unpack_log(pr['w'], 1, D, N)
    model = ogf.assemble(lik, p1, p2, W, kernel1, kernel2, False)
    y = pr['y'].copy()
    for a, b in gaps:
        y[a:b] = np.nan
    if all_missing:
        y[:] = np.nan
    res = ogf.run_predict(model, y, olik.Mom(olik.LIK_POWER_NMF, p=p), 0.5, 0.5 * np.ones(itts), itts)
    return model, y, res, False


def run_case_plain(T, itts):
    """gf_ep_modulator: one modulator per sub-band, balanced, predicts at the first step"""
    c = harness.cfg1(T, 5)
    w = c['w']; param = np.exp(w[1:]); D = c['D']
    model = ogf.assemble(w[:1], param[:3 * D], param[3 * D:], None, c['kernel1'], c['kernel2'], balance=True)
    mom = olik.Mom(olik.LIK_POWER, p=5)
    mom7 = lambda hyp, mu, s2, Wn, a, yy, k: mom(hyp, mu, s2, None, a, yy, k)
    y = c['y'].copy(); y[7:12] = np.nan
    res = ogf.run_predict(model, y, mom7, 0.5, 0.3 * np.ones(itts), itts, predict_at_k1=True)
    return model, y, res, True


CASES = {'T60_gap_2sweeps': lambda: run_case(3, 2, 60, 2, [(20, 35)]), 'T60_1sweep_nan_ends': lambda: run_case(3, 2, 60, 1, [(0, 1), (59, 60)]),
         'T1': lambda: run_case(3, 2, 1, 2), 'T2': lambda: run_case(3, 2, 2, 2), 'T3': lambda: run_case(3, 2, 3, 1),
         'plain_predict_at_k1': lambda: run_case_plain(30, 2), 'all_missing': lambda: run_case(3, 2, 20, 2, all_missing=True)}


def rel(a, b):
    a = np.asarray(a, float); b = np.asarray(b, float)
    assert a.shape == b.shape and not np.any(np.isnan(a)) and not np.any(np.isnan(b))
    return float(np.max(np.abs(a - b)) / (np.max(np.abs(b)) + 1e-300))


@pytest.mark.parametrize('name', sorted(CASES))
def test_restatement_reproduces_the_oracles_filtered_and_smoothed_moments(name):
    model, y, res, pk1 = CASES[name]()
    md = ref.model_of(model['A'], model['Q'], model['Pinf'], model['H'])
    X, F, Sd, MS, cnt, parts = ref.sample(md, res['ttau'], res['tnu'], y, pk1, 1, 3)
    figs = dict(MF=rel(parts['MF'], res['MF']), PF=rel(parts['PF'], res['PF']))
    if name != 'all_missing':
        figs['MS'] = rel(MS, res['MS'])
    else:
        assert not MS.any() and not res['MS'].any()                                  # the prior: MS = 0
    print(name, '  '.join('%s %.1e' % kv for kv in figs.items()), 'counters', cnt)
    assert max(figs.values()) < 1e-12, figs
    assert not cnt.any() and not res['counters']                                     # no jitter retry, no clamped pivot: a condition
    assert np.array_equal(F, np.einsum('ms,nst->nmt', ref.dense_H(md), X))


def exact_law(model, y, res, pk1):
    """the affine map x = m + L z of the restatement from z = 0 and the S T unit vectors; (m, L L' as T x T blocks of S x S)"""
    md = ref.model_of(model['A'], model['Q'], model['Pinf'], model['H'])
    S = model['A'].shape[0]; T = y.size
    z = np.zeros((S * T + 1, T, S))
    for k in range(T):
        for j in range(S):
            z[1 + k * S + j, k, j] = 1.0
    X, _, _, MS, cnt, _ = ref.sample(md, res['ttau'], res['tnu'], y, pk1, S * T + 1, 0, z=z)
    m = X[0]
    Lmap = (X[1:] - m[None]).transpose(2, 1, 0).reshape(T * S, T * S)                # rows (k, state), columns the unit vectors
    assert np.array_equal(m, MS)
    return m, (Lmap @ Lmap.T).reshape(T, S, T, S).transpose(0, 2, 1, 3), cnt


def smoother_gains(model, res):
    A, Q = model['A'], model['Q']; T = res['PF'].shape[0]
    G = []
    for k in range(T - 1):
        PSkp = A @ res['PF'][k] @ A.T + Q
        G.append(np.linalg.solve(PSkp.T, (res['PF'][k] @ A.T).T).T)
    return G


def test_exact_law_of_the_chain_is_the_law_of_the_oracles_smoother():
    """T = 8, D/N = 3/2 (S = 18): 144 unit vectors.  Cov(x_k, x_l) = G_k G_{k+1} .. G_{l-1} PS_l for k <= l, at 1e-10 of the largest entry
    (the restatement alone stays near 1e-13)."""
    model, y, res, pk1 = run_case(3, 2, 8, 2, [(3, 5)])
    m, C, cnt = exact_law(model, y, res, pk1)
    T = 8; PS = res['PS']; G = smoother_gains(model, res)
    scale = np.max(np.abs(PS)); worst = dict(mean=rel(m, res['MS']), diag=0.0, lag1=0.0, far=0.0)
    for l in range(T):
        cov = PS[l]
        for k in range(l, -1, -1):
            if k < l:
                cov = G[k] @ cov
            key = 'diag' if k == l else ('lag1' if k == l - 1 else 'far')
            worst[key] = max(worst[key], float(np.max(np.abs(C[k, l] - cov)) / scale))
    print('exact law: ' + '  '.join('%s %.1e' % kv for kv in worst.items()))
    assert worst['mean'] < 1e-12 and max(worst['diag'], worst['lag1'], worst['far']) < 1e-10, worst
    assert not cnt.any()


def test_with_every_step_missing_the_law_is_the_priors():
    model, y, res, pk1 = run_case(3, 2, 8, 2, all_missing=True)
    m, C, cnt = exact_law(model, y, res, pk1)
    Pinf = model['Pinf']; A = model['A']
    assert not m.any() and not cnt.any()
    worst = 0.0
    for k in range(8):
        cov = Pinf
        for l in range(k, 8):                                                       # Cov(x_k, x_l) = Pinf (A')^(l-k)
            worst = max(worst, float(np.max(np.abs(C[k, l] - cov)) / np.max(np.abs(Pinf))))
            cov = cov @ A.T
    print('prior law: %.1e' % worst)
    assert worst < 1e-10
