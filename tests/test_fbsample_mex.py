"""The MATLAB side of nagp_fastfb_sample: the 'fastfb_sample' command of matlab/nagp_mex.c against the mock MEX API of tests/c
(tests/c/mex_fbsample_driver.c, the pattern of the gateway test of nagp_reconstruct_sources), and the wrapper
matlab/kernel_ss_sampleFastFB.m, whose call of the gateway is checked as text (there is no MATLAB to run it)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nagp
import fbsample_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_driver(tmp_path):
    nagp.build()
    c = os.path.join(ROOT, 'tests', 'c'); pkg = os.path.join(ROOT, 'nonstationary-audio-gp_amd'); exe = str(tmp_path / 'mex_fbsample_driver')
    cmd = ['gcc', '-Wall', '-Werror', '-O1', '-std=c99', '-I', os.path.join(ROOT, 'include'), '-I', c, '-o', exe, os.path.join(c, 'mex_fbsample_driver.c'),
           os.path.join(c, 'mex_mock.c'), os.path.join(ROOT, 'matlab', 'nagp_mex.c'), '-L', pkg, '-lnagp', '-lm', '-Wl,-rpath,' + pkg,
           '-Wl,-rpath,/opt/rocm/lib', '-Wl,-rpath-link,/opt/rocm/lib']
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def dump(tmp_path, arrs):
    with open(tmp_path / 'meta.txt', 'w') as fh:
        for k, a in arrs.items():
            a = np.asfortranarray(np.asarray(a, dtype=np.float64)); a.ravel(order='F').tofile(str(tmp_path / (k + '.bin'))); fh.write('%s %d\n' % (k, a.size))


def inputs(T=120):
    A, Q, H, Pinf = ref.matern32_model(2, 21)
    Lq, Lp = ref.factors(Q, Pinf)
    y = ref.simulate_y(A, Lq, Lp, H, 0.01, T, 22); y[30:50] = np.nan
    A_, H_, R, Sinn, Kg, HA, AKHA, PF2, G, Psm = nagp.fastfb._steady_state(A, Q, H, 0.01)
    return (A, Q, H, Pinf, Lq, Lp, y), dict(S=[A.shape[0]], n_draws=[6], seed=[41], R=[R], A=A, AKHA=AKHA, HA=HA, K=Kg, G=G, H=H.ravel(), Lp=Lp, Lq=Lq, y=y)


def test_gateway_compiles_and_refuses_a_bad_argument_list(tmp_path):
    """without a GPU: the driver builds against the mock MEX API, and a gateway call with a wrong-sized factor ends in a MEX error"""
    exe = build_driver(tmp_path)
    _, arrs = inputs()
    arrs['Lq'] = np.eye(3); arrs['Ydraw'] = arrs['Xdraw'] = arrs['MS'] = np.zeros(1)
    dump(tmp_path, arrs)
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and 'Lq must be S x S' in r.stderr


def test_wrapper_passes_the_gateway_its_argument_list():
    src = open(os.path.join(ROOT, 'matlab', 'kernel_ss_sampleFastFB.m')).read()
    assert src.splitlines()[0] == 'function [Ydraw,Xdraw,Xmean] = kernel_ss_sampleFastFB(A,Q,C,P0,K,vary,y,n_draws,varargin)'
    calls = re.findall(r"nagp_mex\('fastfb_sample', (.*)\);", src)
    assert len(calls) == 3 and all(c == 'A, AKHA, HA(:), Kg(:), G, H(:), R, Lp, Lq, y(:), n_draws, seed' for c in calls)
    usage = re.search(r"nagp_mex\('fastfb_sample',A,AKHA,HA,K,G,H,R,Lp,Lq,y,n_draws,seed\[,device\]\)", open(os.path.join(ROOT, 'matlab', 'nagp_mex.c')).read())
    assert usage is not None
    for line in ("PP = dare(A',H',Q,R);", "Kg = PP*H'/S;", "AKHA = A - Kg*H*A;", "G = PF2*A'/PP;"):      # the set-up lines of kernel_ss_kalmanFastFB.m
        assert line in src and line in open(os.path.join(ROOT, 'matlab', 'kernel_ss_kalmanFastFB.m')).read()


@pytest.mark.gpu
def test_mex_gateway_fastfb_sample(nagp_lib, tmp_path):
    """'fastfb_sample' with three outputs and with one: sizes right, values those of the Python call to 1e-12"""
    (A, Q, H, Pinf, Lq, Lp, y), arrs = inputs()
    Y, X, MS = nagp.kernel_ss_sampleFastFB(A, Q, H, Pinf, 2, 0.01, y, 6, 41, True, Lq, Lp)
    arrs.update(Ydraw=Y.T, Xdraw=X.transpose(1, 2, 0), MS=MS)              # MATLAB shapes: T x n, S x T x n, S x T
    dump(tmp_path, arrs)
    exe = build_driver(tmp_path)
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
