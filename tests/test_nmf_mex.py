"""The MATLAB side of nagp_nmf_fp: the 'nmf_fp' command of matlab/nagp_mex.c against the mock MEX API of tests/c
(tests/c/mex_nmf_driver.c, the pattern of tests/test_slowfb_mex.py), and the wrappers matlab/nmf_fp.m, nmf_inf_fp.m,
kernel_ss_probFB.m and getFBLDSOutput_tau.m, whose calls of the gateway are checked as text (there is no MATLAB to run them)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nagp
import nmf_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_driver(tmp_path):
    nagp.build()
    c = os.path.join(ROOT, 'tests', 'c'); pkg = os.path.join(ROOT, 'nonstationary-audio-gp_amd'); exe = str(tmp_path / 'mex_nmf_driver')
    cmd = ['gcc', '-Wall', '-Werror', '-O1', '-std=c99', '-I', os.path.join(ROOT, 'include'), '-I', c, '-o', exe, os.path.join(c, 'mex_nmf_driver.c'),
           os.path.join(c, 'mex_mock.c'), os.path.join(ROOT, 'matlab', 'nagp_mex.c'), '-L', pkg, '-lnagp', '-lm', '-Wl,-rpath,' + pkg,
           '-Wl,-rpath,/opt/rocm/lib', '-Wl,-rpath-link,/opt/rocm/lib']
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def dump(tmp_path, arrs):
    with open(tmp_path / 'meta.txt', 'w') as fh:
        for k, a in arrs.items():
            a = np.asfortranarray(np.asarray(a, dtype=np.float64)); a.ravel(order='F').tofile(str(tmp_path / (k + '.bin'))); fh.write('%s %d\n' % (k, a.size))


def inputs():
    """case a as two problems: W0 K x D x P, H0 T x K x P in MATLAB's layout"""
    c = ref.case('a'); T, K = c['H0'].shape
    W0 = np.stack([c['W0'], ref.normalise(c['A'][[3, 77, 200]] + 1e-6)]); H0 = np.stack([c['H0'], c['H0'][::-1]])
    return c, W0, H0, dict(T=[T], K=[K], its=[c['its']], update_w=[1], A=c['A'], vary=c['vary'], W0=W0.transpose(1, 2, 0), H0=H0.transpose(1, 2, 0))


def test_gateway_compiles_and_refuses_a_wrong_sized_H0(tmp_path):
    """without a GPU: the driver builds against the mock MEX API with -Wall -Werror, and a call with a wrong-sized H0 ends in a MEX error"""
    exe = build_driver(tmp_path)
    c, W0, H0, arrs = inputs()
    arrs['H0'] = H0.transpose(1, 2, 0)[:, :2, :]; arrs['W'] = arrs['H'] = arrs['Obj'] = np.zeros(1)
    dump(tmp_path, arrs)
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and 'H0 must be T x K x P' in r.stderr


def test_wrappers_pass_the_gateway_its_argument_list():
    m = lambda f: open(os.path.join(ROOT, 'matlab', f)).read()
    fp, inf, pfb, out = m('nmf_fp.m'), m('nmf_inf_fp.m'), m('kernel_ss_probFB.m'), m('getFBLDSOutput_tau.m')
    assert fp.splitlines()[0] == 'function [W,H,info] = nmf_fp(A,W,H,vary,varargin)'
    assert inf.splitlines()[0] == 'function [H,info] = nmf_inf_fp(A,W,H,vary,varargin)'
    assert pfb.splitlines()[0] == 'function [Z,varargout] = kernel_ss_probFB(y,A,Q,C,P0,K,vary,tau,varargin)'
    assert out.splitlines()[0] == 'function [S,varargout] = getFBLDSOutput_tau(Xfin,Pfin,tau)'
    assert re.findall(r"nagp_mex\('nmf_fp', (.*)\);", inf) == ['A, vary, W, H, numIts, 0']
    assert re.findall(r"nagp_mex\('nmf_fp', (.*)\);", fp) == ['A, vary, Wb, Hc, 10, 0', 'A, vary, W, H, numIts, 1']
    # the restart candidates: MATLAB's own stream in the reference's order (ks, then H), and the earliest wins a tie
    assert re.search(r'ks = ceil\(T \* rand\(K, 1\)\); W = A\(ks, :\); H = exp\(randn\(T, K\)\);', fp)
    assert 'if Obj(end, r) < best' in fp
    assert 'if all(rs ~= 1)' in inf and 'if all(rs ~= 1)' in fp                       # the condition of nmf_inf_fp.m:37
    assert 'kernel_ss_kalmanSlowFB(' in pfb and 'kernel_ss_kalmanFastFB(' in pfb and "'sub', rows" in pfb and 'getFBLDSOutput_tau(' in pfb
    assert 'nagp_mex' not in out and 'nagp_mex' not in pfb                           # selection and pairing on the host
    gw = m('nagp_mex.c')
    assert re.search(r"nagp_mex\('nmf_fp',A,vary,W0,H0,n_its,update_w\[,device\]\)", gw) is not None
    assert '!strcmp(cmd, "nmf_fp")' in gw
    readme = m('README.md')
    for f in ('nmf_fp.m', 'nmf_inf_fp.m', 'kernel_ss_probFB.m', 'getFBLDSOutput_tau.m'):
        assert f in readme, f
    assert "nagp_mex('nmf_fp'" in open(os.path.join(ROOT, 'INTEGRATION.md')).read()


@pytest.mark.gpu
def test_mex_gateway_nmf_fp(nagp_lib, tmp_path):
    """'nmf_fp' with three outputs and with one: sizes right, W / H / Obj bit-equal to the ctypes path on case a (two problems)"""
    c, W0, H0, arrs = inputs()
    W, H, Obj = nagp.nmf_run(c['A'], c['vary'], W0, H0, c['its'], update_w=True)
    arrs.update(W=W.transpose(1, 2, 0), H=H.transpose(1, 2, 0), Obj=Obj.T)
    dump(tmp_path, arrs)
    exe = build_driver(tmp_path)
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
