"""The MATLAB side of nagp_slowfb_run: the 'slowfb' command of matlab/nagp_mex.c against the mock MEX API of tests/c
(tests/c/mex_slowfb_driver.c, the pattern of the gateway test of nagp_fastfb_sample), and the wrapper
matlab/kernel_ss_kalmanSlowFB.m, whose call of the gateway is checked as text (there is no MATLAB to run it)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nagp
import slowfb_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_driver(tmp_path):
    nagp.build()
    c = os.path.join(ROOT, 'tests', 'c'); pkg = os.path.join(ROOT, 'nonstationary-audio-gp_amd'); exe = str(tmp_path / 'mex_slowfb_driver')
    cmd = ['gcc', '-Wall', '-Werror', '-O1', '-std=c99', '-I', os.path.join(ROOT, 'include'), '-I', c, '-o', exe, os.path.join(c, 'mex_slowfb_driver.c'),
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
    c = ref.case('m32')
    return c, dict(S=[8], block=[c['block']], A=c['A'], Q=c['Q'], H=c['H'], P0=c['P0'], y=c['y'], vary=c['vary'], sub_idx=[0, 4])


def test_gateway_compiles_and_refuses_a_wrong_sized_vary(tmp_path):
    """without a GPU: the driver builds against the mock MEX API with -Wall -Werror, and a call with a wrong-sized vary ends in a MEX error"""
    exe = build_driver(tmp_path)
    c, arrs = inputs()
    arrs['vary'] = c['vary'][:7]; arrs['lik'] = arrs['MS'] = arrs['Psub'] = np.zeros(1)
    dump(tmp_path, arrs)
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and 'vary must have the size of y' in r.stderr


def test_wrapper_passes_the_gateway_its_argument_list():
    src = open(os.path.join(ROOT, 'matlab', 'kernel_ss_kalmanSlowFB.m')).read()
    assert src.splitlines()[0] == 'function [lik,Xfin,Pfin,varargout] = kernel_ss_kalmanSlowFB(A,Q,C,P0,K,vary,y,varargin)'
    calls = re.findall(r"nagp_mex\('slowfb', (.*)\);", src)
    assert len(calls) == 2 and all(c == 'A, Q, C(:), P0, block, y(:), vary(:), KF == 1, code, sub' for c in calls)
    gw = open(os.path.join(ROOT, 'matlab', 'nagp_mex.c')).read()
    assert re.search(r"nagp_mex\('slowfb',A,Q,H,P0,block,y,vary,filter_only,cov,sub_idx\[,device\]\)", gw) is not None
    assert '!strcmp(cmd, "slowfb")' in gw
    assert re.search(r"if nargout > 3\s+error\('nagp:unsupported', '[^']*sufficient statistics", src)      # the fourth output names what is not built
    assert 'slowfb' in open(os.path.join(ROOT, 'matlab', 'README.md')).read()


@pytest.mark.gpu
def test_mex_gateway_slowfb(nagp_lib, tmp_path):
    """'slowfb' with three outputs and with one: sizes right, lik / MS / Psub bit-equal to the Python binding on m32"""
    c, arrs = inputs()
    lik, MS, _, Ps = nagp.slowfb_run(c['A'], c['Q'], c['H'], c['P0'], c['y'], c['vary'], sub_idx=np.array([0, 4]))
    arrs.update(lik=lik, MS=MS[0], Psub=Ps[0])
    dump(tmp_path, arrs)
    exe = build_driver(tmp_path)
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
