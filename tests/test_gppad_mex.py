"""The MATLAB side of nagp_gppad_obj: the 'gppad_obj' command of matlab/nagp_mex.c against the mock MEX API of tests/c
(tests/c/mex_gppad_driver.c, the pattern of tests/test_segp_mex.py), and the wrapper matlab/GetGPObjFast.m, whose call of the gateway
is checked as text (there is no MATLAB to run it)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nagp
import gppad_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_driver(tmp_path):
    nagp.build()
    c = os.path.join(ROOT, 'tests', 'c'); pkg = os.path.join(ROOT, 'nonstationary-audio-gp_amd'); exe = str(tmp_path / 'mex_gppad_driver')
    cmd = ['gcc', '-Wall', '-Werror', '-O1', '-std=c99', '-I', os.path.join(ROOT, 'include'), '-I', c, '-o', exe, os.path.join(c, 'mex_gppad_driver.c'),
           os.path.join(c, 'mex_mock.c'), os.path.join(ROOT, 'matlab', 'nagp_mex.c'), '-L', pkg, '-lnagp', '-lm', '-Wl,-rpath,' + pkg,
           '-Wl,-rpath,/opt/rocm/lib', '-Wl,-rpath-link,/opt/rocm/lib']
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def dump(tmp_path, arrs):
    with open(tmp_path / 'meta.txt', 'w') as fh:
        for k, a in arrs.items():
            a = np.asfortranarray(np.asarray(a, dtype=np.float64)); a.ravel(order='F').tofile(str(tmp_path / (k + '.bin'))); fh.write('%s %d\n' % (k, a.size))


def inputs(form):
    """case c257_1024 as two problems with their own x, y and parameters, in MATLAB's layout.  form 0: a shared fftCov and a scalar vary
    (what GetGPObjFast.m passes for one problem with Params.vary a scalar); 1: per-problem fftCov and T x P vary"""
    c = ref.case('c257_1024'); T, Tx = c['T'], c['Tx']
    x = np.stack([c['x'], c['x'][::-1]]); y = np.stack([c['y'], 0.5 * c['y'][::-1]])
    varx, mux, varc = np.array([1.7, 0.9]), np.array([-0.4, 0.1]), np.array([0.6, 1.1])
    if form == 0:
        cov = c['fftCov']; vary = 0.03
    else:
        cov = np.stack([c['fftCov'], ref.fft_cov(7.0, Tx)]); vary = np.stack([np.linspace(0, 1, T), np.zeros(T)])
    arrs = dict(Tx=[Tx], T=[T], P=[2], x=x.T, y=y.T, fftCov=cov.T, varx=varx, mux=mux, varc=varc, vary=np.asarray(vary).T)
    return x, y, cov, varx, mux, varc, vary, arrs


def test_gateway_compiles_and_refuses_before_the_library(tmp_path):
    """without a GPU: the driver builds against the mock MEX API with -Wall -Werror; a y that is not T x P, a fftCov of the wrong length
    and a varx of three entries end in a MEX error"""
    exe = build_driver(tmp_path)
    for change, text in ((dict(y=np.zeros((257, 1))), 'y must be T x P'), (dict(fftCov=np.ones(1000)), 'fftCov must be Tx x 1 or Tx x P'),
                         (dict(varx=np.ones(3)), 'varx must be a scalar or hold P entries'), (dict(vary=np.zeros(2)), 'vary must be a scalar, T x 1 or T x P')):
        arrs = inputs(0)[7]; arrs.update(change); arrs['Obj'] = arrs['dObj'] = np.zeros(1)
        dump(tmp_path, arrs)
        r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and text in r.stderr, (change, r.stderr)


def test_wrapper_passes_the_gateway_its_argument_list():
    m = lambda f: open(os.path.join(ROOT, 'matlab', f)).read()
    src = m('GetGPObjFast.m')
    assert src.splitlines()[0] == 'function [Obj,dObjdx] = GetGPObjFast(x,y,fftCov,Params,Dims)'
    assert re.findall(r"nagp_mex\('gppad_obj', (.*)\);", src) == ['x(:), y(:), fftCov(:), Params.varx, Params.mux, Params.varc, Params.vary(:)']
    assert 'max(nargout, 1)' in src and 'if nargout > 1' in src and 'Dims.Tx' in src and 'Dims.T' in src
    gw = m('nagp_mex.c')
    assert "nagp_mex('gppad_obj', x, y, fftCov, varx, mux, varc, vary [,device])" in gw
    assert '!strcmp(cmd, "gppad_obj")' in gw
    assert 'GetGPObjFast.m' in m('README.md') and "nagp_mex('gppad_obj'" in m('README.md')
    assert "nagp_mex('gppad_obj'" in open(os.path.join(ROOT, 'INTEGRATION.md')).read()


@pytest.mark.gpu
@pytest.mark.parametrize('form', [0, 1])
def test_mex_gateway_gppad_obj(nagp_lib, tmp_path, form):
    """'gppad_obj' with two outputs and with one: sizes right, Obj / dObj bit-equal to the ctypes path on case c257_1024 (two problems)"""
    x, y, cov, varx, mux, varc, vary, arrs = inputs(form)
    Obj, dObj = nagp.gppad_obj(x, y, vary, varx, mux, varc, fftCov=cov)
    arrs.update(Obj=Obj, dObj=dObj.T)
    dump(tmp_path, arrs)
    exe = build_driver(tmp_path)
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
