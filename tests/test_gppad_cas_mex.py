"""The MATLAB side of nagp_gppad_cas_obj: the 'gppad_cas_obj' command of matlab/nagp_mex.c against the mock MEX API of tests/c
(tests/c/mex_gppad_cas_driver.c, the pattern of tests/test_tnmf_mex.py), and the wrapper matlab/GetObjCasGPFAST.m, whose call of the
gateway is checked as text (there is no MATLAB to run it)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nagp
import gppad_cas_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_driver(tmp_path):
    nagp.build()
    c = os.path.join(ROOT, 'tests', 'c'); pkg = os.path.join(ROOT, 'nonstationary-audio-gp_amd'); exe = str(tmp_path / 'mex_gppad_cas_driver')
    cmd = ['gcc', '-Wall', '-Werror', '-O1', '-std=c99', '-I', os.path.join(ROOT, 'include'), '-I', c, '-o', exe, os.path.join(c, 'mex_gppad_cas_driver.c'),
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
    """MATLAB's layout.  form 0: case k3_200_256, one cascade, what GetObjCasGPFAST.m passes (x(:), fftCovs Tx x M, varx(:), mux(:), a
    scalar varc); 1: two cascades with their own spectra (Tx x M x P), varx and mux M x P and varc of P entries"""
    c = ref.case('k3_200_256')
    M, T, Tx = c['M'], c['T'], c['Tx']
    if form == 0:
        arrs = dict(M=[M], T=[T], Tx=[Tx], P=[1], vrows=[M], x=c['x'].reshape(-1, 1), y=c['y'][:, None], fftCovs=c['fftCovs'].T, varx=c['varx'], mux=c['mux'], varc=[c['varc']])
        return arrs, lambda: nagp.gppad_cas_obj(c['x'][None], c['y'][None], c['varx'], c['mux'], c['varc'], fftCovs=c['fftCovs'])
    x = np.stack([c['x'], 0.5 * c['x'][:, ::-1]]); y = np.stack([c['y'], 2.0 * c['y'][::-1]])
    covs = np.stack([c['fftCovs'], c['fftCovs'][::-1] + 0.1]); varx = np.stack([c['varx'], c['varx'] + 0.3]); mux = np.stack([c['mux'], c['mux'] - 0.2])
    varc = np.array([c['varc'], 1.9])
    arrs = dict(M=[M], T=[T], Tx=[Tx], P=[2], vrows=[M], x=x.reshape(2, -1).T, y=y.T, fftCovs=np.transpose(covs, (2, 1, 0)), varx=varx.T, mux=mux.T, varc=varc)
    return arrs, lambda: nagp.gppad_cas_obj(x, y, varx, mux, varc, fftCovs=covs)


def test_gateway_compiles_and_refuses_before_the_library(tmp_path):
    """without a GPU: the driver builds against the mock MEX API with -Wall -Werror; an x whose rows are no multiple of Tx, spectra for
    another number of cascades, a y of another width, a varx of two entries for M = 3 and a varc of three entries for one cascade end in a
    MEX error"""
    exe = build_driver(tmp_path)
    for form, change, text in ((0, dict(M=[1], x=np.zeros((256, 1))), 'fftCovs must be Tx x M or Tx x M x P'),
                               (1, dict(fftCovs=np.ones((256, 9))), 'fftCovs must be Tx x M or Tx x M x P'),
                               (1, dict(y=np.zeros((200, 3))), 'y must be T x P'), (0, dict(vrows=[2], varx=np.ones(2)), 'varx must hold M entries or be M x P'),
                               (0, dict(varc=np.ones(3)), 'varc must be a scalar or hold P entries')):
        arrs = inputs(form)[0]; arrs.update(change); arrs['Obj'] = arrs['dObj'] = np.zeros(1)
        dump(tmp_path, arrs)
        r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and text in r.stderr, (change, r.stderr)


def test_wrapper_passes_the_gateway_its_argument_list():
    m = lambda f: open(os.path.join(ROOT, 'matlab', f)).read()
    src = m('GetObjCasGPFAST.m')
    assert src.splitlines()[0] == 'function [Obj,dObjdx] = GetObjCasGPFAST(x,y,fftCovs,Params,Dims)'                            # GetObjCasGPFAST.m:1
    assert re.findall(r"nagp_mex\('gppad_cas_obj', (.*)\);", src) == ['x(:), y(:), fftCovs, Params.varx(:), Params.mux(:), Params.varc']
    assert 'max(nargout, 1)' in src and 'if nargout > 1' in src
    gw = m('nagp_mex.c')
    assert "nagp_mex('gppad_cas_obj', x, y, fftCovs, varx, mux, varc [,device])" in gw and '!strcmp(cmd, "gppad_cas_obj")' in gw
    readme = m('README.md')
    assert 'GetObjCasGPFAST.m' in readme and "nagp_mex('gppad_cas_obj'" in readme
    assert "nagp_mex('gppad_cas_obj'" in open(os.path.join(ROOT, 'INTEGRATION.md')).read()


@pytest.mark.gpu
@pytest.mark.parametrize('form', [0, 1])
def test_mex_gateway_gppad_cas(nagp_lib, tmp_path, form):
    """the command with both outputs and with one: sizes right, Obj / dObj bit-equal to the ctypes path"""
    arrs, run = inputs(form)
    Obj, dObj = run()
    arrs.update(Obj=Obj, dObj=dObj.reshape(dObj.shape[0], -1).T)
    dump(tmp_path, arrs)
    exe = build_driver(tmp_path)
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
