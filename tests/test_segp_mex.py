"""The MATLAB side of nagp_segp_obj: the 'segp_obj' command of matlab/nagp_mex.c against the mock MEX API of tests/c
(tests/c/mex_segp_driver.c, the pattern of tests/test_pstft_mex.py), and the wrapper matlab/getObjSEGP.m, whose calls of the gateway
are checked as text (there is no MATLAB to run it)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nagp
import segp_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_driver(tmp_path):
    nagp.build()
    c = os.path.join(ROOT, 'tests', 'c'); pkg = os.path.join(ROOT, 'nonstationary-audio-gp_amd'); exe = str(tmp_path / 'mex_segp_driver')
    cmd = ['gcc', '-Wall', '-Werror', '-O1', '-std=c99', '-I', os.path.join(ROOT, 'include'), '-I', c, '-o', exe, os.path.join(c, 'mex_segp_driver.c'),
           os.path.join(c, 'mex_mock.c'), os.path.join(ROOT, 'matlab', 'nagp_mex.c'), '-L', pkg, '-lnagp', '-lm', '-Wl,-rpath,' + pkg,
           '-Wl,-rpath,/opt/rocm/lib', '-Wl,-rpath-link,/opt/rocm/lib']
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def dump(tmp_path, arrs):
    with open(tmp_path / 'meta.txt', 'w') as fh:
        for k, a in arrs.items():
            a = np.asfortranarray(np.asarray(a, dtype=np.float64)); a.ravel(order='F').tofile(str(tmp_path / (k + '.bin'))); fh.write('%s %d\n' % (k, a.size))


def inputs(n_param):
    """case t257 as two problems with their own param, specy, vary and varx, in MATLAB's layout; vary / varx empty where not read"""
    c = ref.case('t257'); T = c['T']
    full = np.log(np.array([[4.0, 2.0, 0.1], [5.0, 1.5, 0.2]]))
    param = full[:, :n_param]; spec = np.stack([c['specy'], c['specy'][::-1]])
    vary = np.array([0.1, 0.2]) if n_param <= 2 else None
    varx = np.array([2.0, 1.5]) if n_param == 1 else None
    arrs = dict(n_param=[n_param], T=[T], P=[2], param=param.T, specy=spec.T, vary=np.zeros(0) if vary is None else vary,
                varx=np.zeros(0) if varx is None else varx)
    return param, spec, vary, varx, arrs


def test_gateway_compiles_and_refuses_before_the_library(tmp_path):
    """without a GPU: the driver builds against the mock MEX API with -Wall -Werror; a param of four entries and a missing vary with two
    parameters end in a MEX error"""
    exe = build_driver(tmp_path)
    for n_param, change, text in ((3, dict(n_param=[4], param=np.zeros((4, 1))), 'param must be n_param x P'),
                                  (2, dict(vary=np.zeros(0)), 'vary must be a scalar or hold P entries'),
                                  (1, dict(varx=np.zeros(0)), 'varx must be a scalar or hold P entries')):
        arrs = inputs(n_param)[4]; arrs.update(change); arrs['Obj'] = arrs['dObj'] = np.zeros(1)
        dump(tmp_path, arrs)
        r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and text in r.stderr, (change, r.stderr)


def test_wrapper_passes_the_gateway_its_argument_list():
    m = lambda f: open(os.path.join(ROOT, 'matlab', f)).read()
    src = m('getObjSEGP.m')
    assert src.splitlines()[0] == 'function [obj,dobj] = getObjSEGP(param,specy,varargin)'
    assert re.findall(r"nagp_mex\('segp_obj', (.*)\);", src) == ['reshape(param(1:3), [], 1), specy(:), [], []',
                                                                 'reshape(param(1:2), [], 1), specy(:), varargin{1}, []',
                                                                 'param(1), specy(:), varargin{1}, varargin{2}']
    assert re.findall(r'nargin == (\d)', src) == ['2', '3'] and 'max(nargout, 1)' in src and 'if nargout > 1' in src
    gw = m('nagp_mex.c')
    assert "nagp_mex('segp_obj', param, specy, vary, varx [,device])" in gw
    assert '!strcmp(cmd, "segp_obj")' in gw
    assert 'getObjSEGP.m' in m('README.md') and "nagp_mex('segp_obj'" in m('README.md')
    assert "nagp_mex('segp_obj'" in open(os.path.join(ROOT, 'INTEGRATION.md')).read()


@pytest.mark.gpu
@pytest.mark.parametrize('n_param', [1, 2, 3])
def test_mex_gateway_segp_obj(nagp_lib, tmp_path, n_param):
    """'segp_obj' with two outputs and with one: sizes right, Obj / dObj bit-equal to the ctypes path on case t257 (two problems)"""
    param, spec, vary, varx, arrs = inputs(n_param)
    Obj, dObj = nagp.segp_obj(param, spec, vary=vary, varx=varx)
    arrs.update(Obj=Obj, dObj=dObj.T)
    dump(tmp_path, arrs)
    exe = build_driver(tmp_path)
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
