"""The MATLAB side of nagp_nmf_temp_obj: the 'nmf_temp_obj' command of matlab/nagp_mex.c against the mock MEX API of tests/c
(tests/c/mex_nmf_temp_driver.c, the pattern of tests/test_gppad_mex.py), and the wrappers matlab/getObj_nmf_temp.m and
getObj_nmf_temp_inf.m, whose calls of the gateway are checked as text (there is no MATLAB to run them)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nagp
import nmf_temp_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_driver(tmp_path):
    nagp.build()
    c = os.path.join(ROOT, 'tests', 'c'); pkg = os.path.join(ROOT, 'nonstationary-audio-gp_amd'); exe = str(tmp_path / 'mex_nmf_temp_driver')
    cmd = ['gcc', '-Wall', '-Werror', '-O1', '-std=c99', '-I', os.path.join(ROOT, 'include'), '-I', c, '-o', exe, os.path.join(c, 'mex_nmf_temp_driver.c'),
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
    """two problems in MATLAB's layout.  form 0: case w257_ig_l, the learning form with the inverse-gamma chain, what getObj_nmf_temp.m passes;
    1: case b1999_tg_i, the inference form with the truncated-Gaussian chain, vary = [] and a K x D x P block of weights; 2: case r20_none_i
    with one shared W, what getObj_nmf_temp_inf.m passes"""
    c = ref.case({0: 'w257_ig_l', 1: 'b1999_tg_i', 2: 'r20_none_i'}[form])
    x = np.stack([c['x'], 0.5 * c['x'][::-1]])
    W = None if c['learn'] else (np.stack([c['W'], c['W'][::-1] + 0.2]) if form == 1 else c['W'])
    e = np.zeros(0)
    arrs = dict(X=[x.shape[1]], T=[c['T']], K=[c['K']], P=[2], x=x.T, A=c['A'], vary=e if c['vary'] is None else c['vary'],
                W=e if W is None else (np.transpose(W, (1, 2, 0)) if W.ndim == 3 else W), muinf=e if c['muinf'] is None else c['muinf'],
                varinf=e if c['varinf'] is None else c['varinf'], lam=e if c['lam'] is None else c['lam'])
    return c, x, W, arrs


def test_gateway_compiles_and_refuses_before_the_library(tmp_path):
    """without a GPU: the driver builds against the mock MEX API with -Wall -Werror; a vary that is not T x D, an x that is no multiple of
    T + D, a W with the wrong number of columns, a varinf of three entries for K = 2 and a lam left empty end in a MEX error"""
    exe = build_driver(tmp_path)
    for form, change, text in ((0, dict(vary=np.zeros((257, 2))), 'vary must be T x D or []'), (0, dict(X=[100], x=np.zeros((100, 2))), 'x must be (T K + K D) x P without W'),
                               (2, dict(W=np.ones((2, 4))), 'W must be K x D or K x D x P'), (2, dict(varinf=np.ones(3), lam=np.ones(2)), 'varinf must hold K entries or be []'),
                               (2, dict(varinf=np.ones(2)), 'lam is empty but varinf is not')):
        arrs = inputs(form)[3]; arrs.update(change); arrs['Obj'] = arrs['dObj'] = np.zeros(1)
        dump(tmp_path, arrs)
        r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and text in r.stderr, (change, r.stderr)


def test_wrappers_pass_the_gateway_its_argument_list():
    m = lambda f: open(os.path.join(ROOT, 'matlab', f)).read()
    src = m('getObj_nmf_temp.m')
    assert src.splitlines()[0] == 'function [obj,dobj] = getObj_nmf_temp(logHW,A,vary,varargin)'
    assert re.findall(r"nagp_mex\('nmf_temp_obj', (.*)\);", src) == ['logHW(:), A, vary, [], p{1}, p{2}, p{3}']
    src_i = m('getObj_nmf_temp_inf.m')
    assert src_i.splitlines()[0] == 'function [obj,dobj] = getObj_nmf_temp_inf(logH,A,W,vary,varargin)'
    assert re.findall(r"nagp_mex\('nmf_temp_obj', (.*)\);", src_i) == ['logH(:), A, vary, W, p{1}, p{2}, p{3}']
    for s in (src, src_i):
        assert 'max(nargout, 1)' in s and 'if nargout > 1' in s and 'numel(varargin) == 1' in s and '3 - numel(varargin)' in s
    gw = m('nagp_mex.c')
    assert "nagp_mex('nmf_temp_obj', x, A, vary, W, muinf, varinf, lam [,device])" in gw
    assert '!strcmp(cmd, "nmf_temp_obj")' in gw
    assert 'getObj_nmf_temp.m' in m('README.md') and 'getObj_nmf_temp_inf.m' in m('README.md') and "nagp_mex('nmf_temp_obj'" in m('README.md')
    assert "nagp_mex('nmf_temp_obj'" in open(os.path.join(ROOT, 'INTEGRATION.md')).read()


@pytest.mark.gpu
@pytest.mark.parametrize('form', [0, 1, 2])
def test_mex_gateway_nmf_temp_obj(nagp_lib, tmp_path, form):
    """'nmf_temp_obj' with two outputs and with one: sizes right, Obj / dObj bit-equal to the ctypes path (two problems)"""
    c, x, W, arrs = inputs(form)
    Obj, dObj = nagp.nmf_temp_obj(x, c['A'], c['vary'], W, c['prior'], c['muinf'], c['varinf'], c['lam'])
    arrs.update(Obj=Obj, dObj=dObj.T)
    dump(tmp_path, arrs)
    exe = build_driver(tmp_path)
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
