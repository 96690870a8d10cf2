"""nagp_slowfb_run (the exact filterbank filter / smoother with an observation variance per step) without a GPU: the yardstick
-- tests/slowfb_ref.py against the multi-precision fixture --, the export and its binding, and every argument check of
include/nagp.h, each of which must answer on a machine with no device (they run before any device call)."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nagp
from nagp import _lib as L
import slowfb_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EUNSUPPORTED, ENOMEM = -1, -2, -4


def fixture(name):
    f = np.load(os.path.join(ROOT, 'tests', 'golden', 'slowfb_multiprecision.npz'))
    return {k[len(name) + 1:]: f[k] for k in f.files if k.startswith(name + '_')}


@pytest.mark.parametrize('name', ['m32', 'm52'])
def test_restatement_matches_the_multiprecision_fixture(name):
    """e_ref per output class: what the GPU tests measure the kernels against.  Float64 with a Cholesky-based gain on these
    shapes (S = 8 / 18, a 1e5-variance gap next to 1e-4 steps) is within 1e-12 of the 60-digit run; no jitter retry is needed."""
    c = fixture(name); st = c['steps']
    for k in ('A', 'Q', 'H', 'P0', 'y', 'vary'):                       # the fixture's inputs are those the case builder gives today
        assert np.array_equal(ref.case(name)[k], c[k], equal_nan=True), k
    lik, MS, PS = ref.slowfb(c['A'], c['Q'], c['H'], c['P0'], c['y'], c['vary'])
    fl, MF, PF = ref.slowfb(c['A'], c['Q'], c['H'], c['P0'], c['y'], c['vary'], KF=1)
    e = dict(lik=abs(lik - c['lik']) / abs(c['lik']), MS=ref.dist(MS, c['MS']), Pdiag=ref.dist(np.einsum('iik->ik', PS), c['Pdiag']),
             P=ref.dist(PS[:, :, st], c['P']), MF=ref.dist(MF, c['MF']), PFdiag=ref.dist(np.einsum('iik->ik', PF), c['PFdiag']),
             PF=ref.dist(PF[:, :, st], c['PF']))
    print('e_ref %s: ' % name + '  '.join('%s %.2e' % kv for kv in e.items()))
    assert fl == lik and max(e.values()) < 1e-12, e
    assert c['MS'].shape == (c['A'].shape[0], c['y'].size) and c['P'].shape[2] == st.size
    assert np.isnan(c['y']).sum() == (6 if name == 'm32' else 4) and (c['vary'] == 1e5).sum() == (20 if name == 'm32' else 10)


def test_exported_and_bound():
    nagp.build()
    out = subprocess.run(['nm', '-D', '--defined-only', L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert 'nagp_slowfb_run' in set(re.findall(r' T (nagp_[a-z0-9_]+)', out))
    assert 'nagp_slowfb_run' in L.EXPORTS
    fn = L.lib().nagp_slowfb_run
    assert len(fn.argtypes) == 18 and fn.restype is C.c_int
    assert L.lib().nagp_version() == 300
    assert nagp.kernel_ss_kalmanSlowFB is nagp.slowfb.kernel_ss_kalmanSlowFB


def call(A, Q, H, P0, y, vary, block, filter_only=0, sub=None, psub=True, outputs=True, null=None, S=None, T=None, n=None):
    """the raw entry point; returns the status"""
    A = L.f64(A); Q = L.f64(Q); P0 = L.f64(P0); H = L.f64(np.ravel(H), 'C')
    y = L.f64(np.atleast_2d(y), 'C'); vary = L.f64(np.atleast_2d(vary), 'C')
    S_ = A.shape[0] if S is None else S; n_, T_ = y.shape
    n_ = n_ if n is None else n; T_ = T_ if T is None else T
    sub_a = None if sub is None else np.ascontiguousarray(sub, dtype=np.int32)
    n_sub = 0 if sub_a is None else sub_a.size
    lik = np.zeros(max(n_, 1)); MS = np.zeros(max(n_ * T_ * S_, 1)); Ps = np.zeros(max(n_ * T_ * n_sub * n_sub, 1))
    p = dict(A=L.dptr(A), Q=L.dptr(Q), H=L.dptr(H), P0=L.dptr(P0), y=L.dptr(y), vary=L.dptr(vary))
    if null:
        p[null] = L.c_dp()
    return L.lib().nagp_slowfb_run(S_, block, p['A'], p['Q'], p['H'], p['P0'], n_, p['y'], p['vary'], T_, filter_only, n_sub,
                                   sub_a.ctypes.data_as(L.c_ip) if n_sub else L.c_ip(), L.dptr(lik) if outputs else L.c_dp(),
                                   L.dptr(MS) if outputs else L.c_dp(), L.c_dp(), L.dptr(Ps) if (n_sub and psub) else L.c_dp(), 0)


def refused_time():
    """nagp_slowfb_timings after a refused call: no time of an earlier call on this thread"""
    ms = np.full(3, -1.0)
    assert L.lib().nagp_slowfb_timings(L.dptr(ms)) == 0
    return ms.tolist()


@pytest.fixture(scope='module')
def m32():
    nagp.build()
    A, Q, H, P0, _ = ref.model('matern32', 2)
    return A, Q, H, P0, np.linspace(-1, 1, 12), np.full(12, 1e-2)


def test_einval_cases(m32):
    A, Q, H, P0, y, v = m32
    for name in ('A', 'Q', 'H', 'P0', 'y', 'vary'):
        assert call(A, Q, H, P0, y, v, 4, null=name) == EINVAL, name
    assert call(A, Q, H, P0, y, v, 4, S=0) == EINVAL
    assert call(A, Q, H, P0, y, v, 4, T=0) == EINVAL
    assert call(A, Q, H, P0, y, v, 4, n=0) == EINVAL
    assert call(A, Q, H, P0, y, v, 0) == EINVAL
    assert call(A, Q, H, P0, y, v, 3) == EINVAL                                        # 8 % 3 != 0
    for bad in (-1e-9, np.nan, np.inf):
        vb = v.copy(); vb[7] = bad
        assert call(A, Q, H, P0, y, vb, 4) == EINVAL, bad
    for sub in ([0, 0], [2, 1], [0, 8], [-1, 3]):
        assert call(A, Q, H, P0, y, v, 4, sub=sub) == EINVAL, sub
    assert call(A, Q, H, P0, y, v, 4, sub=[0, 4], psub=False) == EINVAL               # n_sub without Psub
    assert call(A, Q, H, P0, y, v, 4, outputs=False) == EINVAL                        # nothing asked for
    assert b'no output' in L.lib().nagp_last_error()
    assert refused_time() == [0.0, 0.0, 0.0]


def test_eunsupported_cases(m32):
    A, Q, H, P0, y, v = m32
    A65, Q65, H65, P65, _ = ref.model('exp', 65)                                       # S = 130
    assert A65.shape[0] == 130 and call(A65, Q65, H65, P65, y, v, 2) == EUNSUPPORTED
    A16 = np.kron(np.eye(1), np.eye(16)) * 0.5
    assert call(A16, np.eye(16), np.ones(16), np.eye(16), y, v, 16) == EUNSUPPORTED    # block > 8
    Ad = A.copy(); Ad[5, 1] = 1e-300                                                   # a non-zero of A outside its blocks
    assert call(Ad, Q, H, P0, y, v, 4) == EUNSUPPORTED
    assert b'outside the blocks' in L.lib().nagp_last_error()
    Qd = Q.copy(); Qd[0, 7] = 1e-3
    assert call(A, Qd, H, P0, y, v, 4) == EUNSUPPORTED
    assert call(A, Q, H, P0, y, v, 2) == EUNSUPPORTED                                  # blocks of 4 declared as blocks of 2
    assert refused_time() == [0.0, 0.0, 0.0]
    with pytest.raises(L.NagpError, match='outside the blocks'):                       # the mirror detects no block and the library refuses
        nagp.kernel_ss_kalmanSlowFB(np.ones((12, 12)), np.eye(12), np.ones(12), np.eye(12), 12, 0.1, y)


def test_enomem_under_the_budget_switch(m32, monkeypatch):
    """NAGP_SFB_BUDGET_MB=1: a series of 8 T (2 S^2 + 3 S + 2 + 2 + S) bytes = 1 312 T at S = 8 fits up to T = 796"""
    A, Q, H, P0, y, v = m32
    monkeypatch.setenv('NAGP_SFB_BUDGET_MB', '1')
    T = 2000
    assert call(A, Q, H, P0, np.zeros(T), np.full(T, 1e-2), 4) == ENOMEM
    assert b'budget 1048576 B' in L.lib().nagp_last_error()
    assert call(A, Q, H, P0, np.zeros(T), np.full(T, 1e-2), 4, filter_only=1) == ENOMEM           # 8 T (S^2 + S + 2 + S) = 656 T
    assert refused_time() == [0.0, 0.0, 0.0]
    assert call(A, Q, H, P0, np.zeros(1200), np.full(1200, 1e-2), 4, filter_only=1) != ENOMEM        # fits: refused later, for want of a device, or runs


def test_block_detection_and_mirror_arguments(m32):
    A, Q, H, P0, y, v = m32
    assert nagp.slowfb.detect_block(A, Q) == 4
    A6, Q6, _, _, _ = ref.model('matern52', 3)
    assert nagp.slowfb.detect_block(A6, Q6) == 6
    assert nagp.slowfb.detect_block(np.eye(6), np.eye(6)) == 1
    assert nagp.slowfb.detect_block(np.ones((12, 12)), np.eye(12)) is None
    with pytest.raises(ValueError):
        nagp.kernel_ss_kalmanSlowFB(A, Q, H, P0, 4, v[:5], y)
    with pytest.raises(ValueError):
        nagp.kernel_ss_kalmanSlowFB(A, Q, H, P0, 4, v, y, cov='sub')
    A32, Q32, H32, P32, _ = ref.model('matern32', 32)
    with pytest.raises(MemoryError):                                                   # 128^2 x 9000 doubles > 1 GiB
        nagp.kernel_ss_kalmanSlowFB(A32, Q32, H32, P32, 64, 0.1, np.zeros(9000))
