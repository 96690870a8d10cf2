"""The look-up of ihgp_adf8_kernel's site update from ttau alone (csrc/nagp_lookup.hpp: lookup_thresholds, lookup_mid_bits,
nearest_idx3_thr) on the host: the index counts the steps tau_i at or above ttau inside a three-wide window whose centre comes from the bit
pattern of ttau, and no step of the straight path waits for R = 1 / ttau.  tests/c/lookup_thresholds_host.cpp, built with the address and
undefined-behaviour sanitizers, compares nearest_idx3_thr with nearest_idx3_seeded -- which tests/test_ihgp_lookup_seeded_host.py holds
to numpy.argmin(abs(r - 1 / ttau)) -- exactly and with no case left out:

  every step tau_i, t_beyond and the Inf boundary t_inf, each with its four neighbouring doubles on either side;
  0, the smallest denormal, DBL_MIN and its predecessor, +Inf;
  on the reference's grid, the 1 003 627 ttau of tests/test_ihgp_lookup_seeded_host.py.

On the same points: the window holds the index, the seed is monotone, ttau > t_inf agrees with 1 / ttau < Inf (the select of the gain) and
t_inf < ttau <= t_beyond with lookup_beyond (the side branch); two calls give the same table.  Grids: logspace(-2, 4, 200)
(ihgp_ep_modulator_nmf.m:131) and the coarser logspace(-2, 4, 100)."""
import os
import re
import subprocess

import numpy as np
import pytest

from test_ihgp_lookup_seeded_host import _cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def program(tmp_path_factory):
    exe = tmp_path_factory.mktemp('lookup_thr') / 'lookup_thresholds_host'
    cc = subprocess.run(['g++', '-O1', '-g', '-std=c++17', '-Wall', '-Werror', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                         '-I', os.path.join(ROOT, 'nonstationary-audio-gp_amd', 'csrc'), '-o', str(exe),
                         os.path.join(ROOT, 'tests', 'c', 'lookup_thresholds_host.cpp')], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    return str(exe)


def _figures(line):
    return {k: v for k, v in re.findall(r'(\w+) (\S+)', line)}


@pytest.mark.parametrize('NG,full', [(200, True), (100, False)], ids=['reference-grid', 'coarser-grid'])
def test_threshold_lookup_equals_the_seeded_lookup(NG, full, program, tmp_path):
    r = np.logspace(-2, 4, NG)
    r.tofile(tmp_path / 'r.bin')
    args = [program, str(tmp_path / 'r.bin')]
    n_extra = 0
    if full:
        tt = _cases(np.logspace(-2, 4, 200))
        assert tt.size == 1003627
        tt.tofile(tmp_path / 'tt.bin'); args.append(str(tmp_path / 'tt.bin')); n_extra = tt.size
    run = subprocess.run(args, capture_output=True, text=True, timeout=120)
    print(run.stdout.strip())
    assert run.returncode == 0, run.stdout + run.stderr
    f = _figures(run.stdout)
    assert int(f['NG']) == NG and int(f['proved']) == 1
    assert int(f['points']) == 9 * (NG + 1) + 5 + n_extra
    for k in ('bad_table', 'bad_idx', 'bad_near', 'bad_special', 'bad_window', 'bad_inf', 'bad_mono'):
        assert int(f[k]) == 0, (k, run.stdout)
    # the cases reach all three ranges of ttau; the Inf boundary is the double it is known to be: 1 / ttau overflows up to 2^-1024
    assert int(f['straight']) > 9 * (NG - 1) and int(f['beyond']) >= 9 and int(f['inf']) >= 7
    assert float.fromhex(f['t_inf']) == 2.0 ** -1024 and float.fromhex(f['t_beyond']) < 1.0 / r[-1] * (1 + 1e-15)
