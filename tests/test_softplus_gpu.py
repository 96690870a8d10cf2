"""The softplus of the serial link chain of ihgp_adf8_kernel (csrc/nagp_explog.hpp: softplus_short, with its parts log1p_01 and exp_le0)
on the device against the same text compiled for the host, bit pattern by bit pattern.  tests/c/softplus_gpu.hip is a stand-alone HIP
program: one kernel per function evaluates it at every argument, the host evaluates the same function and counts the results whose 64
bits differ (two NaNs count as equal).  tests/test_softplus_host.py holds the host's form against a long double reference; this test
carries that figure over to the device.

  softplus_short  6.3 M arguments: [-750, 750], [-40, 40], round 0, every magnitude from the smallest denormal to 2^1023 in both signs,
                  the special values (+-Inf, NaN, +-0, the largest double) and the edges of the forms
  log1p_01        4.2 M arguments: [0, 1], both sides of the split at 1/2, every magnitude down to the smallest denormal
  exp_le0         the arguments -|z| of the first list

The two sides differ in one place only: the quotient f / (2 + f) of log1p_01 is the host's division and, on the device, the hardware
estimate with two Newton steps and one correction by the exact residual -- the compiler's division sequence without its scaling, which
delivers the correctly rounded quotient for these operands.  Required: no difference at all."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu


def test_device_softplus_gives_the_hosts_bits(tmp_path):
    exe = str(tmp_path / 'softplus_gpu')
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    r = subprocess.run([hipcc, '--offload-arch=gfx950', '-O3', '-std=c++17', '-I', os.path.join(ROOT, 'nonstationary-audio-gp_amd', 'csrc'),
                        '-o', exe, os.path.join(ROOT, 'tests', 'c', 'softplus_gpu.hip')], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    got = {m.group(1): (int(m.group(2)), int(m.group(3))) for m in re.finditer(r'^(\w+): (\d+) arguments, (\d+) differ', r.stdout, re.M)}
    assert set(got) == {'softplus_short', 'log1p_01', 'exp_le0'}, r.stdout
    for name, (n, differ) in got.items():
        assert n >= 4000000, (name, n)
        assert differ == 0, r.stdout
