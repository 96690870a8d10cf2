"""The softplus of the serial link chain of ihgp_adf8_kernel (csrc/nagp_explog.hpp: softplus_short = max(x, 0) + log1p_01(exp_le0(-|x|)))
as the host compiles it, against a long double reference, beside today's form log(1 + exp(x)) evaluated in double against the same
reference.  tests/c/softplus_host.cpp is a stand-alone program under the host sanitizers: no device, no library, nothing loaded into
Python.  It takes x - shift (shifts 0 and 1) on a grid of 1.5 M points over [-750, 750], a million points round 0 at two spacings, every
power of two of both signs, the edges of both forms and the special values; it measures the worst error of both forms in ulps of the
reference and requires the new form's to be no larger than the old form's and below the bound its text derives (3 ulp).

What it prints (host, x86-64, glibc):
  old form: 6004347 arguments, worst error 9.0072e+15 ulp at z = -36.7368...; 80478 arguments where it overflows and the softplus does not
  new form: 6004347 arguments, worst error 1.48584 ulp at z = -2.769..."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_short_softplus_is_no_further_from_the_truth_than_log_of_one_plus_exp(tmp_path):
    exe = str(tmp_path / 'softplus_host')
    r = subprocess.run(['c++', '-std=c++17', '-O1', '-g', '-Wall', '-Werror', '-ffp-contract=off', '-fsanitize=address,undefined',
                        '-fno-sanitize-recover=undefined', '-I', os.path.join(ROOT, 'nonstationary-audio-gp_amd', 'csrc'), '-o', exe,
                        os.path.join(ROOT, 'tests', 'c', 'softplus_host.cpp')], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=dict(os.environ, ASAN_OPTIONS='detect_leaks=1:exitcode=66'))
    print(r.stdout)
    assert r.returncode == 0 and 'special values exact, worst error within the old form' in r.stdout, r.stdout + r.stderr
    assert 'Sanitizer' not in r.stderr and 'runtime error' not in r.stderr, r.stderr
    old = re.search(r'^old form: (\d+) arguments, worst error (\S+) ulp', r.stdout, re.M)
    new = re.search(r'^new form: (\d+) arguments, worst error (\S+) ulp', r.stdout, re.M)
    assert old and new, r.stdout
    assert int(new.group(1)) == int(old.group(1)) >= 5000000
    assert float(new.group(2)) <= float(old.group(2)) and float(new.group(2)) < 3.0, r.stdout
