"""Which form of Q / 2Q / v the three-barrier ihgp_adf8_kernel of a plan is instantiated with (csrc/nagp_qform.hpp: qform_pick and its
companions), as a stand-alone program under the host sanitizers: no device, no library, nothing loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_number_of_sub_bands_takes_the_form_written_out(tmp_path):
    """tests/c/qform_host.cpp: D = 1 .. 63 -- K = 4 / 8 / 16 and PAD against the rule written out, D = 16 -> K4, D = 32 -> K8, D > 32 ->
    K16-pad, every other D and every D under the developer switch -> the run-time form; a fixed form serves exactly the D it is picked for"""
    exe = str(tmp_path / 'qform_host')
    r = subprocess.run(['c++', '-std=c++17', '-O1', '-g', '-Wall', '-Werror', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined', '-I',
                        os.path.join(ROOT, 'nonstationary-audio-gp_amd', 'csrc'), '-o', exe, os.path.join(ROOT, 'tests', 'c', 'qform_host.cpp')],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60, env=dict(os.environ, ASAN_OPTIONS='detect_leaks=1:exitcode=66'))
    assert r.returncode == 0 and 'every D in 1 .. 63 takes the form written out' in r.stdout, r.stdout + r.stderr
    assert 'Sanitizer' not in r.stderr and 'runtime error' not in r.stderr, r.stderr
