"""The arithmetic of the batched entry points (csrc/nagp_api_layout.hpp: budget, device-batch size, offsets of the device blocks) as a
stand-alone program under the host sanitizers: no device, no library, nothing loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_batch_plans_and_block_layouts_under_the_sanitizers(tmp_path):
    """tests/c/batch_layout_check.cpp: batch_plan against the rule written out (n = 1, n around what fits, the 32768 cap, one byte
    under / at / over the budget, the budget switch) and every entry point's block against its hand-chained offsets"""
    exe = str(tmp_path / 'batch_layout_check')
    r = subprocess.run(['c++', '-std=c++17', '-O1', '-g', '-Wall', '-Werror', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined', '-I',
                        os.path.join(ROOT, 'nonstationary-audio-gp_amd', 'csrc'), '-o', exe, os.path.join(ROOT, 'tests', 'c', 'batch_layout_check.cpp')],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60, env=dict(os.environ, ASAN_OPTIONS='detect_leaks=1:exitcode=66'))
    assert r.returncode == 0 and 'all batch plans and block layouts are as written out' in r.stdout, r.stdout + r.stderr
    assert 'Sanitizer' not in r.stderr and 'runtime error' not in r.stderr, r.stderr
