"""The placed copy of the role layout's lists and its position tables (csrc/nagp_msr_desc.hpp: msr_place_weights) as a stand-alone program
under the host sanitizers: no device, no library, nothing loaded into Python.  The three-barrier ihgp_adf8_kernel stores a point's three
weights at pos[k][p] inside c0 / c1 / c2 and reads the bin sums' members from there; tests/c/msr_place_host.cpp checks, for every rule the
role layout accepts -- ut3 / ut5 / ut7 / ut9 in 1 .. 6 dimensions with at most 320 points:

  - each pos[k] is an injection into [0, 64 * MSR_NWK)
  - the placed copy's member addresses, mapped back through the inverse positions, are the second copy of msr_build_desc word for word;
    group flags, terms and reduce words are equal too
  - the 40 sums of msr_sums + msr_reduce, evaluated in integers with the weights stored at their positions, are the dense sums exactly
  - two calls return identical tables, and a call without a search returns the second copy and identity positions
  - modelled LDS cycles (the program's own restatement of the bank rule): member reads of the six waves plus the three weight stores of
    every wave that holds a point (lane = point - 64 wave; a lane without a point does not store and counts for nothing) are no more than
    the second copy's at identity positions, and equal what msr_place_weights reports

For the headline rule (ut7, 6 dimensions, 305 points) reads + stores must be at most 75 % of the second copy's."""
import os
import re
import subprocess

from test_msr_desc_host import _rules, write_rules

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_placed_copy_of_every_rule_of_the_role_layout(tmp_path):
    rules = _rules()
    assert {(p, cd) for p, cd, _ in rules} >= {(3, 1), (5, 2), (7, 6), (9, 4)} and len(rules) >= 20
    rfile = str(tmp_path / 'rules.txt')
    write_rules(rfile, rules)
    exe = str(tmp_path / 'msr_place_host')
    r = subprocess.run(['c++', '-std=c++17', '-O1', '-g', '-Wall', '-Werror', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined', '-I',
                        os.path.join(ROOT, 'nonstationary-audio-gp_amd', 'csrc'), '-o', exe, os.path.join(ROOT, 'tests', 'c', 'msr_place_host.cpp')],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe, rfile], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS='detect_leaks=1:exitcode=66'))
    print(r.stdout)
    assert r.returncode == 0 and 'checked %d rules' % len(rules) in r.stdout, r.stdout + r.stderr
    assert 'Sanitizer' not in r.stderr and 'runtime error' not in r.stderr, r.stderr
    got = {(int(m.group(1)), int(m.group(2))): tuple(int(m.group(i)) for i in range(3, 7))
           for m in re.finditer(r'^rule p=(\d+) CD=(\d+) npt=\d+: reads (\d+) stores (\d+) -> reads (\d+) stores (\d+) LDS cycles \|', r.stdout, re.M)}
    assert set(got) == {(p, cd) for p, cd, _ in rules}, r.stdout
    for rule, (r0, s0, r1, s1) in got.items():
        assert r1 + s1 <= r0 + s0, (rule, r0, s0, r1, s1)
    r0, s0, r1, s1 = got[(7, 6)]
    assert r1 + s1 <= 0.75 * (r0 + s0), (r0, s0, r1, s1)
