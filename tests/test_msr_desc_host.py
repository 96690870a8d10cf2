"""The member / term lists of the role layout's cubature sums (csrc/nagp_msr_desc.hpp: msr_build_desc) as a stand-alone program under the
host sanitizers: no device, no library, nothing loaded into Python.  tests/c/msr_desc_host.cpp builds the lists of every rule the role
layout accepts -- ut3 / ut5 / ut7 / ut9 in 1 .. 6 dimensions with at most 320 points -- and checks both copies (the chunks as they come,
which msr_sums' other users read, and the chunks placed for few LDS bank conflicts, which the three-barrier ihgp_adf8_kernel reads):

  - every bin holds each of its points exactly once, in one kind of weight
  - every level-2 term names a level-1 slot of its own wave, or the zero word (then with zero table factors)
  - the second copy holds exactly the lanes of the first (a lane's member list and group flag): what a sum adds, and in which order, is the
    same; and its member reads cost no more LDS cycles than the first copy's (counted by the program's own restatement of the bank rule)
  - the 40 sums of msr_sums + msr_reduce, evaluated in integers, are the dense sums exactly

and prints which rules fit the six worker waves.  That set is the one the first-fit packing has always accepted; it is listed here.  For the
headline rule (ut7, 6 dimensions, 305 points) the placement must take at least a tenth off the cycles of the member reads."""
import os
import re
import subprocess

import numpy as np

from nagp import cubature

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (p, CD) of the rules with at most 320 points that do NOT fit; every other one fits
NO_FIT = set()


def _rules():
    out = []
    for p in (3, 5, 7, 9):
        for cd in range(1, 7):
            _, sx = cubature.utp_ws(p, cd)
            if sx.shape[1] <= 320:
                out.append((p, cd, sx))
    return out


def write_rules(path, rules):
    with open(path, 'w') as f:
        for p, cd, sx in rules:
            f.write('%d %d %d\n' % (p, cd, sx.shape[1]))
            f.write(' '.join(repr(float(v)) for v in np.ascontiguousarray(sx.T).ravel()) + '\n')


def test_lists_of_every_rule_of_the_role_layout(tmp_path):
    rules = _rules()
    assert {(p, cd) for p, cd, _ in rules} >= {(3, 1), (5, 2), (7, 6), (9, 4)} and len(rules) >= 20
    rfile = str(tmp_path / 'rules.txt')
    write_rules(rfile, rules)
    exe = str(tmp_path / 'msr_desc_host')
    r = subprocess.run(['c++', '-std=c++17', '-O1', '-g', '-Wall', '-Werror', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined', '-I',
                        os.path.join(ROOT, 'nonstationary-audio-gp_amd', 'csrc'), '-o', exe, os.path.join(ROOT, 'tests', 'c', 'msr_desc_host.cpp')],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe, rfile], capture_output=True, text=True, timeout=120, env=dict(os.environ, ASAN_OPTIONS='detect_leaks=1:exitcode=66'))
    print(r.stdout)
    assert r.returncode == 0 and 'checked %d rules' % len(rules) in r.stdout, r.stdout + r.stderr
    assert 'Sanitizer' not in r.stderr and 'runtime error' not in r.stderr, r.stderr
    got = {(int(m.group(1)), int(m.group(2))): (m.group(3) == 'fits', m.group(4) and (int(m.group(4)), int(m.group(5))))
           for m in re.finditer(r'^rule p=(\d+) CD=(\d+) npt=\d+: (fits|does not fit)(?:, member reads (\d+) -> (\d+) LDS cycles)?$', r.stdout, re.M)}
    assert set(got) == {(p, cd) for p, cd, _ in rules}
    assert {k for k, (fits, _) in got.items() if not fits} == NO_FIT, got
    before, after = got[(7, 6)][1]
    assert after <= 0.9 * before, (before, after)
