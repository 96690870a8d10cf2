"""The bin sums and the reduction (msr_sums, msr_reduce; csrc/nagp_momsp.hpp) on the two copies of a rule's lists (csrc/nagp_msr_desc.hpp):
the chunks as they come, which the other role kernels read, and the chunks placed for few LDS bank conflicts, which the three-barrier
ihgp_adf8_kernel reads.  A chunk keeps its members, their lanes within its group and their slots, so every sum must keep its bits.
tests/c/msr_sums_gpu.hip is a stand-alone HIP program: one 512-thread workgroup fills the tables and c0 / c1 / c2 with seeded values of both
signs, runs msr_sums + msr_reduce on the first copy and on the second, and compares every level-2 result the reduction names and the 40 (at
six dimensions) sums.  Three value sets per rule: seeded; seeded with a quarter of the weights +0.0 or -0.0; every weight -0.0.

  rule        points   what it exercises
  ut3, CD 1   3        no pair bins, most lanes empty, five empty waves
  ut5, CD 2   9        one wave, no group of lanes
  ut7, CD 6   305      the headline rule: groups of 4 lanes, six waves, one total per wave in the second copy
  ut9, CD 3   77       two waves, the second partly filled
  ut9, CD 4   193      points with four non-centre coordinates

Required: no difference at all."""
import os
import re
import subprocess

import pytest

from test_msr_desc_host import write_rules
from nagp import cubature

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

RULES = [(3, 1), (5, 2), (7, 6), (9, 3), (9, 4)]


def test_both_forms_of_the_bin_sums_give_the_same_bits(tmp_path):
    rfile = str(tmp_path / 'rules.txt')
    write_rules(rfile, [(p, cd, cubature.utp_ws(p, cd)[1]) for p, cd in RULES])
    exe = str(tmp_path / 'msr_sums_gpu')
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    r = subprocess.run([hipcc, '--offload-arch=gfx950', '-O3', '-std=c++17', '-I', os.path.join(ROOT, 'nonstationary-audio-gp_amd', 'csrc'),
                        '-o', exe, os.path.join(ROOT, 'tests', 'c', 'msr_sums_gpu.hip')], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe, rfile], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    got = {}
    for m in re.finditer(r'^rule p=(\d+) CD=(\d+) npt=(\d+): (\d+) values, (\d+) differ \| lanes((?: \d+){6}) \| lanes((?: \d+){6})$', r.stdout, re.M):
        got[(int(m.group(1)), int(m.group(2)))] = (int(m.group(3)), int(m.group(4)), int(m.group(5)), [int(v) for v in m.group(6).split()],
                                                   [int(v) for v in m.group(7).split()])
    assert set(got) == set(RULES), r.stdout
    for rule, (npt, n, differ, first, second) in got.items():
        assert n >= 3 * (rule[1] + rule[1] * (rule[1] + 1) // 2 + 2 * rule[1] + 1) and differ == 0, r.stdout
        assert sum(first) == sum(second) > 0, (rule, first, second)
    # the edges the rules are chosen for
    assert got[(3, 1)][0] == 3 and got[(3, 1)][3].count(0) == 5
    assert got[(7, 6)][0] == 305 and all(got[(7, 6)][3]) and all(got[(7, 6)][4]) and got[(7, 6)][3] != got[(7, 6)][4]
    assert got[(7, 6)][1] == 3 * (40 + 2 * 6 + 4 * 21 + 6 + 2 * 6 + 1)      # the 40 sums and the level-2 results they name: u, R, g1, g2, Z
    assert any(0 < v < 64 for v in got[(9, 3)][4])
