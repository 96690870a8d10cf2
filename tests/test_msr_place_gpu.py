"""The bin sums and the reduction (msr_sums, msr_reduce; csrc/nagp_momsp.hpp) on the placed copy of a rule's lists with the weights stored
through the position tables (csrc/nagp_msr_desc.hpp: msr_place_weights), against the second copy with the weights at identity positions.
The placement moves where a weight sits in c0 / c1 / c2 and nothing else: a lane adds the same numbers in the same order, so every sum must
keep its bits.  tests/c/msr_place_gpu.hip is a stand-alone HIP program: one 512-thread workgroup fills the tables with seeded values of
both signs, lets worker lane p store the three weights of point p (at c_k + p, then at c_k + pos[k][p]), runs msr_sums + msr_reduce on the
matching copy, and compares every level-2 result the reduction names and the 40 (at six dimensions) sums.  Three value sets per rule: seeded;
seeded with a quarter of the weights +0.0 or -0.0; every weight -0.0.

  rule        points   what it exercises
  ut3, CD 1   3        most lanes empty, five empty waves
  ut5, CD 2   9        one wave, no group of lanes
  ut7, CD 6   305      the headline rule: six waves, weights of most points moved, in three different permutations
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


def test_placed_weights_give_the_bits_of_identity_positions(tmp_path):
    rfile = str(tmp_path / 'rules.txt')
    write_rules(rfile, [(p, cd, cubature.utp_ws(p, cd)[1]) for p, cd in RULES])
    exe = str(tmp_path / 'msr_place_gpu')
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    r = subprocess.run([hipcc, '--offload-arch=gfx950', '-O3', '-std=c++17', '-I', os.path.join(ROOT, 'nonstationary-audio-gp_amd', 'csrc'),
                        '-o', exe, os.path.join(ROOT, 'tests', 'c', 'msr_place_gpu.hip')], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe, rfile], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    got = {}
    for m in re.finditer(r'^rule p=(\d+) CD=(\d+) npt=(\d+): (\d+) values, (\d+) differ \| moved (\d+) (\d+) (\d+)$', r.stdout, re.M):
        got[(int(m.group(1)), int(m.group(2)))] = (int(m.group(3)), int(m.group(4)), int(m.group(5)), [int(m.group(i)) for i in (6, 7, 8)])
    assert set(got) == set(RULES), r.stdout
    for rule, (npt, n, differ, moved) in got.items():
        assert n >= 3 * (rule[1] + rule[1] * (rule[1] + 1) // 2 + 2 * rule[1] + 1) and differ == 0, r.stdout
        assert all(0 <= v <= npt for v in moved), r.stdout
    # the edges the rules are chosen for
    assert got[(3, 1)][0] == 3
    assert got[(7, 6)][0] == 305 and all(v > 150 for v in got[(7, 6)][3])      # a search that moved nothing would compare a copy with itself
    assert got[(7, 6)][1] == 3 * (40 + 2 * 6 + 4 * 21 + 6 + 2 * 6 + 1)      # the 40 sums and the level-2 results they name: u, R, g1, g2, Z
