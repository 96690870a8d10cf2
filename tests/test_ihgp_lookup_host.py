"""The straight-line table look-up of the three-barrier schedule of ihgp_adf8_kernel (csrc/nagp_lookup.hpp: nearest_idx3_sl) on the host:
a small stand-alone program includes the header, reads a grid and a list of R and writes the indices; they are compared, exactly and with
no case left out, with numpy.argmin(abs(r - R)) -- the first minimiser, 0 for a non-finite R -- on the reference's grid
logspace(-2, 4, 200) (ihgp_ep_modulator_nmf.m:131).  lr0 and inv_dlr are formed as the plan forms them (nagp_api_plan.hpp)."""
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "nagp_lookup.hpp"

static std::vector<double> read_doubles(const char* path) {
  FILE* f = fopen(path, "rb");
  if (!f) { perror(path); exit(2); }
  fseek(f, 0, SEEK_END); const long n = ftell(f) / 8; fseek(f, 0, SEEK_SET);
  std::vector<double> v(n);
  if (fread(v.data(), 8, n, f) != (size_t)n) { perror(path); exit(2); }
  fclose(f);
  return v;
}

int main(int argc, char** argv) {
  if (argc != 4) return 2;
  const std::vector<double> r = read_doubles(argv[1]), R = read_doubles(argv[2]);
  const int NG = (int)r.size();
  const double lr0 = std::log10(r[0]);
  const double inv_dlr = (double)(NG - 1) / (std::log10(r[NG - 1]) - lr0);
  std::vector<int> idx(R.size());
  const double* rp = r.data();
  for (size_t i = 0; i < R.size(); ++i) idx[i] = nagp::nearest_idx3_sl(rp, NG, lr0, inv_dlr, r[NG - 1], R[i]);
  FILE* f = fopen(argv[3], "wb");
  if (!f || fwrite(idx.data(), sizeof(int), idx.size(), f) != idx.size()) { perror(argv[3]); return 2; }
  fclose(f);
  return 0;
}
"""


def _ulps(x, n):
    for _ in range(abs(n)):
        x = np.nextafter(x, np.inf if n > 0 else -np.inf)
    return x


def _cases(r):
    lin = 0.5 * (r[:-1] + r[1:]); geo = np.sqrt(r[:-1] * r[1:])
    parts = [r, lin, geo]
    for m in (lin, geo):
        for n in (-3, -2, -1, 1, 2, 3):
            parts.append(_ulps(m, n))
    rmax = r[-1]
    parts.append(np.array([0.0, 5e-324, 1e-310, -1.0, np.inf, -np.inf, np.nan, rmax, np.nextafter(rmax, np.inf), 1e5, 1e20, 1e100, 1e300]))
    rng = np.random.default_rng(90210)
    parts.append(10.0 ** rng.uniform(-6.0, 8.0, 1000000))
    return np.concatenate(parts)


def _argmin_first(r, R):
    out = np.empty(R.size, np.int64)
    with np.errstate(invalid='ignore'):
        for a in range(0, R.size, 50000):
            out[a:a + 50000] = np.argmin(np.abs(r[None, :] - R[a:a + 50000, None]), axis=1)
    out[~np.isfinite(R)] = 0
    return out


def test_straight_line_lookup_equals_argmin_for_every_case(tmp_path):
    r = np.logspace(-2, 4, 200)
    R = _cases(r)
    assert R.size == 200 + 2 * 199 * 7 + 13 + 1000000
    src = tmp_path / 'lookup_host.cpp'; exe = tmp_path / 'lookup_host'
    src.write_text(PROGRAM)
    cc = subprocess.run(['g++', '-O2', '-std=c++17', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'nonstationary-audio-gp_amd', 'csrc'),
                         '-o', str(exe), str(src)], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    r.tofile(tmp_path / 'r.bin'); R.tofile(tmp_path / 'R.bin')
    run = subprocess.run([str(exe), str(tmp_path / 'r.bin'), str(tmp_path / 'R.bin'), str(tmp_path / 'idx.bin')], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr
    got = np.fromfile(tmp_path / 'idx.bin', np.int32)
    ref = _argmin_first(r, R)
    assert got.shape == ref.shape
    bad = np.flatnonzero(got != ref)
    assert bad.size == 0, [(float(R[i]), int(got[i]), int(ref[i])) for i in bad[:10]]
    # the cases do what they are named for: both ends of the grid, every index, the branch beyond the grid and the non-finite inputs
    assert set(ref.tolist()) == set(range(200)) and np.sum(np.isfinite(R) & (R > r[-1])) > 1000 and np.sum(~np.isfinite(R)) == 3
