"""The seeded table look-up of the three-barrier schedule of ihgp_adf8_kernel (csrc/nagp_lookup.hpp: lookup_mid_ttau, nearest_idx3_seeded) on
the host: the centre of the three-point window comes from ttau, beside the division R = 1 / ttau; R only decides the branch beyond the grid
and picks among the three.  A small stand-alone program includes the header, reads a grid and a list of ttau and writes, for each, the
seeded index and nearest_idx3_sl(..., 1 / ttau); the first is compared, exactly and with no case left out, with
numpy.argmin(abs(r - 1 / ttau)) -- the first minimiser, 0 for a non-finite R -- on the reference's grid logspace(-2, 4, 200)
(ihgp_ep_modulator_nmf.m:131), and with the second.  lr0 and inv_dlr are formed as the plan forms them (nagp_api_plan.hpp)."""
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
  const std::vector<double> r = read_doubles(argv[1]), tt = read_doubles(argv[2]);
  const int NG = (int)r.size();
  const double lr0 = std::log10(r[0]);
  const double inv_dlr = (double)(NG - 1) / (std::log10(r[NG - 1]) - lr0);
  std::vector<int> idx(2 * tt.size());
  const double* rp = r.data();
  for (size_t i = 0; i < tt.size(); ++i) {
    volatile double t = tt[i];                 // (the division is the one the kernel performs: no reciprocal folded at compile time)
    idx[2 * i] = nagp::nearest_idx3_seeded(rp, NG, lr0, inv_dlr, r[NG - 1], t);
    idx[2 * i + 1] = nagp::nearest_idx3_sl(rp, NG, lr0, inv_dlr, r[NG - 1], 1.0 / t);
  }
  FILE* f = fopen(argv[3], "wb");
  if (!f || fwrite(idx.data(), sizeof(int), idx.size(), f) != idx.size()) { perror(argv[3]); return 2; }
  fclose(f);
  return 0;
}
"""

DBL_MIN = np.finfo(np.float64).tiny


def _ulps(x, n):
    for _ in range(abs(n)):
        x = np.nextafter(x, np.inf if n > 0 else -np.inf)
    return x


def _cases(r):
    lin = 0.5 * (r[:-1] + r[1:])
    base = np.concatenate([1.0 / r, 1.0 / lin])                        # reciprocals of every grid value and every midpoint
    parts = [base]
    for n in (-4, -3, -2, -1, 1, 2, 3, 4):                             # ... stepped so that 1 / ttau falls on both sides
        parts.append(_ulps(base, n))
    rmax = r[-1]
    edge = [0.0, 5e-324, 1e-320, 1e-310, 2.0 ** -1024, _ulps(2.0 ** -1024, 1), _ulps(2.0 ** -1024, -1), 5.562684646268003e-309,
            _ulps(DBL_MIN, -2), _ulps(DBL_MIN, -1), DBL_MIN, _ulps(DBL_MIN, 1), _ulps(DBL_MIN, 2), 1e-300, 1e-100, 1e-20,
            1e300, np.finfo(np.float64).max, np.inf]
    edge += [_ulps(1.0 / rmax, n) for n in range(-8, 9)]              # the neighbourhood of 1 / rmax: the branch beyond the grid begins here
    parts.append(np.array(edge, np.float64))
    rng = np.random.default_rng(31337)
    parts.append(10.0 ** rng.uniform(-7.0, 5.0, 1000000))
    return np.concatenate(parts)


def _argmin_first(r, R):
    out = np.empty(R.size, np.int64)
    with np.errstate(invalid='ignore'):
        for a in range(0, R.size, 50000):
            out[a:a + 50000] = np.argmin(np.abs(r[None, :] - R[a:a + 50000, None]), axis=1)
    out[~np.isfinite(R)] = 0
    return out


def test_seeded_lookup_equals_argmin_for_every_case(tmp_path):
    r = np.logspace(-2, 4, 200)
    tt = _cases(r)
    assert tt.size == 399 * 9 + 19 + 17 + 1000000 and np.all(tt >= 0.0)
    src = tmp_path / 'lookup_seeded_host.cpp'; exe = tmp_path / 'lookup_seeded_host'
    src.write_text(PROGRAM)
    cc = subprocess.run(['g++', '-O2', '-std=c++17', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'nonstationary-audio-gp_amd', 'csrc'),
                         '-o', str(exe), str(src)], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    r.tofile(tmp_path / 'r.bin'); tt.tofile(tmp_path / 'tt.bin')
    run = subprocess.run([str(exe), str(tmp_path / 'r.bin'), str(tmp_path / 'tt.bin'), str(tmp_path / 'idx.bin')], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr
    got = np.fromfile(tmp_path / 'idx.bin', np.int32).reshape(-1, 2)
    with np.errstate(divide='ignore', over='ignore'):
        R = 1.0 / tt
    ref = _argmin_first(r, R)
    assert got.shape == (ref.size, 2)
    bad = np.flatnonzero(got[:, 0] != ref)
    assert bad.size == 0, [(float(tt[i]), float(R[i]), int(got[i, 0]), int(ref[i])) for i in bad[:10]]
    assert np.array_equal(got[:, 0], got[:, 1])                         # the contract with nearest_idx3_sl, case by case
    # the cases do what they are named for: every index, both sides of every midpoint, the branch beyond the grid, R = Inf (zero and the
    # denormals whose reciprocal overflows: index 0, the other end of the grid from where -log10 ttau points) and R = 0
    assert set(ref.tolist()) == set(range(200))
    mid = slice(200, 399)
    lo = np.stack([ref[399 * (1 + q):399 * (2 + q)][mid] for q in range(8)])
    assert np.all(lo.min(axis=0) + 1 == lo.max(axis=0))
    assert np.sum(np.isfinite(R) & (R > r[-1])) > 1000 and np.sum(np.isinf(R)) >= 6 and np.sum(np.isinf(R) & (tt > 0.0)) >= 5 and np.sum(R == 0.0) == 1
    assert np.all(got[np.isinf(R), 0] == 0)
