// The threshold table of the look-up from ttau (csrc/nagp_lookup.hpp: lookup_thresholds, lookup_mid_bits, nearest_idx3_thr) on the host.
//   lookup_thresholds_host r.bin [tt.bin]
// r.bin: the grid; tt.bin: further ttau values.  lr0 and inv_dlr are formed as the plan forms them (nagp_api_plan.hpp).  Every check
// counts its failures; the program prints one line of figures and returns 1 when any count is not zero.
// Built with -fsanitize=address,undefined -fno-sanitize-recover=all by tests/test_ihgp_lookup_thresholds_host.py.
#include <algorithm>
#include <cfloat>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
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
  if (argc != 2 && argc != 3) return 2;
  using namespace nagp;
  const std::vector<double> r = read_doubles(argv[1]);
  const int NG = (int)r.size();
  const double lr0 = std::log10(r[0]);
  const double inv_dlr = (double)(NG - 1) / (std::log10(r[NG - 1]) - lr0);
  const double rmax = r[NG - 1];
  const double* rp = r.data();
  std::vector<double> ext(lookup_thr_doubles(NG)), ext2(lookup_thr_doubles(NG), -1.0);
  const auto t0 = std::chrono::steady_clock::now();
  const bool ok1 = lookup_thresholds(rp, NG, lr0, inv_dlr, ext.data());
  const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
  const bool ok2 = lookup_thresholds(rp, NG, lr0, inv_dlr, ext2.data());
  long bad_table = (!ok1) + (!ok2) + (std::memcmp(ext.data(), ext2.data(), ext.size() * sizeof(double)) != 0);
  const double* ep = ext.data();
  const double t_beyond = ext[NG - 1], t_inf = ext[NG];
  const unsigned int c1 = (unsigned int)ext[NG + 1]; const int c0 = (int)ext[NG + 2];
  for (int i = 1; i < NG - 1; ++i) bad_table += !(ext[i] <= ext[i - 1]);
  bad_table += !(t_inf < t_beyond) || !(t_beyond < ext[NG - 2]);

  // the neighbourhoods: every step, t_beyond and the Inf boundary, four doubles on either side
  std::vector<double> pts;
  auto around = [&](double c) {
    unsigned long long u = lookup_to_bits(c);
    for (int d = -4; d <= 4; ++d)
      if (d >= 0 || u >= (unsigned long long)(-d)) pts.push_back(lookup_from_bits(u + d));
  };
  for (int i = 0; i < NG - 1; ++i) around(ext[i]);
  around(t_beyond); around(t_inf);
  const size_t n_near = pts.size();
  // the special values
  const double specials[] = {0.0, lookup_from_bits(1), DBL_MIN, lookup_from_bits(lookup_to_bits(DBL_MIN) - 1), INFINITY};
  for (double s : specials) pts.push_back(s);
  const size_t n_special = pts.size() - n_near;
  if (argc == 3) { const std::vector<double> tt = read_doubles(argv[2]); pts.insert(pts.end(), tt.begin(), tt.end()); }

  long bad_idx = 0, bad_window = 0, bad_inf = 0, bad_near = 0, bad_special = 0, n_straight = 0, n_beyond = 0, n_inf = 0;
  for (size_t q = 0; q < pts.size(); ++q) {
    volatile double t = pts[q];                // (the division is the one the kernel performs: no reciprocal folded at compile time)
    const int want = nearest_idx3_seeded(rp, NG, lr0, inv_dlr, rmax, t);
    const int got = nearest_idx3_thr(rp, ep, NG, t);
    const bool miss = got != want;
    bad_idx += miss;
    if (q < n_near) bad_near += miss; else if (q < n_near + n_special) bad_special += miss;
    const double R = 1.0 / t;
    // the comparison that replaces Rn < INFINITY in the gain, and the one that enters the branch beyond the grid
    bad_inf += ((t > t_inf) != (R < INFINITY)) + ((t <= t_beyond && t > t_inf) != lookup_beyond(rmax, R));
    if (t <= t_inf) ++n_inf;
    else if (t <= t_beyond) ++n_beyond;
    else {
      ++n_straight;
      const int mid = lookup_mid_bits(NG - 2, c1, c0, t);
      bad_window += !(want >= mid - 1 && want <= mid + 1);
    }
  }
  // the seed is monotone (non-increasing in ttau) over everything above
  std::vector<double> s(pts);
  std::sort(s.begin(), s.end());
  long bad_mono = 0;
  for (size_t q = 1; q < s.size(); ++q)
    bad_mono += lookup_mid_bits(NG - 2, c1, c0, s[q]) > lookup_mid_bits(NG - 2, c1, c0, s[q - 1]);
  printf("NG %d proved %d search_us %.1f points %zu straight %ld beyond %ld inf %ld t_inf %a t_beyond %a c1 %u c0 %d bad_table %ld bad_idx %ld bad_near %ld "
         "bad_special %ld bad_window %ld bad_inf %ld bad_mono %ld\n", NG, (int)ok1, us, pts.size(), n_straight, n_beyond, n_inf, t_inf, t_beyond, c1, c0, bad_table, bad_idx,
         bad_near, bad_special, bad_window, bad_inf, bad_mono);
  return (bad_table || bad_idx || bad_window || bad_inf || bad_mono) ? 1 : 0;
}
