// eps_layout_check.cpp -- the device block and the budget rule of nagp_ep_sample (eps_block, eps_fixed_bytes, eps_draw_bytes of
// csrc/nagp_api_layout.hpp) with their own main, on the CPU under -fsanitize=address,undefined (built and run by
// tests/test_epsample_host.py, as tests/c/batch_layout_check.cpp is for the other batched entry points): the block against its offsets
// chained by hand, for every combination of the optional parts, and the budget rule of include/nagp.h against the block it must cover.
#include "nagp_api_layout.hpp"

#include <cstdio>
#include <initializer_list>

using namespace nagp;

static int bad = 0;
#define CHECK(x) do { if (!(x)) { fprintf(stderr, "line %d: %s\n", __LINE__, #x); ++bad; } } while (0)
#define SAME(got, want) do { const size_t g_ = (got), w_ = (want); if (g_ != w_) { fprintf(stderr, "line %d: %s = %zu, expected %zu\n", __LINE__, #got, g_, w_); ++bad; } } while (0)

int main() {
  for (int bits = 0; bits < 16; ++bits)
    for (size_t nb : {(size_t)1, (size_t)3, (size_t)16})
      for (size_t DN : {(size_t)0, (size_t)6}) {
        const bool z = bits & 1, x = bits & 2, f = bits & 4, sd = bits & 8;
        const size_t S = 7, M = 3, T = 5, nb2 = 2 * 2 + 2 * 2 + 3 * 3, SS = S * S;            // blocks of 2, 2, 3 states; an odd count of ints
        const size_t o_A = 0, o_Q = o_A + SS, o_p0 = o_Q + SS, o_ab = o_p0 + SS, o_qb = o_ab + nb2, o_h = o_qb + nb2, o_idx = o_h + M,
                     o_w = o_idx + (2 * M + 2 + S) / 2 + 1, o_tt = o_w + DN, o_tn = o_tt + T * M, o_y = o_tn + T * M, o_mf = o_y + T, o_pg = o_mf + T * S,
                     o_lc = o_pg + T * SS, o_ms = o_lc + T * SS, o_cnt = o_ms + T * S, o_z = o_cnt + 4, o_x = o_z + (z ? nb * T * S : 0),
                     o_f = o_x + (x ? nb * T * S : 0), o_sd = o_f + (f || sd ? nb * T * M : 0), total = o_sd + (sd ? nb * T : 0) + 2;
        const EpsBlock o = eps_block(S, M, T, nb2, DN, z, x, f, sd, nb);
        SAME(o.A, o_A); SAME(o.Q, o_Q); SAME(o.p0, o_p0); SAME(o.ab, o_ab); SAME(o.qb, o_qb); SAME(o.h, o_h); SAME(o.idx, o_idx); SAME(o.w, o_w);
        SAME(o.tt, o_tt); SAME(o.tn, o_tn); SAME(o.y, o_y); SAME(o.mf, o_mf); SAME(o.pg, o_pg); SAME(o.lc, o_lc); SAME(o.ms, o_ms); SAME(o.cnt, o_cnt);
        SAME(o.z, o_z); SAME(o.x, o_x); SAME(o.f, o_f); SAME(o.sd, o_sd); SAME(o.total, total);
        CHECK((2 * M + 2 + S) * sizeof(int) <= (o_w - o_idx) * sizeof(double));                // the three index tables fit their part
        // the budget rule of the header covers the block, and is the formula written there
        const size_t fixed = eps_fixed_bytes(S, M, T, nb2, DN), per = eps_draw_bytes(S, M, T, z, x, f, sd);
        SAME(fixed, 8 * (T * (2 * SS + 2 * S + 2 * M + 1) + 3 * SS + 2 * nb2 + M + DN + 8) + 4 * (2 * M + 2 + S) + 4096);
        SAME(per, bits ? 8 * T * ((z ? S : 0) + (x ? S : 0) + (f || sd ? M : 0) + (sd ? 1 : 0)) : 8);
        CHECK(o.total * sizeof(double) <= fixed + nb * per);
        const BatchPlan p = batch_plan(50, fixed + 3 * per, fixed, per);                       // room for three draws: batches of three
        CHECK(p.ok && p.nb == 3);
        CHECK(!batch_plan(50, fixed + per - 1, fixed, per).ok);
      }
  if (bad) { fprintf(stderr, "%d mismatches\n", bad); return 1; }
  printf("the block and the budget rule of nagp_ep_sample are as written out\n");
  return 0;
}
