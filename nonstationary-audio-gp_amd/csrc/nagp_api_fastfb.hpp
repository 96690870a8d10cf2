// part of nagp_api.hip: stationary filterbank: kernel_ss_kalmanFastFB (see include/nagp.h)
extern "C" int nagp_fastfb_run(int32_t S, const double* A, const double* AKHA, const double* HA, const double* K, const double* G,
                               const double* y, int64_t T, double* MS, double* sum_v2, int32_t device) {
  if (!A || !AKHA || !HA || !K || !y || !MS) FAIL(NAGP_EINVAL, "null argument");
  if (S < 1 || T < 1) FAIL(NAGP_EINVAL, "bad sizes (S=%d T=%lld)", S, (long long)T);
  // S <= 96: both constant S x S matrices of a pass live in the LDS; 96 < S <= 256 (a thread per state): they stay in global memory (L2-resident)
  const int mat_global = (fb_lds_doubles(S) * sizeof(double) > 160 * 1024) ? 1 : 0;
  const size_t lds = fb_lds_doubles(S, mat_global) * sizeof(double);
  if (S > 256) FAIL(NAGP_EUNSUPPORTED, "S=%d: the stationary filterbank runs a thread per state (S <= 256)", S);
  if (hipSetDevice(device) != hipSuccess) FAIL(NAGP_EHIP, "hipSetDevice(%d)", device);
  // spans of the parallel-in-time form (needs two more (S+4) x (S+4) work matrices in LDS: fb_compose_lds_doubles fits 160 KiB up to S = 69); short series run as one span
  const size_t lds_c = fb_compose_lds_doubles(S) * sizeof(double);
  int ns = 1;
  if (lds_c <= 160 * 1024 && T >= 2048 && !read_dev_switches().fb_sequential) ns = (int)std::min<int64_t>(512, T / 128);
  const int64_t L = (T + ns - 1) / ns;
  ns = (int)((T + L - 1) / L);
  const size_t SS = (size_t)S * S, SP = (size_t)S + 4;
  const size_t o_A = 0, o_B = o_A + SS, o_G = o_B + SS, o_ha = o_G + SS, o_k = o_ha + S, o_y = o_k + S, o_ms = o_y + T,
               o_sv = o_ms + (size_t)T * S, o_phi = o_sv + ns + 1, o_st = o_phi + (size_t)ns * S * SP, total = o_st + (size_t)ns * S + 2;
  DevBlock blk;
  API_ALLOC(blk, device, total); double* const dev = blk.p;
  int st = NAGP_OK;
  API_HIP(nagp_fastfb_run, hipMemcpy(dev + o_A, A, SS * 8, hipMemcpyHostToDevice));
  API_HIP(nagp_fastfb_run, hipMemcpy(dev + o_B, AKHA, SS * 8, hipMemcpyHostToDevice));
  if (G) API_HIP(nagp_fastfb_run, hipMemcpy(dev + o_G, G, SS * 8, hipMemcpyHostToDevice));
  API_HIP(nagp_fastfb_run, hipMemcpy(dev + o_ha, HA, (size_t)S * 8, hipMemcpyHostToDevice));
  API_HIP(nagp_fastfb_run, hipMemcpy(dev + o_k, K, (size_t)S * 8, hipMemcpyHostToDevice));
  API_HIP(nagp_fastfb_run, hipMemcpy(dev + o_y, y, (size_t)T * 8, hipMemcpyHostToDevice));
  const int NT = std::max(64, roundup64(S));
  if (st == NAGP_OK) st = set_lds(fastfb_filter_kernel, lds);
  if (st == NAGP_OK) st = set_lds(fastfb_smoother_kernel, lds);
  if (st == NAGP_OK && ns > 1) st = set_lds(fastfb_compose_kernel<false>, lds_c);
  if (st == NAGP_OK && ns > 1) st = set_lds(fastfb_compose_kernel<true>, lds_c);
  if (st == NAGP_OK) {
    FbPar fp{S, T, dev + o_A, dev + o_B, dev + o_ha, dev + o_k, dev + o_y, dev + o_ms, dev + o_sv, L, ns, dev + o_phi,
             ns > 1 ? dev + o_st : nullptr, mat_global};
    if (ns > 1) {
      hipLaunchKernelGGL(fastfb_compose_kernel<false>, dim3(ns), dim3(256), lds_c, 0, fp);
      hipLaunchKernelGGL(fastfb_boundary_kernel<false>, dim3(1), dim3(256), 0, 0, fp);
    }
    hipLaunchKernelGGL(fastfb_filter_kernel, dim3(ns), dim3(NT), lds, 0, fp);
    if (G && T > 1) {
      fp.B = dev + o_G;
      // the T-1 smoothing steps are partitioned with the same span length
      const int nss = (int)((T - 1 + L - 1) / L);
      fp.ns = nss;
      if (ns > 1) {
        hipLaunchKernelGGL(fastfb_compose_kernel<true>, dim3(nss), dim3(256), lds_c, 0, fp);
        hipLaunchKernelGGL(fastfb_boundary_kernel<true>, dim3(1), dim3(256), 0, 0, fp);
      }
      hipLaunchKernelGGL(fastfb_smoother_kernel, dim3(nss), dim3(NT), lds, 0, fp);
    }
  }
  API_HIP(nagp_fastfb_run, hipGetLastError());
  API_HIP(nagp_fastfb_run, hipDeviceSynchronize());
  API_HIP(nagp_fastfb_run, hipMemcpy(MS, dev + o_ms, (size_t)T * S * 8, hipMemcpyDeviceToHost));
  if (sum_v2) {
    std::vector<double> part((size_t)ns);
    API_HIP(nagp_fastfb_run, hipMemcpy(part.data(), dev + o_sv, (size_t)ns * 8, hipMemcpyDeviceToHost));
    double acc = 0.0;
    for (int j = 0; j < ns; ++j) acc += part[j];      // fixed order
    *sum_v2 = acc;
  }
  return st;
}

// ---------------------------------------------------------------------------------------------
// stationary filterbank: joint posterior draws by the simulation smoother (see include/nagp.h, nagp_fbsample.hpp)
constexpr size_t FBS_BUDGET_BYTES = (size_t)8 << 30;      // device memory of one call: the draws run in device batches under it
constexpr int FBS_ONE_SPAN_DRAWS = 256;                   // from this many draws on, one span per draw fills the chip

// M^n of a column-major S x S matrix in the layout of the boundary pass: out[i * (S+4) + l] = (M^n)(i,l)
static void fbs_matrix_power(const double* M, int S, int64_t n, double* out) {
  const size_t SS = (size_t)S * S;
  std::vector<double> r(SS, 0.0), b(SS), t(SS);
  for (int i = 0; i < S; ++i) { r[(size_t)i * S + i] = 1.0; for (int l = 0; l < S; ++l) b[(size_t)i * S + l] = M[i + (size_t)l * S]; }
  auto mul = [&](const std::vector<double>& x, const std::vector<double>& z) {
    std::fill(t.begin(), t.end(), 0.0);
    for (int i = 0; i < S; ++i)
      for (int q = 0; q < S; ++q) { const double xv = x[(size_t)i * S + q]; for (int l = 0; l < S; ++l) t[(size_t)i * S + l] += xv * z[(size_t)q * S + l]; }
  };
  for (; n > 0; n >>= 1) {
    if (n & 1) { mul(r, b); r.swap(t); }
    if (n > 1) { mul(b, b); b.swap(t); }
  }
  for (int i = 0; i < S; ++i) for (int l = 0; l < S + 4; ++l) out[(size_t)i * (S + 4) + l] = l < S ? r[(size_t)i * S + l] : 0.0;
}

extern "C" int nagp_fastfb_sample(int32_t S, const double* A, const double* AKHA, const double* HA, const double* K, const double* G,
                                  const double* H, double R, const double* Lp, const double* Lq, const double* y, int64_t T,
                                  int32_t n_draws, uint64_t seed, double* Ydraw, double* Xdraw, double* MS, int32_t device) {
  if (!A || !AKHA || !HA || !K || !G || !H || !Lp || !Lq || !y) FAIL(NAGP_EINVAL, "null argument (there is no filter-only form: G is required)");
  if (S < 1 || T < 1 || n_draws < 1) FAIL(NAGP_EINVAL, "bad sizes (S=%d T=%lld n_draws=%d)", S, (long long)T, n_draws);
  if (!(R > 0.0) || !std::isfinite(R)) FAIL(NAGP_EINVAL, "the observation variance R must be positive and finite");
  if (!Ydraw && !Xdraw && !MS) FAIL(NAGP_EINVAL, "no output requested");
  if (S > 256) FAIL(NAGP_EUNSUPPORTED, "S=%d: the stationary filterbank runs a thread per state (S <= 256)", S);
  const DevSwitches dev_sw = read_dev_switches();
  const int mat_global = (fb_lds_doubles(S) * sizeof(double) > 160 * 1024) ? 1 : 0;
  const size_t lds = fb_lds_doubles(S, mat_global) * sizeof(double);
  const size_t lds_c = fb_compose_lds_doubles(S) * sizeof(double);
  // spans as in nagp_fastfb_run (the filter's span matrices come from its compose pass); one span per draw for short series and large batches
  int ns = 1;
  if (lds_c <= 160 * 1024 && T >= 2048 && n_draws < FBS_ONE_SPAN_DRAWS && !dev_sw.fb_sequential) ns = (int)std::min<int64_t>(512, T / 128);
  const int64_t L = (T + ns - 1) / ns;
  ns = (int)((T + L - 1) / L);
  const int nss = T > 1 ? (int)((T - 1 + L - 1) / L) : 0;      // spans of the T-1 smoothing steps
  const size_t SS = (size_t)S * S, SP = (size_t)S + 4, TS = (size_t)T * S;
  const size_t budget = budget_bytes(dev_sw.budget_mb[DevSwitches::FBS], FBS_BUDGET_BYTES);
  const size_t fixed = (5 * SS + 3 * (size_t)S + (size_t)T + ((size_t)ns + 3) * S * SP + 8) * sizeof(double);
  const size_t per_draw = (2 * TS + 2 * (size_t)T + 2 * (size_t)ns * S) * sizeof(double);
  const BatchPlan bp = batch_plan((size_t)n_draws, budget, fixed, per_draw);
  if (!bp.ok) FAIL(NAGP_ENOMEM, "one draw takes %zu B of device memory (budget %zu B)", fixed + per_draw, budget);
  if (MS) {                                                     // S_y(y): the smoother itself, same launches and bits
    const int st0 = nagp_fastfb_run(S, A, AKHA, HA, K, G, y, T, MS, nullptr, device);
    if (st0 != NAGP_OK) return st0;
  }
  if (!Ydraw && !Xdraw) return NAGP_OK;
  if (hipSetDevice(device) != hipSuccess) FAIL(NAGP_EHIP, "hipSetDevice(%d)", device);
  const FbsBlock o = fbs_block((size_t)S, (size_t)T, (size_t)ns, bp.nb);
  DevBlock blk;
  API_ALLOC(blk, device, o.total); double* const dev = blk.p;
  int st = NAGP_OK;
  API_HIP(nagp_fastfb_sample, hipMemcpy(dev + o.A, A, SS * 8, hipMemcpyHostToDevice));
  API_HIP(nagp_fastfb_sample, hipMemcpy(dev + o.B, AKHA, SS * 8, hipMemcpyHostToDevice));
  API_HIP(nagp_fastfb_sample, hipMemcpy(dev + o.G, G, SS * 8, hipMemcpyHostToDevice));
  API_HIP(nagp_fastfb_sample, hipMemcpy(dev + o.lq, Lq, SS * 8, hipMemcpyHostToDevice));
  API_HIP(nagp_fastfb_sample, hipMemcpy(dev + o.lp, Lp, SS * 8, hipMemcpyHostToDevice));
  API_HIP(nagp_fastfb_sample, hipMemcpy(dev + o.k, K, (size_t)S * 8, hipMemcpyHostToDevice));
  API_HIP(nagp_fastfb_sample, hipMemcpy(dev + o.h, H, (size_t)S * 8, hipMemcpyHostToDevice));
  API_HIP(nagp_fastfb_sample, hipMemcpy(dev + o.ha, HA, (size_t)S * 8, hipMemcpyHostToDevice));
  API_HIP(nagp_fastfb_sample, hipMemcpy(dev + o.y, y, (size_t)T * 8, hipMemcpyHostToDevice));
  if (ns > 1) {                                                 // the span matrices that do not depend on y: A^L, G^L, G^(last span)
    std::vector<double> ph(3 * S * SP);
    fbs_matrix_power(A, S, L, ph.data());
    fbs_matrix_power(G, S, L, ph.data() + S * SP);
    fbs_matrix_power(G, S, (T - 1) - (int64_t)(nss - 1) * L, ph.data() + 2 * S * SP);
    API_HIP(nagp_fastfb_sample, hipMemcpy(dev + o.pha, ph.data(), ph.size() * 8, hipMemcpyHostToDevice));
  }
  const int NT = std::max(64, roundup64(S));
  if (st == NAGP_OK) st = set_lds(fbs_prior_kernel<false>, lds);
  if (st == NAGP_OK) st = set_lds(fbs_filter_kernel<false>, lds);
  if (st == NAGP_OK) st = set_lds(fbs_smoother_kernel<false>, lds);
  if (st == NAGP_OK && ns > 1) st = set_lds(fbs_prior_kernel<true>, lds);
  if (st == NAGP_OK && ns > 1) st = set_lds(fbs_filter_kernel<true>, lds);
  if (st == NAGP_OK && ns > 1) st = set_lds(fbs_smoother_kernel<true>, lds);
  if (st == NAGP_OK && ns > 1) st = set_lds(fastfb_compose_kernel<false>, lds_c);
  if (st == NAGP_OK && ns > 1) {                                // the filter's span matrices: a function of the NaN pattern of y alone
    FbPar cp{S, T, dev + o.A, dev + o.B, dev + o.ha, dev + o.k, dev + o.y, nullptr, nullptr, L, ns, dev + o.phf, nullptr, 0};
    hipLaunchKernelGGL(fastfb_compose_kernel<false>, dim3(ns), dim3(256), lds_c, 0, cp);
  }
  run_batches("nagp_fastfb_sample", st, n_draws, (int)bp.nb, nullptr, 0, nullptr, [](int, int) {},      // nothing to upload, nothing timed
    [&](int i0, int nbk, int) {
      FbsPar fq{};
      fq.S = S; fq.T = T; fq.L = L; fq.ns = ns; fq.draw0 = i0; fq.seed = seed; fq.sqrtR = std::sqrt(R);
      fq.A = dev + o.A; fq.Lp = dev + o.lp; fq.H = dev + o.h; fq.K = dev + o.k; fq.y = dev + o.y;
      fq.xs = dev + o.xs; fq.d = dev + o.d; fq.ms = dev + o.ms; fq.yd = dev + o.yd; fq.want_x = Xdraw ? 1 : 0;
      fq.c = dev + o.c; fq.starts = ns > 1 ? dev + o.st : nullptr; fq.mat_global = mat_global;
      // prior draw x*, d = y - y*
      fq.B = dev + o.lq; fq.Phi = dev + o.pha; fq.phi_stride = 0; fq.PhiLast = dev + o.pha;
      if (ns > 1) {
        hipLaunchKernelGGL(fbs_prior_kernel<true>, dim3(ns, nbk), dim3(NT), lds, 0, fq);
        hipLaunchKernelGGL(fbs_boundary_kernel<false>, dim3(nbk), dim3(256), 0, 0, fq);
      }
      hipLaunchKernelGGL(fbs_prior_kernel<false>, dim3(ns, nbk), dim3(NT), lds, 0, fq);
      // filter of d
      fq.B = dev + o.B; fq.Phi = dev + o.phf; fq.phi_stride = (size_t)S * SP; fq.PhiLast = dev + o.phf + (size_t)(ns - 1) * S * SP;
      if (ns > 1) {
        hipLaunchKernelGGL(fbs_filter_kernel<true>, dim3(ns, nbk), dim3(NT), lds, 0, fq);
        hipLaunchKernelGGL(fbs_boundary_kernel<false>, dim3(nbk), dim3(256), 0, 0, fq);
      }
      hipLaunchKernelGGL(fbs_filter_kernel<false>, dim3(ns, nbk), dim3(NT), lds, 0, fq);
      // step T-1, then the T-1 smoothing steps with + x* and the product with H in the replay
      if (Xdraw) hipLaunchKernelGGL(fbs_last_kernel<true>, dim3(nbk), dim3(256), 0, 0, fq);
      else hipLaunchKernelGGL(fbs_last_kernel<false>, dim3(nbk), dim3(256), 0, 0, fq);
      if (T > 1) {
        fq.B = dev + o.G; fq.ns = nss; fq.Phi = dev + o.phg; fq.phi_stride = 0; fq.PhiLast = dev + o.phl;
        if (ns > 1) {
          hipLaunchKernelGGL(fbs_smoother_kernel<true>, dim3(nss, nbk), dim3(NT), lds, 0, fq);
          hipLaunchKernelGGL(fbs_boundary_kernel<true>, dim3(nbk), dim3(256), 0, 0, fq);
        }
        hipLaunchKernelGGL(fbs_smoother_kernel<false>, dim3(nss, nbk), dim3(NT), lds, 0, fq);
      }
    }, [&](int i0, int nbk) {
      if (Ydraw) API_HIP(nagp_fastfb_sample, hipMemcpy(Ydraw + (size_t)i0 * T, dev + o.yd, (size_t)nbk * T * 8, hipMemcpyDeviceToHost));
      if (Xdraw) API_HIP(nagp_fastfb_sample, hipMemcpy(Xdraw + (size_t)i0 * TS, dev + o.xs, (size_t)nbk * TS * 8, hipMemcpyDeviceToHost));
    });
  return st;
}
