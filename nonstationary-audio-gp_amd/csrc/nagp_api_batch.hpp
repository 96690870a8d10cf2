// nagp_api_batch.hpp -- part of the ONE translation unit nagp_api.hip: what the per-call entry points share around their kernels
// ("Batched entry points") -- the error macro, the owner of "device block + events", the device-batch loop, the timings export.
#include "nagp_api_layout.hpp"

// device calls of the per-call entry points: the first failure is kept (st, the text names the entry point) and the thread's last HIP
// error is cleared; the calls after it are skipped
#define API_HIP_S(fn_text, x) do { if (st == NAGP_OK) { hipError_t _e = (x); if (_e != hipSuccess) { g_last_error = std::string(fn_text) + ": " #x " -> " + hipGetErrorString(_e); (void)hipGetLastError(); st = NAGP_EHIP; } } } while (0)
#define API_HIP(fn, x) API_HIP_S(#fn, x)

// one device block of doubles and up to four events, released on the device they were made on
struct DevBlock {
  int device = 0; double* p = nullptr; hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
  DevBlock() = default; DevBlock(const DevBlock&) = delete; DevBlock& operator=(const DevBlock&) = delete;
  hipError_t alloc(int dev, size_t n_doubles) {
    device = dev; const hipError_t e = hipMalloc(&p, n_doubles * sizeof(double));
    if (e != hipSuccess) { p = nullptr; (void)hipGetLastError(); }
    return e;
  }
  hipError_t events(int n) { hipError_t e = hipSuccess; for (int i = 0; i < n && e == hipSuccess; ++i) e = hipEventCreate(&ev[i]); return e; }
  ~DevBlock() {
    if (!p && !ev[0]) return;
    (void)hipSetDevice(device);
    for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
    if (p) (void)hipFree(p);
  }
};
#define API_ALLOC(blk, dev, n_doubles) do { if ((blk).alloc(dev, n_doubles) != hipSuccess) FAIL(NAGP_ENOMEM, "hipMalloc(%zu)", (size_t)(n_doubles) * sizeof(double)); } while (0)

// The device-batch loop: items [i0, i0 + nbk) of n at a time, nb at the most.  Per batch: upload(i0, nbk); launch(i0, nbk, s) for every timed segment s,
// ev[s] recorded before it and ev[s + 1] after it (n_ev = 0: one untimed segment); hipGetLastError; hipDeviceSynchronize; the segments' elapsed times
// added to ms[s]; download(i0, nbk).  The callbacks record their own failures in st (API_HIP); the loop stops at the first one.
template <class Upload, class Launch, class Download>
static void run_batches(const char* fn, int& st, int n, int nb, hipEvent_t* ev, int n_ev, double* ms, Upload upload, Launch launch, Download download) {
  const int n_seg = std::max(1, n_ev - 1);
  for (int i0 = 0; i0 < n && st == NAGP_OK; i0 += nb) {
    const int nbk = std::min(nb, n - i0);
    upload(i0, nbk);
    if (st == NAGP_OK) {
      for (int s = 0; s < n_seg; ++s) {
        if (n_ev) (void)hipEventRecord(ev[s], 0);
        launch(i0, nbk, s);
      }
      if (n_ev) (void)hipEventRecord(ev[n_seg], 0);
    }
    API_HIP_S(fn, hipGetLastError());
    API_HIP_S(fn, hipDeviceSynchronize());
    for (int s = 0; s + 1 < n_ev && st == NAGP_OK; ++s) { float t = 0.f; if (hipEventElapsedTime(&t, ev[s], ev[s + 1]) == hipSuccess) ms[s] += t; }
    download(i0, nbk);
  }
}

// behind every nagp_*_timings: the device time of the last call on this thread
static int timings_out(double* ms, const double* src, int n) {
  if (!ms) FAIL(NAGP_EINVAL, "null argument");
  for (int i = 0; i < n; ++i) ms[i] = src[i];
  return NAGP_OK;
}
