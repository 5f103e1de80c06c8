// dtw_internal.hpp -- what the DTW translation units share on the host: the per-thread scratch with its staging ring, the
// LDS budget, the padded row lengths and the functions that cross files (dtw.hip: entries, dispatcher, pad kernel;
// dtw_fused.hip: the fused path; dtw_twokernel.hip: observation + recurrence kernels and the generic kernel).
#pragma once
#include <algorithm>

#include "vcmi_common.hpp"
#include "dtw_plan.hpp"

namespace vcmi {

static const size_t kLdsLimit = 160 * 1024 - 256;   // dynamic LDS budget; leaves room for the kernels' static __shared__

static inline int dtw_dmax(int D) {
  return D <= 8 ? 8 : D <= 16 ? 16 : D <= 24 ? 24 : D <= 32 ? 32 : D <= 40 ? 40 : D <= 48 ? 48 : D <= 64 ? 64 : 96;
}

// per-thread scratch shared by the DTW entry points
struct DtwScratch {
  DevBuf<unsigned char> codes, longscr;      // longscr: cost columns / path / lists of the generic kernel beyond the LDS lengths
  DevBuf<DtwPair> dpairs;
  DevBuf<double> feats, cost, newtgt, obs, spad;
  DevBuf<int64_t> paths, bp;
  // Stream ordering of the shared workspaces (descriptors, observation costs, step codes): a call on ANY stream first
  // waits for the previous call's last kernel (`last_use`), and the descriptors travel to the device by an asynchronous
  // copy on the caller's stream from a small ring of pinned slots (a slot is reused only after its copy completed).
  // The ring is DEEP on purpose: a caller that issues calls back to back blocks in stage() once every slot is in flight, and
  // a blocked host thread wakes up late when the machine is busy (measured on a box with load average 30: 3-4.5 ms per
  // call instead of the GPU's 1.6 ms with 6 slots = two calls in flight) -- with 24 slots the GPU has many calls queued
  // and a late wake-up costs nothing.  (256 KB of pinned memory per slot at the benchmark batch.)
  static constexpr int kSlots = 24;
  hipEvent_t last_use = nullptr, slot_done[kSlots] = {};
  unsigned char *slot[kSlots] = {};
  size_t slot_cap[kSlots] = {};
  int next_slot = 0, device = -1;
  // fused path: strip descriptors, packed step codes, strip boundaries, last cost columns, strip-completion flags
  DevBuf<unsigned char> ddesc;   // fused path: pair, strip and job descriptors of the call (one upload)
  DevBuf<uint32_t> fcodes;
  DevBuf<double> bnd, clast;
  DevBuf<int32_t> path32;        // fused path: 0-based paths (dtw_fused_backward_kernel -> dtw_fused_align_kernel)
  DevBuf<int> flags;
  int epoch = 0;
  int init() {
    int dev = 0;
    VCMI_HIP(hipGetDevice(&dev));
    if (last_use && dev == device) return VCMI_OK;
    release_sync();
    VCMI_HIP(hipEventCreateWithFlags(&last_use, hipEventDisableTiming));
    for (auto &e : slot_done) VCMI_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    device = dev;
    return VCMI_OK;
  }
  // pinned copy of `n` descriptors, valid until the returned slot's event (recorded by the caller) completes
  template <typename Desc>
  int stage(const Desc *src, size_t n, Desc **out, hipEvent_t *ev) {
    unsigned char *raw = nullptr;
    VCMI_TRY(stage_raw(n * sizeof(Desc), &raw, ev));
    memcpy(raw, src, n * sizeof(Desc));
    *out = reinterpret_cast<Desc *>(raw);
    return VCMI_OK;
  }
  // `bytes` of the next pinned slot (to be filled by the caller), valid until the slot's event -- recorded by the caller
  // after the copy it issues -- completes
  int stage_raw(size_t bytes, unsigned char **out, hipEvent_t *ev) {
    const int s = next_slot;
    next_slot = (next_slot + 1) % kSlots;
    VCMI_HIP(hipEventSynchronize(slot_done[s]));
    if (bytes > slot_cap[s]) {
      if (slot[s]) (void)hipHostFree(slot[s]);
      slot[s] = nullptr;
      slot_cap[s] = 0;
      const size_t cap = std::max<size_t>(bytes, (size_t)128 << 10);
      VCMI_HIP(hipHostMalloc(reinterpret_cast<void **>(&slot[s]), cap, hipHostMallocDefault));
      slot_cap[s] = cap;
    }
    *out = slot[s];
    *ev = slot_done[s];
    return VCMI_OK;
  }
  // asynchronous upload of descriptors on `st` through a pinned slot
  template <typename Desc>
  int upload(Desc *dst, const Desc *src, size_t n, hipStream_t st) {
    Desc *pinned = nullptr;
    hipEvent_t copied = nullptr;
    VCMI_TRY(stage(src, n, &pinned, &copied));
    VCMI_HIP(hipMemcpyAsync(dst, pinned, sizeof(Desc) * n, hipMemcpyHostToDevice, st));
    VCMI_HIP(hipEventRecord(copied, st));
    return VCMI_OK;
  }
  void release_sync() {
    if (last_use) (void)hipEventDestroy(last_use);
    last_use = nullptr;
    for (int i = 0; i < kSlots; ++i) {
      if (slot_done[i]) (void)hipEventDestroy(slot_done[i]);
      if (slot[i]) (void)hipHostFree(slot[i]);
      slot_done[i] = nullptr;
      slot[i] = nullptr;
      slot_cap[i] = 0;
    }
  }
  ~DtwScratch() { release_sync(); }
};

// dtw.hip: dtw_pad_kernel on `st` (no error check of its own: the caller's next hipGetLastError covers it), for both paths
void dtw_launch_pad(const double *feats, const DtwPair *dpairs, int n, int D, int dmax, double *spad, hipStream_t st);

// dtw_fused.hip: the fused path takes fstep = 0, bstep in {1, 2}, D <= kFusedMaxD, path-only calls whose LDS arrays fit
static constexpr int kFusedMaxD = 48;
bool dtw_fused_fits(int Smax, int Tmax);
int dtw_run_fused(const double *feats, std::vector<DtwPair> &pairs, int D, int bstep, DtwScratch &sc, hipStream_t st, int Smax,
                  int Tmax);

// dtw_twokernel.hip: every other call (validated by dtw_run, Tmax > 0)
int dtw_run_twokernel(const double *feats, std::vector<DtwPair> &pairs, int D, int fstep, int bstep, DtwScratch &sc,
                      hipStream_t st, int Smax, int Tmax);

}  // namespace vcmi
