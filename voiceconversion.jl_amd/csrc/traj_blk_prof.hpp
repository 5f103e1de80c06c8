// traj_blk_prof.hpp -- cycle counters per phase of the probe build (make EXTRA=-DTRAJ_BLK_PROF): one array per file that
// includes this (traj_solve.hip, traj_gv.hip), printed by that file's *_prof_dump from traj_check_status.
#pragma once
#ifdef TRAJ_BLK_PROF
static __device__ long long blk_prof[32];   // cycles of workgroup 0 per phase
#define BLK_PROF_T0() long long pt_ = (long long)__builtin_readcyclecounter()
#define BLK_PROF(k)                                                     \
  do {                                                                  \
    const long long n_ = (long long)__builtin_readcyclecounter();       \
    if (blockIdx.x == 0 && threadIdx.x == 0) blk_prof[k] += n_ - pt_;   \
    pt_ = n_;                                                           \
  } while (0)
// time since the last BLK_PROF mark, seen by thread `thr` (does not move the mark)
#define BLK_PROF_AT(k, thr)                                                                                         \
  do {                                                                                                              \
    if (blockIdx.x == 0 && threadIdx.x == (thr)) blk_prof[k] += (long long)__builtin_readcyclecounter() - pt_;      \
  } while (0)
static inline void blk_prof_fetch(long long (&h)[32], hipStream_t st) {   // host: this file's counters, then zeroed
  const long long z[32] = {0};
  (void)hipStreamSynchronize(st);
  (void)hipMemcpyFromSymbol(h, HIP_SYMBOL(blk_prof), sizeof(h));
  (void)hipMemcpyToSymbol(HIP_SYMBOL(blk_prof), z, sizeof(z));
}
#else
#define BLK_PROF_T0()
#define BLK_PROF(k)
#define BLK_PROF_AT(k, thr)
#endif
