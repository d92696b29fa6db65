// gnnb_k_repack.h -- the scorer's operand packs built on the device from the trainer's parameter blob.
//
// Two launches on the caller's stream, no atomics, no workgroup waits on another, nothing allocated:
//   k_repack_fold : grid (ceil(kFoldJobElems / 256), kFoldJobs), one thread per folded entry -- repack_fold_elem of gnnb_pack.h: a
//                   64-term (128 for WAS) fp64 fma chain, k ascending, rounded to fp32 where build_packs rounds.  Latency-bound:
//                   238 workgroups of 256 threads, every entry's chain independent of every other's.
//   k_repack_emit : one thread per destination float, or per 16-byte group of bf16 pieces, of the 14 packs -- repack_emit_elem over
//                   the segment table of repack_segments (uploaded once per trainer); a workgroup lies inside ONE segment and
//                   finds it by a search that is uniform over the workgroup.
// The arithmetic and the layout are the shared functions of gnnb_pack.h, which tests/test_repack_cpu.py runs on the CPU against
// build_packs; tests/test_gpu_repack.py compares what these kernels write with that CPU run bit for bit.
#pragma once
#include "gnnb_pack.h"

namespace gnnb {

__global__ __launch_bounds__(kRepackBlock) void k_repack_fold(const float* __restrict__ blob, float* __restrict__ scr) {
  const int e = (int)(blockIdx.x * kRepackBlock + threadIdx.x);
  if (e < kFoldJobElems) repack_fold_elem(blob, scr, (int)blockIdx.y, e);
}

__global__ __launch_bounds__(kRepackBlock) void k_repack_emit(const RepackSeg* __restrict__ segs, int nseg, const float* __restrict__ blob,
                                                              const float* __restrict__ scr, float* __restrict__ block) {
  const int b = (int)blockIdx.x;
  int lo = 0, hi = nseg - 1;                  // the last segment whose block0 <= b
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (segs[mid].block0 <= b) lo = mid; else hi = mid - 1;
  }
  const RepackSeg s = segs[lo];
  const int t = (b - s.block0) * kRepackBlock + (int)threadIdx.x;
  if (t < s.threads) repack_emit_elem(s, t, blob, scr, block);
}

}  // namespace gnnb
