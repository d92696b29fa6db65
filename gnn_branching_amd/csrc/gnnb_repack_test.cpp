// CPU-only test shim for the device pack builder (built with g++ by tests/test_repack_cpu.py): the fold and emit functions of
// gnnb_pack.h that gnnb_k_repack.h runs one thread per element, run here as plain loops over the kernels' grids.
#include "gnnb_pack.h"

namespace {
// the whole pack block from a parameter blob, as k_repack_fold + k_repack_emit build it
std::vector<float> repack_block(const float* blob) {
  std::vector<float> scr(gnnb::RepackScr::FLOATS, 0.f);
  for (int j = 0; j < gnnb::kFoldJobs; ++j)
    for (int e = 0; e < gnnb::kFoldJobElems; ++e) gnnb::repack_fold_elem(blob, scr.data(), j, e);
  int nblocks = 0;
  const std::vector<gnnb::RepackSeg> segs = gnnb::repack_segments(&nblocks);
  std::vector<float> block(gnnb::pack_block_offset(gnnb::kPacks), 0.f);
  for (int b = 0; b < nblocks; ++b) {                 // the emit grid: workgroup b, thread t
    int lo = 0, hi = (int)segs.size() - 1;            // the last segment whose block0 <= b
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (segs[mid].block0 <= b) lo = mid; else hi = mid - 1;
    }
    for (int t = 0; t < gnnb::kRepackBlock; ++t) {
      const int e = (b - segs[lo].block0) * gnnb::kRepackBlock + t;
      if (e < segs[lo].threads) gnnb::repack_emit_elem(segs[lo], e, blob, scr.data(), block.data());
    }
  }
  return block;
}
}  // namespace

extern "C" {
// pack `which` (the order of gnnb_pt_pack) as the device builder builds it; returns its floats (copied when cap holds them), 0: bad `which`
size_t gnnb_pt_repack(const float* blob, int which, float* out, size_t cap) {
  if (which < 0 || which >= gnnb::kPacks) return 0;
  const size_t n = (size_t)gnnb::kPackFloats[which];
  if (out && cap >= n) {
    const std::vector<float> block = repack_block(blob);
    std::memcpy(out, block.data() + gnnb::pack_block_offset(which), n * sizeof(float));
  }
  return n;
}
// how many floats of pack `which` the segments write, and how many they write more than once: a cover of the pack has (n, 0)
void gnnb_pt_repack_cover(int which, size_t* written, size_t* twice) {
  const std::vector<gnnb::RepackSeg> segs = gnnb::repack_segments(nullptr);
  const size_t lo = gnnb::pack_block_offset(which), n = (size_t)gnnb::kPackFloats[which];
  std::vector<int> cnt(n, 0);
  for (const gnnb::RepackSeg& s : segs)
    for (int q = 0; q < gnnb::repack_seg_floats(s); ++q)
      if ((size_t)s.dst + q >= lo && (size_t)s.dst + q < lo + n) ++cnt[(size_t)s.dst + q - lo];
  *written = 0; *twice = 0;
  for (int c : cnt) { *written += c > 0; *twice += c > 1; }
}
}
