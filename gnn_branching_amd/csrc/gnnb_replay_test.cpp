// CPU-only test shim for the replay buffer's sampler (built with g++ by tests/test_replay_cpu.py): the key functions of gnnb_k_replay.h,
// which k_replay_sample runs one thread per slot, run here as plain loops, and the rule of gnnb_replay_sample stated with a sort.
#include <algorithm>
#include <cstdint>
#include <utility>
#include <vector>

#define __host__
#define __device__
#define __forceinline__ inline
#include "gnnb_k_starts.h"
#include "gnnb_k_replay.h"

extern "C" {
// key_j of the slots j = 0..filled - 1 of draw `draw` under `seed`
void gnnb_rt_keys(int filled, uint64_t seed, uint64_t draw, uint64_t* out) {
  const unsigned long long base = rp_base(seed, draw);
  for (int j = 0; j < filled; ++j) out[j] = rp_key(base, (unsigned long long)j);
}
// idx[0..n): the min(n, filled) slots with the smallest (key_j, j) in ascending order of (key_j, j), -1 beyond
void gnnb_rt_sample(int filled, int n, uint64_t seed, uint64_t draw, int32_t* idx) {
  const unsigned long long base = rp_base(seed, draw);
  std::vector<std::pair<unsigned long long, int>> k(filled > 0 ? filled : 0);
  for (int j = 0; j < filled; ++j) k[j] = {rp_key(base, (unsigned long long)j), j};
  const int m = n < filled ? n : (filled > 0 ? filled : 0);
  std::partial_sort(k.begin(), k.begin() + m, k.end());
  for (int q = 0; q < n; ++q) idx[q] = q < m ? k[q].second : -1;
}
int gnnb_rt_max_sample(void) { return RP_MAX_SAMPLE; }
int gnnb_rt_max_capacity(void) { return RP_MAX_CAPACITY; }
}
