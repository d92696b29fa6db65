// gnnb_k_replay.h -- a device-resident replay buffer of strong-branching tables: the piece in front of
// gnnb_imitation_step_rows (fill a ring of C batch rows with the useful rows of a round) and the piece around it (draw a minibatch of
// distinct slots that a seed reproduces).  The step itself is the existing one: the buffer IS a gnnb_batch of C rows, a minibatch a row list.
//
//   * k_replay_rank    ONE workgroup: classify the n listed rows of the source table (a wave per row), an exclusive prefix over the n
//                      flags, a ring slot per stored row (-1: not stored) and the buffer's new state word.
//   * k_replay_store   the copy: row rows[i] of every tensor the step reads goes to row slot[i] of the buffer's, a row spread over the
//                      TG_SPLIT workgroups of blockIdx.y as k_trows_gather spreads it, 16-byte copies where width and alignment allow.
//   * k_replay_sample  ONE workgroup: the n slots of [0, filled) with the smallest keys, in ascending key order.
//
// The rule of a row (k_replay_rank) is k_tloss_table's own refusal raised at the door, so that the buffer never holds a row that fails
// every time it is drawn: STORED iff its table row has at least two candidates (entries that are not NaN), every candidate is finite and
// every candidate's mask entry is not 0.  0 or 1 candidates: skipped silently (the step would get no gradient from it).  A candidate at a
// decided node or with tau = +-inf, or a rows entry outside [0, K): skipped, and bit 3 (value 8) of *status.
//
// No atomics, no workgroup waits on another; every count is per-thread partials in a fixed order plus a fixed tree.
// (Behind gnnb_k_starts.h: the keys are its ns_mix and NS_GOLDEN.  The key functions compile on the host as well:
// csrc/gnnb_replay_test.cpp includes this file with a plain C++ compiler, which sees nothing below the kernels' guard.)

#define RP_THREADS 256
#define RP_MAX_SAMPLE 256       // n of a draw: 1..RP_MAX_SAMPLE
#define RP_MAX_CAPACITY 65536   // C: 1..RP_MAX_CAPACITY
// the state word of a buffer, int32[4]
#define RP_HEAD 0
#define RP_FILLED 1
#define RP_STORED 2
#define RP_SKIPPED 3

// ---- the sampler's keys: a pure function of (seed, draw, j) ----
// base = ns_mix(seed ^ ns_mix(draw + 1)); key_j = ns_mix(base + NS_GOLDEN (j + 1)).  ns_mix is a bijection of the 64-bit words and
// NS_GOLDEN is odd, so the keys of distinct j are distinct: the order (key_j, j) never needs its second component.
__host__ __device__ __forceinline__ unsigned long long rp_base(unsigned long long seed, unsigned long long draw) {
  return ns_mix(seed ^ ns_mix(draw + 1ull));
}
__host__ __device__ __forceinline__ unsigned long long rp_key(unsigned long long base, unsigned long long j) {
  return ns_mix(base + NS_GOLDEN * (j + 1ull));
}

#ifdef __HIPCC__

typedef float rp_f4 __attribute__((ext_vector_type(4)));

// ---- k_replay_rank ----
struct ReplayRank {
  const double* table; const float* mask;       // the SOURCE batch's (K, R) table and mask
  const int* rows; int n, K, R, C;
  int* slot;                                    // (n): the ring slot of listed row i, -1: not stored
  int* state; int* status;                      // int32[4]; int32[1] or null
};

__global__ __launch_bounds__(RP_THREADS) void k_replay_rank(ReplayRank a) {
  __shared__ int part[RP_THREADS];
  __shared__ int s_bad[RP_THREADS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = a.n, R = a.R;
  const int head = a.state[RP_HEAD], filled = a.state[RP_FILLED];      // (read by everybody before thread 0 writes the new word)
  // 1. classify: wave w takes the rows w, w + 4, ...; a row's entries in lane-strided order, the counts added over the lanes
  int any_bad = 0;
  for (int i = wave; i < n; i += RP_THREADS / 64) {
    const int r = a.rows[i];
    int cnt = 0, bad = 0;
    if (r < 0 || r >= a.K) {
      bad = 1;
    } else {
      const double* tau = a.table + (long)r * R;
      const float* mk = a.mask + (long)r * R;
      for (int j = lane; j < R; j += 64) {
        const double v = tau[j];
        if (v != v) continue;
        ++cnt;
        if (mk[j] == 0.0f || v - v != 0.0) bad = 1;
      }
    }
    for (int o = 32; o; o >>= 1) { cnt += __shfl_xor(cnt, o, 64); bad |= __shfl_xor(bad, o, 64); }
    if (lane == 0) a.slot[i] = (!bad && cnt >= 2) ? 1 : 0;
    any_bad |= bad;
  }
  s_bad[tid] = any_bad;
  __threadfence_block();
  __syncthreads();
  // 2. the exclusive prefix of the flags: thread t owns the listed rows [t per, (t + 1) per), its count, then a scan over the threads
  const int per = (n + RP_THREADS - 1) / RP_THREADS;
  const int i0 = min(tid * per, n), i1 = min(i0 + per, n);
  int mine = 0;
  for (int i = i0; i < i1; ++i) mine += a.slot[i];
  part[tid] = mine;
  __syncthreads();
  for (int o = 1; o < RP_THREADS; o <<= 1) {     // (Hillis-Steele: an inclusive scan in 8 fixed steps)
    const int v = tid >= o ? part[tid - o] : 0, vb = tid >= o ? s_bad[tid - o] : 0;
    __syncthreads();
    part[tid] += v;
    s_bad[tid] |= vb;
    __syncthreads();
  }
  const int stored = part[RP_THREADS - 1];
  int before = part[tid] - mine;
  for (int i = i0; i < i1; ++i) {
    const int f = a.slot[i];
    a.slot[i] = f ? (head + before) % a.C : -1;
    before += f;
  }
  if (tid == 0) {
    const int nf = filled + stored;
    a.state[RP_HEAD] = (head + stored) % a.C;
    a.state[RP_FILLED] = nf < a.C ? nf : a.C;
    a.state[RP_STORED] = stored;
    a.state[RP_SKIPPED] = n - stored;
    if (s_bad[RP_THREADS - 1] && a.status) *a.status = *a.status | 8;
  }
}

// ---- k_replay_store ----
// t: the tensors the step reads and the table (a fp64 row is 2 R floats), source and buffer side; blockIdx.x = listed row.
struct ReplayStore { gnnb_train::TGatherT t[TG_MAXT]; int nt; const int* rows; const int* slot; };
static_assert(sizeof(ReplayStore) <= 4096, "kernel arguments: 4 KiB");
__global__ __launch_bounds__(TG_THREADS) void k_replay_store(ReplayStore a) {
  const int i = blockIdx.x, t0 = blockIdx.y * TG_THREADS + threadIdx.x, dt = TG_SPLIT * TG_THREADS;
  const int to = a.slot[i];
  if (to < 0) return;                            // (not stored: rows[i] may name no row at all)
  const int r = a.rows[i];
  for (int q = 0; q < a.nt; ++q) {
    const gnnb_train::TGatherT& t = a.t[q];
    const float* s = t.src + (long)r * t.w;
    float* d = t.dst + (long)to * t.w;
    if ((t.w & 3) == 0 && (((unsigned long long)s | (unsigned long long)d) & 15ull) == 0) {
      const rp_f4* s4 = reinterpret_cast<const rp_f4*>(s);
      rp_f4* d4 = reinterpret_cast<rp_f4*>(d);
      for (int j = t0; j < (t.w >> 2); j += dt) d4[j] = s4[j];
    } else {
      for (int j = t0; j < t.w; j += dt) d[j] = s[j];
    }
  }
}

// ---- k_replay_sample ----
// m = min(n, filled) slots.  The keys are distinct, so the m-th smallest key T is the least 64-bit word with count(key_j <= T) >= m:
// a bisection over the word (at most 64 counts; thread t counts j = t, t + 256, ... and a fixed tree adds the 256 counts), skipped when
// m = filled.  Then the m selected (key, j) are listed in LDS behind an exclusive scan of the threads' counts and ranked by key (each
// of the first m threads counts the selected keys below its own): idx[rank] = j.  idx[m..n) = -1.
struct ReplaySample { const int* state; int C, n; unsigned long long seed, draw; int* idx; };

__global__ __launch_bounds__(RP_THREADS) void k_replay_sample(ReplaySample a) {
  __shared__ int part[RP_THREADS];
  __shared__ unsigned long long s_key[RP_MAX_SAMPLE];
  __shared__ int s_j[RP_MAX_SAMPLE];
  const int tid = threadIdx.x, n = a.n;
  int filled = a.state[RP_FILLED];
  filled = filled < 0 ? 0 : (filled > a.C ? a.C : filled);
  const int m = n < filled ? n : filled;
  for (int q = m + tid; q < n; q += RP_THREADS) a.idx[q] = -1;
  if (m == 0) return;
  const unsigned long long base = rp_base(a.seed, a.draw);
  unsigned long long lo = 0ull, hi = ~0ull;      // count(<= hi) >= m always holds
  if (m < filled) {
    while (lo < hi) {                             // (uniform: every thread reads the same total)
      const unsigned long long mid = lo + ((hi - lo) >> 1);
      int c = 0;
      for (int j = tid; j < filled; j += RP_THREADS) c += rp_key(base, (unsigned long long)j) <= mid ? 1 : 0;
      part[tid] = c;
      __syncthreads();
      for (int o = RP_THREADS / 2; o; o >>= 1) {
        if (tid < o) part[tid] += part[tid + o];
        __syncthreads();
      }
      const int total = part[0];
      __syncthreads();                            // everybody holds the total before part is reused
      if (total >= m) hi = mid; else lo = mid + 1ull;
    }
  }
  const unsigned long long T = hi;
  int c = 0;
  for (int j = tid; j < filled; j += RP_THREADS) c += rp_key(base, (unsigned long long)j) <= T ? 1 : 0;
  part[tid] = c;
  __syncthreads();
  for (int o = 1; o < RP_THREADS; o <<= 1) {      // inclusive scan of the threads' counts
    const int v = tid >= o ? part[tid - o] : 0;
    __syncthreads();
    part[tid] += v;
    __syncthreads();
  }
  int at = part[tid] - c;                         // (part[255] == m: the keys are distinct)
  for (int j = tid; j < filled; j += RP_THREADS) {
    const unsigned long long k = rp_key(base, (unsigned long long)j);
    if (k <= T && at < RP_MAX_SAMPLE) { s_key[at] = k; s_j[at] = j; ++at; }
  }
  __syncthreads();
  for (int q = tid; q < m; q += RP_THREADS) {
    const unsigned long long k = s_key[q];
    int rank = 0;
    for (int p = 0; p < m; ++p) rank += s_key[p] < k ? 1 : 0;
    a.idx[rank] = s_j[q];
  }
}

#endif  // __HIPCC__
