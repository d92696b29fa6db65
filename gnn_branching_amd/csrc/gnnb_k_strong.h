// gnnb_k_strong.h -- strong branching in the device frontier: gnnb_strong_list, gnnb_strong_pick.  For every
// parent row of a round the candidate splits are listed densely, their 2n children bounded by the existing batch kernels
// (gnnb_frontier_expand, gnnb_kw_bounds, gnnb_dual_ascent, in chunks), and the split whose two children improve the parent's bound most
// is the row's decision.
//
//   * k_strong_count    one workgroup per row: the number of undecided nodes (scorer_mask != 0) and, with top_m = M > 0 and more than M
//                       of them, the CUT of the total order (score descending, flat index ascending): the order-preserving integer key
//                       T of the M-th score, found by bisection over the key's 32 bits (32 counts over the row), and the number of nodes
//                       with key == T that still fit, which are the first in index order.  Scores are compared as VALUES: -0.0 is
//                       keyed as +0.0; +-inf are ordinary keys.  A NaN at an undecided node empties the row (top_m > 0 only; no score
//                       is read with top_m = 0), a NaN at a decided node is never looked at.
//   * k_strong_compact  one workgroup per row: the exclusive prefix of the rows' counts in row order (every workgroup sums the counts
//                       before its own: whole numbers, no workgroup waits on another), then the row's candidates in ascending flat index
//                       by a block scan over tiles of FR_THREADS nodes: cand_row, cand_slot, cand_dec = [layer, idx].
//   * k_strong_pick     one workgroup per row: imp of each of the row's candidates from its two child rows (fr_improvement, fr_child_lb:
//                       the operation order of the fall-back), the arg-max on (value descending, list position ascending) by per-thread
//                       partials in position order and a fixed tree, NaN below every number; optionally the (K, R) table.
//
//   * k_strong_rows_jobs  many jobs in one pool (gnnb_strong_rows_jobs): the boxes and property rows of a chunk's
//                       candidate child rows 2q, 2q + 1 from the per-segment tables, by the segment cand_slot[q] / seg_cap of the
//                       candidate's slot.  Grid (2c, FR_SPLIT); the copy is fr_seg_row, k_frontier_rows_sel's, and the kernel launches
//                       under that kernel's profile class (PC_FR_ROWS_SEL): it has none of its own.  A slot < 0 or of a segment
//                       >= segments leaves its two rows unwritten and reads no table.
//
//   * k_strong_union_count / k_strong_union_compact  the union of two shortlists (gnnb_strong_list_union): behind
//                       one k_strong_count per array, the walk that takes a node if either array's cut takes it -- the row's total, then
//                       k_strong_compact's prefix and the entries with their source.  They launch under k_strong_count's and
//                       k_strong_compact's profile classes.
//
// No atomics, no workgroup waits on another; nothing depends on K or on a row's place.

enum { SC_MODE, SC_COUNT_, SC_KEY, SC_TIES, SC_FIELDS };     // workspace of gnnb_strong_list: (K, SC_FIELDS) int32
enum { SM_NONE, SM_ALL, SM_CUT };                            // SC_MODE: no candidate; every undecided node; the cut (SC_KEY, SC_TIES)

struct StrongListArgs {
  FrShape s; FrPool p;
  const int32_t* slots; int K;
  const float* amb; const float* scores;                // (K, R); scores: null with top_m = 0
  int top_m;
  int32_t* cand0; int32_t* cand_row; int32_t* cand_slot; int32_t* cand_dec;
  int32_t* rows;                                        // workspace (K, SC_FIELDS)
};

struct StrongPickArgs {
  FrShape s; FrPool p;
  const int32_t* slots; int K;
  const int32_t* cand0; const int32_t* cand_dec;
  const int32_t* live; const int32_t* infeasible; const double* bound;          // (2n), list order
  int32_t* decisions; double* best; double* imp; double* table;
};
struct StrongRowsArgs {
  const int32_t* cand_slot; int c, S, seg_cap;          // (c) slots of the chunk's candidates; the pool's segments
  FrSegRows r;
};
static_assert(sizeof(StrongListArgs) <= 4096 && sizeof(StrongPickArgs) <= 4096 && sizeof(StrongRowsArgs) <= 4096, "kernel arguments: 4 KiB");

// The order-preserving key of a score: a > b as floats <=> key(a) > key(b) as unsigned, with -0.0 keyed as +0.0.  (Not for NaN.)
__device__ __forceinline__ unsigned st_key(float v) {
  unsigned u = __float_as_uint(v);
  if (v == 0.0f) u = 0u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// the sum of one whole number per thread over the workgroup, on every thread
__device__ __forceinline__ int st_block_sum(int* red, int v, int tid) {
  __syncthreads();
  red[tid] = v;
  __syncthreads();
  for (int s = FR_THREADS / 2; s > 0; s >>= 1) {
    if (tid < s) red[tid] += red[tid + s];
    __syncthreads();
  }
  const int out = red[0];
  __syncthreads();
  return out;
}

__global__ __launch_bounds__(FR_THREADS) void k_strong_count(StrongListArgs a) {
  __shared__ int red[FR_THREADS];
  const int i = blockIdx.x, tid = threadIdx.x, R = a.s.R, M = a.top_m;
  int32_t* out = a.rows + (long)i * SC_FIELDS;
  int mode = SM_NONE, count = 0;
  unsigned T = 0u;
  int ties = 0;
  if (fr_slot_ok(a.p, a.slots[i])) {                    // (uniform over the workgroup)
    const float* amb = a.amb + (long)i * R;
    const float* sc = M > 0 ? a.scores + (long)i * R : nullptr;
    int open = 0, nan = 0;
    for (int r = tid; r < R; r += FR_THREADS)
      if (amb[r] != 0.0f) {
        ++open;
        if (sc) { const float v = sc[r]; nan |= v != v; }
      }
    open = st_block_sum(red, open, tid);
    nan = st_block_sum(red, nan, tid);
    if (open > 0 && !nan) {
      if (M == 0 || open <= M) {
        mode = SM_ALL; count = open;
      } else {                                          // the largest T with at least M keys >= T: the key of the M-th score
        for (unsigned bit = 0x80000000u; bit; bit >>= 1) {
          const unsigned t = T | bit;
          int c = 0;
          for (int r = tid; r < R; r += FR_THREADS) c += amb[r] != 0.0f && st_key(sc[r]) >= t;
          if (st_block_sum(red, c, tid) >= M) T = t;
        }
        int above = 0;
        for (int r = tid; r < R; r += FR_THREADS) above += amb[r] != 0.0f && st_key(sc[r]) > T;
        above = st_block_sum(red, above, tid);
        mode = SM_CUT; count = M; ties = M - above;     // (1 <= ties: fewer than M keys lie above T)
      }
    }
  }
  if (tid == 0) { out[SC_MODE] = mode; out[SC_COUNT_] = count; out[SC_KEY] = (int32_t)T; out[SC_TIES] = ties; }
}

// the exclusive scan of one flag per thread over the workgroup and the flags' total (ballots per wave, then the waves in order)
__device__ __forceinline__ int st_block_scan(int* wsum, bool flag, int tid, int* total) {
  const int lane = tid & 63, wave = tid >> 6;
  const unsigned long long b = __ballot(flag);
  const int before = __popcll(b & ((1ull << lane) - 1ull));
  __syncthreads();
  if (lane == 0) wsum[wave] = __popcll(b);
  __syncthreads();
  int base = 0, all = 0;
  for (int w = 0; w < FR_THREADS / 64; ++w) {
    if (w < wave) base += wsum[w];
    all += wsum[w];
  }
  *total = all;
  return base + before;
}

__global__ __launch_bounds__(FR_THREADS) void k_strong_compact(StrongListArgs a) {
  __shared__ int red[FR_THREADS];
  __shared__ int wsum[FR_THREADS / 64];
  const int i = blockIdx.x, tid = threadIdx.x, R = a.s.R;
  int before = 0;
  for (int j = tid; j < i; j += FR_THREADS) before += a.rows[(long)j * SC_FIELDS + SC_COUNT_];
  const int q0 = st_block_sum(red, before, tid);
  const int32_t* row = a.rows + (long)i * SC_FIELDS;
  const int mode = row[SC_MODE], count = row[SC_COUNT_], ties = row[SC_TIES];
  const unsigned T = (unsigned)row[SC_KEY];
  if (tid == 0) {
    a.cand0[i] = q0;
    if (i == a.K - 1) a.cand0[a.K] = q0 + count;
  }
  if (mode == SM_NONE) return;                          // (uniform over the workgroup)
  const int slot = a.slots[i];
  const float* amb = a.amb + (long)i * R;
  const float* sc = mode == SM_CUT ? a.scores + (long)i * R : nullptr;
  int n_ties = 0, n_out = 0;                            // ties seen / candidates emitted in the tiles before this one
  for (int r0 = 0; r0 < R; r0 += FR_THREADS) {
    const int r = r0 + tid;
    const bool open = r < R && amb[r] != 0.0f;
    bool sel = open;
    if (mode == SM_CUT) {
      const unsigned key = open ? st_key(sc[r]) : 0u;
      const bool tie = open && key == T;
      int tile_ties;
      const int rank = n_ties + st_block_scan(wsum, tie, tid, &tile_ties);
      n_ties += tile_ties;
      sel = open && (key > T || (tie && rank < ties));
    }
    int tile_out;
    const int pos = n_out + st_block_scan(wsum, sel, tid, &tile_out);
    n_out += tile_out;
    if (sel && pos < count) {                           // (pos < count always holds: the bound of the lists' size, kept as a guard)
      int k = 1;
      while (k < a.s.L && r >= a.s.off[k + 1]) ++k;
      const long q = (long)q0 + pos;
      a.cand_row[q] = i;
      a.cand_slot[q] = slot;
      a.cand_dec[2 * q] = k - 1;
      a.cand_dec[2 * q + 1] = r - a.s.off[k];
    }
  }
}

// ---- the union of two shortlists (gnnb_strong_list_union; include/gnnb.h states the rule) ----
// k_strong_count runs once per array and leaves one (mode, count, key, ties) record per row and array; a row takes part when both records
// do (a bad slot, no undecided node, a NaN in either array: none).  The walk below goes over the row in tiles of FR_THREADS nodes with one
// running tie rank PER ARRAY, so "the first `ties` nodes with key == T in index order" holds for each array on its own; a node is taken if
// either array takes it.  k_strong_union_count keeps the walk's total per row (under k_strong_count's profile class), k_strong_union_compact
// walks again behind the prefix over those totals in row order and emits (under k_strong_compact's class).
struct StrongUnionArgs {
  FrShape s;
  const int32_t* slots; int K;
  const float* amb; const float* scores_a; const float* scores_b;        // (K, R)
  int32_t* cand0; int32_t* cand_row; int32_t* cand_slot; int32_t* cand_dec; int32_t* cand_src;
  const int32_t* rows_a; const int32_t* rows_b;         // workspace: (K, SC_FIELDS) each, k_strong_count's records
  int32_t* count;                                       // workspace: (K), the rows' union counts
};
static_assert(sizeof(StrongUnionArgs) <= 4096, "kernel arguments: 4 KiB");

struct StCut {                                          // one array's record of a row and its running tie rank
  int mode, ties, n_ties;
  unsigned T;
  const float* sc;
};

__device__ __forceinline__ StCut st_cut(const int32_t* rec, const float* sc) {
  return StCut{rec[SC_MODE], rec[SC_TIES], 0, (unsigned)rec[SC_KEY], sc};
}

// whether the array takes node r of the tile (every thread of the workgroup calls it: mode is uniform over the workgroup)
__device__ __forceinline__ bool st_takes(StCut& c, int* wsum, bool open, int r, int tid) {
  if (c.mode != SM_CUT) return open;                    // (SM_ALL: every undecided node)
  const unsigned key = open ? st_key(c.sc[r]) : 0u;
  const bool tie = open && key == c.T;
  int tile_ties;
  const int rank = c.n_ties + st_block_scan(wsum, tie, tid, &tile_ties);
  c.n_ties += tile_ties;
  return open && (key > c.T || (tie && rank < c.ties));
}

// The walk over row i: the number of nodes either array takes and, with EMIT, their entries from list position q0 on (at most `count`).
template <bool EMIT>
__device__ __forceinline__ int st_union_walk(const StrongUnionArgs& a, int i, int* wsum, int q0, int count) {
  const int tid = threadIdx.x, R = a.s.R;
  StCut ca = st_cut(a.rows_a + (long)i * SC_FIELDS, a.scores_a + (long)i * R), cb = st_cut(a.rows_b + (long)i * SC_FIELDS, a.scores_b + (long)i * R);
  if (ca.mode == SM_NONE || cb.mode == SM_NONE) return 0;      // (uniform over the workgroup)
  const int slot = a.slots[i];
  const float* amb = a.amb + (long)i * R;
  int n_out = 0;
  for (int r0 = 0; r0 < R; r0 += FR_THREADS) {
    const int r = r0 + tid;
    const bool open = r < R && amb[r] != 0.0f;
    const bool in_a = st_takes(ca, wsum, open, r, tid), in_b = st_takes(cb, wsum, open, r, tid);
    const bool sel = in_a || in_b;
    int tile_out;
    const int pos = n_out + st_block_scan(wsum, sel, tid, &tile_out);
    n_out += tile_out;
    if (EMIT && sel && pos < count) {                   // (pos < count always holds: the bound of the lists' size, kept as a guard)
      int k = 1;
      while (k < a.s.L && r >= a.s.off[k + 1]) ++k;
      const long q = (long)q0 + pos;
      a.cand_row[q] = i;
      a.cand_slot[q] = slot;
      a.cand_dec[2 * q] = k - 1;
      a.cand_dec[2 * q + 1] = r - a.s.off[k];
      a.cand_src[q] = (in_a ? 1 : 0) | (in_b ? 2 : 0);
    }
  }
  return n_out;
}

__global__ __launch_bounds__(FR_THREADS) void k_strong_union_count(StrongUnionArgs a) {
  __shared__ int wsum[FR_THREADS / 64];
  const int i = blockIdx.x;
  const int n = st_union_walk<false>(a, i, wsum, 0, 0);
  if (threadIdx.x == 0) a.count[i] = n;
}

__global__ __launch_bounds__(FR_THREADS) void k_strong_union_compact(StrongUnionArgs a) {
  __shared__ int red[FR_THREADS];
  __shared__ int wsum[FR_THREADS / 64];
  const int i = blockIdx.x, tid = threadIdx.x;
  int before = 0;
  for (int j = tid; j < i; j += FR_THREADS) before += a.count[j];
  const int q0 = st_block_sum(red, before, tid), count = a.count[i];
  if (tid == 0) {
    a.cand0[i] = q0;
    if (i == a.K - 1) a.cand0[a.K] = q0 + count;
  }
  st_union_walk<true>(a, i, wsum, q0, count);
}

__global__ __launch_bounds__(FR_THREADS) void k_strong_pick(StrongPickArgs a) {
  __shared__ double sv[FR_THREADS];
  __shared__ int sq[FR_THREADS];
  const int i = blockIdx.x, tid = threadIdx.x, R = a.s.R;
  const double nan = __longlong_as_double(0x7ff8000000000000LL);
  const int s = a.slots[i];
  const bool ok = fr_slot_ok(a.p, s);
  const int q0 = a.cand0[i], q1 = ok ? a.cand0[i + 1] : q0;
  const double b = ok ? a.p.bound[s] : 0.0;
  if (a.table) {
    for (int r = tid; r < R; r += FR_THREADS) a.table[(long)i * R + r] = nan;
    __syncthreads();                                    // the fill, then the candidates' entries (one workgroup writes both)
  }
  double bv = 0.0;
  int bq = -1;
  for (int q = q0 + tid; q < q1; q += FR_THREADS) {     // position order: a strict comparison keeps the first of equal values
    double imp = nan;
    if (a.live[2L * q] && a.live[2L * q + 1])
      imp = b < 0.0 ? fr_improvement(fr_child_lb(a.infeasible, a.bound, 2L * q), fr_child_lb(a.infeasible, a.bound, 2L * q + 1), b) : 1.0;
    a.imp[q] = imp;
    int node;
    if (a.table && fr_node(a.s, a.cand_dec[2L * q], a.cand_dec[2L * q + 1], &node)) a.table[(long)i * R + node] = imp;
    if (imp == imp && (bq < 0 || imp > bv)) { bv = imp; bq = q; }
  }
  sv[tid] = bv; sq[tid] = bq;
  __syncthreads();
  for (int w = FR_THREADS / 2; w > 0; w >>= 1) {        // the total order (value descending, position ascending); -1: no number yet
    if (tid < w) {
      const int o = sq[tid + w];
      if (o >= 0 && (sq[tid] < 0 || sv[tid + w] > sv[tid] || (sv[tid + w] == sv[tid] && o < sq[tid]))) { sv[tid] = sv[tid + w]; sq[tid] = o; }
    }
    __syncthreads();
  }
  if (tid == 0) {
    const int q = sq[0];
    a.decisions[2 * i] = q >= 0 ? a.cand_dec[2L * q] : -1;
    a.decisions[2 * i + 1] = q >= 0 ? a.cand_dec[2L * q + 1] : -1;
    a.best[i] = q >= 0 ? sv[0] : nan;
  }
}

__global__ __launch_bounds__(FR_THREADS) void k_strong_rows_jobs(StrongRowsArgs a) {
  const int row = blockIdx.x, q = row >> 1;
  if (q >= a.c) return;
  const int s = a.cand_slot[q];
  if (s < 0 || s / a.seg_cap >= a.S) return;            // (gnnb_strong_list lists no such slot: the guard protects memory)
  fr_seg_row(a.r, s / a.seg_cap, row);
}
